"""CPU: so_icp_set_batch_priors -- what can be held without a device: the symbol and its declaration, the device-free decision which
batched solve kernel a round launches (reg_plan.h), the refusals on a host-only context, and -- with the Seam C host loop on the oracle,
the prior in every Sums -- that the guesses and priors tests/test_gpu_batch_priors.py uses are discriminating: a prior moves its
hypothesis' result, and the hypotheses leave the rounds at different times."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import batch_priors_data as bpd

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "native", "batch_priors_host.cpp")
LIB = os.path.join(HERE, "native", "libbatch_priors_host.so")
HDR = os.path.join(ROOT, "superodom_amd", "csrc")
ORACLE_HYPOTHESES = 12  # of "tiny70", whose first five are "tiny5": every residue of the guesses' h % 7 and h % 5, three of each mode


@pytest.fixture(scope="module")
def native():
    deps = [SRC] + [os.path.join(HDR, h) for h in ("reg_plan.h", "so_math.h")]
    if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-fPIC", "-shared", "-I", HDR, SRC, "-o", LIB])
    L = C.CDLL(LIB)
    L.bp_batch_solve_kernel.argtypes = [C.POINTER(C.c_uint8), C.POINTER(C.c_uint32), C.c_uint32]
    L.bp_batch_solve_kernel_kinds.argtypes = [C.POINTER(C.c_int)]; L.bp_batch_solve_kernel_kinds.restype = None
    return L


def test_symbol_and_declaration(soicp):
    L = soicp.load()
    assert "so_icp_set_batch_priors" in soicp.EXPORTED and L.so_icp_set_batch_priors
    header = open(os.path.join(ROOT, "include", "so_icp.h")).read()
    assert re.search(r"int so_icp_set_batch_priors\(so_icp_ctx \*ctx, int n_hyp, const so_icp_pose_prior \*priors[^)]*const uint8_t \*modes[^)]*\);", header)
    assert L.so_icp_abi_version() == 4  # (no version bump, as for the two setters before it)
    assert hasattr(soicp.LidarSlamGpu, "set_batch_priors")


def test_host_only_context_and_bad_arguments(soicp):
    L = soicp.load()
    host = soicp.LidarSlamGpu(device_id=-1, plane_res=0.2)
    prior = soicp.pose_prior([0, 0, 0, 0, 0, 0, 1.0], np.eye(6))
    arr = (soicp.PosePrior * 2)(prior, prior)
    assert L.so_icp_set_batch_priors(None, 2, arr, None) == -1
    assert L.so_icp_set_batch_priors(host.h, -1, arr, None) == -1
    assert L.so_icp_set_batch_priors(host.h, 2, arr, None) == -2 and b"no CPU fallback" in L.so_icp_last_error(host.h)
    assert L.so_icp_set_batch_priors(host.h, 0, None, None) == -2
    with pytest.raises(soicp.SoIcpError, match="no CPU fallback"):
        host.set_batch_priors([prior, prior], [bpd.GIVEN, bpd.AT_GUESS])
    host.close()


def _kernel(native, modes, active):
    m = None if modes is None else (C.c_uint8 * len(modes))(*modes)
    a = (C.c_uint32 * max(1, len(active)))(*active)
    return native.bp_batch_solve_kernel(m, a, len(active))


def test_which_kernel_a_round_of_a_batch_launches(native):
    kinds = (C.c_int * 2)()
    native.bp_batch_solve_kernel_kinds(kinds)
    plain, prior = kinds[0], kinds[1]
    assert (plain, prior) == (0, 1)
    modes = [bpd.GIVEN, bpd.NONE, bpd.AT_GUESS, bpd.NONE, bpd.NONE]
    # a batch without priors, and a list none of whose hypotheses carries one: the kernel that was always launched
    assert _kernel(native, None, [0, 1, 2, 3, 4]) == plain
    assert _kernel(native, [bpd.NONE] * 5, [0, 1, 2, 3, 4]) == plain
    assert _kernel(native, modes, [1, 3, 4]) == plain and _kernel(native, modes, [4]) == plain and _kernel(native, modes, []) == plain
    # any prior in the list, given or at the guess, wherever it stands: the kernel with the table
    assert _kernel(native, modes, [0, 1, 2, 3, 4]) == prior
    assert _kernel(native, modes, [1, 3, 0]) == prior and _kernel(native, modes, [2]) == prior and _kernel(native, modes, [3, 2, 4]) == prior
    # the list indexes the group's hypotheses, not positions of the list
    assert _kernel(native, [bpd.NONE, bpd.NONE, bpd.NONE, bpd.NONE, bpd.GIVEN], [4]) == prior
    assert _kernel(native, [bpd.GIVEN, bpd.NONE, bpd.NONE, bpd.NONE, bpd.NONE], [4]) == plain


def test_reg_plan_still_needs_no_device_headers():
    text = open(os.path.join(HDR, "reg_plan.h")).read()
    assert sorted(re.findall(r'#include\s+[<"]([^>"]+)[>"]', text)) == ["algorithm", "cstddef", "cstdint", "so_math.h"]
    assert "batch_solve_kernel" in text and "sequence_solve_kernel" in text


def test_the_cases_and_their_modes():
    assert {c: bpd.CASES[c][:2] for c in bpd.CASES} == {"tiny5": ("tiny", 5), "tiny70": ("tiny", 70), "small9": ("small", 9)}
    assert bpd.modes_of(5) == [bpd.GIVEN, bpd.NONE, bpd.AT_GUESS, bpd.AT_GUESS, bpd.GIVEN]
    sc, scan, poses, priors, modes, sub = bpd.batch_inputs("tiny70", "dense")
    assert len(poses) == len(priors) == len(modes) == 70 and sub is None
    for h in range(70):
        assert np.isnan(np.array(priors[h].T_meas[:])).all() == (modes[h] != bpd.GIVEN), h
    # a wrong table index across the group boundary would show: hypotheses h and 64 + h carry the same mode and different priors
    for h in range(6):
        assert modes[h] == modes[64 + h]
        a, b = [bpd.hypothesis_prior(priors, modes, k, poses[k]) for k in (h, 64 + h)]
        assert (a is None) == (b is None) == (modes[h] == bpd.NONE)
        assert a is None or bytes(a) != bytes(b), h
    # the shorter case is the head of the longer one
    sc5, _, poses5, priors5, modes5, _ = bpd.batch_inputs("tiny5", "dense")
    assert np.array_equal(poses5, poses[:5]) and modes5 == modes[:5]
    assert all(np.array_equal(np.array(a.sqrt_information[:]), np.array(b.sqrt_information[:])) for a, b in zip(priors5, priors))


@pytest.mark.parametrize("kind", bpd.U_KINDS)
def test_the_inputs_of_the_gpu_tests_are_discriminating(oracle, kind):
    """On the oracle, through the Seam C host loop with the prior in every Sums: every hypothesis of "tiny" that carries a prior ends at
    another pose than its plain registration (a batch that dropped, or misplaced, its priors could not pass the GPU tests), and the
    hypotheses run different numbers of outer iterations (chained rounds meet lists that have gone stale)."""
    rows = bpd.oracle_hypotheses(oracle, "tiny70", kind, ORACLE_HYPOTHESES)
    assert len(rows) == ORACLE_HYPOTHESES
    for h, (mode, iters, pose, plain_iters, plain_pose) in enumerate(rows):
        print(kind, h, "mode", mode, "outer iterations", iters, "plain", plain_iters, "|dt|", float(np.linalg.norm(pose[:3] - plain_pose[:3])))
        if mode == bpd.NONE:
            assert iters == plain_iters and pose.tobytes() == plain_pose.tobytes()
        else:
            assert pose.tobytes() != plain_pose.tobytes(), (kind, h, "the prior does not move the result")
    assert sorted({r[0] for r in rows}) == [bpd.NONE, bpd.GIVEN, bpd.AT_GUESS]
    assert len({r[1] for r in rows}) >= 2, "every hypothesis runs the same number of outer iterations"
