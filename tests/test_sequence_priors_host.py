"""CPU: so_icp_set_sequence_priors -- what can be held without a device: the symbol and its constants, the device-free decision which
solve kernel a frame of the chained path launches (reg_plan.h), the split form of pose_prior.h (T_meas apart from the other words)
against so_icp_pose_prior_sums to the bit, the refusal on a host-only context, and -- with the Seam C host loop on the oracle, the prior
in every Sums -- that the priors tests/test_gpu_sequence_priors.py uses make its runs take the paths its conditions name."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import pose_prior_ref as ppr
import sequence_priors_data as spd
from test_pose_prior_host import COUNTS, prior_cases

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "native", "sequence_priors_host.cpp")
LIB = os.path.join(HERE, "native", "libsequence_priors_host.so")
HDR = os.path.join(ROOT, "superodom_amd", "csrc")
F64P = C.POINTER(C.c_double)


@pytest.fixture(scope="module")
def native():
    deps = [SRC] + [os.path.join(HDR, h) for h in ("reg_plan.h", "pose_prior.h", "lm_solver.h", "so_math.h")]
    if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-fPIC", "-shared", "-I", HDR, SRC, "-o", LIB])
    L = C.CDLL(LIB)
    L.sp_sequence_solve_kernel.argtypes = [C.c_int, C.c_int]
    L.sp_solve_kernel_kinds.argtypes = [C.POINTER(C.c_int)]; L.sp_solve_kernel_kinds.restype = None
    L.sp_prior_add.argtypes = [F64P, F64P, F64P]; L.sp_prior_add.restype = None
    L.sp_prior_add_at.argtypes = [F64P, F64P, F64P, F64P]; L.sp_prior_add_at.restype = None
    return L


def test_symbol_and_constants(soicp):
    L = soicp.load()
    assert "so_icp_set_sequence_priors" in soicp.EXPORTED and L.so_icp_set_sequence_priors
    header = open(os.path.join(ROOT, "include", "so_icp.h")).read()
    for name, value in (("NONE", 0), ("GIVEN", 1), ("AT_GUESS", 2)):
        assert re.search(rf"#define SO_ICP_PRIOR_{name}\s+{value}\b", header), name
        assert getattr(soicp, "PRIOR_" + name) == value
    assert re.search(r"int so_icp_set_sequence_priors\(so_icp_ctx \*ctx, int count, const so_icp_pose_prior \*priors[^)]*const uint8_t \*modes[^)]*\);", header)
    assert L.so_icp_abi_version() == 4  # (no version bump, as for so_icp_set_pose_prior)
    assert hasattr(soicp.LidarSlamGpu, "set_sequence_priors")


def test_which_kernel_a_frame_of_the_chained_path_launches(native):
    kinds = (C.c_int * 3)()
    native.sp_solve_kernel_kinds(kinds)
    plain, prior, at_guess = kinds[0], kinds[1], kinds[2]
    assert (plain, prior, at_guess) == (0, 1, 2)
    # no prior: the kernel that was always launched, chained or not
    assert native.sp_sequence_solve_kernel(spd.NONE, 0) == plain and native.sp_sequence_solve_kernel(spd.NONE, 1) == plain
    # a given measurement: the host has every word
    assert native.sp_sequence_solve_kernel(spd.GIVEN, 0) == prior and native.sp_sequence_solve_kernel(spd.GIVEN, 1) == prior
    # at the guess: the host knows the guess of a start that is not chained (frame 0, an unchained start, the start after a broken chain)
    # exactly and fills T_meas itself; a chained frame's guess is formed on the device, and only there
    assert native.sp_sequence_solve_kernel(spd.AT_GUESS, 0) == prior
    assert native.sp_sequence_solve_kernel(spd.AT_GUESS, 1) == at_guess


def test_reg_plan_still_needs_no_device_headers():
    text = open(os.path.join(HDR, "reg_plan.h")).read()
    assert sorted(re.findall(r'#include\s+[<"]([^>"]+)[>"]', text)) == ["algorithm", "cstddef", "cstdint", "so_math.h"]
    assert "sequence_solve_kernel" in text


def _words(s):
    return np.frombuffer(bytes(s), np.float64).copy()


def test_split_form_equals_pose_prior_sums_to_the_bit(soicp, native):
    """pose_prior_add_at(Tm, P, ...) with Tm inside the struct, and with Tm in a buffer of its own beside a struct whose T_meas words are
    poisoned, against so_icp_pose_prior_sums (the library's build of pose_prior_add): every word of the sums, on empty sums and on sums
    that hold something"""
    rng = np.random.default_rng(7)
    A = rng.standard_normal((6, 6))
    n = 0
    for tag, prior, pose in prior_cases(soicp):
        pose = np.ascontiguousarray(pose, np.float64)
        P = _words(prior)
        assert P.size == 55
        Tm = P[:7].copy()
        poisoned = P.copy(); poisoned[:7] = np.nan
        for count in COUNTS:
            for base in (ppr.empty_sums(count), soicp.LmDriver.sums(12.5, float(count), rng.standard_normal(6), A @ A.T, list(range(16)))):
                start = _words(base)
                want = _words(soicp.pose_prior_sums(prior, pose, base))
                for Tm_arg, P_arg, how in ((P[:7], P, "inside"), (Tm, poisoned, "apart")):
                    got = start.copy()
                    native.sp_prior_add_at(np.ascontiguousarray(Tm_arg).ctypes.data_as(F64P), P_arg.ctypes.data_as(F64P), pose.ctypes.data_as(F64P), got.ctypes.data_as(F64P))
                    assert got.tobytes() == want.tobytes(), (tag, count, how, np.flatnonzero(got != want))
                got = start.copy()
                native.sp_prior_add(P.ctypes.data_as(F64P), pose.ctypes.data_as(F64P), got.ctypes.data_as(F64P))
                assert got.tobytes() == want.tobytes(), (tag, count, "unsplit")
                n += 1
    assert n == len(prior_cases(soicp)) * len(COUNTS) * 2


def test_host_only_context_and_bad_arguments(soicp):
    L = soicp.load()
    host = soicp.LidarSlamGpu(device_id=-1, plane_res=0.2)
    prior = soicp.pose_prior([0, 0, 0, 0, 0, 0, 1.0], np.eye(6))
    arr = (soicp.PosePrior * 2)(prior, prior)
    assert L.so_icp_set_sequence_priors(None, 2, arr, None) == -1
    assert L.so_icp_set_sequence_priors(host.h, -1, arr, None) == -1
    assert L.so_icp_set_sequence_priors(host.h, 2, arr, None) == -2 and b"no CPU fallback" in L.so_icp_last_error(host.h)
    assert L.so_icp_set_sequence_priors(host.h, 0, None, None) == -2
    with pytest.raises(soicp.SoIcpError, match="no CPU fallback"):
        host.set_sequence_priors([prior, prior], [spd.GIVEN, spd.AT_GUESS])
    host.close()


def test_the_schedule_restated_on_iteration_counts():
    # two iterations each, two enqueued ahead: everything behind frame 0 is chained
    assert spd.schedule([2, 2, 2, 2]) == ([False, True, True, True], 0)
    # frame 1 needs three where two were enqueued: frame 2 starts again; frame 2 then gets three
    assert spd.schedule([2, 3, 2, 2]) == ([False, True, False, True], 1)
    # the last frame breaks nothing
    assert spd.schedule([2, 2, 4]) == ([False, True, True], 0)
    # frame 0 needs one: frame 2, enqueued while frame 1 runs, gets one, needs two and breaks the chain for frame 3
    assert spd.schedule([1, 2, 2, 2]) == ([False, True, True, False], 1)


@pytest.mark.parametrize("kind", spd.U_KINDS)
@pytest.mark.parametrize("run", list(spd.RUNS))
def test_the_priors_make_the_runs_take_the_paths_the_gpu_tests_need(oracle, run, kind):
    """The GPU tests need chained frames whose prior is measured at the guess (the new kernel runs nowhere else) and, in the broken run, a
    chain break.  Whether a frame is chained follows from the outer iterations of the frames in front of it; those are taken here from
    the host loop on the oracle with the prior in every Sums."""
    iters = spd.oracle_iterations(oracle, run, kind)
    chained, breaks = spd.schedule(iters)
    modes = spd.modes_of(run)
    print(run, kind, "outer iterations", iters, "chained", chained, "breaks", breaks, "modes", modes)
    assert sum(chained) >= 2
    assert any(c and m == spd.AT_GUESS for c, m in zip(chained, modes)), "no chained frame measures at its guess"
    if run == "broken":
        assert breaks >= 1 and max(iters) > min(iters)
    else:
        assert sorted(set(modes)) == [spd.NONE, spd.GIVEN, spd.AT_GUESS]
