"""CPU: so_icp_keep_batch_correspondences / so_icp_batch_correspondences / so_icp_batch_correspondence_sums -- what can be held without
a device: the symbols and their declarations, the refusals on a host-only context (code and whole text; every export reports
valid = 0), the device-free layout of an export (reg_plan.h: the selection's check, the record ranges from reported counts, ticket ->
(entry, tile)), and -- with the Seam C host loop on the oracle -- that the guesses tests/test_gpu_batch_correspondences.py uses give
the export something to tell apart."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import batch_correspondences_data as bcd

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "native", "batch_correspondences_host.cpp")
LIB = os.path.join(HERE, "native", "libbatch_correspondences_host.so")
HDR = os.path.join(ROOT, "superodom_amd", "csrc")
NO_DEVICE = "host-only context (device_id < 0): no compute path -- libsoicp has no CPU fallback"


@pytest.fixture(scope="module")
def native():
    deps = [SRC] + [os.path.join(HDR, h) for h in ("reg_plan.h", "so_math.h")]
    if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-fPIC", "-shared", "-I", HDR, SRC, "-o", LIB])
    L = C.CDLL(LIB)
    i32p = C.POINTER(C.c_int32)
    L.bc_selection_first_bad.argtypes = [i32p, C.c_int, C.c_int]
    L.bc_record_ranges.argtypes = [C.POINTER(C.c_uint32), C.POINTER(C.c_uint8), i32p, C.c_int, C.POINTER(C.c_uint64)]
    L.bc_record_ranges.restype = C.c_uint64
    L.bc_ticket.argtypes = [C.c_uint32, C.POINTER(C.c_uint32), C.c_uint32, C.POINTER(C.c_uint32)]; L.bc_ticket.restype = None
    return L


def test_symbols_and_declarations(soicp):
    L = soicp.load()
    names = ["so_icp_keep_batch_correspondences", "so_icp_batch_correspondences", "so_icp_batch_correspondence_sums"]
    assert soicp.EXPORTED[-3:] == names, "the three symbols, in this order, behind the others"
    for name in names:
        assert getattr(L, name)
    header = open(os.path.join(ROOT, "include", "so_icp.h")).read()
    assert re.search(r"int so_icp_keep_batch_correspondences\(so_icp_ctx \*ctx, int on\);", header)
    assert re.search(r"int so_icp_batch_correspondences\(so_icp_ctx \*ctx, const int32_t \*hyp[^)]*int n_sel,\s*const double \*poses[^)]*"
                     r"so_icp_correspondence \*records, size_t cap_records,\s*uint64_t \*first_record[^)]*uint8_t \*status_out[^)]*size_t cap_status,\s*"
                     r"void \*\*d_records_out, so_icp_correspondence_info \*info[^)]*\);", header)
    assert re.search(r"int so_icp_batch_correspondence_sums\(so_icp_ctx \*ctx, const int32_t \*hyp, int n_sel,\s*const double \*poses[^)]*"
                     r"int n_poses[^)]*so_icp_sums \*sums_out[^)]*\);", header)
    assert header.index("so_icp_keep_batch_correspondences(so_icp_ctx") < header.index("so_icp_batch_correspondences(so_icp_ctx") < header.index("so_icp_batch_correspondence_sums(so_icp_ctx")
    m = re.search(r"#define SO_ICP_BATCH_MAX_SELECTION (\d+)", header)
    assert m and int(m.group(1)) == soicp.BATCH_MAX_SELECTION >= 64
    assert L.so_icp_abi_version() == 4  # (no version bump: no struct changed)
    for method in ("keep_batch_correspondences", "batch_correspondences", "batch_correspondence_sums"):
        assert hasattr(soicp.LidarSlamGpu, method)
    assert "Not exported: the correspondences of so_icp_register_batch" not in header


def test_host_only_context_refusals_and_nothing_to_export(soicp):
    L = soicp.load()
    host = soicp.LidarSlamGpu(device_id=-1, plane_res=0.2)
    err = lambda: L.so_icp_last_error(host.h).decode()
    # the switch
    assert L.so_icp_keep_batch_correspondences(None, 1) == -1
    for on in (1, 0):
        assert L.so_icp_keep_batch_correspondences(host.h, on) == -2 and err() == NO_DEVICE
    assert host.keep_batch_correspondences(True) == -2
    # the export: refused, and every entry reports valid = 0 with zero counts and ranges
    n_sel = 3
    info = (soicp.CorrespondenceInfo * n_sel)()
    C.memset(info, 0xFF, C.sizeof(info))
    first = np.full(n_sel + 1, 7, np.uint64)
    d = C.c_void_p(1)
    assert L.so_icp_batch_correspondences(None, None, n_sel, None, None, 0, None, None, 0, None, None) == -1
    rc = L.so_icp_batch_correspondences(host.h, None, n_sel, None, None, 0, first.ctypes.data_as(C.POINTER(C.c_uint64)), None, 0, C.byref(d), info)
    assert rc == -2 and err() == NO_DEVICE
    assert bytes(info) == bytes(C.sizeof(info)) and not first.any() and d.value is None
    assert all(info[k].valid == 0 and info[k].n_accepted == 0 for k in range(n_sel))
    for bad in (-1, soicp.BATCH_MAX_SELECTION + 1):
        assert L.so_icp_batch_correspondences(host.h, None, bad, None, None, 0, None, None, 0, None, None) == -1
        assert err() == "so_icp_batch_correspondences: n_sel must be 0 .. SO_ICP_BATCH_MAX_SELECTION"
    with pytest.raises(soicp.SoIcpError) as e:
        host.batch_correspondences(n_sel=2)
    assert str(e.value) == "so_icp error -2: " + NO_DEVICE
    # the sums: argument checks first, then the refusal; the output is zeroed
    poses = np.tile(np.array([0, 0, 0, 0, 0, 0, 1.0]), (n_sel, 2, 1))
    pp = poses.ctypes.data_as(C.POINTER(C.c_double))
    out = (soicp.Sums * (n_sel * 2))()
    C.memset(out, 0xFF, C.sizeof(out))
    assert L.so_icp_batch_correspondence_sums(None, None, n_sel, pp, 2, out) == -1
    assert L.so_icp_batch_correspondence_sums(host.h, None, n_sel, pp, 2, out) == -2 and err() == NO_DEVICE
    assert bytes(out) == bytes(C.sizeof(out))
    for n_poses in (0, soicp.SUMS_MAX_POSES + 1):
        assert L.so_icp_batch_correspondence_sums(host.h, None, n_sel, pp, n_poses, out) == -1
        assert err() == "so_icp_batch_correspondence_sums: n_poses must be 1 .. SO_ICP_SUMS_MAX_POSES"
    for bad in (-1, soicp.BATCH_MAX_SELECTION + 1):
        assert L.so_icp_batch_correspondence_sums(host.h, None, bad, pp, 2, out) == -1
        assert err() == "so_icp_batch_correspondence_sums: n_sel must be 0 .. SO_ICP_BATCH_MAX_SELECTION"
    for a, b in ((None, out), (pp, None)):
        assert L.so_icp_batch_correspondence_sums(host.h, None, n_sel, a, 2, b) == -1
        assert err() == "so_icp_batch_correspondence_sums: poses and sums_out must not be NULL"
    with pytest.raises(soicp.SoIcpError) as e:
        host.batch_correspondence_sums(poses)
    assert str(e.value) == "so_icp error -2: " + NO_DEVICE
    # the batch itself is refused as before
    assert L.so_icp_register_batch(host.h, None, None, 0, 12, pp, 1, pp, None, None) == -2
    host.close()


def _ranges(native, accepted, valid, hyp, n_sel=None):
    a = (C.c_uint32 * max(1, len(accepted)))(*accepted)
    v = (C.c_uint8 * max(1, len(valid)))(*valid)
    n_sel = len(hyp) if hyp is not None else n_sel
    h = None if hyp is None else (C.c_int32 * max(1, n_sel))(*hyp)
    first = (C.c_uint64 * (n_sel + 1))(*([99] * (n_sel + 1)))
    total = native.bc_record_ranges(a, v, h, n_sel, first)
    return total, list(first)


def test_record_ranges_from_reported_counts(native):
    accepted, valid = [10, 0, 7, 4096, 3], [1, 1, 0, 1, 1]
    # NULL: hypotheses 0 .. n_sel - 1; an invalid hypothesis has width 0 whatever it counted; a valid one of no accepted point too
    assert _ranges(native, accepted, valid, None, 5) == (4109, [0, 10, 10, 10, 4106, 4109])
    assert _ranges(native, accepted, valid, None, 2) == (10, [0, 10, 10])
    assert _ranges(native, accepted, valid, None, 0) == (0, [0])
    # any order, a subset
    assert _ranges(native, accepted, valid, [4, 3, 0]) == (4109, [0, 3, 4099, 4109])
    assert _ranges(native, accepted, valid, [2]) == (0, [0, 0])
    # an index that repeats gets a range of its own each time
    assert _ranges(native, accepted, valid, [0, 0, 2, 0]) == (30, [0, 10, 20, 20, 30])
    # counts near 2^32 do not wrap
    assert _ranges(native, [0xFFFFFFFF, 0xFFFFFFFF], [1, 1], [0, 1, 0]) == (3 * 0xFFFFFFFF, [0, 0xFFFFFFFF, 2 * 0xFFFFFFFF, 3 * 0xFFFFFFFF])


def test_selection_check(native):
    bad = lambda hyp, n_hyp, n_sel=None: native.bc_selection_first_bad(None if hyp is None else (C.c_int32 * max(1, len(hyp)))(*hyp),
                                                                       len(hyp) if hyp is not None else n_sel, n_hyp)
    assert bad([0, 4, 2, 2], 5) == -1 and bad([], 5) == -1 and bad(None, 5, 5) == -1 and bad(None, 0, 0) == -1
    assert bad([0, 5], 5) == 1 and bad([-1, 0], 5) == 0 and bad([0, 1, 2, 70], 70) == 3
    assert bad(None, 5, 6) == 5 and bad([0], 0) == 0


@pytest.mark.parametrize("nblk, n_sel", [(1, 1), (1, 5), (2, 3), (4, 3), (5, 7), (128, 2)])
def test_every_ticket_of_small_grids(native, nblk, n_sel):
    """hypothesis-major: over a batch's prefix table, tile_first[k] = k * nblk, the tickets of entry k are k * nblk .. (k + 1) * nblk - 1,
    tile after tile -- so a workgroup's look-back (tiles below its own, same entry) only ever names smaller tickets, and every
    (entry, tile) is worked on exactly once"""
    seen = []
    out = (C.c_uint32 * 2)()
    tile_first = (C.c_uint32 * (n_sel + 1))(*[k * nblk for k in range(n_sel + 1)])
    for t in range(nblk * n_sel):
        native.bc_ticket(t, tile_first, n_sel, out)
        k, tile = out[0], out[1]
        assert (k, tile) == (t // nblk, t % nblk) and k < n_sel and tile < nblk
        assert all(k * nblk + below < t for below in range(tile)), "a predecessor of the chain with a larger ticket"
        seen.append((k, tile))
    assert seen == [(k, b) for k in range(n_sel) for b in range(nblk)]


def test_reg_plan_still_needs_no_device_headers():
    text = open(os.path.join(HDR, "reg_plan.h")).read()
    assert sorted(re.findall(r'#include\s+[<"]([^>"]+)[>"]', text)) == ["algorithm", "cstddef", "cstdint", "so_math.h"]
    assert "batch_record_ranges" in text and "selection_ticket" in text


def test_the_cases():
    assert {c: bcd.CASES[c] for c in bcd.CASES} == {"tiny5": ("tiny", 5, None), "tiny70": ("tiny", 70, None), "small9": ("small", 9, 1500)}
    sc, scan, poses, sub = bcd.batch_inputs("tiny70")
    assert len(scan) == 4096 and poses.shape == (70, 7) and sub is None
    sc, scan5, poses5, _ = bcd.batch_inputs("tiny5")
    assert np.array_equal(poses5, poses[:5]) and np.array_equal(scan5, scan)
    assert len({p.tobytes() for p in poses}) == 70, "hypotheses 64 .. 69 (the second group's slices) start elsewhere than 0 .. 5"
    assert bcd.SIZES == [0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4096] and max(bcd.SIZES) == len(scan)
    near = bcd.poses_near(poses[0], 64, 5)
    assert near.shape == (64, 7) and np.array_equal(near[0], poses[0]) and len({p.tobytes() for p in near}) == 64


@pytest.mark.parametrize("case", bcd.ADEQUACY_CASES)
def test_the_inputs_of_the_gpu_tests_are_discriminating(oracle, case):
    """On the oracle, through the Seam C host loop: every hypothesis accepts at least one point, the hypotheses do not all end in the
    same outer iteration (pose_fit / outer_iteration differ between entries), and at least two hypotheses accept different points (an
    export that read another hypothesis' slice could not pass the GPU tests)."""
    rows = bcd.oracle_sets(oracle, case)
    assert len(rows) == bcd.CASES[case][1]
    for h, (iters, idx) in enumerate(rows):
        print(case, h, "outer iterations", iters, "accepted", len(idx))
        assert len(idx) >= 1, (case, h)
    assert len({r[0] for r in rows}) >= 2, "every hypothesis ends in the same outer iteration"
    assert len({r[1].tobytes() for r in rows}) >= 2, "every hypothesis accepts the same points"
