"""CPU: so_icp_match_batch -- what can be held without a device: the symbol, its declaration and its binding; the refusals a host-only
context can reach (code and whole text); the rule by which a pending prior of any kind refuses the entry (reg_plan.h refused_prior: a
host-only context cannot hold a pending prior, its setters are refused first, so the refusal's code, text and the prior that stays
pending are held on the device, tests/test_gpu_match_batch.py); the device-free mapping of the launch (reg_plan.h: workgroup ->
(hypothesis, virtual workgroup), a hypothesis' record words and ticket word); and, on the oracle, that the poses of
tests/match_batch_data.py are what the GPU tests take them for."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import match_batch_data as mbd

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "native", "match_batch_host.cpp")
LIB = os.path.join(HERE, "native", "libmatch_batch_host.so")
HDR = os.path.join(ROOT, "superodom_amd", "csrc")
NO_DEVICE = "host-only context (device_id < 0): no compute path -- libsoicp has no CPU fallback"
# the batch's reservations per hypothesis (kernels.h; test_the_reservations_are_the_batchs holds them against its text)
N_VALUES, MAX_GRID, PARTIAL_STRIDE, SYNC_STRIDE = 29, 256, 256 * 40 * 2, (16 * 32 * 4 + 8 * 16) // 4


@pytest.fixture(scope="module")
def native():
    deps = [SRC] + [os.path.join(HDR, h) for h in ("reg_plan.h", "so_math.h")]
    if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-fPIC", "-shared", "-I", HDR, SRC, "-o", LIB])
    L = C.CDLL(LIB)
    u32 = C.c_uint32
    L.mb_slot.argtypes = [u32, u32, C.POINTER(u32)]; L.mb_slot.restype = None
    L.mb_partial_word.argtypes = [C.c_ulonglong, u32, u32, u32, u32]; L.mb_partial_word.restype = C.c_ulonglong
    L.mb_ticket_word.argtypes = [C.c_ulonglong, u32]; L.mb_ticket_word.restype = C.c_ulonglong
    L.mb_refused_by.argtypes = [C.c_int]
    L.mb_check_grid.argtypes = [u32] * 6
    return L


def test_symbol_declaration_and_binding(soicp):
    L = soicp.load()
    assert L.so_icp_match_batch and "so_icp_match_batch" in soicp.EXPORTED
    assert L.so_icp_abi_version() == 4  # (no version bump: no struct changed)
    header = open(os.path.join(ROOT, "include", "so_icp.h")).read()
    assert re.search(r"int so_icp_match_batch\(so_icp_ctx \*ctx, const float \*scan_xyz, const void \*d_scan_xyz, size_t n, size_t stride_bytes,\s*"
                     r"const double \*poses[^,]*, int n_poses,\s*so_icp_stats \*stats[^,]*, int32_t \*rc_out[^)]*\);", header)
    assert hasattr(soicp.LidarSlamGpu, "match_batch")


def test_refusals_on_a_host_only_context(soicp):
    L = soicp.load()
    host = soicp.LidarSlamGpu(device_id=-1, plane_res=0.2)
    err = lambda: L.so_icp_last_error(host.h).decode()
    poses = np.tile(np.array([0, 0, 0, 0, 0, 0, 1.0]), (2, 1))
    pp, f32p = poses.ctypes.data_as(C.POINTER(C.c_double)), C.POINTER(C.c_float)
    scan = np.zeros((4, 3), np.float32)
    st = (soicp.Stats * 2)()
    rcs = (C.c_int32 * 2)(7, 7)
    # the arguments first: SO_ICP_E_INVALID
    assert L.so_icp_match_batch(None, scan.ctypes.data_as(f32p), None, 4, 12, pp, 2, st, rcs) == -1
    assert L.so_icp_match_batch(host.h, scan.ctypes.data_as(f32p), None, 4, 12, None, 2, st, rcs) == -1, "NULL poses"
    assert L.so_icp_match_batch(host.h, scan.ctypes.data_as(f32p), None, 4, 12, pp, 2, None, rcs) == -1, "NULL stats"
    assert L.so_icp_match_batch(host.h, scan.ctypes.data_as(f32p), None, 4, 12, pp, -1, st, rcs) == -1, "n_poses < 0"
    assert L.so_icp_match_batch(host.h, None, None, 4, 12, pp, 2, st, rcs) == -1, "n > 0 without a scan"
    # then the context: no device, whatever the rest (n_poses == 0 and an empty scan included)
    for n, n_poses in ((4, 2), (4, 0), (0, 2)):
        assert L.so_icp_match_batch(host.h, scan.ctypes.data_as(f32p), None, n, 12, pp, n_poses, st, rcs) == -2 and err() == NO_DEVICE, (n, n_poses)
    assert list(rcs) == [7, 7], "a refused call writes no rc_out"
    with pytest.raises(soicp.SoIcpError) as e:
        host.match_batch(scan, poses)
    assert str(e.value) == "so_icp error -2: " + NO_DEVICE
    # no prior can be pending here -- the setters are refused the same way --, so the pending-prior refusals are the device suite's
    assert L.so_icp_set_batch_priors(host.h, 1, None, None) == -2 and L.so_icp_set_pose_prior(host.h, None) == -2
    host.close()


def test_a_pending_prior_of_any_kind_refuses_the_entry(native):
    none, single, run, batch = 0, 1, 2, 3  # reg_plan.h PriorKind (tests/test_reg_plan_host.py holds the numbers)
    assert native.mb_refused_by(none) == none, "nothing pending: the entry goes on"
    for pending in (single, run, batch):
        assert native.mb_refused_by(pending) == pending, "refused because of what is pending (refuse_pending names it and leaves it)"
    text = open(os.path.join(HDR, "batch.cpp")).read()
    assert 'refuse_pending(c, "so_icp_match_batch", kPriorsNone)' in text


def test_the_reservations_are_the_batchs():
    text = open(os.path.join(HDR, "kernels.h")).read()
    const = lambda name: re.search(r"\b%s = ([A-Za-z0-9_]+)" % name, text).group(1)
    assert re.search(r"#define SO_SOLVE_BLOCKS 256", text) and const("kFitBlocksMax") == "SO_SOLVE_BLOCKS" and const("kRecordChunksMax") == "40"
    assert const("kArriveCounters") == "16" and const("kArriveStrideWords") == "32" and "kHandoffWordOffset * 4 + 8 * 16" in text
    batch = open(os.path.join(HDR, "batch.cpp")).read()
    assert "(size_t)kFitBlocksMax * kRecordChunksMax * 2), (uint32_t)(kSyncBytes / 4)" in batch, "BatchView::partial_stride / sync_stride"
    assert "(size_t)kFitBlocksMax * kRecordChunksMax * 16" in batch and "cap * kSyncBytes" in batch, "batch_reserve"
    plane = open(os.path.join(HDR, "plane_factor.h")).read()
    assert re.search(r"kPlaneFactorSums = 29\b", plane)


@pytest.mark.parametrize("V", [1, 2, 16, 256])
@pytest.mark.parametrize("n_act", [1, 5, 64])
def test_every_workgroup_of_the_launch(native, V, n_act):
    """every (hypothesis, virtual workgroup) is served exactly once; the record words of different hypotheses are disjoint and inside the
    hypothesis' share of the record table, never on a chunk's tag half; the ticket words are distinct and inside the hand-off block"""
    assert native.mb_check_grid(V, n_act, N_VALUES, PARTIAL_STRIDE, SYNC_STRIDE, MAX_GRID) == 0
    out = (C.c_uint32 * 2)()
    seen = []
    for b in range(V * n_act):
        native.mb_slot(b, V, out)
        seen.append((out[0], out[1]))
    assert seen == [(e, vb) for e in range(n_act) for vb in range(V)], "hypothesis-major: a hypothesis' workgroups are dispatched together"
    words, tickets = set(), set()
    for h in sorted({0, n_act // 2, n_act - 1}):
        mine = {native.mb_partial_word(h, PARTIAL_STRIDE, a, vb, MAX_GRID) for a in range(N_VALUES) for vb in sorted({0, V // 2, V - 1})}
        assert all(h * PARTIAL_STRIDE <= w < (h + 1) * PARTIAL_STRIDE and (w - h * PARTIAL_STRIDE) % 2 == 0 for w in mine)
        assert not (mine & words)
        words |= mine
        t = native.mb_ticket_word(h, SYNC_STRIDE)
        assert h * SYNC_STRIDE <= t < (h + 1) * SYNC_STRIDE and t not in tickets
        tickets.add(t)
    # the largest word a full grid touches lies in the chunks the batched solve itself uses (256 x 29 of the 256 x 40)
    assert native.mb_partial_word(0, PARTIAL_STRIDE, N_VALUES - 1, MAX_GRID - 1, MAX_GRID) == 2 * (MAX_GRID * N_VALUES - 1) < PARTIAL_STRIDE


def test_a_check_that_can_fail(native):
    assert native.mb_check_grid(16, 5, N_VALUES, 2 * 16 * N_VALUES - 2, SYNC_STRIDE, 16) > 0, "a share one chunk too small"
    assert native.mb_check_grid(16, 5, N_VALUES, PARTIAL_STRIDE, SYNC_STRIDE, 8) > 0, "a grid larger than the table's rows: words collide"


def test_the_stand_alone_program(tmp_path):
    exe = str(tmp_path / "match_batch_host")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Wall", "-I", HDR, SRC, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "match_batch_host: 0 violations", (out.stdout, out.stderr)


def test_reg_plan_still_needs_no_device_headers():
    text = open(os.path.join(HDR, "reg_plan.h")).read()
    assert sorted(re.findall(r'#include\s+[<"]([^>"]+)[>"]', text)) == ["algorithm", "cstddef", "cstdint", "so_math.h"]
    assert "match_batch_slot" in text and "match_batch_partial_word" in text and "match_batch_ticket_word" in text


def test_the_cases():
    assert {c: mbd.CASES[c] for c in mbd.CASES} == {"tiny5": ("tiny", 5, None), "tiny70": ("tiny", 70, None), "small9": ("small", 9, 1500)}
    for case, n_points in (("tiny5", 4096), ("tiny70", 4096), ("small9", 16384)):
        sc, scan, poses, sub = mbd.inputs(case)
        extra = 3 if case in mbd.WITH_EXTRAS else 0
        assert len(scan) == n_points and poses.shape == (mbd.CASES[case][1] + extra, 7) and sub == mbd.CASES[case][2]
        if extra:
            gt = np.asarray(sc.gt_pose(mbd.SCAN_ID), np.float64)
            assert np.array_equal(poses[mbd.REPEAT], poses[0])
            assert np.array_equal(poses[mbd.LOST] - gt, [0, 0, 10.0, 0, 0, 0, 0]) and np.array_equal(poses[mbd.SHIFTED] - gt, [5.0, 0, 0, 0, 0, 0, 0])
    assert mbd.SIZES == [0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4096]
    sc = mbd.inputs("tiny5")[0]
    three = mbd.three_poses(sc)
    assert three.shape == (3, 7) and np.array_equal(three[0], three[1]) and np.array_equal(three[:2], mbd.inputs("tiny5")[2][[0, mbd.REPEAT]])
    assert np.array_equal(three[2], mbd.inputs("tiny5")[2][mbd.LOST])


@pytest.mark.parametrize("case, max_feat", [("tiny5", -1), ("small9", -1), ("small9", 1500)])
def test_the_poses_are_what_the_gpu_tests_take_them_for(oracle, case, max_feat):
    """On the oracle (SampledOracleSeam.match; sub-sampled: the match of a one-iteration orc_register): accepted counts differ between the hypotheses, the lost pose judges every sampled point and
    accepts none (status 2), the repeat equals pose 0, and every pose of the case lies in one map block."""
    rows = mbd.oracle_matches(oracle, case, max_feat)
    sc, scan, poses, sub = mbd.inputs(case)
    n = len(scan)
    accepted = [r[1] for r in rows]
    print(case, "max_surface_features", max_feat, "accepted", accepted)
    assert len({tuple(r[0]) for r in rows}) == 1, "all poses share pos_in_localmap (one map block)"
    assert len(set(accepted[:-3])) >= 2, "accepted counts differ between the hypotheses"
    # the repeat
    assert accepted[mbd.REPEAT] == accepted[0] and np.array_equal(rows[mbd.REPEAT][2], rows[0][2])
    if rows[0][3] is not None:
        assert bytes(rows[mbd.REPEAT][3]) == bytes(rows[0][3])
    # the lost pose: nothing accepted, every judged point too far from the map
    lost = rows[mbd.LOST][2]
    judged = lost[lost < 7]
    assert accepted[mbd.LOST] == 0 and len(judged) and (judged == 2).all()
    if max_feat < 0:
        assert len(judged) == n, "at full sampling every point is judged"
    else:
        assert 0 < len(judged) <= max_feat + 2 < n, "sub-sampled: the others are not judged"
    assert 0 < accepted[mbd.SHIFTED] < min(accepted[:-3])
    if case == "tiny5" and max_feat < 0:
        assert n == 4096 and accepted[:5] == mbd.TINY5_ACCEPTED and accepted[mbd.SHIFTED] == mbd.TINY_SHIFTED_ACCEPTED
    if case == "small9" and max_feat < 0:
        assert n == 16384
