"""-m gpu: so_icp_keep_sequence_correspondences / so_icp_sequence_correspondences / so_icp_sequence_correspondence_sums -- the
correspondence sets of ALL frames of a run (so_icp_register_sequence, so_icp_localization_sequence), exported and summed for a whole
selection of frames in one launch.  The yardstick throughout is a TWIN context with the same map: so_icp_keep_correspondences on,
so_icp_register from guesses_out[k] (with the frame's prior P_k where the run had priors), then so_icp_correspondences /
so_icp_correspondence_sums -- the registration a frame of a run equals bit for bit.  Every comparison is of bytes.  Inputs:
tests/sequence_correspondences_data.py, which the CPU suite shows to do what the tests here need."""
import ctypes as C
import os

import numpy as np
import pytest

import sequence_correspondences_data as scd
import sequence_priors_data as spd
from helpers import CARRIED_OVER_FIELDS, assert_same_bits, scene_with_oracle
from superodom_amd import synth

pytestmark = pytest.mark.gpu
U64P = C.POINTER(C.c_uint64)


def _make(make, run, seq_keep=False, keep=False, with_map=True):
    sc = synth.Scene(scd.RUN_SCENE[run])
    slam = make(plane_res=sc.plane_res, line_res=sc.plane_res / 2, max_surface_features=scd.RUN_MAX_FEAT[run], max_iterations=scd.MAX_OUTER)
    if with_map:
        slam.add_surf_point_cloud(sc.map_points)
    if seq_keep:
        assert slam.keep_sequence_correspondences(True) == 0
    if keep:
        assert slam.keep_correspondences(True) == 0
    return slam


def _twin_frame(twin, scan, guess, P=None, poses=()):
    """the yardstick for one frame: the twin registers it alone; -> rc, [(records bytes, status bytes, info bytes) at the default pose and
    at each of `poses`], the default export's info"""
    if P is not None:
        twin.set_pose_prior(P)
    rc = twin.register(scan, guess)[0]
    out, first_info = [], None
    for pose in (None, *poses):
        rec, status, _, info = twin.correspondences(pose=pose, cap=len(scan))
        out.append((rec.tobytes(), status.tobytes(), bytes(info)))
        first_info = first_info or info
    return rc, out, first_info


def _entry(exp, k):
    rec, first, status, first_status, infos = exp
    return rec[int(first[k]):int(first[k + 1])].tobytes(), status[int(first_status[k]):int(first_status[k + 1])].tobytes(), bytes(infos[k])


def _check_against_twin(slam, twin, scans, res, priors=None, modes=None, tag=""):
    """every frame of the run `res` left on `slam`, at its own pose and at a pose of the caller's, against the twin"""
    rc, poses, guesses, stats, n_done = res
    n = len(scans)
    assert rc == 0 and n_done == n, (tag, rc, n_done, slam.last_error())
    at = np.stack([synth.perturb_pose(poses[k], 300 + k, 0.03, 0.3) for k in range(n)])
    exp, exp_at = slam.sequence_correspondences(n_sel=n), slam.sequence_correspondences(n_sel=n, poses=at)
    assert np.array_equal(exp[1], exp_at[1]) and np.array_equal(exp[3], exp_at[3]) and int(exp[1][0]) == 0 == int(exp[3][0])
    assert [int(v) for v in np.diff(exp[3])] == [len(s) for s in scans]
    outer, rows = [], set()
    for k in range(n):
        P = spd.frame_prior(priors, modes, k, guesses[k]) if priors is not None else None
        trc, (t_def, t_at), info = _twin_frame(twin, scans[k], guesses[k], P, poses=(at[k],))
        assert trc == 0 and info.valid == 1, (tag, k)
        last = stats[k].iterations[stats[k].n_iterations - 1]
        assert int(exp[1][k + 1] - exp[1][k]) == info.n_accepted == exp[4][k].n_accepted, (tag, k)
        if len(scans[k]):
            assert info.n_accepted == last.num_surf_from_scan
        assert _entry(exp, k) == t_def, (tag, k, "default pose")
        assert _entry(exp_at, k) == t_at, (tag, k, "given pose")
        assert exp[4][k].n_points == len(scans[k]) and exp[4][k].outer_iteration == stats[k].n_iterations - 1
        assert bytes(exp[4][k].pose_eval) == bytes(last.pose_after) and bytes(exp_at[4][k].pose_eval) == at[k].tobytes()
        outer.append(exp[4][k].outer_iteration)
        rows.add(_entry(exp, k)[1])
    return exp, outer, rows


def _run(slam, run, resident=False, pinned=True):
    sc, scans, pose0, deltas, priors, modes = scd.run_inputs(run)
    if priors is not None:
        slam.set_sequence_priors(priors, modes)
    if resident:
        return scans, priors, modes, slam.register_sequence([slam.upload_scan(s) for s in scans], pose0, deltas, on_device=True)
    return scans, priors, modes, slam.register_sequence([slam.host_alloc_like(s) if len(s) else s for s in scans] if pinned else scans, pose0, deltas)


# ---- 1. every frame against its twin -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("resident", [False, True])
@pytest.mark.parametrize("run", scd.PLAIN_RUNS)
def test_every_frame_equals_its_twin(soicp, gpu_slam_factory, run, resident):
    slam, twin = _make(gpu_slam_factory, run, seq_keep=True), _make(gpu_slam_factory, run, keep=True)
    scans, priors, modes, res = _run(slam, run, resident)
    exp, outer, rows = _check_against_twin(slam, twin, scans, res, tag=(run, resident))
    timing = slam.timing()
    flags = [st.flags for st in res[3]]
    print(run, resident, "outer iterations", outer, "chained", timing.seq_chained, "breaks", timing.seq_chain_breaks, "flags", [hex(f) for f in flags])
    assert len(set(outer)) >= 2 and len(rows) == len(scans), "the frames should differ (tests/test_sequence_correspondences_host.py)"
    qw = run != "small_chunked"
    assert all(bool(f & soicp.FLAG_QUERY_WAVES) == qw for f in flags)
    assert timing.seq_chained >= 2 and sum(bool(f & soicp.FLAG_CHAINED) for f in flags) >= 2
    if run == "small_chunked":
        assert all(f & soicp.FLAG_BINNED_AHEAD for f in flags)
    if run == "small_sampled":
        assert any((exp[2][int(exp[3][k]):int(exp[3][k + 1])] == 254).any() for k in range(len(scans))), "a sampled scan has points that were not sampled"
    slam.close(); twin.close()


# ---- 2. sizes inside one run ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sizes_run(gpu_slam_factory):
    """the run `sizes` left on a context with the switch on, and a twin; one registration after the other (the data module says why)"""
    assert "SOICP_SEQ_CHAIN" not in os.environ
    os.environ["SOICP_SEQ_CHAIN"] = "0"  # (read when the context is made)
    try:
        slam = _make(gpu_slam_factory, "sizes", seq_keep=True)
    finally:
        del os.environ["SOICP_SEQ_CHAIN"]
    twin = _make(gpu_slam_factory, "sizes", keep=True)
    scans, _, _, res = _run(slam, "sizes")
    yield slam, twin, scans, res
    slam.close(); twin.close()


def test_frames_of_every_size_in_one_run(soicp, sizes_run):
    slam, twin, scans, res = sizes_run
    assert [len(s) for s in scans] == scd.SIZES
    exp, outer, rows = _check_against_twin(slam, twin, scans, res, tag="sizes")
    infos = exp[4]
    assert [i.n_points for i in infos] == scd.SIZES and all(i.valid == 1 for i in infos)
    empty = scd.SIZES.index(0)
    assert 0 < empty < len(scans) - 1 and infos[empty].n_accepted == 0 and infos[empty].cost == 0.0 and exp[1][empty] == exp[1][empty + 1]
    assert not any(st.flags & soicp.FLAG_CHAINED for st in res[3]), "every frame, the empty one included, takes the ordinary entry"
    assert sum(i.n_accepted > 0 for i in infos) >= 8
    print("sizes: accepted", [i.n_accepted for i in infos], "chained", [bool(st.flags & soicp.FLAG_CHAINED) for st in res[3]])


def test_unequal_frames_on_the_chained_path(soicp, gpu_slam_factory):
    slam, twin = _make(gpu_slam_factory, "sizes_chained", seq_keep=True), _make(gpu_slam_factory, "sizes_chained", keep=True)
    scans, _, _, res = _run(slam, "sizes_chained")
    assert [len(s) for s in scans] == scd.SIZES_CHAINED
    exp, outer, rows = _check_against_twin(slam, twin, scans, res, tag="sizes_chained")
    timing = slam.timing()
    print("sizes_chained: outer iterations", outer, "accepted", [i.n_accepted for i in exp[4]], "chained", timing.seq_chained, "breaks", timing.seq_chain_breaks)
    assert timing.seq_chained >= 1 and len(rows) == len(scans) and all(i.n_accepted > 0 for i in exp[4])
    slam.close(); twin.close()


# ---- 3. selections ------------------------------------------------------------------------------------------------------------------------
def test_selection_order_repeats_and_the_device_copy(soicp, sizes_run):
    slam, twin, scans, res = sizes_run
    n = len(scans)
    exp = slam.sequence_correspondences(n_sel=n)
    whole = [_entry(exp, k) for k in range(n)]
    exp2 = slam.sequence_correspondences(n_sel=n)
    assert [_entry(exp2, k) for k in range(n)] == whole, "two calls give identical bytes"
    for frames in ([3, 1], list(range(n))[::-1], [2], [0, 5, 5, 0], [2, 2], [1, 2, 0, 2, 3], [11]):
        e = slam.sequence_correspondences(frames=frames)
        assert [_entry(e, k) for k in range(len(frames))] == [whole[f] for f in frames], frames
        assert int(e[1][-1]) == len(e[0]) == sum(len(whole[f][0]) // 72 for f in frames)
        assert int(e[3][-1]) == len(e[2]) == sum(scd.SIZES[f] for f in frames)
    e = slam.sequence_correspondences(n_sel=4)  # frames = NULL: a prefix
    assert [_entry(e, k) for k in range(4)] == whole[:4]
    e = slam.sequence_correspondences(n_sel=0)
    assert len(e[0]) == 0 and len(e[2]) == 0 and list(e[1]) == [0] and e[4] == []
    # a repeated index with two different poses: each entry at its own pose, as the twin evaluates them
    at = np.stack([synth.perturb_pose(res[1][0], 41, 0.03, 0.3), synth.perturb_pose(res[1][0], 42, 0.03, 0.3)])
    e = slam.sequence_correspondences(frames=[0, 0], poses=at)
    _, t, _ = _twin_frame(twin, scans[0], res[2][0], poses=(at[0], at[1]))
    assert [_entry(e, 0), _entry(e, 1)] == t[1:] and t[1][0] != t[2][0]
    # the device copy of the records
    frames = [3, 0, 2, 10]
    d, first, infos = slam.sequence_correspondences_dev(frames=frames)
    total = int(first[-1])
    assert d and total == sum(len(whole[f][0]) // 72 for f in frames)
    assert slam.download_bytes(d, total * 72).tobytes() == b"".join(whole[f][0] for f in frames)


# ---- 4. every path of a run ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env, run", [("SOICP_SEQ_CHAIN", "tiny"), ("SOICP_SEQ_CHAIN", "small_chunked"), ("SOICP_QUERY_WAVES", "tiny"),
                                      ("SOICP_PREBIN", "small_chunked")])
def test_the_other_paths(soicp, gpu_slam_factory, monkeypatch, env, run):
    monkeypatch.setenv(env, "0")  # (read when the context is made)
    slam = _make(gpu_slam_factory, run, seq_keep=True)
    monkeypatch.delenv(env)
    twin = _make(gpu_slam_factory, run, keep=True)
    scans, priors, modes, res = _run(slam, run)
    _check_against_twin(slam, twin, scans, res, tag=(env, run))
    flags = [st.flags for st in res[3]]
    if env == "SOICP_SEQ_CHAIN":
        assert not any(f & soicp.FLAG_CHAINED for f in flags) and slam.timing().seq_chained == 0
    if env == "SOICP_QUERY_WAVES":
        assert not any(f & soicp.FLAG_QUERY_WAVES for f in flags)
    if env == "SOICP_PREBIN":
        assert not any(f & soicp.FLAG_BINNED_AHEAD for f in flags)
    slam.close(); twin.close()


def test_a_broken_chain_with_priors_at_the_guess(soicp, gpu_slam_factory):
    slam, twin = _make(gpu_slam_factory, "broken", seq_keep=True), _make(gpu_slam_factory, "broken", keep=True)
    scans, priors, modes, res = _run(slam, "broken")
    assert modes == [spd.AT_GUESS] * len(scans)
    _check_against_twin(slam, twin, scans, res, priors, modes, tag="broken")
    timing = slam.timing()
    print("broken: outer iterations", [st.n_iterations for st in res[3]], "chained", timing.seq_chained, "breaks", timing.seq_chain_breaks)
    assert timing.seq_chain_breaks >= 1 and timing.seq_chained >= 1
    assert all(st.flags & soicp.FLAG_POSE_PRIOR for st in res[3])
    slam.close(); twin.close()


def test_a_second_run_replaces_the_set(soicp, gpu_slam_factory):
    slam, twin = _make(gpu_slam_factory, "tiny", seq_keep=True), _make(gpu_slam_factory, "tiny", keep=True)
    scans, _, _, res = _run(slam, "tiny")
    first_run = slam.sequence_correspondences(n_sel=len(scans))
    sc, scans, pose0, deltas, _, _ = scd.run_inputs("tiny")
    # frames 2 .. 4 as a run of their own, from unpinned host scans
    sub = scans[2:5]
    sub_deltas = deltas[2:5]
    res2 = slam.register_sequence(sub, sc.guess(scd.RUNS["tiny"]["ids"][2]), sub_deltas)
    exp, _, _ = _check_against_twin(slam, twin, sub, res2, tag="second run")
    assert _entry(exp, 0) != _entry(first_run, 0)
    with pytest.raises(soicp.SoIcpError, match="so_icp error -1: so_icp_sequence_correspondences: a frame index lies outside the last run"):
        slam.sequence_correspondences(frames=[3])
    slam.close(); twin.close()


# ---- 5. so_icp_localization_sequence --------------------------------------------------------------------------------------------------------
def _localization_context(factory, sc):
    slam = scene_with_oracle(sc, None, factory, oracle_too=False, max_iterations=scd.MAX_OUTER)[1]
    slam.shift_map(sc.gt_pose(0)[:3])
    return slam


@pytest.mark.parametrize("resident", [False, True])
def test_localization_sequence_against_the_per_frame_loop(soicp, gpu_slam_factory, resident):
    sc, scans, pose0, deltas, _, _ = scd.run_inputs("tiny")
    n = len(scans)
    times = 0.1 * np.arange(1, n + 1)
    seq = _localization_context(gpu_slam_factory, sc)
    assert seq.keep_sequence_correspondences(True) == 0
    given = [seq.upload_scan(s) for s in scans] if resident else scans
    rc, poses, guesses, stats, n_done = seq.localization_sequence(given, pose0, deltas, times, on_device=resident)
    assert rc == 0 and n_done == n, (rc, n_done, seq.last_error())
    at = np.stack([synth.perturb_pose(poses[k], 500 + k, 0.03, 0.3) for k in range(n)])
    exp, exp_at = seq.sequence_correspondences(n_sel=n), seq.sequence_correspondences(n_sel=n, poses=at)
    loop = _localization_context(gpu_slam_factory, sc)  # its map grows with every frame, as the run's did
    assert loop.keep_correspondences(True) == 0
    rows = set()
    for k in range(n):
        lrc, lpose, lst = loop.localization(True, guesses[k], scans[k], times[k])
        assert lrc == 0 and lpose.tobytes() == poses[k].tobytes()
        for e, pose in ((exp, None), (exp_at, at[k])):
            rec, status, _, info = loop.correspondences(pose=pose, cap=len(scans[k]))
            assert info.valid == 1 and _entry(e, k) == (rec.tobytes(), status.tobytes(), bytes(info)), (k, pose is None)
        rows.add(_entry(exp, k)[1])
    assert len(rows) == n
    assert seq.export_map_records(stride=12).tobytes() == loop.export_map_records(stride=12).tobytes() and seq.map_size() == loop.map_size() > 0
    seq.close(); loop.close()


# ---- 6. the sums ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_poses", scd.SUMS_POSES)
def test_sums_equal_the_twins(soicp, sizes_run, n_poses):
    slam, twin, scans, res = sizes_run
    frames = scd.SUMS_FRAMES
    assert [len(scans[f]) for f in frames] == [1, 255, scd.TILE, scd.TILE + 1, 2049]
    poses = np.stack([scd.poses_near(res[1][f], n_poses, 700 + 64 * f) for f in frames])
    sums = slam.sequence_correspondence_sums(poses, frames)
    counts = []
    for k, f in enumerate(frames):
        assert twin.register(scans[f], res[2][f])[0] == 0
        want = twin.correspondence_sums(poses[k])
        for j in range(n_poses):
            assert bytes(sums[k * n_poses + j]) == bytes(want[j]), (f, j)
        counts.append(want[0].count)
    print("sums: frames", frames, "accepted", counts)
    assert sum(c > 0 for c in counts) >= 4
    if n_poses == 64:  # a pose's sums do not depend on the other poses of the call
        for j in (0, 17, 63):
            one = slam.sequence_correspondence_sums(poses[:, j:j + 1], frames)
            assert [bytes(one[k]) for k in range(len(frames))] == [bytes(sums[k * n_poses + j]) for k in range(len(frames))]
    # frames = NULL, an empty frame in the selection: its sums are zero, its histograms its own
    m = scd.SIZES.index(0) + 2
    allp = np.stack([scd.poses_near(res[1][f], n_poses, 900 + f) for f in range(m)])
    s_all = slam.sequence_correspondence_sums(allp)
    for f in range(m):
        assert twin.register(scans[f], res[2][f])[0] == 0
        want = twin.correspondence_sums(allp[f])
        assert [bytes(s_all[f * n_poses + j]) for j in range(n_poses)] == [bytes(want[j]) for j in range(n_poses)], f
    assert s_all[scd.SIZES.index(0) * n_poses].count == 0.0


# ---- 7. what stays untouched ---------------------------------------------------------------------------------------------------------------
COUNTERS = ("knn_launches", "knn_queries", "eval_launches", "registrations", "seq_chained", "seq_chain_breaks", "staged_direct", "staged_copied")


@pytest.mark.parametrize("run", ["small_chunked", "tiny"])
def test_switch_off_and_switch_on_leave_the_run_as_it_was(soicp, gpu_slam_factory, run):
    results = {}
    for mode in ("never", "off", "on"):
        slam = _make(gpu_slam_factory, run, keep=True)
        if mode != "never":
            assert slam.keep_sequence_correspondences(True) == 0
        if mode == "off":
            assert slam.keep_sequence_correspondences(False) == 0
        scans, _, _, res = _run(slam, run)
        rec, status, resid, info = slam.correspondences(cap=len(scans[-1]))
        t = slam.timing()
        results[mode] = (res, (rec.tobytes(), status.tobytes(), resid.tobytes(), bytes(info)), {c: getattr(t, c) for c in COUNTERS})
        if mode == "off":
            e = slam.sequence_correspondences(n_sel=len(scans))
            assert all(bytes(i) == bytes(C.sizeof(i)) for i in e[4]) and not e[1].any() and len(e[0]) == 0
            poses = np.tile(np.array([0, 0, 0, 0, 0, 0, 1.0]), (len(scans), 1, 1))
            assert bytes(slam.sequence_correspondence_sums(poses)) == bytes(C.sizeof(soicp.Sums) * len(scans))
        slam.close()
    never = results["never"]
    assert never[0][0] == 0 and never[2]["seq_chained"] >= 2
    for mode in ("off", "on"):
        res, single, counters = results[mode]
        assert res[0] == 0 and res[1].tobytes() == never[0][1].tobytes() and res[2].tobytes() == never[0][2].tobytes(), mode
        for k, (a, b) in enumerate(zip(res[3], never[0][3])):
            assert_same_bits(a, b, (run, mode, k))
            assert a.flags == b.flags
        assert single == never[1], (mode, "the single set of the last frame")
        assert counters == never[2], (mode, counters, never[2])


def test_the_set_survives_other_entries_and_both_switches_hold(soicp, gpu_slam_factory):
    slam, twin = _make(gpu_slam_factory, "tiny", seq_keep=True, keep=True), _make(gpu_slam_factory, "tiny", keep=True)
    scans, _, _, res = _run(slam, "tiny")
    n = len(scans)
    # both switches on: every frame's set, and the last registration's
    exp, _, _ = _check_against_twin(slam, twin, scans, res, tag="both switches")  # (the twin ends on the last frame)
    rec, status, _, info = slam.correspondences(cap=len(scans[-1]))
    t_rec, t_status, _, t_info = twin.correspondences(cap=len(scans[-1]))
    assert (rec.tobytes(), status.tobytes(), bytes(info)) == (t_rec.tobytes(), t_status.tobytes(), bytes(t_info)) == _entry(exp, n - 1)
    whole = [_entry(exp, k) for k in range(n)]
    sc = synth.Scene("tiny")
    # a single registration, a match, a batch, a map insert: the set stays
    assert slam.register(scans[1], res[2][1])[0] == 0
    assert slam.match(scans[2], res[2][2])[0] == 0
    assert slam.register_batch(scans[3], np.stack([res[2][3], res[2][2]]))[0] == 2
    slam.add_surf_point_cloud(sc.map_points[:1000] + np.float32(0.01))
    e = slam.sequence_correspondences(n_sel=n)
    assert [_entry(e, k) for k in range(n)] == whole
    # the switch off drops it; on again: nothing until the next run
    assert slam.keep_sequence_correspondences(False) == 0 and slam.keep_sequence_correspondences(True) == 0
    e = slam.sequence_correspondences(n_sel=n)
    assert all(i.valid == 0 and i.n_points == 0 for i in e[4]) and len(e[0]) == 0
    slam.close(); twin.close()


# ---- 8. nothing to export ------------------------------------------------------------------------------------------------------------------
def test_a_run_that_stops_and_argument_errors(soicp, gpu_slam_factory):
    sc, scans, pose0, deltas, _, _ = scd.run_inputs("tiny")
    n, stop = len(scans), 3
    deltas = deltas.copy()
    deltas[stop, 0] += 400.0  # the prediction of frame `stop` lands where the map has nothing: SO_ICP_NOT_ENOUGH_MAP_FEATURES
    slam, twin = _make(gpu_slam_factory, "tiny", seq_keep=True), _make(gpu_slam_factory, "tiny", keep=True)
    rc, poses, guesses, stats, n_done = slam.register_sequence(scans, pose0, deltas)
    assert rc == 1 and n_done == stop, (rc, n_done)
    e = slam.sequence_correspondences(n_sel=n)
    assert [i.valid for i in e[4]] == [1] * stop + [0] * (n - stop)
    assert [i.n_points for i in e[4]] == [len(s) for s in scans]
    for k in range(stop):
        trc, (t_def,), info = _twin_frame(twin, scans[k], guesses[k])
        assert trc == 0 and _entry(e, k) == t_def, k
    for k in range(stop, n):
        rec, status, info = _entry(e, k)
        assert rec == b"" and status == b"\xfe" * len(scans[k]) and e[4][k].n_accepted == 0 and e[4][k].cost == 0.0
    poses1 = np.tile(np.array([0, 0, 0, 0, 0, 0, 1.0]), (n, 1, 1))
    poses1[:stop, 0] = poses[:stop]
    sums = slam.sequence_correspondence_sums(poses1)
    assert all(sums[k].count > 0 for k in range(stop)) and all(bytes(sums[k]) == bytes(C.sizeof(soicp.Sums)) for k in range(stop, n))
    # argument errors, by code and whole text
    L, err = slam.L, lambda: slam.L.so_icp_last_error(slam.h).decode()
    i32 = lambda v: (C.c_int32 * len(v))(*v)
    for bad in ([0, n], [-1], [1, 2, 1 << 20]):
        assert L.so_icp_sequence_correspondences(slam.h, i32(bad), len(bad), None, None, 0, None, None, 0, None, None, None) == -1
        assert err() == "so_icp_sequence_correspondences: a frame index lies outside the last run (0 .. count - 1)"
        p = np.tile(np.array([0, 0, 0, 0, 0, 0, 1.0]), (len(bad), 1, 1))
        out = (soicp.Sums * len(bad))()
        assert L.so_icp_sequence_correspondence_sums(slam.h, i32(bad), len(bad), p.ctypes.data_as(C.POINTER(C.c_double)), 1, out) == -1
        assert err() == "so_icp_sequence_correspondence_sums: a frame index lies outside the last run (0 .. count - 1)"
    assert L.so_icp_sequence_correspondences(slam.h, None, n + 1, None, None, 0, None, None, 0, None, None, None) == -1
    assert err() == "so_icp_sequence_correspondences: a frame index lies outside the last run (0 .. count - 1)"
    status = np.zeros(sum(len(s) for s in scans), np.uint8)
    first_status = np.full(n + 1, 5, np.uint64)
    rc = L.so_icp_sequence_correspondences(slam.h, None, n, None, None, 0, None, status.ctypes.data_as(C.POINTER(C.c_uint8)), len(status) - 1,
                                           first_status.ctypes.data_as(U64P), None, None)
    assert rc == -1 and err() == "so_icp_sequence_correspondences: status_out needs cap_status >= the points of all selected frames"
    assert not status.any() and not first_status.any()
    for bad in (-1, soicp.SEQUENCE_MAX_SELECTION + 1):
        assert L.so_icp_sequence_correspondences(slam.h, None, bad, None, None, 0, None, None, 0, None, None, None) == -1
        assert err() == "so_icp_sequence_correspondences: n_sel must be 0 .. SO_ICP_SEQUENCE_MAX_SELECTION"
    slam.close(); twin.close()
    # an empty map: the run stops at frame 0 and leaves no frame's set
    empty = _make(gpu_slam_factory, "tiny", seq_keep=True, with_map=False)
    assert empty.register_sequence(scans, pose0, scd.run_inputs("tiny")[3])[0] == 1
    e = empty.sequence_correspondences(n_sel=n)
    assert all(i.valid == 0 and i.n_accepted == 0 for i in e[4]) and len(e[0]) == 0 and (e[2] == 254).all() and len(e[2]) == sum(len(s) for s in scans)
    empty.close()
    # a sharded context
    sharded = gpu_slam_factory(plane_res=sc.plane_res, world_size=2, rank=0)
    assert sharded.keep_sequence_correspondences(True) == -5
    assert sharded.last_error() == "so_icp_keep_sequence_correspondences: a sharded context (world_size > 1) keeps its correspondences per rank"
    sharded.close()
