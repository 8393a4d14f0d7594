"""-m gpu: so_icp_match_batch -- one scan matched at many poses in one call, nothing solved.  The yardstick throughout is a TWIN context
that runs so_icp_match_dev at one pose alone (so_icp_keep_correspondences on), then so_icp_correspondences /
so_icp_correspondence_sums: what hypothesis h of the batch reports, and what the batch's kept set exports for it, are the twin's bytes.
Inputs: tests/match_batch_data.py, which the CPU suite (tests/test_match_batch_host.py) shows to be what they are named."""
import ctypes as C

import numpy as np
import pytest

import batch_correspondences_data as bcd
import batch_priors_data as bpd
import match_batch_data as mbd
import seam_c_ref
from helpers import assert_follows_oracle, assert_same_bits, chain_deltas, scene_with_oracle, stats_bits
from superodom_amd import binding, synth

pytestmark = pytest.mark.gpu
MAX_OUTER, LM_MAX = bcd.MAX_OUTER, bcd.LM_MAX


def _make(make, scene, sub=None, batch_keep=False, keep=False, **cfg):
    cfg.setdefault("max_iterations", MAX_OUTER)
    _, slam, _ = scene_with_oracle(scene, None, make, oracle_too=False, **cfg)
    if sub:
        slam.set_max_surface_features(sub)
    if batch_keep:
        assert slam.keep_batch_correspondences(True) == 0
    if keep:
        assert slam.keep_correspondences(True) == 0
    return slam


def _twin_match(twin, scan, pose, d=None):
    """so_icp_match_dev at `pose` on the twin (so_icp_match for an empty scan: nothing to upload) -> (rc, Stats)"""
    if len(scan) == 0:
        return twin.match(scan, pose)
    return twin.match_dev(d, len(scan), pose)


def _export_bytes(rec, status, info):
    return rec.tobytes(), status.tobytes(), bytes(info)


def _entry(rec, first, status, infos, k):
    return rec[int(first[k]):int(first[k + 1])].tobytes(), status[k].tobytes(), bytes(infos[k])


def _check_match_stats(st, pose, tag):
    """what so_icp_match documents of its report"""
    it = st.iterations[0]
    assert st.n_iterations == 1 and it.lm_iterations == 0 and it.num_successful_steps == 0, tag
    assert np.float64(it.initial_cost).tobytes() == np.float64(it.final_cost).tobytes(), tag
    assert bytes(it.pose_after) == np.asarray(pose, np.float64).tobytes(), tag


def _all_bits(sts):
    return [stats_bits(s) for s in sts]


@pytest.fixture(scope="module")
def tiny(gpu_slam_factory):
    """(scene, a context with the batch switch on, its twin) on scene tiny, shared by the tests that only need them in that state"""
    slam, twin = _make(gpu_slam_factory, "tiny", batch_keep=True), _make(gpu_slam_factory, "tiny", keep=True)
    yield synth.Scene("tiny"), slam, twin
    slam.close(); twin.close()


# ---- 1. every hypothesis against the twin ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(mbd.CASES))
def test_every_hypothesis_equals_its_twin(gpu_slam_factory, case):
    sc, scan, poses, sub = mbd.inputs(case)
    B, n = len(poses), len(scan)
    scene = mbd.CASES[case][0]
    slam = _make(gpu_slam_factory, scene, sub, batch_keep=True)
    off = _make(gpu_slam_factory, scene, sub)
    twin = _make(gpu_slam_factory, scene, sub, keep=True)
    d, dn = slam.upload_scan(scan)
    ok, rcs, sts = slam.match_batch(None, poses, d_scan=d, n=dn)
    assert ok == B and (rcs == 0).all()
    ok_off, rcs_off, sts_off = off.match_batch(scan, poses)
    assert ok_off == B and _all_bits(sts_off) == _all_bits(sts), "the switch off: the same bytes"
    assert all(i.valid == 0 for i in off.batch_correspondences(n_sel=B, cap_points=n, cap_records=0)[3])
    at = np.stack([synth.perturb_pose(poses[h], 300 + h, 0.03, 0.3) for h in range(B)])     # a pose of the caller's per entry
    at2 = np.stack([poses, at], axis=1)                                                       # [B, 2, 7]
    rec, first, status, infos = slam.batch_correspondences(n_sel=B, cap_points=n, cap_records=B * n)
    rec_at, first_at, status_at, infos_at = slam.batch_correspondences(n_sel=B, poses=at, cap_points=n, cap_records=B * n)
    sums1, sums2 = slam.batch_correspondence_sums(at2[:, :1]), slam.batch_correspondence_sums(at2)
    assert np.array_equal(first, first_at) and int(first[0]) == 0
    dt, _ = twin.upload_scan(scan)
    accepted = []
    for h in range(B):
        rc, st = _twin_match(twin, scan, poses[h], dt)
        assert rc == int(rcs[h]) == 0, (case, h)
        _check_match_stats(sts[h], poses[h], (case, h))
        assert_same_bits(sts[h], st, f"{case} hypothesis {h}")
        t_rec, t_status, _, t_info = twin.correspondences(cap=n)
        assert t_info.valid == 1 and t_info.outer_iteration == 0 and bytes(t_info.pose_fit) == bytes(t_info.pose_eval) == poses[h].tobytes()
        assert int(first[h + 1] - first[h]) == t_info.n_accepted == sts[h].iterations[0].num_surf_from_scan, (case, h)
        assert _entry(rec, first, status, infos, h) == _export_bytes(t_rec, t_status, t_info), (case, h, "default pose")
        t_rec2, t_status2, _, t_info2 = twin.correspondences(pose=at[h], cap=n)
        assert _entry(rec_at, first_at, status_at, infos_at, h) == _export_bytes(t_rec2, t_status2, t_info2), (case, h, "given pose")
        t_sums = twin.correspondence_sums(at2[h])
        assert bytes(sums1[h]) == bytes(t_sums[0]) and bytes(sums2[2 * h]) == bytes(t_sums[0]) and bytes(sums2[2 * h + 1]) == bytes(t_sums[1]), (case, h)
        accepted.append(int(t_info.n_accepted))
    print(case, "accepted", accepted)
    assert len(set(accepted)) >= 2, "the hypotheses should differ (tests/test_match_batch_host.py)"
    if case in mbd.WITH_EXTRAS:
        assert accepted[mbd.LOST] == 0 and accepted[mbd.REPEAT] == accepted[0] and 0 < accepted[mbd.SHIFTED] < min(accepted[:-3])
        assert stats_bits(sts[B + mbd.REPEAT]) == stats_bits(sts[0]) and (status[B + mbd.REPEAT] == status[0]).all()
        lost = status[B + mbd.LOST]
        assert (lost[lost != 254] == 2).all() and sts[B + mbd.LOST].iterations[0].termination == 4, "nothing accepted: so_icp_lm_begin's termination 4"
    if case == "tiny5":
        assert accepted[:5] == mbd.TINY5_ACCEPTED and accepted[mbd.SHIFTED] == mbd.TINY_SHIFTED_ACCEPTED
    if sub:
        assert (status == 254).any(), "a sub-sampled scan has points that were not sampled"
    for c in (slam, off, twin):
        c.close()


# ---- 2. sizes -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", mbd.SIZES)
def test_every_size(tiny, n):
    sc, slam, twin = tiny
    scan = np.ascontiguousarray(sc.scan(mbd.SCAN_ID)[:n], np.float32)
    poses = mbd.three_poses(sc)
    ok, rcs, sts = slam.match_batch(scan, poses)
    assert ok == 3 and (rcs == 0).all()
    rec, first, status, infos = slam.batch_correspondences(n_sel=3, cap_points=n, cap_records=3 * n)
    assert status.shape == (3, n)
    dt = twin.upload_scan(scan)[0] if n else None
    for h in range(3):
        rc, st = _twin_match(twin, scan, poses[h], dt)
        assert rc == 0
        _check_match_stats(sts[h], poses[h], (n, h))
        assert_same_bits(sts[h], st, f"n = {n}, pose {h}")
        t_rec, t_status, _, t_info = twin.correspondences(cap=n)
        assert t_info.valid == 1 and infos[h].n_points == n
        assert _entry(rec, first, status, infos, h) == _export_bytes(t_rec, t_status, t_info), (n, h)
        assert bytes(slam.batch_correspondence_sums(poses[h][None, None, :], hyp=[h])[0]) == bytes(twin.correspondence_sums(poses[h])[0]), (n, h)
    if n:
        twin.free_scan(dt)
    assert int(first[3] - first[2]) == 0 and sts[2].iterations[0].termination == 4, "the lost pose"
    if n == 0:
        assert not first.any() and all(i.valid == 1 and i.n_accepted == 0 and i.cost == 0.0 for i in infos)
        assert all(s.iterations[0].termination == 4 and not any(s.iterations[0].reject_hist) for s in sts)


# ---- 3. independence and cleanliness --------------------------------------------------------------------------------------------------
def test_order_group_sizes_and_a_repeated_call(tiny):
    sc, slam, twin = tiny
    sc, scan, poses, _ = mbd.inputs("tiny70")
    ok, rcs, sts = slam.match_batch(scan, poses)
    assert ok == 70
    bits = _all_bits(sts)
    export = lambda B: (lambda r, f, s, i: (r.tobytes(), f.tobytes(), s.tobytes(), [bytes(x) for x in i]))(*slam.batch_correspondences(n_sel=B, cap_points=len(scan), cap_records=B * len(scan)))
    whole = export(70)
    # the call repeated
    ok, rcs, sts2 = slam.match_batch(scan, poses)
    assert ok == 70 and _all_bits(sts2) == bits and export(70) == whole, "a second call"
    # the same poses in reversed order
    ok, rcs, sts_r = slam.match_batch(scan, poses[::-1])
    assert ok == 70 and _all_bits(sts_r) == bits[::-1], "reversed order"
    rec, first, status, infos = slam.batch_correspondences(n_sel=70, cap_points=len(scan), cap_records=70 * len(scan))
    fwd_first = np.frombuffer(whole[1], np.uint64)
    fwd_rec = np.frombuffer(whole[0], rec.dtype)
    for k in (0, 5, 6, 63, 64, 69):
        h = 69 - k
        assert rec[int(first[k]):int(first[k + 1])].tobytes() == fwd_rec[int(fwd_first[h]):int(fwd_first[h + 1])].tobytes() and bytes(infos[k]) == whole[3][h], k
    # n_poses 1, 64 and 65: one group, a full group, a full group and one more
    for B in (1, 64, 65):
        ok, rcs, sts_b = slam.match_batch(scan, poses[:B])
        assert ok == B and _all_bits(sts_b) == bits[:B], B
        assert [bytes(i) for i in slam.batch_correspondences(n_sel=B, cap_points=len(scan), cap_records=0)[3]] == whole[3][:B], B


def test_a_registration_batch_between_two_match_batches(gpu_slam_factory):
    sc, scan, poses, _ = mbd.inputs("tiny5")
    B = len(poses)
    slam = _make(gpu_slam_factory, "tiny", batch_keep=True)
    never = _make(gpu_slam_factory, "tiny", batch_keep=True)   # a context that never matched
    ok, rcs, first_sts = slam.match_batch(scan, poses)
    assert ok == B
    first_export = [bytes(i) for i in slam.batch_correspondences(n_sel=B, cap_points=len(scan), cap_records=0)[3]]
    ok_a, rcs_a, out_a, sts_a = slam.register_batch(scan, poses)
    ok_b, rcs_b, out_b, sts_b = never.register_batch(scan, poses)
    assert ok_a == ok_b and np.array_equal(rcs_a, rcs_b) and out_a.tobytes() == out_b.tobytes(), "the batch behind a match batch: poses"
    for h in range(B):
        assert_same_bits(sts_a[h], sts_b[h], f"the batch behind a match batch, hypothesis {h}")
    assert max(s.n_iterations for s in sts_a) > 1, "the batch solved"
    ok, rcs, second_sts = slam.match_batch(scan, poses)
    assert ok == B and _all_bits(second_sts) == _all_bits(first_sts), "the match batch behind a batch"
    assert [bytes(i) for i in slam.batch_correspondences(n_sel=B, cap_points=len(scan), cap_records=0)[3]] == first_export
    # and the later batches chain their rounds as if no match had run (the survivors' statistics are the batch's own)
    ok_a, rcs_a, out_a2, sts_a2 = slam.register_batch(scan, poses)
    ok_b, rcs_b, out_b2, sts_b2 = never.register_batch(scan, poses)
    assert out_a2.tobytes() == out_b2.tobytes() == out_a.tobytes() and _all_bits(sts_a2) == _all_bits(sts_b2)
    slam.close(); never.close()


# ---- 4. front ends and switches -------------------------------------------------------------------------------------------------------
_default = {}


@pytest.fixture(scope="module")
def default_small9(gpu_slam_factory):
    def get():
        if not _default:
            sc, scan, poses, sub = mbd.inputs("small9")
            slam = _make(gpu_slam_factory, "small", sub, batch_keep=True)
            ok, rcs, sts = slam.match_batch(scan, poses)
            assert ok == len(poses)
            rec, first, status, infos = slam.batch_correspondences(n_sel=len(poses), cap_points=len(scan), cap_records=len(poses) * len(scan))
            _default["v"] = (scan, poses, sub, _all_bits(sts), rec.tobytes(), first.copy(), status.tobytes(), [bytes(i) for i in infos])
            slam.close()
        return _default["v"]
    yield get
    _default.clear()


def _same_as_default(slam, ref, sts, tag):
    scan, poses, sub, bits, rec_b, first, status_b, info_b = ref
    B, n = len(poses), len(scan)
    assert _all_bits(sts) == bits, tag
    rec, f, status, infos = slam.batch_correspondences(n_sel=B, cap_points=n, cap_records=B * n)
    assert rec.tobytes() == rec_b and np.array_equal(f, first) and status.tobytes() == status_b and [bytes(i) for i in infos] == info_b, tag


@pytest.mark.parametrize("env", [{}, {"SOICP_KNN_PACK": "0"}, {"SOICP_BATCH_MODE": "lanes"}, {"SOICP_BATCH_MODE": "one_per_cu"}, {"SOICP_ABLATE": "128"}])
def test_front_ends_and_switches(gpu_slam_factory, monkeypatch, default_small9, env):
    ref = default_small9()
    scan, poses, sub = ref[:3]
    B, n = len(poses), len(scan)
    for k, v in env.items():
        monkeypatch.setenv(k, v)  # read by so_icp_create
    slam = _make(gpu_slam_factory, "small", sub, batch_keep=True)
    if env:  # (SOICP_BATCH_MODE does not apply to a match; SOICP_ABLATE=128 launches the instrumented instantiations)
        ok, rcs, sts = slam.match_batch(scan, poses)
        assert ok == B
        _same_as_default(slam, ref, sts, env)
    else:
        # a resident scan
        d, dn = slam.upload_scan(scan)
        ok, rcs, sts = slam.match_batch(None, poses, d_scan=d, n=dn)
        assert ok == B
        _same_as_default(slam, ref, sts, "resident scan")
        # records of 16 bytes
        wide = np.zeros((n, 4), np.float32)
        wide[:, :3] = scan
        wide[:, 3] = 7.0
        st = (binding.Stats * B)()
        rcs = np.zeros(B, np.int32)
        ok = slam.L.so_icp_match_batch(slam.h, wide.ctypes.data_as(C.POINTER(C.c_float)), None, n, 16, poses.ctypes.data_as(C.POINTER(C.c_double)), B, st,
                                       rcs.ctypes.data_as(C.POINTER(C.c_int32)))
        assert ok == B and not rcs.any()
        _same_as_default(slam, ref, list(st), "stride_bytes 16")
        # rc_out is nullable
        assert slam.L.so_icp_match_batch(slam.h, wide.ctypes.data_as(C.POINTER(C.c_float)), None, n, 16, poses.ctypes.data_as(C.POINTER(C.c_double)), B, st, None) == B
    slam.close()


# ---- 5. moves nothing -----------------------------------------------------------------------------------------------------------------
def test_a_match_batch_moves_nothing(gpu_slam_factory):
    sc = synth.Scene("tiny")
    plain, probed = _make(gpu_slam_factory, "tiny", keep=True), _make(gpu_slam_factory, "tiny", keep=True)
    scans = [np.ascontiguousarray(sc.scan(i), np.float32) for i in range(3)]
    poses = mbd.inputs("tiny5")[2]
    res = []
    for slam in (plain, probed):
        a = slam.register(scans[0], sc.guess(0))
        single = (lambda r, s, q, i: (r.tobytes(), s.tobytes(), q.tobytes(), bytes(i)))(*slam.correspondences(cap=len(scans[0])))
        registrations = slam.timing().registrations
        if slam is probed:
            for keep in (False, True):
                assert slam.keep_batch_correspondences(keep) == 0
                ok, rcs, sts = slam.match_batch(scans[2], poses)
                assert ok == len(poses) and all(s.n_iterations == 1 for s in sts)
        assert slam.timing().registrations == registrations
        assert (lambda r, s, q, i: (r.tobytes(), s.tobytes(), q.tobytes(), bytes(i)))(*slam.correspondences(cap=len(scans[0]))) == single, "the single kept set"
        b = slam.register(scans[1], sc.guess(1))
        c = slam.register(scans[2], sc.guess(2))
        res.append((a, b, c, slam.export_map().tobytes(), slam.map_size()))
    for k in range(3):
        assert res[0][k][0] == res[1][k][0] == 0 and np.array_equal(res[0][k][1], res[1][k][1]), f"registration {k}: pose"
        assert_same_bits(res[0][k][2], res[1][k][2], f"registration {k} with match batches in between")  # (uncertainty and startup_count included)
    assert any(res[0][2][2].uncertainty), "the registrations carry an observability histogram over"
    assert res[0][3] == res[1][3] and res[0][4] == res[1][4], "the map"
    plain.close(); probed.close()


def test_a_match_batch_leaves_staged_scans_and_the_sequence_chain(gpu_slam_factory, soicp):
    sc = synth.Scene("small")
    plain, probed = _make(gpu_slam_factory, "small"), _make(gpu_slam_factory, "small")
    ids = [0, 1, 2, 3]
    scans = [np.ascontiguousarray(sc.scan(i), np.float32) for i in ids]
    poses = bpd.guesses(sc, 3)
    out = []
    for slam in (plain, probed):
        first = slam.register_sequence(scans, sc.guess(0), chain_deltas(sc, ids))
        if slam is probed:
            assert slam.match_batch(scans[2], poses)[0] == 3
        second = slam.register_sequence(scans, sc.guess(0), chain_deltas(sc, ids))
        out.append((first, second))
    for run in (0, 1):
        (rc_a, poses_a, _, stats_a, n_a), (rc_b, poses_b, _, stats_b, n_b) = out[0][run], out[1][run]
        assert rc_a == rc_b == 0 and n_a == n_b == len(ids) and np.array_equal(poses_a, poses_b)
        for k in range(len(ids)):
            assert_same_bits(stats_a[k], stats_b[k], f"run {run} registration {k}")
            assert (stats_a[k].flags & soicp.FLAG_CHAINED) == (stats_b[k].flags & soicp.FLAG_CHAINED), (run, k)
    assert any(st.flags & soicp.FLAG_CHAINED for st in out[1][1][3]), "the sequence behind the match batch still runs chained"
    # a scan announced before the match batch is still there for its registration
    staged = probed.host_alloc_like(scans[1])
    probed.stage_scan(staged)
    assert probed.match_batch(staged, poses)[0] == 3
    rc, pose, st = probed.register(staged, sc.guess(1))
    assert rc == 0 and (st.flags & soicp.FLAG_STAGED_SCAN)
    rc, pose_p, st_p = plain.register(scans[1], sc.guess(1))
    assert np.array_equal(pose, pose_p)
    assert_same_bits(st, st_p, "the staged registration behind a match batch")
    plain.close(); probed.close()


# ---- 6. refusals and empty cases on a device context ----------------------------------------------------------------------------------
def test_refusals_and_empty_cases(soicp, gpu_slam_factory):
    sc, scan, poses, _ = mbd.inputs("tiny5")
    n, B = len(scan), len(poses)
    slam = _make(gpu_slam_factory, "tiny", batch_keep=True)
    prior = bpd.priors_for(sc, 1, bpd.U_KINDS[0], [bpd.GIVEN])[0]
    pending = {
        "single": (lambda: slam.set_pose_prior(prior), lambda: slam.set_pose_prior(None),
                   ": a pose prior is pending (so_icp_set_pose_prior); it goes into so_icp_register(_dev) or so_icp_localization(_dev) -- withdraw it with "
                   "so_icp_set_pose_prior(ctx, NULL) first"),
        "run": (lambda: slam.set_sequence_priors([prior]), lambda: slam.set_sequence_priors(None),
                ": the priors of a run are pending (so_icp_set_sequence_priors); they go into so_icp_register_sequence or so_icp_localization_sequence -- "
                "withdraw them with so_icp_set_sequence_priors(ctx, 0, NULL, NULL) first"),
        "batch": (lambda: slam.set_batch_priors([prior] * B), lambda: slam.set_batch_priors(None),
                  ": the priors of a batch are pending (so_icp_set_batch_priors); they go into so_icp_register_batch -- withdraw them with "
                  "so_icp_set_batch_priors(ctx, 0, NULL, NULL) first"),
    }
    for kind, (arm, withdraw, text) in pending.items():
        arm()
        for _ in range(2):  # (the prior is still pending after the first refusal)
            with pytest.raises(soicp.SoIcpError) as e:
                slam.match_batch(scan, poses)
            assert str(e.value) == "so_icp error -5: so_icp_match_batch" + text and slam.last_error() == "so_icp_match_batch" + text, kind
        withdraw()
        assert slam.match_batch(scan, poses)[0] == B, kind
    # ... and a pending batch prior still goes into the batch it was set for
    slam.set_batch_priors([prior] * B)
    with pytest.raises(soicp.SoIcpError):
        slam.match_batch(scan, poses)
    ok, rcs, out, sts = slam.register_batch(scan, poses)
    assert ok == B and all(s.flags & soicp.FLAG_POSE_PRIOR for s in sts)
    # n_poses = 0: returns 0 and leaves a set nothing can be selected from
    assert slam.match_batch(scan, poses)[0] == B
    st = (soicp.Stats * 1)()
    assert slam.L.so_icp_match_batch(slam.h, scan.ctypes.data_as(C.POINTER(C.c_float)), None, n, 12, poses.ctypes.data_as(C.POINTER(C.c_double)), 0, st, None) == 0
    assert slam.L.so_icp_batch_correspondences(slam.h, None, 0, None, None, 0, None, None, 0, None, None) == 0
    assert slam.L.so_icp_batch_correspondences(slam.h, None, 1, None, None, 0, None, None, 0, None, None) == -1
    # NULL arguments on a device context
    assert slam.L.so_icp_match_batch(slam.h, scan.ctypes.data_as(C.POINTER(C.c_float)), None, n, 12, None, B, st, None) == -1
    assert slam.L.so_icp_match_batch(slam.h, None, None, n, 12, poses.ctypes.data_as(C.POINTER(C.c_double)), 1, st, None) == -1
    slam.close()
    # an empty map: every rc_out NOT_ENOUGH_MAP_FEATURES, the call returns 0, nothing kept
    empty = gpu_slam_factory(plane_res=sc.plane_res, line_res=sc.plane_res / 2, max_surface_features=-1, max_iterations=MAX_OUTER)
    assert empty.keep_batch_correspondences(True) == 0
    ok, rcs, sts = empty.match_batch(scan, poses)
    assert ok == 0 and (rcs == soicp.NOT_ENOUGH_MAP_FEATURES).all() and all(s.n_iterations == 0 for s in sts)
    assert all(i.valid == 0 and i.n_accepted == 0 for i in empty.batch_correspondences(n_sel=B, cap_points=n, cap_records=0)[3])
    empty.close()
    # a sharded context
    sharded = gpu_slam_factory(plane_res=sc.plane_res, world_size=2, rank=0)
    with pytest.raises(soicp.SoIcpError) as e:
        sharded.match_batch(scan, poses)
    assert str(e.value) == "so_icp error -5: so_icp_match_batch needs the whole map on one device (world_size == 1)"
    sharded.close()


# ---- 7. the seam suffices for a batch -------------------------------------------------------------------------------------------------
def _register_batch_through_seam(slam, scan, guesses, max_outer, lm_max):
    """tests/seam_c_ref.register_through_seam for every hypothesis at once: per outer iteration ONE so_icp_match_batch on the hypotheses
    still running, then per LM step ONE so_icp_batch_correspondence_sums at the candidates of the controllers that ask for one, the
    controllers (so_icp_lm_begin / _feed) on the host.  -> the per-hypothesis namespaces register_through_seam returns"""
    from types import SimpleNamespace
    B = len(guesses)
    T = np.array(guesses, np.float64)
    res = [SimpleNamespace(pose=T[h].copy(), n_iterations=0, iters=[], JtJ=np.zeros((6, 6)), Jtr=np.zeros(6)) for h in range(B)]
    running = list(range(B))
    calls = dict(match=0, sums=0)
    for it in range(max_outer):
        ok, rcs, sts = slam.match_batch(scan, T[running])
        calls["match"] += 1
        assert ok == len(running)
        at_x = [seam_c_ref.sums_of_match(st) for st in sts]
        drv = [binding.LmDriver() for _ in running]
        nxt, more = [None] * len(running), [False] * len(running)
        for k, h in enumerate(running):
            more[k], nxt[k] = drv[k].begin(T[h], at_x[k], lm_max)
        while any(more):
            sel = [k for k in range(len(running)) if more[k]]
            sums = slam.batch_correspondence_sums(np.stack([nxt[k] for k in sel])[:, None, :], hyp=sel)
            calls["sums"] += 1
            for j, k in enumerate(sel):
                s = binding.Sums.from_buffer_copy(bytes(sums[j]))
                before = drv[k].result()[1].num_successful_steps
                more[k], nxt[k] = drv[k].feed(s)
                if drv[k].result()[1].num_successful_steps > before:
                    at_x[k] = s
        still = []
        for k, h in enumerate(running):
            x, ist = drv[k].result()
            s = at_x[k]
            res[h].iters.append(SimpleNamespace(num_surf=int(s.count), lm_iterations=ist.lm_iterations, num_successful_steps=ist.num_successful_steps,
                                                termination=ist.termination, initial_cost=ist.initial_cost, final_cost=ist.final_cost,
                                                reject_hist=[int(v) for v in s.hist[:7]], obs_hist=[int(v) for v in s.hist[7:16]], pose_after=x.copy()))
            res[h].n_iterations = it + 1
            T[h] = x
            res[h].pose = x.copy()
            if ist.num_successful_steps == 1 or it == max_outer - 1:  # LidarSlam.cpp:141
                if s.count >= 1.0:
                    i = 0
                    for a in range(6):
                        for b in range(a, 6):
                            res[h].JtJ[a, b] = res[h].JtJ[b, a] = s.JtJ[i]; i += 1
                    res[h].Jtr[:] = s.Jtr[:]
            else:
                still.append(h)
        running = still
        if not running:
            break
    return res, calls


def test_the_host_loop_over_a_batch_follows_so_icp_register_batch(gpu_slam_factory):
    sc, scan, poses, _ = bcd.batch_inputs("tiny5")
    B = len(poses)
    slam, ref = _make(gpu_slam_factory, "tiny", batch_keep=True), _make(gpu_slam_factory, "tiny")
    ok, rcs, out, sts = ref.register_batch(scan, poses)
    assert ok == B
    res, calls = _register_batch_through_seam(slam, scan, poses, MAX_OUTER, LM_MAX)
    print("outer iterations", [r.n_iterations for r in res], "calls", calls)
    assert calls["match"] == max(r.n_iterations for r in res) <= MAX_OUTER
    for h in range(B):
        st = sts[h]
        last = st.iterations[st.n_iterations - 1]
        assert_follows_oracle(st, res[h], f"tiny5 hypothesis {h}", pose=np.array(last.pose_after), opose=res[h].pose)
        for got, want in ((res[h].JtJ, np.array(st.JtJ).reshape(6, 6)), (res[h].Jtr, np.array(st.Jtr))):
            assert np.allclose(got, want, rtol=1e-7, atol=1e-7 * np.abs(want).max()), h
    slam.close(); ref.close()
