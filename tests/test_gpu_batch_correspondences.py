"""-m gpu: so_icp_keep_batch_correspondences / so_icp_batch_correspondences / so_icp_batch_correspondence_sums -- the correspondence
sets of so_icp_register_batch's hypotheses, exported and summed for a whole selection in one launch.  The yardstick throughout is a TWIN
context: so_icp_keep_correspondences on, so_icp_register_dev from poses_in[h] (so_icp_register where a test only needs the sums or a
second look at one hypothesis), then so_icp_correspondences / so_icp_correspondence_sums -- the registration a batch's hypothesis equals
bit for bit.  Every comparison is of bytes.  Inputs: tests/batch_correspondences_data.py,
which the CPU suite shows to be discriminating."""
import ctypes as C

import numpy as np
import pytest

import batch_correspondences_data as bcd
import batch_priors_data as bpd
import pose_prior_ref as ppr
from helpers import scene_with_oracle, stats_bits
from superodom_amd import synth

pytestmark = pytest.mark.gpu
IU = np.triu_indices(6)


def _make(make, scene, sub=None, batch_keep=False, keep=False):
    _, slam, _ = scene_with_oracle(scene, None, make, oracle_too=False, max_iterations=bcd.MAX_OUTER)
    if sub:
        slam.set_max_surface_features(sub)
    if batch_keep:
        assert slam.keep_batch_correspondences(True) == 0
    if keep:
        assert slam.keep_correspondences(True) == 0
    return slam


def _twin_export(twin, scan, guess, pose=None):
    """the yardstick for one hypothesis: (rc, records bytes, status bytes, info bytes, info) of so_icp_correspondences on the twin"""
    n = len(scan)
    if n:
        d, _ = twin.upload_scan(scan)
        rc, _, st = twin.register_dev(d, n, guess)
    else:  # (nothing to upload)
        rc, _, st = twin.register(scan, guess)
    rec, status, _, info = twin.correspondences(pose=pose, cap=n)
    if n:
        twin.free_scan(d)
    return rc, rec.tobytes(), status.tobytes(), bytes(info), info, st


def _entry(rec, first, status, infos, k):
    return rec[int(first[k]):int(first[k + 1])].tobytes(), status[k].tobytes(), bytes(infos[k])


@pytest.fixture(scope="module")
def tiny(gpu_slam_factory):
    """(scene, a context with the batch switch on, its twin) on scene tiny, shared by the tests that only need them in that state"""
    slam, twin = _make(gpu_slam_factory, "tiny", batch_keep=True), _make(gpu_slam_factory, "tiny", keep=True)
    yield synth.Scene("tiny"), slam, twin
    slam.close(); twin.close()


# ---- 1. every hypothesis against its twin -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(bcd.CASES))
def test_every_hypothesis_equals_its_twin(gpu_slam_factory, case):
    sc, scan, poses, sub = bcd.batch_inputs(case)
    B, n = len(poses), len(scan)
    slam = _make(gpu_slam_factory, bcd.CASES[case][0], sub, batch_keep=True)
    twin = _make(gpu_slam_factory, bcd.CASES[case][0], sub, keep=True)
    d, dn = slam.upload_scan(scan)
    ok, rcs, out, sts = slam.register_batch(None, poses, d_scan=d, n=dn)
    assert ok == B and (rcs == 0).all()
    at = np.stack([synth.perturb_pose(out[h], 300 + h, 0.03, 0.3) for h in range(B)])  # a pose of the caller's per entry
    rec, first, status, infos = slam.batch_correspondences(n_sel=B, cap_points=n, cap_records=B * n)
    rec_at, first_at, status_at, infos_at = slam.batch_correspondences(n_sel=B, poses=at, cap_points=n, cap_records=B * n)
    assert np.array_equal(first, first_at) and int(first[0]) == 0
    outer, sets = [], set()
    for h in range(B):
        rc, t_rec, t_status, t_info, info, st = _twin_export(twin, scan, poses[h])
        assert rc == 0 and info.valid == 1
        assert int(first[h + 1] - first[h]) == info.n_accepted == sts[h].iterations[sts[h].n_iterations - 1].num_surf_from_scan > 0, (case, h)
        assert _entry(rec, first, status, infos, h) == (t_rec, t_status, t_info), (case, h, "default pose")
        assert bytes(infos[h].pose_eval) == bytes(st.iterations[st.n_iterations - 1].pose_after) and infos[h].outer_iteration == sts[h].n_iterations - 1
        t_rec2, t_status2, _, t_info2 = twin.correspondences(pose=at[h], cap=n)
        assert _entry(rec_at, first_at, status_at, infos_at, h) == (t_rec2.tobytes(), t_status2.tobytes(), bytes(t_info2)), (case, h, "given pose")
        assert bytes(infos_at[h].pose_eval) == at[h].tobytes() and infos_at[h].cost != infos[h].cost
        outer.append(infos[h].outer_iteration)
        sets.add(status[h].tobytes())
    print(case, "outer iterations", outer, "distinct status rows", len(sets))
    assert len(set(outer)) >= 2 and len(sets) >= 2, "the hypotheses should differ (tests/test_batch_correspondences_host.py)"
    if sub:
        assert (status == 254).any(), "a sub-sampled scan has points that were not sampled"
    slam.close(); twin.close()


# ---- 2. sizes: every entry ends in a partial tile, the next entry's chain starts afresh ----------------------------------------------
@pytest.mark.parametrize("n", bcd.SIZES)
def test_export_of_every_size(tiny, n):
    sc, slam, twin = tiny
    scan = np.ascontiguousarray(sc.scan(bcd.SCAN_ID)[:n], np.float32)
    poses = bpd.guesses(sc, 3)
    ok, rcs, out, sts = slam.register_batch(scan, poses)
    rec, first, status, infos = slam.batch_correspondences(n_sel=3, cap_points=n, cap_records=3 * n)
    assert status.shape == (3, n)
    for h in range(3):
        rc, t_rec, t_status, t_info, info, _ = _twin_export(twin, scan, poses[h])
        assert rc == int(rcs[h]) == 0 and info.valid == 1 and infos[h].n_points == n, (n, h, rc, int(rcs[h]))
        assert int(first[h + 1] - first[h]) == info.n_accepted
        assert _entry(rec, first, status, infos, h) == (t_rec, t_status, t_info), (n, h)
    if n == 0:
        assert not first.any() and all(i.valid == 1 and i.n_accepted == 0 and i.cost == 0.0 for i in infos)


# ---- 3. selection ---------------------------------------------------------------------------------------------------------------------
def test_selection_order_repeats_and_the_device_copy(tiny):
    sc, slam, twin = tiny
    sc, scan, poses, _ = bcd.batch_inputs("tiny5")
    n = len(scan)
    ok, rcs, out, sts = slam.register_batch(scan, poses)
    assert ok == 5
    rec, first, status, infos = slam.batch_correspondences(n_sel=5, cap_points=n, cap_records=5 * n)
    whole = [_entry(rec, first, status, infos, h) for h in range(5)]
    assert len({w[0] for w in whole}) >= 2
    # two calls give identical bytes
    rec2, first2, status2, infos2 = slam.batch_correspondences(n_sel=5, cap_points=n, cap_records=5 * n)
    assert rec2.tobytes() == rec.tobytes() and np.array_equal(first, first2) and status2.tobytes() == status.tobytes()
    assert [bytes(i) for i in infos2] == [bytes(i) for i in infos]
    # a subset, reversed order, hyp = NULL for a prefix
    for hyp in ([3, 1], [4, 3, 2, 1, 0], [2], [0, 4, 4, 0]):
        r, f, s, i = slam.batch_correspondences(hyp=hyp, cap_points=n, cap_records=len(hyp) * n)
        assert [_entry(r, f, s, i, k) for k in range(len(hyp))] == [whole[h] for h in hyp], hyp
        assert int(f[-1]) == len(r) == sum(len(whole[h][0]) // 72 for h in hyp)
    r, f, s, i = slam.batch_correspondences(n_sel=3, cap_points=n, cap_records=3 * n)
    assert [_entry(r, f, s, i, k) for k in range(3)] == whole[:3]
    # an n_sel = 1 call is the slice of the all-hypotheses call
    for h in range(5):
        r, f, s, i = slam.batch_correspondences(hyp=[h], cap_points=n, cap_records=n)
        assert _entry(r, f, s, i, 0) == whole[h] and int(f[0]) == 0
    # a repeated index with two different poses: each entry at its own pose, as the twin evaluates them
    at = np.stack([synth.perturb_pose(out[2], 41, 0.03, 0.3), synth.perturb_pose(out[2], 42, 0.03, 0.3)])
    r, f, s, i = slam.batch_correspondences(hyp=[2, 2], poses=at, cap_points=n, cap_records=2 * n)
    rc = twin.register(scan, poses[2])[0]
    assert rc == 0
    for k in range(2):
        t_rec, t_status, _, t_info = twin.correspondences(pose=at[k], cap=n)
        assert _entry(r, f, s, i, k) == (t_rec.tobytes(), t_status.tobytes(), bytes(t_info)), k
    assert _entry(r, f, s, i, 0)[0] != _entry(r, f, s, i, 1)[0]
    # counts only: records NULL or too small a capacity; the ranges and the infos are the same
    r, f, s, i = slam.batch_correspondences(n_sel=5, cap_points=n, cap_records=int(first[5]) - 1, want_status=False)
    assert np.array_equal(f, first) and [bytes(x) for x in i] == [bytes(x) for x in infos] and not r.view(np.uint8).any()
    # d_records_out holds the same bytes
    d_rec, f, i = slam.batch_correspondences_dev(n_sel=5)
    assert np.array_equal(f, first) and [bytes(x) for x in i] == [bytes(x) for x in infos]
    assert slam.download_bytes(d_rec, 72 * int(first[5])).tobytes() == rec.tobytes()


# ---- 4. every path of a batch to the same bytes -----------------------------------------------------------------------------------------
_default = {}


@pytest.fixture(scope="module")
def default_small9(gpu_slam_factory):
    def get():
        if not _default:
            sc, scan, poses, sub = bcd.batch_inputs("small9")
            slam = _make(gpu_slam_factory, "small", sub, batch_keep=True)
            ok, rcs, out, sts = slam.register_batch(scan, poses)
            assert ok == len(poses)
            rec, first, status, infos = slam.batch_correspondences(n_sel=len(poses), cap_points=len(scan), cap_records=len(poses) * len(scan))
            _default["v"] = (scan, poses, sub, out.copy(), [stats_bits(s) for s in sts], rec.tobytes(), first.copy(), status.tobytes(), [bytes(i) for i in infos])
            slam.close()
        return _default["v"]
    yield get
    _default.clear()


def _same_export(slam, ref, tag, order=None):
    scan, poses, sub, out, bits, rec_b, first, status_b, info_b = ref
    B, n = len(poses), len(scan)
    rec, f, status, infos = slam.batch_correspondences(hyp=order, n_sel=B, cap_points=n, cap_records=B * n)
    if order is None:
        assert rec.tobytes() == rec_b and np.array_equal(f, first) and status.tobytes() == status_b and [bytes(i) for i in infos] == info_b, tag
    else:  # entry k of this batch is hypothesis order[k] of the reference batch
        ref_rec, ref_status = np.frombuffer(rec_b, rec.dtype), np.frombuffer(status_b, np.uint8).reshape(B, n)
        for k, h in enumerate(order):
            assert rec[int(f[k]):int(f[k + 1])].tobytes() == ref_rec[int(first[h]):int(first[h + 1])].tobytes(), (tag, k)
            assert status[k].tobytes() == ref_status[h].tobytes() and bytes(infos[k]) == info_b[h], (tag, k)


@pytest.mark.parametrize("env", [{"SOICP_BATCH_MODE": "lanes"}, {"SOICP_BATCH_MODE": "one_per_cu"}, {"SOICP_BATCH_CHAIN": "0"}])
def test_the_other_paths_of_a_batch_leave_the_same_set(gpu_slam_factory, monkeypatch, default_small9, env):
    ref = default_small9()
    scan, poses, sub, out = ref[:4]
    for k, v in env.items():
        monkeypatch.setenv(k, v)  # read by so_icp_create
    alt = _make(gpu_slam_factory, "small", sub, batch_keep=True)
    ok, rcs, out2, sts2 = alt.register_batch(scan, poses)
    assert ok == len(poses) and np.array_equal(out2, out)
    _same_export(alt, ref, env)
    alt.close()


def test_a_resident_scan_and_a_second_batch_which_replaces_the_set(gpu_slam_factory, default_small9):
    ref = default_small9()
    scan, poses, sub, out = ref[:4]
    B = len(poses)
    slam = _make(gpu_slam_factory, "small", sub, batch_keep=True)
    d, n = slam.upload_scan(scan)
    ok, rcs, out2, _ = slam.register_batch(None, poses, d_scan=d, n=n)
    assert ok == B and np.array_equal(out2, out)
    _same_export(slam, ref, "resident scan")
    # a second batch on the same context, of fewer hypotheses in another order: its set replaces the first
    order = [7, 0, 5, 2]
    ok, rcs, out3, _ = slam.register_batch(None, poses[order], d_scan=d, n=n)
    assert ok == len(order) and np.array_equal(out3, out[order])
    rec, f, status, infos = slam.batch_correspondences(n_sel=len(order), cap_points=n, cap_records=len(order) * n)
    ref_rec, first, ref_status = np.frombuffer(ref[5], rec.dtype), ref[6], np.frombuffer(ref[7], np.uint8).reshape(B, n)
    for k, h in enumerate(order):
        assert rec[int(f[k]):int(f[k + 1])].tobytes() == ref_rec[int(first[h]):int(first[h + 1])].tobytes(), k
        assert status[k].tobytes() == ref_status[h].tobytes() and bytes(infos[k]) == ref[8][h], k
    assert slam.L.so_icp_batch_correspondences(slam.h, (C.c_int32 * 1)(len(order)), 1, None, None, 0, None, None, 0, None, None) == -1, "hypothesis 4 of the first batch is gone"
    slam.close()


@pytest.mark.parametrize("kind", bpd.U_KINDS)
def test_a_batch_with_priors_plane_sums_plus_the_host_prior(soicp, gpu_slam_factory, kind):
    """so_icp_set_batch_priors: the sums of a hypothesis are those of its planes; with so_icp_pose_prior_sums added on the host at the
    default pose they are the normal equations so_icp_stats reports -- the comparison of
    test_gpu_batch_priors.py::test_last_outer_iteration_against_correspondence_sums_and_the_host_prior, for every hypothesis in one call."""
    sc, scan, poses, priors, modes, sub = bpd.batch_inputs("tiny5", kind)
    B = len(poses)
    slam = _make(gpu_slam_factory, "tiny", batch_keep=True)
    slam.set_batch_priors(priors, modes)
    ok, rcs, out, sts = slam.register_batch(scan, poses)
    assert ok == B
    x1 = np.stack([np.array(st.iterations[st.n_iterations - 1].pose_after) for st in sts])
    sums = slam.batch_correspondence_sums(x1[:, None, :])
    for h in range(B):
        st, planes = sts[h], sums[h]
        last = st.iterations[st.n_iterations - 1]
        assert planes.count == last.num_surf_from_scan > 0, h
        P = bpd.hypothesis_prior(priors, modes, h, poses[h])
        assert (P is not None) == bool(st.flags & soicp.FLAG_POSE_PRIOR)
        prior_cost = 0.0 if P is None else ppr.host_prior_sums(P, x1[h], planes.count).cost
        print(f"{kind} hypothesis {h}: final_cost {last.final_cost!r}, planes {planes.cost!r} + prior {prior_cost!r}")
        assert abs((last.final_cost - prior_cost) - planes.cost) <= 1e-9 * max(1.0, abs(planes.cost)), (h, last.final_cost, prior_cost, planes.cost)
        JtJ_p, Jtr_p = (np.zeros(21), np.zeros(6)) if P is None else (lambda b: (np.array(b.JtJ[:]), np.array(b.Jtr[:])))(ppr.host_prior_sums(P, x1[h], planes.count))
        for got, want in ((np.array(st.JtJ).reshape(6, 6)[IU] - JtJ_p, np.array(planes.JtJ[:])), (np.array(st.Jtr) - Jtr_p, np.array(planes.Jtr[:]))):
            assert np.allclose(got, want, rtol=1e-9, atol=1e-9 * np.abs(want).max()), (h, got, want)
    slam.close()


# ---- 5. sums ----------------------------------------------------------------------------------------------------------------------------
_sized = {}


@pytest.fixture(scope="module")
def sized_batches(gpu_slam_factory):
    """size -> (scan, guesses, final poses, the twin's kept contexts are not needed: the twin's sums at 64 poses per hypothesis)"""
    ctx = {}

    def get(n):
        if n not in _sized:
            if not ctx:
                ctx["twin"] = _make(gpu_slam_factory, "tiny", keep=True)
            sc = synth.Scene("tiny")
            scan = np.ascontiguousarray(sc.scan(bcd.SCAN_ID)[:n], np.float32)
            poses = bpd.guesses(sc, 3)
            twin_sums, at = [], []
            for h in range(3):
                rc, pose, st = ctx["twin"].register(scan, poses[h])
                assert rc == 0
                at.append(bcd.poses_near(st.iterations[st.n_iterations - 1].pose_after, 64, 500 + 64 * h))
                twin_sums.append([bytes(s) for s in ctx["twin"].correspondence_sums(at[-1])])
            _sized[n] = (scan, poses, np.stack(at), twin_sums)
        return _sized[n]
    yield get
    for c in ctx.values():
        c.close()
    _sized.clear()


@pytest.mark.parametrize("n", bcd.SUMS_SIZES)
@pytest.mark.parametrize("n_poses", bcd.SUMS_POSES)
def test_sums_equal_the_twins_to_the_bit(tiny, sized_batches, n_poses, n):
    sc, slam, _ = tiny
    scan, poses, at, twin_sums = sized_batches(n)
    ok, rcs, out, sts = slam.register_batch(scan, poses)
    assert ok == 3
    sums = slam.batch_correspondence_sums(at[:, :n_poses])
    for k in range(3):
        for j in range(n_poses):
            assert bytes(sums[k * n_poses + j]) == twin_sums[k][j], (n, n_poses, k, j)
    # cost is the export's cost at that pose, to the bit; the counts are the export's
    for j in sorted({0, n_poses // 2, n_poses - 1}):
        _, first, _, infos = slam.batch_correspondences(n_sel=3, poses=at[:, j], want_status=False, want_records=False, cap_points=n, cap_records=0)
        for k in range(3):
            s = sums[k * n_poses + j]
            assert np.float64(s.cost).tobytes() == np.float64(infos[k].cost).tobytes() and s.count == infos[k].n_accepted == int(first[k + 1] - first[k]), (n, j, k)
    # a selection of the sums: repeated and reordered entries
    hyp = [2, 0, 2]
    sel = slam.batch_correspondence_sums(at[hyp, :n_poses], hyp=hyp)
    for k, h in enumerate(hyp):
        assert [bytes(sel[k * n_poses + j]) for j in range(n_poses)] == twin_sums[h][:n_poses], (n, n_poses, k)


# ---- 6. nothing to export, and what must be left alone ----------------------------------------------------------------------------------
def test_switch_off_exports_nothing_and_changes_nothing(soicp, gpu_slam_factory):
    sc, scan, poses, _ = bcd.batch_inputs("tiny5")
    n, B = len(scan), len(poses)
    slam = _make(gpu_slam_factory, "tiny")
    # before any batch, switch off and switch on: valid = 0
    for on in (False, True):
        assert slam.keep_batch_correspondences(on) == 0
        rec, first, status, infos = slam.batch_correspondences(n_sel=B, cap_points=n, cap_records=B * n)
        assert len(rec) == 0 and not first.any() and all(i.valid == 0 and bytes(i) == bytes(C.sizeof(i)) for i in infos)
        assert bytes(slam.batch_correspondence_sums(np.tile(poses[:, None, :], (1, 2, 1)))) == bytes(2 * B * C.sizeof(soicp.Sums)), "zero sums"
    assert slam.keep_batch_correspondences(False) == 0
    ok, rcs, out_off, sts_off = slam.register_batch(scan, poses)
    assert ok == B
    assert all(i.valid == 0 for i in slam.batch_correspondences(n_sel=B, cap_points=n, cap_records=0)[3]), "the switch was off during the batch"
    assert slam.keep_batch_correspondences(True) == 0
    assert all(i.valid == 0 for i in slam.batch_correspondences(n_sel=B, cap_points=n, cap_records=0)[3]), "no batch has run with the switch on"
    ok, rcs, out_on, sts_on = slam.register_batch(scan, poses)
    assert ok == B and out_on.tobytes() == out_off.tobytes(), "poses with the switch on and off"
    for h in range(B):
        assert stats_bits(sts_on[h]) == stats_bits(sts_off[h]) and sts_on[h].flags == sts_off[h].flags, h
    infos = slam.batch_correspondences(n_sel=B, cap_points=n, cap_records=0)[3]
    assert all(i.valid == 1 and i.n_accepted > 0 for i in infos)
    # turning the switch off drops the set
    assert slam.keep_batch_correspondences(False) == 0 and slam.keep_batch_correspondences(True) == 0
    assert all(i.valid == 0 for i in slam.batch_correspondences(n_sel=B, cap_points=n, cap_records=0)[3])
    # n_hyp = 0: a set nothing can be selected from
    ok, rcs, out, sts = slam.register_batch(scan, poses)
    assert ok == B
    assert slam.L.so_icp_register_batch(slam.h, scan.ctypes.data_as(C.POINTER(C.c_float)), None, n, 12, poses.ctypes.data_as(C.POINTER(C.c_double)), 0,
                                        out.ctypes.data_as(C.POINTER(C.c_double)), None, None) == 0
    assert slam.L.so_icp_batch_correspondences(slam.h, None, 0, None, None, 0, None, None, 0, None, None) == 0
    assert slam.L.so_icp_batch_correspondences(slam.h, None, 1, None, None, 0, None, None, 0, None, None) == -1
    assert slam.last_error() == "so_icp_batch_correspondences: a hypothesis index lies outside the last batch (0 .. n_hyp - 1)"
    slam.close()


def test_an_empty_map_and_an_empty_scan(soicp, gpu_slam_factory):
    sc, scan, poses, _ = bcd.batch_inputs("tiny5")
    n, B = len(scan), 3
    poses = poses[:B]
    empty = gpu_slam_factory(plane_res=sc.plane_res, line_res=sc.plane_res / 2, max_surface_features=-1, max_iterations=bcd.MAX_OUTER)
    assert empty.keep_batch_correspondences(True) == 0
    ok, rcs, out, sts = empty.register_batch(scan, poses)
    assert ok == 0 and (rcs == soicp.NOT_ENOUGH_MAP_FEATURES).all()
    rec, first, status, infos = empty.batch_correspondences(n_sel=B, cap_points=n, cap_records=B * n)
    assert len(rec) == 0 and not first.any() and all(i.valid == 0 and i.n_accepted == 0 for i in infos)
    raw = np.zeros(B * n, np.uint8)
    assert empty.L.so_icp_batch_correspondences(empty.h, None, B, None, None, 0, None, raw.ctypes.data_as(C.POINTER(C.c_uint8)), len(raw), None, None) == 0
    assert (raw == 254).all(), "an entry without a set: nothing was sampled"
    assert bytes(empty.batch_correspondence_sums(poses[:, None, :])) == bytes(B * C.sizeof(soicp.Sums))
    empty.close()
    slam = _make(gpu_slam_factory, "tiny", batch_keep=True)
    none = np.zeros((0, 3), np.float32)
    ok, rcs, out, sts = slam.register_batch(none, poses)
    rec, first, status, infos = slam.batch_correspondences(n_sel=B, cap_points=0, cap_records=0)
    assert (rcs == 0).all() and len(rec) == 0 and not first.any()
    assert all(i.valid == 1 and i.n_points == 0 and i.n_accepted == 0 and i.cost == 0.0 for i in infos)
    twin = _make(gpu_slam_factory, "tiny", keep=True)
    for h in range(B):
        assert twin.register(none, poses[h])[0] == 0
        assert bytes(twin.correspondences(cap=0)[3]) == bytes(infos[h]), h
        assert bytes(twin.correspondence_sums(poses[h])[0]) == bytes(slam.batch_correspondence_sums(poses[h][None, None, :], hyp=[h])[0]), h
    slam.close(); twin.close()


def test_the_set_survives_other_entries_and_leaves_the_single_set_alone(gpu_slam_factory):
    sc, scan, poses, _ = bcd.batch_inputs("tiny5")
    n, B = len(scan), len(poses)
    slam = _make(gpu_slam_factory, "tiny", batch_keep=True, keep=True)  # both switches on
    ok, rcs, out, sts = slam.register_batch(scan, poses)
    assert ok == B
    assert slam.correspondences(cap=n)[3].valid == 0, "a batch still ends the single kept set"
    export = lambda: (lambda r, f, s, i: (r.tobytes(), f.tobytes(), s.tobytes(), [bytes(x) for x in i]))(*slam.batch_correspondences(n_sel=B, cap_points=n, cap_records=B * n))
    sums = lambda: bytes(slam.batch_correspondence_sums(np.tile(out[:, None, :], (1, 2, 1))))
    first_export, first_sums = export(), sums()
    # a registration of another scan, a match, a map insert and a change of resolution between the batch and the export
    other = np.ascontiguousarray(sc.scan(0)[:1500], np.float32)
    rc, pose, st = slam.register(other, sc.guess(0))
    assert rc == 0
    single = (lambda r, s, q, i: (r.tobytes(), s.tobytes(), q.tobytes(), bytes(i)))(*slam.correspondences(cap=len(other)))
    assert export() == first_export and sums() == first_sums, "after so_icp_register"
    # the single kept set of a context with both switches on is untouched by the batch exports
    assert (lambda r, s, q, i: (r.tobytes(), s.tobytes(), q.tobytes(), bytes(i)))(*slam.correspondences(cap=len(other))) == single
    assert slam.match(other, sc.guess(0))[0] == 0
    assert export() == first_export and sums() == first_sums, "after so_icp_match"
    slam.add_surf_point_cloud(other)
    assert export() == first_export and sums() == first_sums, "after so_icp_map_add_surf"
    slam.set_resolution(sc.plane_res, 2 * sc.plane_res)
    assert export() == first_export and sums() == first_sums, "after so_icp_set_resolution (the loss is that of the batch)"
    slam.close()


def test_refusals_by_code_and_whole_text(soicp, gpu_slam_factory):
    sc, scan, poses, _ = bcd.batch_inputs("tiny5")
    n, B = len(scan), len(poses)
    slam = _make(gpu_slam_factory, "tiny", batch_keep=True)
    ok, rcs, out, sts = slam.register_batch(scan, poses)
    assert ok == B
    outside = "a hypothesis index lies outside the last batch (0 .. n_hyp - 1)"
    for hyp in ([0, B], [-1], [1, 2, 70]):
        with pytest.raises(soicp.SoIcpError) as e:
            slam.batch_correspondences(hyp=hyp, cap_points=n, cap_records=len(hyp) * n)
        assert str(e.value) == "so_icp error -1: so_icp_batch_correspondences: " + outside and slam.last_error() == "so_icp_batch_correspondences: " + outside
        with pytest.raises(soicp.SoIcpError) as e:
            slam.batch_correspondence_sums(np.tile(out[0], (len(hyp), 1, 1)), hyp=hyp)
        assert str(e.value) == "so_icp error -1: so_icp_batch_correspondence_sums: " + outside
    with pytest.raises(soicp.SoIcpError) as e:
        slam.batch_correspondences(n_sel=B + 1, cap_points=n, cap_records=0)  # (hyp = NULL names hypothesis B)
    assert str(e.value) == "so_icp error -1: so_icp_batch_correspondences: " + outside
    status = np.zeros(B * n - 1, np.uint8)
    info = (soicp.CorrespondenceInfo * B)()
    rc = slam.L.so_icp_batch_correspondences(slam.h, None, B, None, None, 0, None, status.ctypes.data_as(C.POINTER(C.c_uint8)), len(status), None, info)
    assert rc == -1 and slam.last_error() == "so_icp_batch_correspondences: status_out needs cap_status >= n_sel x the points of the batch's scan"
    assert not status.any()
    # a sharded context
    sharded = gpu_slam_factory(plane_res=sc.plane_res, world_size=2, rank=0)
    assert sharded.keep_batch_correspondences(True) == -5
    assert sharded.last_error() == "so_icp_keep_batch_correspondences: so_icp_register_batch needs the whole map on one device (world_size == 1)"
    sharded.close()
    slam.close()
