"""-m gpu: so_icp_keep_correspondences / so_icp_correspondences -- the correspondence set of the last registration (the reference's
features_corres, LidarSlam.h:209-222) exported from the device: against the status bytes of so_icp_debug_match_status, against the
oracle's correspondences, against numpy from the records' own fields, against the registration's own statistics (costs, JtJ, Jtr),
through every registration entry and sweep / solve path, and the cases in which there is nothing to export."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import correspondences_ref as cref
import plane_factor_host as pfh
from helpers import assert_same_bits, chain_deltas, run_staged_stream, scene_with_oracle
from superodom_amd import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "adapter", "adapter_driver")
TILE = 1024  # corr_kernels.h kCorrTile


def _ctx(oracle, make, scene="tiny", keep=True, **cfg):
    cfg.setdefault("max_iterations", 5)
    sc, slam, om = scene_with_oracle(scene, oracle, make, **cfg)
    if keep:
        assert slam.keep_correspondences(True) == 0
    return sc, slam, om


@pytest.fixture(scope="module")
def tiny(oracle, gpu_slam_factory):
    sc, slam, om = _ctx(oracle, gpu_slam_factory)
    yield sc, slam, om
    slam.close()


def _info_bytes(info):
    return bytes(info)


def _export_bytes(slam, n, pose=None):
    rec, status, resid, info = slam.correspondences(pose=pose, cap=n)
    return rec.tobytes(), status.tobytes(), resid.tobytes(), _info_bytes(info)


def check_export(slam, scan, guess, st, plane_res, *, ocorrs=None, variant=0, tag=""):
    """everything the issue holds in every case, for the registration (guess, st) of `scan` that `slam` ran last"""
    n = len(scan)
    rec, status, resid, info = slam.correspondences(cap=n)
    n_it = st.n_iterations
    last = st.iterations[n_it - 1]
    assert info.valid == 1 and info.n_points == n and info.outer_iteration == n_it - 1, (tag, info.valid, info.n_points)
    assert bytes(info.pose_eval) == bytes(last.pose_after), tag
    want_fit = np.asarray(guess, np.float64) if n_it == 1 else np.array(st.iterations[n_it - 2].pose_after)
    assert np.array_equal(np.array(info.pose_fit), want_fit), (tag, "pose_fit")
    # status bytes, positions, points
    assert np.array_equal(status, slam.match_status(n)), (tag, "status against so_icp_debug_match_status")
    if ocorrs is not None:
        assert np.array_equal(status, np.where(ocorrs["status"] < 0, cref.NOT_SAMPLED, ocorrs["status"]).astype(np.uint8)), (tag, "status against the oracle")
    idx = np.flatnonzero(status == 0)
    assert info.n_accepted == len(rec) == last.num_surf_from_scan == len(idx), (tag, info.n_accepted, len(rec), last.num_surf_from_scan, len(idx))
    assert np.array_equal(rec["index"], idx), (tag, "ascending positions of status 0")
    assert np.array_equal(rec["p"].view(np.uint32), np.ascontiguousarray(scan[idx]).view(np.uint32)), (tag, "the scan's bits")
    want_res = np.full(n, np.nan, np.float32); want_res[idx] = rec["residual"].astype(np.float32)
    assert np.array_equal(resid.view(np.uint32)[idx], want_res.view(np.uint32)[idx]) and np.all(np.isnan(resid[status != 0])), (tag, "residual_out")
    a2 = cref.tukey_a2(plane_res)
    if ocorrs is not None and len(idx):
        o = ocorrs[idx]
        for f in ("n", "d", "coeff"):
            err = np.abs(rec[f] - o[f]).max()
            print(f"{tag}: max |{f} - oracle| {err:.3e}")
            assert err <= 1e-10, (tag, f, err)
    for pose, name in ((np.array(info.pose_eval), "default pose"),):
        cref.check_fields_at(rec, pose, a2, variant, f"{tag} {name}")
    # costs: at the default pose the registration's final cost, at pose_fit its initial cost
    assert abs(info.cost - last.final_cost) <= 1e-9 * max(1.0, abs(last.final_cost)), (tag, info.cost, last.final_cost)
    _, _, _, info_fit = slam.correspondences(pose=np.array(info.pose_fit), cap=n)
    assert abs(info_fit.cost - last.initial_cost) <= 1e-9 * max(1.0, abs(last.initial_cost)), (tag, info_fit.cost, last.initial_cost)
    assert bytes(info_fit.pose_eval) == bytes(info.pose_fit)
    # the normal equations summed on the host from the records against so_icp_stats
    JtJ, Jtr, JtJ_abs, Jtr_abs = cref.normal_equations(rec["p"], rec["n"], rec["residual"], rec["weight"], np.array(info.pose_eval))
    for got, want, absum, what in ((JtJ, np.array(st.JtJ).reshape(6, 6), JtJ_abs, "JtJ"), (Jtr, np.array(st.Jtr), Jtr_abs, "Jtr")):
        err, bound = np.abs(got - want), cref.sum_bound(len(rec), absum)
        print(f"{tag}: {what} max |difference| {err.max():.3e}, largest |difference| / bound {np.max(err[bound > 0] / bound[bound > 0], initial=0.0):.3f}")
        assert np.all(err <= bound), (tag, what, err.max())
    # determinism, and the device copy of the records
    first = (rec.tobytes(), status.tobytes(), resid.tobytes(), _info_bytes(info))
    assert _export_bytes(slam, n) == first, (tag, "a second call returns identical bytes")
    d_rec, info_d = slam.correspondences_dev()
    assert _info_bytes(info_d) == first[3]
    if len(rec):
        assert slam.download_bytes(d_rec, 72 * len(rec)).tobytes() == first[0], (tag, "d_records_out")
    return rec, status, resid, info


_oracle_cache = {}


def _oracle_corrs(oracle, om, scan, guess, msf=-1, variant=0, key=None):
    if key is None or key not in _oracle_cache:
        rc, pose, st, corrs = om.register(scan, guess, oracle.default_config(max_iterations=5, max_surface_features=msf, tukey_variant=variant), want_corrs=True)
        assert rc == 0
        if key is None:
            return corrs
        _oracle_cache[key] = corrs
    return _oracle_cache[key]


# ---- sizes: prefixes of tiny's scan 0, each a real registration -------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, TILE - 1, TILE, TILE + 1, 4096])
def test_export_of_every_size(oracle, tiny, n):
    sc, slam, om = tiny
    scan = np.ascontiguousarray(sc.scan(0)[:n], np.float32)
    rc, pose, st = slam.register(scan, sc.guess(0))
    assert rc == 0
    if n == 0:
        rec, status, resid, info = slam.correspondences(cap=0)
        assert info.valid == 1 and info.n_points == 0 and info.n_accepted == 0 and len(rec) == 0 and info.cost == 0.0
        return
    check_export(slam, scan, sc.guess(0), st, sc.plane_res, ocorrs=_oracle_corrs(oracle, om, scan, sc.guess(0), key=("tiny", n)), tag=f"n={n}")


def test_export_of_the_binned_sweep(oracle, gpu_slam_factory):
    sc, slam, om = _ctx(oracle, gpu_slam_factory, "small")
    scan = np.ascontiguousarray(sc.scan(0), np.float32)
    assert len(scan) == 16384
    rc, pose, st = slam.register(scan, sc.guess(0))
    assert rc == 0 and not (st.flags & 512)  # (not swept by query waves: binned)
    check_export(slam, scan, sc.guess(0), st, sc.plane_res, ocorrs=_oracle_corrs(oracle, om, scan, sc.guess(0)), tag="small")
    slam.close()


# ---- composite scan: whole tiles and whole wavefronts without an accepted point; both branches of the loss; the other variant -----
@pytest.mark.parametrize("variant", [0, 1])
def test_composite_scan_and_both_tukey_branches(oracle, gpu_slam_factory, variant):
    sc, slam, om = _ctx(oracle, gpu_slam_factory, tukey_variant=variant)
    scan, far = cref.composite_scan(np.ascontiguousarray(sc.scan(0), np.float32), TILE)
    rc, pose, st = slam.register(scan, sc.guess(0))
    assert rc == 0
    ocorrs = _oracle_corrs(oracle, om, scan, sc.guess(0), variant=variant)
    rec, status, resid, info = check_export(slam, scan, sc.guess(0), st, sc.plane_res, ocorrs=ocorrs, variant=variant, tag=f"composite v{variant}")
    assert np.all(status[far] == 1) and np.all(status[TILE:2 * TILE] == 1), "a whole tile without an accepted point"
    # 1 m above the optimised pose part of the set lies outside the loss's window
    up = np.array(info.pose_eval); up[2] += 1.0
    rec_up, status_up, resid_up, info_up = slam.correspondences(pose=up, cap=len(scan))
    a2 = cref.tukey_a2(sc.plane_res)
    outside = rec_up["residual"] ** 2 > a2
    assert outside.any() and (~outside).any() and np.all(rec_up["weight"][outside] == 0)
    assert np.array_equal(status_up, status) and np.array_equal(rec_up["index"], rec["index"]) and bytes(info_up.pose_eval) == up.tobytes()
    for f in ("p", "n", "d", "coeff"):
        assert rec_up[f].tobytes() == rec[f].tobytes()
    cref.check_fields_at(rec_up, up, a2, variant, f"composite v{variant} +1 m")
    term, _ = cref.loss(rec_up["residual"], rec_up["coeff"], a2, variant)
    assert abs(info_up.cost - term.sum()) <= cref.sum_bound(len(rec_up), np.abs(term).sum())
    ocost = oracle.evaluate(ocorrs, up, sc.plane_res, variant)[0]
    assert abs(info_up.cost - ocost) <= 1e-9 * max(1.0, abs(ocost))
    slam.close()


# ---- residual and weight are the bits of the host build of plane_factor.h ------------------------------------------------------------
@pytest.mark.parametrize("variant", [0, 1])
def test_residual_and_weight_are_the_host_builds_bits(oracle, gpu_slam_factory, tiny, variant):
    """The kernels and g++ (tests/plane_factor_host.py) compile the same text of plane_factor.h with -ffp-contract=off, and it uses only
    + - * / and explicit fma, all correctly rounded on both sides: the export's residual and weight equal the host's to the bit -- at the
    last evaluation's pose, with that pose passed as pose=, and at a displaced pose where both branches of the loss run.  Two tiles, the
    second holding one point."""
    sc, slam, _ = tiny if variant == 0 else _ctx(oracle, gpu_slam_factory, tukey_variant=variant, oracle_too=False)
    scan = np.ascontiguousarray(sc.scan(0)[:TILE + 1], np.float32)
    rc, pose, st = slam.register(scan, sc.guess(0))
    assert rc == 0
    a2 = cref.tukey_a2(sc.plane_res)
    rec0, _, _, info = slam.correspondences(cap=len(scan))
    assert info.valid == 1 and info.n_points == TILE + 1 and len(rec0) > 200
    at_eval = np.array(info.pose_eval)
    for tag, pose_arg, at in (("default pose", None, at_eval), ("pose=pose_eval", at_eval, at_eval), ("displaced", pfh.displaced(at_eval), None)):
        rec, _, _, info_k = slam.correspondences(pose=pose_arg, cap=len(scan))
        at = pose_arg if at is None else at
        assert bytes(info_k.pose_eval) == at.tobytes() and np.array_equal(rec["index"], rec0["index"])
        r, w, _, _ = pfh.evaluate(rec["p"], rec["n"], rec["d"], rec["coeff"], at, a2, variant)
        if tag == "displaced":
            outside = r * r > a2
            assert outside.any() and (~outside).any(), "both branches of the loss must run"
        assert rec["residual"].tobytes() == r.tobytes(), (variant, tag, "residual", int((rec["residual"] != r).sum()))
        assert rec["weight"].tobytes() == w.tobytes(), (variant, tag, "weight", int((rec["weight"] != w).sum()))
    if variant != 0:
        slam.close()


# ---- sampling: 254 bytes are present and the records skip them ---------------------------------------------------------------------
def test_sampled_scan(oracle, gpu_slam_factory):
    sc, slam, om = _ctx(oracle, gpu_slam_factory, max_surface_features=2000)
    scan = np.ascontiguousarray(sc.scan(0), np.float32)
    rc, pose, st = slam.register(scan, sc.guess(0))
    assert rc == 0
    rec, status, resid, info = check_export(slam, scan, sc.guess(0), st, sc.plane_res, ocorrs=_oracle_corrs(oracle, om, scan, sc.guess(0), msf=2000), tag="sampled")
    assert (status == cref.NOT_SAMPLED).sum() == len(scan) - 2000 and not np.isin(rec["index"], np.flatnonzero(status == cref.NOT_SAMPLED)).any()
    slam.close()


# ---- paths: each gives the bytes of the default path --------------------------------------------------------------------------------
@pytest.mark.parametrize("env", ["SOICP_PERSISTENT", "SOICP_QUERY_WAVES", "SOICP_SPECULATE"])
def test_other_paths_give_the_same_bytes(oracle, gpu_slam_factory, tiny, monkeypatch, env):
    sc, slam0, _ = tiny
    scan = np.ascontiguousarray(sc.scan(0), np.float32)
    rc, pose0, st0 = slam0.register(scan, sc.guess(0))
    want = _export_bytes(slam0, len(scan))
    monkeypatch.setenv(env, "0")  # (read when the context is made)
    sc, slam, _ = _ctx(oracle, gpu_slam_factory, oracle_too=False)
    rc, pose, st = slam.register(scan, sc.guess(0))
    assert rc == 0
    if env == "SOICP_PERSISTENT":
        assert st.flags & 1
    if env == "SOICP_QUERY_WAVES":
        assert not (st.flags & 512) and (st0.flags & 512)
    assert _export_bytes(slam, len(scan)) == want
    slam.close()


# ---- entries ---------------------------------------------------------------------------------------------------------------------------
def test_register_dev_and_staged_stream(oracle, gpu_slam_factory, soicp):
    sc, slam, _ = _ctx(oracle, gpu_slam_factory, "small", oracle_too=False)
    scans = [slam.host_alloc_like(np.ascontiguousarray(sc.scan(i), np.float32)) for i in range(4)]
    guesses = [sc.guess(i) for i in range(4)]
    n = len(scans[2])
    rc, pose, st = slam.register(scans[2], guesses[2])
    assert rc == 0
    want = _export_bytes(slam, n)
    check_export(slam, np.asarray(scans[2]), guesses[2], st, sc.plane_res, tag="register on a host scan")
    d_scan, _ = slam.upload_scan(scans[2])
    rc, pose_d, st_d = slam.register_dev(d_scan, n, guesses[2])
    assert rc == 0 and _export_bytes(slam, n) == want, "register_dev"
    # the staged stream: the export is of the registered scan, also with the next scan announced (its copy, and its binning, in flight)
    got = run_staged_stream(slam, scans, guesses, [0, 1, 2])
    assert got[-1][0] == 0 and (got[-1][2].flags & soicp.FLAG_STAGED_SCAN)
    slam.stage_scan(scans[3])
    assert _export_bytes(slam, n) == want, "staged stream"
    check_export(slam, np.asarray(scans[2]), guesses[2], got[-1][2], sc.plane_res, tag="staged")
    slam.stage_cancel(scans[3])
    slam.close()


def test_localization_entries_export_after_the_insert(oracle, gpu_slam_factory):
    sc, slam, _ = _ctx(oracle, gpu_slam_factory, oracle_too=False)
    sc, ref, _ = _ctx(oracle, gpu_slam_factory, oracle_too=False)
    scan = np.ascontiguousarray(sc.scan(0), np.float32)
    rc, pose_r, st_r = ref.register(scan, sc.guess(0))
    want = _export_bytes(ref, len(scan))
    size0 = slam.map_size()
    rc, pose, st = slam.localization(True, sc.guess(0), scan, 0.1)
    assert rc == 0 and slam.map_size() != size0  # (the insert has completed: map_size settles it)
    assert _export_bytes(slam, len(scan)) == want, "so_icp_localization: the set of its registration, after the insert"
    check_export(slam, scan, sc.guess(0), st, sc.plane_res, tag="localization")
    # the node's order: pre-filter, then the resident entry on its output; a further pre-filter does not disturb the set
    raw = np.ascontiguousarray(sc.scan(1), np.float32)
    d_f, n_f, _ = slam.prefilter_scan(raw, False, sc.plane_res / 2, sc.plane_res)
    filtered = slam.download_scan(d_f, n_f)
    rc, pose, st = slam.localization_dev(True, sc.guess(1), d_f, n_f, 0.2)
    assert rc == 0
    slam.map_size()
    first = _export_bytes(slam, n_f)
    slam.prefilter_scan(np.ascontiguousarray(sc.scan(2), np.float32), False, sc.plane_res / 2, sc.plane_res)
    assert _export_bytes(slam, n_f) == first, "a further pre-filter overwrote the registered scan"
    check_export(slam, filtered, sc.guess(1), st, sc.plane_res, tag="prefilter + localization_dev")
    # nothing else invalidates the set: a Seam B query
    slam.nearest_k_search_surf(filtered[:16])
    assert _export_bytes(slam, n_f) == first
    slam.close(); ref.close()


@pytest.mark.parametrize("count", [3, 4])
@pytest.mark.parametrize("scene", ["tiny", "small"])
def test_register_sequence_exports_its_last_registration(oracle, gpu_slam_factory, scene, count):
    sc, slam, _ = _ctx(oracle, gpu_slam_factory, scene, oracle_too=False)
    ids = list(range(count))
    scans = [np.ascontiguousarray(sc.scan(i), np.float32) for i in ids]
    rc, poses, guesses, stats, n_done = slam.register_sequence(scans, sc.guess(0), chain_deltas(sc, ids))
    assert rc == 0 and n_done == count
    print(f"register_sequence {scene}: flags {[hex(st.flags) for st in stats]}, chained {slam.timing().seq_chained}")
    # (the chained path copies the exported scan behind the last report.  On these scenes every second registration is chained: the
    #  run of three ends with an ordinary start after a broken chain, the run of four with a chained registration)
    assert slam.timing().seq_chained >= count // 2
    last = count - 1
    rec, status, resid, info = check_export(slam, scans[last], guesses[last], stats[last], sc.plane_res, tag=f"register_sequence {scene} x {count}")
    want = _export_bytes(slam, len(scans[last]))
    # the same registration through the plain entry, from the guess the chain formed
    rc, pose, st = slam.register(scans[last], guesses[last])
    assert rc == 0 and np.array_equal(pose, poses[last])
    assert _export_bytes(slam, len(scans[last])) == want
    slam.close()


def test_localization_sequence_exports_its_last_frame(oracle, gpu_slam_factory):
    sc, slam, _ = _ctx(oracle, gpu_slam_factory, oracle_too=False)
    ids = [0, 1, 2]
    scans = [np.ascontiguousarray(sc.scan(i), np.float32) for i in ids]
    rc, poses, guesses, stats, n_done = slam.localization_sequence(scans, sc.guess(0), chain_deltas(sc, ids), [0.1, 0.2, 0.3])
    assert rc == 0 and n_done == 3
    check_export(slam, scans[2], guesses[2], stats[2], sc.plane_res, tag="localization_sequence")
    slam.close()


# ---- validity ------------------------------------------------------------------------------------------------------------------------
def _raw_call(slam, soicp, *, cap_records=0, cap_points=0, want_status=False):
    rec = np.full(max(cap_records, 1), 7, np.uint8).repeat(72)
    status = np.full(max(cap_points, 1), 9, np.uint8)
    info = soicp.CorrespondenceInfo()
    rc = slam.L.so_icp_correspondences(slam.h, None, rec.ctypes.data_as(C.c_void_p), cap_records, status.ctypes.data_as(C.POINTER(C.c_uint8)) if want_status else None,
                                       None, cap_points, None, C.byref(info))
    return rc, rec, status, info


def test_nothing_to_export(oracle, gpu_slam_factory, soicp):
    sc, slam, _ = _ctx(oracle, gpu_slam_factory, keep=False, oracle_too=False)
    scan = np.ascontiguousarray(sc.scan(0), np.float32)
    n = len(scan)

    def invalid(why):
        rc, rec, status, info = _raw_call(slam, soicp, cap_records=n, cap_points=n, want_status=True)
        assert rc == 0 and info.valid == 0 and info.n_points == 0 and info.n_accepted == 0, why
        assert np.all(rec == 7) and np.all(status == 9), (why, "outputs untouched")
    invalid("no registration yet, switch off")
    assert slam.register(scan, sc.guess(0))[0] == 0
    invalid("the switch was off during the last registration")
    assert slam.keep_correspondences(True) == 0
    invalid("switched on after the registration")
    assert slam.register(scan, sc.guess(0))[0] == 0
    rc, rec, status, info = _raw_call(slam, soicp, cap_records=n, cap_points=n, want_status=True)
    assert rc == 0 and info.valid == 1 and info.n_accepted > 0
    # counts only when the records do not fit; a per-point output needs room for every point
    rc, rec, status, info2 = _raw_call(slam, soicp, cap_records=int(info.n_accepted) - 1)
    assert rc == 0 and info2.valid == 1 and info2.n_accepted == info.n_accepted and info2.cost == info.cost and np.all(rec == 7)
    rc, rec, status, info2 = _raw_call(slam, soicp, cap_records=n, cap_points=n - 1, want_status=True)
    assert rc == -1 and np.all(status == 9)
    # a batch keeps its hypotheses' records elsewhere
    slam.register_batch(scan, np.stack([sc.guess(0), sc.guess(0)]))
    invalid("after so_icp_register_batch")
    assert slam.register(scan, sc.guess(0))[0] == 0 and _raw_call(slam, soicp)[3].valid == 1
    assert slam.keep_correspondences(False) == 0
    invalid("switched off")
    assert slam.keep_correspondences(True) == 0
    assert slam.register(scan, sc.guess(0))[0] == 0 and _raw_call(slam, soicp)[3].valid == 1
    # a seeding call (last: it moves the map's origin)
    assert slam.localization(False, sc.gt_pose(0), scan[:64], 0.0)[0] == 2
    invalid("after a seeding call")
    slam.close()
    # too little map
    empty = gpu_slam_factory(plane_res=sc.plane_res, max_surface_features=-1)
    assert empty.keep_correspondences(True) == 0
    assert empty.register(scan, sc.guess(0))[0] == 1  # SO_ICP_NOT_ENOUGH_MAP_FEATURES
    assert _raw_call(empty, soicp)[3].valid == 0
    empty.close()
    # contexts that do not have the feature
    sharded = gpu_slam_factory(plane_res=sc.plane_res, world_size=2, rank=0)
    assert sharded.keep_correspondences(True) == -5  # SO_ICP_E_UNSUPPORTED
    sharded.close()
    host = soicp.LidarSlamGpu(device_id=-1, plane_res=sc.plane_res)
    assert host.keep_correspondences(True) == -2     # SO_ICP_E_HIP
    assert _raw_call(host, soicp)[0] == -2
    host.close()


def test_switch_off_changes_nothing(oracle, gpu_slam_factory):
    sc, plain, _ = _ctx(oracle, gpu_slam_factory, "small", keep=False, oracle_too=False)
    sc, toggled, _ = _ctx(oracle, gpu_slam_factory, "small", keep=False, oracle_too=False)
    sc, on, _ = _ctx(oracle, gpu_slam_factory, "small", oracle_too=False)
    assert toggled.keep_correspondences(True) == 0 and toggled.keep_correspondences(False) == 0
    for i in range(3):
        scan = np.ascontiguousarray(sc.scan(i), np.float32)
        res = [s.register(scan, sc.guess(i)) for s in (plain, toggled, on)]
        for r, tag in zip(res[1:], ("turned on and off again", "on")):
            assert r[0] == res[0][0] == 0 and np.array_equal(r[1], res[0][1])
            assert_same_bits(r[2], res[0][2], tag)
    for s in (plain, toggled, on):
        s.close()


# ---- the adapter -------------------------------------------------------------------------------------------------------------------
def test_adapter_driver_correspondences(gpu_slam_factory, soicp, tmp_path):
    assert os.path.exists(DRIVER), "adapter/adapter_driver not built: run python __graft_entry__.py"
    sc = synth.Scene("tiny")
    n_frames, max_it = 3, 4
    scans = [np.ascontiguousarray(sc.scan(i), np.float32) for i in range(n_frames)]
    guesses = [sc.gt_pose(0)] + [sc.guess(i) for i in range(1, n_frames)]
    times = [0.1 * i for i in range(n_frames)]
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(fin, "wb") as f:
        f.write(struct.pack("<ifii", n_frames, sc.plane_res, max_it, -1))
        for i in range(n_frames):
            f.write(struct.pack("<i", len(scans[i])))
            f.write(np.asarray(guesses[i], np.float64).tobytes()); f.write(struct.pack("<d", times[i])); f.write(scans[i].tobytes())
    r = subprocess.run([DRIVER, str(fin), str(fout), "--correspondences"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    raw = open(fout, "rb").read()
    frame = struct.Struct("<5i7d2i7diI")
    off = n_frames * frame.size
    (n_map,) = struct.unpack_from("<Q", raw, off)
    off += 8 + 12 * n_map
    info_cpp = soicp.CorrespondenceInfo.from_buffer_copy(raw, off)
    off += C.sizeof(soicp.CorrespondenceInfo)
    assert info_cpp.valid == 1 and len(raw) == off + 72 * info_cpp.n_accepted
    slam = gpu_slam_factory(plane_res=sc.plane_res, line_res=sc.plane_res / 2, max_surface_features=-1, max_iterations=max_it)
    assert slam.keep_correspondences(True) == 0
    for i in range(n_frames):
        rc, pose, st = slam.localization(i > 0, guesses[i], scans[i], times[i])
    assert rc == 0
    rec, _, _, info = slam.correspondences(want_points=False, cap=len(scans[-1]))
    assert _info_bytes(info) == bytes(info_cpp) and rec.tobytes() == raw[off:]
    slam.close()
