"""-m gpu: so_icp_keep_correspondence_geometry / so_icp_correspondence_geometry -- per accepted correspondence of the last registration
the five neighbours it matched, the PCA of their scatter and the three observability labels, refitted on the device from the snapshot
the registration left: record for record against so_icp_correspondences, the refit's plane against its records bit for bit, the
histogram against the registration's own, the neighbours against so_icp_debug_neighbours, the map and a Seam B query, everything
against the oracle; through every registration entry and sweep / solve path; the snapshot against later map changes; and the cases in
which there is nothing to export.

Refit bits: through the test-only entry so_icp_debug_correspondence_refit (the 192-byte record stays as the issue states it).

Differences measured on an MI355X against the oracle, over every case below (tolerance 1e-12 for each, correspondence_geometry_ref.py):
profiles/correspondence_geometry/README.md."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import correspondence_geometry_ref as gref
import correspondences_ref as cref
import knn_edge_data as ked
from helpers import assert_same_bits, chain_deltas, run_staged_stream, scene_with_oracle
from superodom_amd import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "adapter", "adapter_driver")
TILE = 1024  # corr_kernels.h kCorrTile: the geometry export's own tile too
TOL_EIG, TOL_NORMAL, TOL_MEAN_ABS = (gref.gpu_tolerance(m) for m in (gref.EIG_REL_MEASURED, gref.NORMAL_MEASURED, gref.MEAN_ABS_MEASURED))


def _ctx(oracle, make, scene="tiny", keep=True, **cfg):
    cfg.setdefault("max_iterations", 5)
    sc, slam, om = scene_with_oracle(scene, oracle, make, **cfg)
    if keep:
        assert slam.keep_correspondences(True) == 0 and slam.keep_correspondence_geometry(True) == 0
    return sc, slam, om


@pytest.fixture(scope="module")
def tiny(oracle, gpu_slam_factory):
    sc, slam, om = _ctx(oracle, gpu_slam_factory)
    yield sc, slam, om, slam.export_map()
    slam.close()


def _export_bytes(slam, n):
    rec, labels, info = slam.correspondence_geometry(cap=n)
    return rec.tobytes(), labels.tobytes(), bytes(info)


_oracle_cache = {}


def _oracle_corrs(oracle, om, scan, guess, msf=-1, key=None):
    if key is None or key not in _oracle_cache:
        rc, pose, st, corrs = om.register(scan, guess, oracle.default_config(max_iterations=5, max_surface_features=msf), want_corrs=True)
        assert rc == 0
        if key is None:
            return corrs
        _oracle_cache[key] = corrs
    return _oracle_cache[key]


CAP_PER_SLOT = 1 << 20  # a canonical index of the device map is (slot of the cube) * 2^20 + position inside the cube (device_map.h)


def _export_rows(exp, nbr_index, nbr):
    """canonical indices [n, 5] -> rows of export_map(), which walks the cubes in window order and each cube by ascending position (as
    tests/test_gpu_knn_edges.py does it).  Which slot holds which cube is learnt from the neighbours' own coordinates and must be one
    consistent assignment; that the rows are the right ones is then settled by comparing their bits."""
    ec = ked.cube_of(exp)
    starts = np.nonzero(np.r_[True, (np.diff(ec, axis=0) != 0).any(1)])[0]
    offset = {tuple(ec[s]): int(s) for s in starts}
    assert len(offset) == len(starts), "export_map() lists every cube in one run"
    cube = ked.cube_of(nbr.reshape(-1, 3))
    slot = (nbr_index >> 20).ravel()
    slot_cube, off = {}, np.zeros(len(slot), np.int64)
    for i, (s_, c_) in enumerate(zip(slot.tolist(), map(tuple, cube.tolist()))):
        assert slot_cube.setdefault(s_, c_) == c_, "one cube per slot"
        off[i] = offset[c_]
    return (off + (nbr_index.ravel().astype(np.int64) & (CAP_PER_SLOT - 1))).reshape(nbr_index.shape)


def check_geometry(slam, scan, st, *, oracle=None, ocorrs=None, map_pts=None, knn=True, tag=""):
    """the common check, for the registration `st` of `scan` that `slam` ran last.  map_pts: export_map() as it was during that
    registration; knn: the map is still that map, so a Seam B query finds the same neighbours"""
    n = len(scan)
    rec, status, _, cinfo = slam.correspondences(cap=n)
    g, labels, info = slam.correspondence_geometry(cap=n)
    last = st.iterations[st.n_iterations - 1]
    # pairing and counts
    assert info.valid == 1 and cinfo.valid == 1 and info.n_points == n, (tag, info.valid, info.n_points)
    assert info.n_accepted == len(g) == last.num_surf_from_scan == len(rec), (tag, info.n_accepted, len(g), last.num_surf_from_scan)
    assert bytes(info.pose_fit) == bytes(cinfo.pose_fit) and info.outer_iteration == cinfo.outer_iteration == st.n_iterations - 1, tag
    assert np.array_equal(g["index"], rec["index"]), (tag, "index pairs with so_icp_correspondences")
    assert not g["reserved"].any() and not g["pad"].any(), tag
    idx = g["index"]
    # the refit's plane is the registration's, bit for bit
    refit = slam.debug_correspondence_refit(n)
    want = np.ascontiguousarray(np.concatenate([rec["n"], rec["d"][:, None], rec["coeff"][:, None]], axis=1))
    assert refit.shape == want.shape and refit.tobytes() == want.tobytes(), (tag, "refit n, d, coeff", int((refit != want).sum()))
    # histogram and labels
    hist = np.array(info.obs_hist)
    assert np.array_equal(hist, np.array(last.obs_hist)), (tag, hist, list(last.obs_hist))
    assert np.array_equal(hist, gref.hist_of(g["obs"])), (tag, "histogram of the records' labels")
    want_labels = np.full((n, 3), 255, np.uint8); want_labels[idx] = g["obs"]
    assert np.array_equal(labels, want_labels) and np.array_equal(labels[:, 0] != 255, status == 0), (tag, "labels_out")
    # neighbours
    assert np.array_equal(g["nbr_index"], slam.neighbours(n)[idx]), (tag, "so_icp_debug_neighbours")
    nbr = g["nbr"].reshape(-1, 5, 3)
    if map_pts is not None and len(g):
        assert nbr.tobytes() == np.ascontiguousarray(map_pts[_export_rows(map_pts, g["nbr_index"], nbr)]).tobytes(), (tag, "nbr = export_map()[nbr_index]")
    pose_fit = np.array(info.pose_fit)
    if len(g):
        err = np.abs(g["pw"] - gref.world(pose_fit, scan[idx])).max(1)
        assert np.all(err <= gref.pw_bound(scan[idx], pose_fit)), (tag, "pw", err.max())
        assert np.all(np.einsum("ij,ij->i", g["pca_normal"], g["pw"]) >= 0) and np.all(np.diff(g["eig"], axis=1) >= 0), tag
    if knn and len(g):
        found, k_nbr, k_d2, k_idx = slam.nearest_k_search_surf(g["pw"].astype(np.float32))
        assert found.all() and np.array_equal(k_idx.astype(np.uint32), g["nbr_index"]), (tag, "Seam B indices")
        assert k_nbr.tobytes() == nbr.tobytes() and k_d2.tobytes() == g["d2"].tobytes(), (tag, "Seam B neighbours and d2")
    # the oracle
    if ocorrs is not None:
        assert np.array_equal(np.flatnonzero(ocorrs["status"] == 0), idx), (tag, "accepted points against the oracle")
        o = ocorrs[idx]
        assert np.array_equal(hist, gref.hist_of(np.asarray(o["obs"])[:, :3])), (tag, "histogram against the oracle")
        if len(g):
            assert np.array_equal(g["obs"], np.asarray(o["obs"])[:, :3].astype(np.uint8)), (tag, "labels against the oracle", int((g["obs"] != np.asarray(o["obs"])[:, :3]).any(1).sum()))
            assert g["nbr"].tobytes() == np.ascontiguousarray(o["nbr"]).tobytes() and g["d2"].tobytes() == np.ascontiguousarray(o["d2"]).tobytes(), (tag, "nbr / d2 against the oracle")
            o_pw, o_eig, o_normal, o_mean_abs = gref.oracle_geometry(oracle, o, pose_fit)
            d = gref.differences(g["eig"], g["pca_normal"], g["mean_abs_dist"], o_eig, o_normal, o_mean_abs)
            print(f"{tag}: {len(g)} records, against the oracle: eig / eig[2] {d[0]:.3e}, pca normal {d[1]:.3e}, mean_abs_dist {d[2]:.3e}, "
                  f"pw {np.abs(g['pw'] - o_pw).max():.3e}")
            assert d[0] <= TOL_EIG and d[1] <= TOL_NORMAL and d[2] <= TOL_MEAN_ABS, (tag, d)
    # determinism, and the device copy of the records
    first = (g.tobytes(), labels.tobytes(), bytes(info))
    assert _export_bytes(slam, n) == first, (tag, "a second call returns identical bytes")
    d_rec, info_d = slam.correspondence_geometry_dev()
    assert bytes(info_d) == first[2]
    if len(g):
        assert slam.download_bytes(d_rec, 192 * len(g)).tobytes() == first[0], (tag, "d_records_out")
    return g, labels, info


# ---- sizes: prefixes of tiny's scan 0, each a real registration -------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, TILE - 1, TILE, TILE + 1, 4096])
def test_geometry_of_every_size(oracle, tiny, n):
    sc, slam, om, map_pts = tiny
    scan = np.ascontiguousarray(sc.scan(0)[:n], np.float32)
    rc, pose, st = slam.register(scan, sc.guess(0))
    assert rc == 0
    if n == 0:
        rec, labels, info = slam.correspondence_geometry(cap=0)
        assert info.valid == 1 and info.n_points == 0 and info.n_accepted == 0 and len(rec) == 0 and not any(info.obs_hist)
        return
    check_geometry(slam, scan, st, oracle=oracle, ocorrs=_oracle_corrs(oracle, om, scan, sc.guess(0), key=("tiny", n)), map_pts=map_pts, tag=f"n={n}")


def test_geometry_of_the_binned_sweep(oracle, gpu_slam_factory):
    sc, slam, om = _ctx(oracle, gpu_slam_factory, "small")
    scan = np.ascontiguousarray(sc.scan(0), np.float32)
    assert len(scan) == 16384
    rc, pose, st = slam.register(scan, sc.guess(0))
    assert rc == 0 and not (st.flags & 512)  # (not swept by query waves: binned)
    check_geometry(slam, scan, st, oracle=oracle, ocorrs=_oracle_corrs(oracle, om, scan, sc.guess(0)), map_pts=slam.export_map(), tag="small")
    slam.close()


def test_sampled_scan(oracle, gpu_slam_factory):
    sc, slam, om = _ctx(oracle, gpu_slam_factory, max_surface_features=2000)
    scan = np.ascontiguousarray(sc.scan(0), np.float32)
    rc, pose, st = slam.register(scan, sc.guess(0))
    assert rc == 0
    g, labels, info = check_geometry(slam, scan, st, oracle=oracle, ocorrs=_oracle_corrs(oracle, om, scan, sc.guess(0), msf=2000), map_pts=slam.export_map(), tag="sampled")
    assert 0 < len(g) <= 2000 and (labels[:, 0] == 255).sum() >= len(scan) - 2000
    slam.close()


def test_whole_tiles_rejected(oracle, tiny):
    sc, slam, om, map_pts = tiny
    scan, far = cref.composite_scan(np.ascontiguousarray(sc.scan(0), np.float32), TILE)
    rc, pose, st = slam.register(scan, sc.guess(0))
    assert rc == 0
    g, labels, info = check_geometry(slam, scan, st, oracle=oracle, ocorrs=_oracle_corrs(oracle, om, scan, sc.guess(0)), map_pts=map_pts, tag="composite")
    assert np.all(labels[far] == 255) and np.all(labels[TILE:2 * TILE] == 255) and not np.isin(g["index"], np.flatnonzero(far)).any(), "a whole tile without an accepted point"


# ---- paths: each gives the bytes of the default path --------------------------------------------------------------------------------
@pytest.mark.parametrize("env", ["SOICP_PERSISTENT", "SOICP_QUERY_WAVES", "SOICP_SPECULATE"])
def test_other_paths_give_the_same_bytes(oracle, gpu_slam_factory, tiny, monkeypatch, env):
    sc, slam0, _, _ = tiny
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
    check_geometry(slam, scan, st, map_pts=slam.export_map(), tag=f"{env}=0")
    slam.close()


# ---- entries ---------------------------------------------------------------------------------------------------------------------------
def test_register_dev_and_staged_stream(oracle, gpu_slam_factory, soicp):
    sc, slam, _ = _ctx(oracle, gpu_slam_factory, "small", oracle_too=False)
    map_pts = slam.export_map()
    scans = [slam.host_alloc_like(np.ascontiguousarray(sc.scan(i), np.float32)) for i in range(4)]
    guesses = [sc.guess(i) for i in range(4)]
    n = len(scans[2])
    rc, pose, st = slam.register(scans[2], guesses[2])
    assert rc == 0
    want = _export_bytes(slam, n)
    d_scan, _ = slam.upload_scan(scans[2])
    rc, pose_d, st_d = slam.register_dev(d_scan, n, guesses[2])
    assert rc == 0 and _export_bytes(slam, n) == want, "register_dev"
    check_geometry(slam, np.asarray(scans[2]), st_d, map_pts=map_pts, tag="register_dev")
    # the staged stream: the export is of the registered scan, also with the next scan announced (its copy, and its binning, in flight)
    got = run_staged_stream(slam, scans, guesses, [0, 1, 2])
    assert got[-1][0] == 0 and (got[-1][2].flags & soicp.FLAG_STAGED_SCAN)
    slam.stage_scan(scans[3])
    assert _export_bytes(slam, n) == want, "staged stream"
    check_geometry(slam, np.asarray(scans[2]), got[-1][2], map_pts=map_pts, tag="staged")
    slam.stage_cancel(scans[3])
    slam.close()


def test_match_leaves_the_geometry_at_its_pose(oracle, tiny):
    sc, slam, om, map_pts = tiny
    scan = np.ascontiguousarray(sc.scan(1), np.float32)
    pose = np.asarray(sc.guess(1), np.float64)
    rc, st = slam.match(scan, pose)
    assert rc == 0 and st.n_iterations == 1
    g, labels, info = check_geometry(slam, scan, st, map_pts=map_pts, tag="match")
    assert info.outer_iteration == 0 and np.array(info.pose_fit).tobytes() == pose.tobytes() and len(g) > 500


@pytest.mark.parametrize("count", [3, 4])
@pytest.mark.parametrize("scene", ["tiny", "small"])
def test_register_sequence_leaves_its_last_registration(oracle, gpu_slam_factory, soicp, scene, count):
    sc, slam, _ = _ctx(oracle, gpu_slam_factory, scene, oracle_too=False)
    map_pts = slam.export_map()
    ids = list(range(count))
    scans = [np.ascontiguousarray(sc.scan(i), np.float32) for i in ids]
    rc, poses, guesses, stats, n_done = slam.register_sequence(scans, sc.guess(0), chain_deltas(sc, ids))
    assert rc == 0 and n_done == count
    last = count - 1
    print(f"register_sequence {scene} x {count}: flags {[hex(st.flags) for st in stats]}, chained {slam.timing().seq_chained}")
    # (on these scenes every second registration is chained: the run of four ends with a chained registration, whose snapshot is taken
    #  behind its report beside the scan copy; the run of three with an ordinary start after a broken chain)
    assert slam.timing().seq_chained >= count // 2
    if count == 4:
        assert stats[last].flags & soicp.FLAG_CHAINED, "the last registration of the run of four must be a chained one"
    check_geometry(slam, scans[last], stats[last], map_pts=map_pts, tag=f"register_sequence {scene} x {count}")
    want = _export_bytes(slam, len(scans[last]))
    # the same registration through the plain entry, from the guess the chain formed
    rc, pose, st = slam.register(scans[last], guesses[last])
    assert rc == 0 and np.array_equal(pose, poses[last])
    assert _export_bytes(slam, len(scans[last])) == want
    slam.close()


def test_localization_sequence_leaves_its_last_frame(oracle, gpu_slam_factory):
    sc, slam, _ = _ctx(oracle, gpu_slam_factory, oracle_too=False)
    ids = [0, 1, 2]
    scans = [np.ascontiguousarray(sc.scan(i), np.float32) for i in ids]
    rc, poses, guesses, stats, n_done = slam.localization_sequence(scans, sc.guess(0), chain_deltas(sc, ids), [0.1, 0.2, 0.3])
    assert rc == 0 and n_done == 3
    slam.map_size()  # (the last frame's insert has completed)
    # (the map has taken three scans since: neither the map as it was nor a Seam B query can be compared any more)
    check_geometry(slam, scans[2], stats[2], knn=False, tag="localization_sequence")
    slam.close()


# ---- the snapshot is a snapshot ----------------------------------------------------------------------------------------------------------
def test_localization_exports_what_its_registration_read(oracle, gpu_slam_factory):
    sc, slam, _ = _ctx(oracle, gpu_slam_factory, oracle_too=False)
    sc, twin, _ = _ctx(oracle, gpu_slam_factory, oracle_too=False)
    scan = np.ascontiguousarray(sc.scan(0), np.float32)
    map_pts = twin.export_map()
    rc, pose_t, st_t = twin.register(scan, sc.guess(0))
    assert rc == 0
    want = _export_bytes(twin, len(scan))
    size0 = slam.map_size()
    rc, pose, st = slam.localization(True, sc.guess(0), scan, 0.1)
    assert rc == 0 and slam.map_size() != size0  # (the insert has completed: map_size settles it)
    assert _export_bytes(slam, len(scan)) == want, "so_icp_localization: the bytes of the twin that never inserted"
    check_geometry(slam, scan, st, map_pts=map_pts, knn=False, tag="localization")
    slam.close(); twin.close()


def test_a_later_map_insert_does_not_change_the_export(oracle, gpu_slam_factory):
    sc, slam, _ = _ctx(oracle, gpu_slam_factory, oracle_too=False)
    map_pts = slam.export_map()
    scan = np.ascontiguousarray(sc.scan(2), np.float32)
    rc, pose, st = slam.register(scan, sc.guess(2))
    assert rc == 0
    a = _export_bytes(slam, len(scan))
    # a cloud into the cubes the registration touched: the scan itself at its registered pose, shifted by a third of a voxel
    cloud = (gref.world(pose, scan) + sc.plane_res / 3).astype(np.float32)
    size0 = slam.map_size()
    slam.add_surf_point_cloud(cloud)
    changed = slam.export_map()
    assert slam.map_size() != size0 and (len(changed) != len(map_pts) or changed.tobytes() != map_pts.tobytes())
    assert _export_bytes(slam, len(scan)) == a, "export B (after so_icp_map_add_surf) equals export A"
    check_geometry(slam, scan, st, map_pts=map_pts, knn=False, tag="after so_icp_map_add_surf")
    slam.close()


# ---- validity ------------------------------------------------------------------------------------------------------------------------
def _raw_call(slam, soicp, *, cap_records=0, cap_points=0, want_labels=False):
    rec = np.full(max(cap_records, 1), 7, np.uint8).repeat(192)
    labels = np.full(3 * max(cap_points, 1), 9, np.uint8)
    info = soicp.CorrespondenceGeometryInfo()
    rc = slam.L.so_icp_correspondence_geometry(slam.h, rec.ctypes.data_as(C.c_void_p), cap_records, labels.ctypes.data_as(C.POINTER(C.c_uint8)) if want_labels else None,
                                               cap_points, None, C.byref(info))
    return rc, rec, labels, info


def test_nothing_to_export(oracle, gpu_slam_factory, soicp):
    sc, slam, _ = _ctx(oracle, gpu_slam_factory, keep=False, oracle_too=False)
    scan = np.ascontiguousarray(sc.scan(0), np.float32)
    n = len(scan)

    def invalid(why):
        rc, rec, labels, info = _raw_call(slam, soicp, cap_records=n, cap_points=n, want_labels=True)
        assert rc == 0 and info.valid == 0 and info.n_points == 0 and info.n_accepted == 0 and not any(info.obs_hist), why
        assert np.all(rec == 7) and np.all(labels == 9), (why, "outputs untouched")
    invalid("no registration yet, switches off")
    assert slam.keep_correspondence_geometry(True) == -1, "the switch without keep_correspondences: SO_ICP_E_INVALID"
    assert slam.register(scan, sc.guess(0))[0] == 0
    invalid("keep_correspondences off")
    assert slam.keep_correspondences(True) == 0
    assert slam.register(scan, sc.guess(0))[0] == 0 and slam.correspondences(cap=n)[3].valid == 1
    invalid("this switch off during the registration")
    assert slam.keep_correspondence_geometry(True) == 0
    invalid("switched on after the registration")
    assert slam.register(scan, sc.guess(0))[0] == 0
    rc, rec, labels, info = _raw_call(slam, soicp, cap_records=n, cap_points=n, want_labels=True)
    assert rc == 0 and info.valid == 1 and info.n_accepted > 0
    # counts only when the records do not fit; labels_out needs room for every point
    rc, rec, labels, info2 = _raw_call(slam, soicp, cap_records=int(info.n_accepted) - 1)
    assert rc == 0 and info2.valid == 1 and info2.n_accepted == info.n_accepted and list(info2.obs_hist) == list(info.obs_hist) and np.all(rec == 7)
    rc, rec, labels, info2 = _raw_call(slam, soicp, cap_records=n, cap_points=n - 1, want_labels=True)
    assert rc == -1 and np.all(labels == 9)
    # a batch keeps its hypotheses' records elsewhere
    slam.register_batch(scan, np.stack([sc.guess(0), sc.guess(0)]))
    invalid("after so_icp_register_batch")
    assert slam.register(scan, sc.guess(0))[0] == 0 and _raw_call(slam, soicp)[3].valid == 1
    # turning keep_correspondences off turns this switch off too
    assert slam.keep_correspondences(False) == 0
    invalid("keep_correspondences switched off")
    assert slam.keep_correspondences(True) == 0
    assert slam.register(scan, sc.guess(0))[0] == 0 and slam.correspondences(cap=n)[3].valid == 1
    invalid("keep_correspondences on again: this switch stayed off")
    assert slam.keep_correspondence_geometry(True) == 0
    assert slam.register(scan, sc.guess(0))[0] == 0 and _raw_call(slam, soicp)[3].valid == 1
    # a seeding call (last: it moves the map's origin)
    assert slam.localization(False, sc.gt_pose(0), scan[:64], 0.0)[0] == 2
    invalid("after a seeding call (SO_ICP_MAP_SEEDED)")
    slam.close()
    # too little map
    empty = gpu_slam_factory(plane_res=sc.plane_res, max_surface_features=-1)
    assert empty.keep_correspondences(True) == 0 and empty.keep_correspondence_geometry(True) == 0
    assert empty.register(scan, sc.guess(0))[0] == 1  # SO_ICP_NOT_ENOUGH_MAP_FEATURES
    assert _raw_call(empty, soicp)[3].valid == 0
    empty.close()
    # contexts that do not have the feature
    sharded = gpu_slam_factory(plane_res=sc.plane_res, world_size=2, rank=0)
    assert sharded.keep_correspondence_geometry(True) == -5  # SO_ICP_E_UNSUPPORTED
    sharded.close()
    host = soicp.LidarSlamGpu(device_id=-1, plane_res=sc.plane_res)
    assert host.keep_correspondence_geometry(True) == -2     # SO_ICP_E_HIP
    assert _raw_call(host, soicp)[0] == -2
    host.close()


def test_switch_off_changes_nothing(oracle, gpu_slam_factory):
    sc, plain, _ = _ctx(oracle, gpu_slam_factory, "small", keep=False, oracle_too=False)
    sc, toggled, _ = _ctx(oracle, gpu_slam_factory, "small", keep=False, oracle_too=False)
    sc, on, _ = _ctx(oracle, gpu_slam_factory, "small", oracle_too=False)
    assert plain.keep_correspondences(True) == 0
    assert toggled.keep_correspondences(True) == 0 and toggled.keep_correspondence_geometry(True) == 0 and toggled.keep_correspondence_geometry(False) == 0
    for i in range(3):
        scan = np.ascontiguousarray(sc.scan(i), np.float32)
        res = [s.register(scan, sc.guess(i)) for s in (plain, toggled, on)]
        want = plain.correspondences(cap=len(scan))
        for s, r, tag in zip((toggled, on), res[1:], ("turned on and off again", "on")):
            assert r[0] == res[0][0] == 0 and np.array_equal(r[1], res[0][1])
            assert_same_bits(r[2], res[0][2], tag)
            got = s.correspondences(cap=len(scan))
            assert all(a.tobytes() == b.tobytes() for a, b in zip(got[:3], want[:3])) and bytes(got[3]) == bytes(want[3]), (tag, "so_icp_correspondences")
        assert toggled.correspondence_geometry(cap=len(scan))[2].valid == 0
    for s in (plain, toggled, on):
        s.close()


# ---- the adapter -------------------------------------------------------------------------------------------------------------------
def test_adapter_driver_geometry(gpu_slam_factory, soicp, tmp_path):
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
    r = subprocess.run([DRIVER, str(fin), str(fout), "--geometry"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    lines = [l for l in r.stdout.splitlines() if "geometry" in l]
    assert len(lines) == n_frames - 1, r.stdout
    slam = gpu_slam_factory(plane_res=sc.plane_res, line_res=sc.plane_res / 2, max_surface_features=-1, max_iterations=max_it)
    assert slam.keep_correspondences(True) == 0 and slam.keep_correspondence_geometry(True) == 0
    for i in range(n_frames):
        rc, pose, st = slam.localization(i > 0, guesses[i], scans[i], times[i])
        assert rc == (0 if i else 2)
        if not i:
            continue
        rec, _, info = slam.correspondence_geometry(want_points=False, cap=len(scans[i]))
        hist = " ".join(str(v) for v in info.obs_hist)
        assert info.valid == 1 and list(info.obs_hist) == list(st.iterations[st.n_iterations - 1].obs_hist)
        assert lines[i - 1] == f"frame {i}: geometry valid 1 n_accepted {info.n_accepted} records {len(rec)} obs_hist {hist} | stats {hist}", (lines[i - 1], hist)
    slam.close()
