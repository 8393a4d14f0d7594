"""-m gpu: point intensity through the scan pre-filter, the map insert and the map export (so_icp_set_cloud_intensity), against the
four-channel restatements of map_intensity_ref.py (whose inputs and properties test_map_intensity_host.py checks on the CPU).  Every
comparison is bit for bit, a NaN by its bit pattern; records are compared in ascending x y z, which no two rows of an input share."""
import numpy as np
import pytest

import map_edge_data as med
import map_intensity_ref as mir
import registered_scan_ref as rsr
from helpers import CorridorScene, assert_same_bits

pytestmark = pytest.mark.gpu
f32 = np.float32

MODES = {"default": {}, "host_rounds": {"SOICP_MAP_FAST": "0"}, "sync": {"SOICP_MAP_FAST": "sync"}, "sort": {"SOICP_MAP_GROUPING": "sort"}}


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def _same_records(got, want, tag):
    """uint8 [n, 32] records, both put into ascending x y z: x y z first (a point in the wrong place must not pass for a wrong
    intensity), then all 32 bytes"""
    assert got.shape == want.shape, (tag, got.shape, want.shape)
    g, w = mir.sorted_by_xyz(got), mir.sorted_by_xyz(want)
    assert np.array_equal(g[:, :12], w[:, :12]), (tag, "x y z differ")
    bad = np.nonzero((g != w).any(1))[0]
    assert len(bad) == 0, (tag, f"{len(bad)} of {len(g)} records differ; first: got {g[bad[0]].view(f32)} want {w[bad[0]].view(f32)}")


def _insert_all(slam, inp, on, stride32=True, after=None):
    """the input's inserts through so_icp_map_add_surf (stride 32 or 12), a resolution change where the input has one; after(step)"""
    if on:
        assert slam.set_cloud_intensity(16) == 0
    inside = []
    for step, (cloud, res) in enumerate(zip(inp.clouds, inp.plane_res)):
        if step and res != inp.plane_res[step - 1]:
            slam.set_resolution(res / 2, res)
        inside.append(slam.add_surf_records(mir.to_records(cloud)) if stride32 else slam.add_surf_point_cloud(cloud[:, :3]))
        if after:
            after(step)
    return inside


def _make(factory, inp):
    return factory(plane_res=inp.plane_res[0], line_res=inp.plane_res[0] / 2)


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", ["classes", "overflow", "cubes_33", "retable"])
def test_insert_parity_in_every_mode(gpu_slam_factory, monkeypatch, name, mode):
    """after every insert, the 32 bytes of every exported record are PlainMapI's"""
    inp = mir.get_input(name)
    exports, _ = mir.reference(name)
    for k, v in MODES[mode].items():
        monkeypatch.setenv(k, v)
    slam = _make(gpu_slam_factory, inp)

    def check(step):
        _same_records(slam.export_map_records(32), mir.xyzi_records(exports[step]), (name, mode, step))
    inside = _insert_all(slam, inp, True, after=check)
    assert inside == [len(c) for c in inp.clouds]
    built, handed_back = slam.map_insert_stats()
    print(name, mode, "inserts laid out by the device:", built, "handed back:", handed_back)
    if name == "overflow" and mode in ("default", "sync"):
        assert handed_back >= 1, "the leaf of 4 097 members sends its round to the sort path"
    # other record sizes: 16 bytes end with the 1.0f, 20 with the intensity, 12 are x y z
    r32 = mir.sorted_by_xyz(slam.export_map_records(32))
    for stride in (12, 16, 20, 48):
        r = mir.sorted_by_xyz(slam.export_map_records(stride))
        k = min(stride, 32)
        assert np.array_equal(r[:, :k], r32[:, :k]) and not r[:, k:].any(), (name, mode, stride)
    slam.close()


def test_stride_12_with_the_switch_on_inserts_intensity_zero(gpu_slam_factory):
    inp = mir.get_input("classes")
    slam, ref = _make(gpu_slam_factory, inp), _make(gpu_slam_factory, inp)
    _insert_all(slam, inp, True, stride32=False)
    _insert_all(ref, inp, False, stride32=False)
    rec, xyz = slam.export_map_records(32), ref.export_map()
    assert np.array_equal(rec[:, :12], xyz.view(np.uint8).reshape(-1, 12)), "same points in the same order"
    assert (rec[:, 12:16].copy().view(f32) == 1.0).all() and not rec[:, 16:].any()
    # a record too short for the intensity but not for x y z: 0 as well
    short = _make(gpu_slam_factory, inp)
    assert short.set_cloud_intensity(16) == 0
    for cloud in inp.clouds:
        short.add_surf_records(np.ascontiguousarray(mir.to_records(cloud)[:, :4]))
    assert np.array_equal(short.export_map_records(32), rec)
    for s in (slam, ref, short):
        s.close()


@pytest.fixture(scope="module")
def probes():
    rng = np.random.default_rng(5)
    inp = mir.get_input("classes")
    return np.ascontiguousarray(inp.clouds[0][::37, :3] + rng.uniform(-0.05, 0.05, (len(inp.clouds[0][::37]), 3)).astype(f32))


def _knn_bits(slam, q):
    found, nbr, d2, idx = slam.nearest_k_search_surf(q, 5)
    return found.tobytes(), _bits(nbr).tobytes(), _bits(d2).tobytes(), idx.tobytes()


@pytest.mark.parametrize("name", ["classes", "retable", "non_finite"])
def test_nothing_but_the_intensity_follows_the_switch(gpu_slam_factory, probes, name):
    """the same inserts with the switch on and off: packed export (order included), 5-NN of probes, insert statistics and counts are
    equal; the off context's records are zero behind x y z; a NaN or infinite intensity makes its leaves' intensity non-finite, theirs
    alone, and changes nothing else"""
    inp = mir.get_input(name)
    exports, _ = mir.reference(name)
    on, off = _make(gpu_slam_factory, inp), _make(gpu_slam_factory, inp)
    assert _insert_all(on, inp, True) == _insert_all(off, inp, False)
    a, b = on.export_map(), off.export_map()
    assert a.shape == b.shape and np.array_equal(_bits(a), _bits(b)), "x y z and their order"
    assert np.isfinite(a).all()
    assert on.map_size() == off.map_size() and on.map_insert_stats() == off.map_insert_stats()
    assert _knn_bits(on, probes) == _knn_bits(off, probes)
    r_off, r_on = off.export_map_records(32), on.export_map_records(32)
    assert np.array_equal(r_off[:, :12], r_on[:, :12]) and not r_off[:, 12:].any()
    _same_records(r_on, mir.xyzi_records(exports[-1]), (name, "switch on"))
    if name == "non_finite":
        inten = r_on[:, 16:20].copy().view(f32).reshape(-1)
        bad = np.nonzero(~np.isfinite(inten))[0]
        assert len(bad) == 4, inten[bad]
        xyz = r_on[bad, :12].copy().view(f32).reshape(-1, 3)
        want = np.array([mir.site_centre(k) for k in inp.poisoned])
        assert sorted(map(tuple, med.leaf_index(xyz, 0.2).tolist())) == sorted(map(tuple, med.leaf_index(want, 0.2).tolist()))
        assert sorted(np.isnan(inten[bad]).tolist()) == [False, False, True, True]
    # the switch changes between calls: what is in the map keeps its intensity, what arrives with the switch off has none
    assert on.set_cloud_intensity(-1) == 0
    extra = np.array([[30.11, 30.12, 3.13, 77.0, 88.0, 99.0, 1.0, 2.0]], f32)
    on.add_surf_records(extra)
    assert np.array_equal(on.export_map_records(32)[:, 12:], np.zeros((on.map_size(), 20), np.uint8)), "off: the records are today's"
    assert on.set_cloud_intensity(16) == 0
    r2 = mir.sorted_by_xyz(on.export_map_records(32))
    want = np.concatenate([mir.xyzi_records(exports[-1]), mir.xyzi_records(np.array([[30.11, 30.12, 3.13, 0.0]], f32))])
    _same_records(r2, want, (name, "after a point that came with the switch off"))
    on.close(); off.close()


def _upload_records(slam, rec):
    """float32 [n, w] records into HBM through upload_scan, which takes whole x y z triples"""
    flat = np.zeros(-(-rec.size // 3) * 3, f32)
    flat[:rec.size] = rec.reshape(-1)
    return slam.upload_scan(flat)[0]


@pytest.mark.parametrize("fast", ["1", "0"])
@pytest.mark.parametrize("name", ["pass_through", "leaves_of_64", "long_leaves"])
def test_prefilter_averages_the_intensity_per_leaf(gpu_slam_factory, monkeypatch, name, fast):
    pc = med.prefilter_cloud(name)
    monkeypatch.setenv("SOICP_PREFILTER_FAST", fast)
    xyzi, want = mir.prefilter_reference(name)
    rec = mir.to_records(xyzi)
    slam = gpu_slam_factory(plane_res=pc.plane_res, line_res=pc.line_res)
    d, n, _ = slam.prefilter_scan_records(rec, False, pc.line_res, pc.plane_res)
    plain = slam.download_scan(d, n)
    inten, d_i = slam.prefilter_intensity(n)
    assert len(inten) == 0 and d_i is None, "switch off: no intensities"
    assert slam.set_cloud_intensity(16) == 0
    d_rec = _upload_records(slam, rec)
    try:
        for entry in ("host", "dev"):
            if entry == "host":
                d, m, _ = slam.prefilter_scan_records(rec, False, pc.line_res, pc.plane_res)
            else:
                d, m, _ = slam.prefilter_scan_dev(d_rec, len(rec), 32, False, pc.line_res, pc.plane_res)
            got = slam.download_scan(d, m)
            assert m == n == len(want) and np.array_equal(_bits(got), _bits(plain)), (name, fast, entry, "x y z follow the switch-off run")
            assert np.array_equal(_bits(got), _bits(want[:, :3])), (name, fast, entry)
            inten, d_i = slam.prefilter_intensity(m)
            assert d_i is not None and np.array_equal(_bits(inten), _bits(want[:, 3])), (name, fast, entry, "intensities")
        # records without room for the intensity: zeros, one per output point
        d, m, _ = slam.prefilter_scan_records(np.ascontiguousarray(rec[:, :4]), False, pc.line_res, pc.plane_res)
        inten, _ = slam.prefilter_intensity(m)
        assert m == n and len(inten) == n and not inten.view(np.uint32).any()
        assert slam.set_cloud_intensity(-1) == 0
        d, m, _ = slam.prefilter_scan_records(rec, False, pc.line_res, pc.plane_res)
        assert len(slam.prefilter_intensity(m)[0]) == 0 and np.array_equal(_bits(slam.download_scan(d, m)), _bits(plain))
    finally:
        slam.free_scan(d_rec)
    slam.close()


# ------------------------------------------------------------------------------------------------------------------------
# Localization(): seed + 3 frames
# ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def corridor():
    sc = CorridorScene()
    scans = [mir.with_intensity_column(sc.scan(i), 100 + i) for i in range(4)]
    return sc, scans, [np.ascontiguousarray(mir.to_records(s)) for s in scans]


def _empty(factory, sc):
    return factory(plane_res=sc.plane_res, line_res=sc.plane_res / 2, max_surface_features=-1, max_iterations=3)


def _run_frames(slam, sc, recs, way):
    """seed with scan 0 at its ground truth, then frames 1..3 from their guesses; way: unstaged, staged, prefilter -> resident entry"""
    out = []
    bufs = [slam.host_alloc_like(r) for r in recs] if way == "staged" else recs
    for i in range(4):
        T = sc.gt_pose(0) if i == 0 else sc.guess(i)
        if way == "prefilter":
            d, n, _ = slam.prefilter_scan_records(recs[i], False, sc.plane_res / 2, sc.plane_res)
            res = slam.localization_dev(i > 0, T, d, n, 0.1 * i)
        else:
            if way == "staged" and i > 0:
                slam.stage_scan_records(bufs[i])
            res = slam.localization_records(i > 0, T, bufs[i], 0.1 * i)
        out.append(res)
    return out


def _reference_map(sc, clouds, frames):
    """PlainMapI fed with the frames' world points: the fp64 transform of registered_scan_ref.transform at the pose each frame returned
    (the seed: at the pose it was given), the window set by the seed and rolled by every frame's guess"""
    pm = mir.PlainMapI(sc.plane_res)
    for i, (cloud, (rc, pose, st)) in enumerate(zip(clouds, frames)):
        T = sc.gt_pose(0) if i == 0 else sc.guess(i)
        if i == 0:
            pm.set_origin(T[:3])
        else:
            pm.shift(T[:3])
        p = np.ascontiguousarray(cloud[:, :3])
        x, y, z = (p[:, k].astype(np.float64) for k in range(3))
        tx, ty, tz, qx, qy, qz, qw = (float(v) for v in (T if i == 0 else pose))
        ux, uy, uz = qy * z - qz * y, qz * x - qx * z, qx * y - qy * x
        ux, uy, uz = ux + ux, uy + uy, uz + uz
        w = np.stack([(x + qw * ux + (qy * uz - qz * uy)) + tx, (y + qw * uy + (qz * ux - qx * uz)) + ty,
                      (z + qw * uz + (qx * uy - qy * ux)) + tz], 1).astype(f32)
        wr, near, _ = rsr.transform(p, T if i == 0 else pose)  # (the same expressions; the node's "near the sensor" rule is not the insert's)
        assert np.array_equal(_bits(w[~near]), _bits(wr[~near]))
        pm.add(np.c_[w, cloud[:, 3]])
    return pm


def _same_frames(a, b, tag):
    for i, ((rc_a, pose_a, st_a), (rc_b, pose_b, st_b)) in enumerate(zip(a, b)):
        assert rc_a == rc_b and pose_a.tobytes() == pose_b.tobytes(), (tag, i, rc_a, rc_b)
        if i:
            assert_same_bits(st_a, st_b, (tag, i))


def test_localization_carries_the_intensity_staged_or_not(gpu_slam_factory, soicp, corridor):
    sc, scans, recs = corridor
    off = _empty(gpu_slam_factory, sc)
    frames_off = _run_frames(off, sc, recs, "unstaged")
    assert [f[0] for f in frames_off] == [soicp.MAP_SEEDED, 0, 0, 0]
    maps = {}
    for way in ("unstaged", "staged"):
        slam = _empty(gpu_slam_factory, sc)
        assert slam.set_cloud_intensity(16) == 0
        frames = _run_frames(slam, sc, recs, way)
        _same_frames(frames, frames_off, way)
        if way == "staged":
            assert all(f[2].flags & soicp.FLAG_STAGED_SCAN for f in frames[1:])
        assert np.array_equal(_bits(slam.export_map()), _bits(off.export_map())), (way, "map x y z follow the switch-off run")
        maps[way] = slam.export_map_records(32)
        slam.close()
    assert not off.export_map_records(32)[:, 12:].any()
    assert np.array_equal(maps["unstaged"], maps["staged"]), "staged and unstaged maps are byte-equal"
    pm = _reference_map(sc, scans, frames_off)
    _same_records(maps["unstaged"], pm.records(), "host scans")
    off.close()


def test_localization_dev_inserts_the_prefilters_intensities(gpu_slam_factory, soicp, corridor):
    sc, scans, recs = corridor
    off = _empty(gpu_slam_factory, sc)
    frames_off = _run_frames(off, sc, recs, "prefilter")
    assert [f[0] for f in frames_off] == [soicp.MAP_SEEDED, 0, 0, 0]
    slam = _empty(gpu_slam_factory, sc)
    assert slam.set_cloud_intensity(16) == 0
    frames = _run_frames(slam, sc, recs, "prefilter")
    _same_frames(frames, frames_off, "prefilter")
    assert np.array_equal(_bits(slam.export_map()), _bits(off.export_map()))
    filtered = [mir.voxel_grid_xyzi(s, sc.plane_res) for s in scans]
    pm = _reference_map(sc, filtered, frames_off)
    _same_records(slam.export_map_records(32), pm.records(), "pre-filtered scans through the resident entry")
    # any other resident scan inserts intensity 0: the same cloud uploaded by the caller
    other = _empty(gpu_slam_factory, sc)
    assert other.set_cloud_intensity(16) == 0
    for i in range(4):
        d, n = other.upload_scan(np.ascontiguousarray(filtered[i][:, :3]))
        other.localization_dev(i > 0, sc.gt_pose(0) if i == 0 else sc.guess(i), d, n, 0.1 * i)
    rec = other.export_map_records(32)
    assert np.array_equal(_bits(other.export_map()), _bits(off.export_map())) and (rec[:, 12:16].copy().view(f32) == 1.0).all() and not rec[:, 16:].any()
    for s in (off, slam, other):
        s.close()


# ------------------------------------------------------------------------------------------------------------------------
# the node shell: SOICP_NODE_MAP_INTENSITY
# ------------------------------------------------------------------------------------------------------------------------
def test_node_shell_publishes_the_prior_maps_intensities(tmp_path):
    """test_gpu_node.py::test_node_shell_localization_mode_against_a_prior_map with an intensity column in the .pcd: with
    SOICP_NODE_MAP_INTENSITY=1 the laser_cloud_map of frame 19 carries 1.0f at byte 12 and, where no scan point joined a prior point's
    leaf (the point is still there bit for bit), that point's intensity; without the variable the payload is x y z and zeros."""
    from scipy.spatial.transform import Rotation as R

    from superodom_amd import synth
    from test_gpu_node import P, by_frame, make_frames, run_node
    sc = synth.Scene("tiny")
    n_frames = 20
    frames = make_frames(sc, n_frames)
    g0 = sc.gt_pose(0)
    roll, pitch, yaw = R.from_quat(g0[3:]).as_euler("xyz")
    mp = np.ascontiguousarray(sc.map_points, f32)
    inten = np.random.default_rng(9).uniform(0.0, 255.0, len(mp)).astype(f32)
    pcd = tmp_path / "pointcloud_local.pcd"
    with open(pcd, "wb") as f:
        f.write((f"# .PCD v0.7 - Point Cloud Data file format\nVERSION 0.7\nFIELDS x y z intensity\nSIZE 4 4 4 4\nTYPE F F F F\nCOUNT 1 1 1 1\n"
                 f"WIDTH {len(mp)}\nHEIGHT 1\nVIEWPOINT 0 0 0 1 0 0 0\nPOINTS {len(mp)}\nDATA binary\n").encode())
        f.write(np.c_[mp, inten].astype("<f4").tobytes())
    params = tmp_path / "loc.yaml"
    params.write_text(f"/**:\n  ros__parameters:\n    laser_mapping_node:\n        mapping_line_resolution: {sc.plane_res / 2}\n"
                      f"        mapping_plane_resolution: {sc.plane_res}\n        max_iterations: 4\n        max_surface_features: -1\n"
                      f"        auto_voxel_size: false\n        localization_mode: true\n        init_x: {float(g0[0])!r}\n        init_y: {float(g0[1])!r}\n"
                      f"        init_z: {float(g0[2])!r}\n        init_roll: {float(roll)!r}\n        init_pitch: {float(pitch)!r}\n        init_yaw: {float(yaw)!r}\n"
                      f'    map_dir: "{pcd}"\n')
    payload = {}
    for on in (False, True):
        out = tmp_path / ("on" if on else "off")
        out.mkdir()
        pubs, failed, err = run_node(out, frames, 0.05, 0.05, 1, 7, params=params, env={"SOICP_NODE_MAP_INTENSITY": "1"} if on else None)
        assert failed == 0, err
        msgs, _ = by_frame(pubs, n_frames)
        m = msgs[19][P + "/laser_cloud_map"]
        assert m["point_step"] == 32
        payload[on] = np.frombuffer(m["data"], np.uint8).reshape(-1, 32)
    off, on = payload[False], payload[True]
    assert off.shape == on.shape and np.array_equal(off[:, :12], on[:, :12]), "the same map, in the same order"
    assert not off[:, 12:].any(), "without the variable: today's payload"
    assert (on[:, 12:16].copy().view(f32) == 1.0).all() and not on[:, 20:].any()
    prior = {p.tobytes(): v for p, v in zip(mp, inten)}
    assert len(prior) == len(mp)
    rows = [(i, prior[r.tobytes()]) for i, r in enumerate(on[:, :12]) if r.tobytes() in prior]
    assert len(rows) > len(mp) // 10, (len(rows), len(mp))
    got = on[[i for i, _ in rows], 16:20].copy().view(f32).reshape(-1)
    assert np.array_equal(_bits(got), _bits(np.array([v for _, v in rows], f32)))
    assert len(np.unique(on[:, 16:20].copy().view(np.uint32))) > len(rows) // 2
