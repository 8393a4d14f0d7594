"""-m gpu: the path-directed map and pre-filter inputs (map_edge_data.py; their properties are asserted on the CPU by
test_map_edges_host.py) through the device-resident LocalMap and so_icp_prefilter_scan, against the oracle's OWN map: the oracle
receives the same clouds, never the device's export, so a point the device files in the wrong cube shows -- in the insert's return
value, in the export, and in the 5-NN lists of the probes, which never leave the query's cube.  Every comparison is bit for bit."""
import numpy as np
import pytest

import map_edge_data as med

pytestmark = pytest.mark.gpu

# (environment, is the map held on the device): every round laid out by the device / by the host, the sort-based first stage, the host map
MODES = {"default": ({}, True), "host_rounds": ({"SOICP_MAP_FAST": "0"}, True), "sort": ({"SOICP_MAP_GROUPING": "sort"}, True),
         "host_map": ({"SOICP_HOST_MAP": "1"}, False)}


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _sorted(a):
    return a[np.lexsort(a.T)]


def _pair(oracle, make, fam):
    """a device map and an oracle map set up the way the family asks"""
    res = fam.create_res or fam.plane_res
    slam, om = make(plane_res=res, line_res=res / 2), oracle.OracleMap(plane_res=res, line_res=res / 2)
    if fam.window_t is not None:
        t = np.array(fam.window_t)
        assert list(slam.set_origin(t)) == list(om.set_origin(t)) == list(med.origin_after_set(t))
        assert list(slam.shift_map(t)) == list(om.shift(t)) == list(med.shift(med.origin_after_set(t), t)[1])
    if fam.create_res:
        assert slam.add_surf_point_cloud(fam.warmup) == om.add_surf(fam.warmup)
        slam.set_resolution(fam.plane_res / 2, fam.plane_res); om.set_resolution(fam.plane_res / 2, fam.plane_res)
    assert list(slam.origin()) == list(om.origin()) == list(fam.origin())
    return slam, om


def _follows_the_oracle(fam, slam, om, tag):
    """The one comparison of a device map with the oracle's own: after every insert the return value, the size and the sorted export;
    at the end the 5-NN of every probe (found flags, bits of d2, neighbour coordinates) and count_5x5 at every probed cube.
    Returns the exports (device order)."""
    exports = []
    for step, cloud in enumerate(fam.clouds):
        got, want = slam.add_surf_point_cloud(cloud), om.add_surf(cloud)
        assert got == want, (tag, step, "points inside the window", got, want)
        assert slam.map_size() == om.size(), (tag, step, slam.map_size(), om.size())
        e = slam.export_map()
        assert len(e) == om.size() and np.array_equal(_bits(_sorted(e)), _bits(_sorted(om.export()))), (tag, step, "export")
        exports.append(e)
    assert np.isfinite(exports[-1]).all(), tag
    found, nbr, d2, _ = slam.nearest_k_search_surf(fam.probes, 5)
    of, onbr, od2, _, _ = om.knn(fam.probes, 5, use_grid=1)
    bad = np.nonzero(found != of)[0]
    assert len(bad) == 0, (tag, f"found differs at {len(bad)} probes; first: {fam.probes[bad[0]]} device {found[bad[0]]} oracle {of[bad[0]]}")
    f = of.astype(bool)
    bad = np.nonzero((_bits(d2[f]) != _bits(od2[f])).any(1) | (_bits(nbr[f]) != _bits(onbr[f])).any(axis=(1, 2)))[0]
    assert len(bad) == 0, (tag, f"{len(bad)} of {int(f.sum())} lists differ; first: probe {fam.probes[f][bad[0]]}", nbr[f][bad[0]], onbr[f][bad[0]])
    for pos in fam.probe_positions():
        assert slam.count_5x5(pos) == om.count_5x5(pos), (tag, pos)
    return exports


@pytest.mark.parametrize("name", list(med.SMALL_FAMILIES))
def test_insert_family_follows_the_oracle(oracle, gpu_slam_factory, monkeypatch, name):
    """Every insert family in the default mode; cube_faces, window_edge, non_finite and rounds also with every round laid out by the host,
    with the sort-based first stage and on the host map.  The device modes leave the same map in the same order."""
    fam = med.family(name)
    exports = {}
    for mode in (MODES if name in med.EVERY_MODE else ["default"]):
        env, on_device = MODES[mode]
        with monkeypatch.context() as mp:
            for k, v in env.items():
                mp.setenv(k, v)
            slam, om = _pair(oracle, gpu_slam_factory, fam)
            out = _follows_the_oracle(fam, slam, om, (name, mode))
            slam.close()
        if on_device:
            exports[mode] = out
    for mode, out in exports.items():
        for step, (a, b) in enumerate(zip(exports["default"], out)):
            assert np.array_equal(_bits(a), _bits(b)), f"{name}, insert {step}: mode {mode} left another map (or order) than the default mode"


def test_non_finite_queries_find_nothing(oracle, gpu_slam_factory):
    """NaN and infinite query rows report found == 0, as the reference's cube rule does on x86-64, and leave the other rows as they are"""
    fam = med.family("non_finite")
    slam, om = _pair(oracle, gpu_slam_factory, fam)
    for cloud, bad in zip(fam.clouds, fam.info["bad_rows"]):  # (the finite rows only: this test is about the queries)
        assert slam.add_surf_point_cloud(cloud[~bad]) == om.add_surf(cloud[~bad]) == int((~bad).sum())
    q = np.ascontiguousarray(fam.probes[:128]).copy()
    plain = slam.nearest_k_search_surf(q, 5)
    rows = [0, 5, 63, 64, 70, 100, 127]
    values = [np.nan, np.inf, -np.inf, np.nan, np.inf, -np.inf, np.nan]
    for r, v in zip(rows, values):
        q[r, r % 3] = v
    q[100] = np.nan
    found, nbr, d2, _ = slam.nearest_k_search_surf(q, 5)
    of, onbr, od2, _, _ = om.knn(q, 5, use_grid=1)
    assert not of[rows].any() and of.sum() == len(q) - len(rows)
    assert np.array_equal(found, of), ("found", found[rows])
    keep = np.setdiff1d(np.arange(len(q)), rows)
    assert np.array_equal(_bits(d2[keep]), _bits(plain[2][keep])) and np.array_equal(_bits(nbr[keep]), _bits(plain[1][keep]))
    assert np.array_equal(_bits(d2[keep]), _bits(od2[keep])) and np.array_equal(_bits(nbr[keep]), _bits(onbr[keep]))
    slam.close()


@pytest.mark.parametrize("name", list(med.ESCAPE_FAMILIES))
def test_centroid_outside_its_cube_stays_in_its_cube(oracle, gpu_slam_factory, monkeypatch, name):
    """400 000 points of one leaf whose float centroid lands 0.48 m beyond the cube's face (2.4 to 9.6 leaves: more than the two leaves
    of margin of the insert's leaf keys): the centroid stays a point of the cube it was summed in through the inserts that follow."""
    fam = med.family(name)
    exports = []
    for mode in ("default", "sort"):
        with monkeypatch.context() as mp:
            for k, v in MODES[mode][0].items():
                mp.setenv(k, v)
            slam, om = _pair(oracle, gpu_slam_factory, fam)
            exports.append(_follows_the_oracle(fam, slam, om, (name, mode)))
            # the centroid itself, asked from inside its cube and from the cube it lies in
            q = np.array([fam.info["inside"], fam.info["centroid"]], np.float32)
            found, nbr, d2, _ = slam.nearest_k_search_surf(q, 1)
            of, onbr, od2, _, _ = om.knn(q, 1, use_grid=1)
            assert np.array_equal(found, of) and np.array_equal(_bits(nbr), _bits(onbr)) and np.array_equal(_bits(d2), _bits(od2))
            slam.close()
    assert np.array_equal(_bits(exports[0][0]), _bits(fam.info["centroid"][None]))
    for a, b in zip(*exports):
        assert np.array_equal(_bits(a), _bits(b)), f"{name}: the two first stages left different maps (or orders)"


INFO_FIELDS = ("average_distance", "count_far_points", "increase_blind_radius", "line_res", "plane_res", "statistic_in_input_order")


@pytest.mark.parametrize("name", list(med.PREFILTER))
def test_prefilter_follows_the_voxel_grid_restatement(oracle, gpu_slam_factory, monkeypatch, name):
    """so_icp_prefilter_scan decided on the device and decided on the host (SOICP_PREFILTER_FAST=0), with and without auto_voxel_size:
    the filtered cloud is the oracle's pcl::VoxelGrid of the cloud at the resolution the call reports, the two modes report the same."""
    pc = med.prefilter_cloud(name)
    want = {}
    outs = []
    for fast in ("1", "0"):
        monkeypatch.setenv("SOICP_PREFILTER_FAST", fast)
        slam = gpu_slam_factory(plane_res=pc.plane_res, line_res=pc.line_res)
        res = []
        for auto in (True, False):
            slam.set_resolution(pc.line_res, pc.plane_res)
            d, n, info = slam.prefilter_scan(pc.cloud, auto, pc.line_res, pc.plane_res)
            got = slam.download_scan(d, n)
            leaf = float(info.plane_res)
            if not auto:
                assert abs(leaf - pc.plane_res) < 1e-7
            if leaf not in want:
                want[leaf] = oracle.voxel_grid(pc.cloud, leaf)
            assert n == len(want[leaf]) and np.array_equal(_bits(got), _bits(want[leaf])), (name, fast, auto, leaf, n, len(want[leaf]))
            if name in med.PASS_THROUGH and not auto or name.startswith("pass_through"):
                assert n == len(pc.cloud) and np.array_equal(_bits(got), _bits(pc.cloud)), (name, fast, auto, "the cloud passes through")
            res.append((got,) + tuple(getattr(info, k) for k in INFO_FIELDS))
        outs.append(res)
        slam.close()
    for a, b in zip(*outs):
        assert np.array_equal(_bits(a[0]), _bits(b[0])) and a[1:] == b[1:], (name, a[1:], b[1:])


def test_pass_through_from_a_resident_cloud_and_into_localization(oracle, gpu_slam_factory, soicp):
    """The pass-through of a cloud that is already on the device, as records of 16 bytes (the strided device-to-device copy), equals the
    host entry's; and a passed-through cloud, outliers 900 m away included, goes through so_icp_localization_dev like any other."""
    pc = med.prefilter_cloud("pass_through")
    n = len(pc.cloud)
    slam = gpu_slam_factory(plane_res=pc.plane_res, line_res=pc.line_res, max_iterations=2)
    rec = np.zeros((n, 4), np.float32)
    rec[:, :3] = pc.cloud; rec[:, 3] = 77.0
    flat = np.zeros(-(-n * 4 // 3) * 3, np.float32)  # (upload_scan takes whole xyz triples)
    flat[:n * 4] = rec.reshape(-1)
    d_rec, _ = slam.upload_scan(flat)
    try:
        for auto in (True, False):
            slam.set_resolution(pc.line_res, pc.plane_res)
            d, m, info = slam.prefilter_scan_dev(d_rec, n, 16, auto, pc.line_res, pc.plane_res)
            got = slam.download_scan(d, m)
            slam.set_resolution(pc.line_res, pc.plane_res)
            d_h, m_h, info_h = slam.prefilter_scan(pc.cloud, auto, pc.line_res, pc.plane_res)
            assert m == m_h == n and np.array_equal(_bits(got), _bits(pc.cloud)) and np.array_equal(_bits(slam.download_scan(d_h, m_h)), _bits(pc.cloud))
            assert all(getattr(info, k) == getattr(info_h, k) for k in INFO_FIELDS)
    finally:
        slam.free_scan(d_rec)
    rng = np.random.default_rng(3)
    floor = np.c_[rng.uniform(-8, 8, (20000, 2)), rng.normal(-1.0, 0.01, 20000)].astype(np.float32)
    assert slam.add_surf_point_cloud(floor) == len(floor)
    d, m, _ = slam.prefilter_scan(pc.cloud, False, pc.line_res, pc.plane_res)
    assert m == n
    size = slam.map_size()
    try:
        rc, pose, st = slam.localization_dev(True, np.array([0, 0, 0, 0, 0, 0, 1.0]), d, m, 0.1)
    except soicp.SoIcpError as e:  # (an error code is an answer too; a fault would not come back)
        rc = str(e)
    print("localization_dev on a passed-through cloud:", rc)
    assert slam.map_size() >= size and np.isfinite(slam.export_map()).all()
    slam.close()


def test_origin_and_shift_on_cube_faces(oracle, gpu_slam_factory):
    """set_origin / shift_map with translations on the listed faces and one float to either side: the triples are the oracle's and the
    restatement's (the face itself of a negative face belongs to the cube below: truncate, then decrement)"""
    slam, om = gpu_slam_factory(plane_res=0.2), oracle.OracleMap(plane_res=0.2)
    ts = []
    for x in med.CUBE_FACES:
        for y in (-75.0, 25.0, 75.0):
            for z in med.Z_FACES:
                ts += [(x, y, z), (float(med.up(x)), float(med.down(y)), float(med.up(z))), (float(med.down(x)), float(med.up(y)), float(med.down(z))),
                       (np.nextafter(x, np.inf), np.nextafter(y, -np.inf), z)]
    for t in ts:
        t = np.array(t, np.float64)
        o = med.origin_after_set(t)
        assert list(slam.set_origin(t)) == list(om.set_origin(t)) == list(o), t
        o2, pos = med.shift(o, t)
        assert list(slam.shift_map(t)) == list(om.shift(t)) == list(pos), t
        assert list(slam.origin()) == list(om.origin()) == list(o2), t
        t2 = t + np.array([400.0, -250.0, 100.0])  # a roll of several cubes, landing on faces again
        o3, pos = med.shift(o2, t2)
        assert list(slam.shift_map(t2)) == list(om.shift(t2)) == list(pos), t2
        assert list(slam.origin()) == list(om.origin()) == list(o3), t2
    slam.close()
