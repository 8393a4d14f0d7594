"""-m gpu: the two entries of one Localization() frame -- so_icp_localization (host scan, staged or uploaded) and
so_icp_localization_dev (scan resident in HBM) -- are the same frame: poses, statistics and the map after it, bit for bit, with the
device map and with SOICP_HOST_MAP=1; the resident entry seeds a map on its own; a frame that returns early (not enough map) gives
its stage slot back."""
import ctypes as C

import numpy as np
import pytest

from helpers import CorridorScene, assert_same_bits
from superodom_amd import synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def corridor():
    sc = CorridorScene()
    return sc, [np.ascontiguousarray(sc.scan(i), dtype=np.float32) for i in range(4)]


def _empty(factory, sc):
    return factory(plane_res=sc.plane_res, line_res=sc.plane_res / 2, max_surface_features=-1, max_iterations=3)


def _load_map(slam, sc):
    """the scene's map around the first pose (the corridor lies outside the default window: origin first)"""
    t0 = sc.gt_pose(0)[:3]
    slam.set_origin(t0)
    assert slam.add_surf_point_cloud(sc.map_points) == slam.map_size() > 0
    slam.shift_map(t0)
    return slam


def _assert_same_frame(a, b, slam_a, slam_b, tag):
    (rc_a, pose_a, st_a), (rc_b, pose_b, st_b) = a, b
    assert rc_a == rc_b, (tag, rc_a, rc_b)
    assert pose_a.tobytes() == pose_b.tobytes(), (tag, pose_a, pose_b)
    assert_same_bits(st_a, st_b, tag)  # (time_elapsed_ms and the flags -- STAGED_SCAN -- are not part of the set)
    assert slam_a.map_size() == slam_b.map_size() and np.array_equal(slam_a.export_map(), slam_b.export_map()), (tag, "maps differ")


@pytest.mark.parametrize("staged", [False, True])
def test_host_and_resident_entries_are_the_same_frame(gpu_slam_factory, soicp, corridor, staged):
    sc, scans = corridor
    host, res = _load_map(_empty(gpu_slam_factory, sc), sc), _load_map(_empty(gpu_slam_factory, sc), sc)
    assert np.array_equal(host.export_map(), res.export_map())
    bufs = [host.host_alloc_like(s) for s in scans] if staged else scans
    n0 = host.map_size()
    for i in (1, 2, 3):
        if staged:
            host.stage_scan(bufs[i])
        a = host.localization(True, sc.guess(i), bufs[i], 0.1 * i)
        d, n = res.upload_scan(scans[i])
        b = res.localization_dev(True, sc.guess(i), d, n, 0.1 * i)
        assert a[0] == 0 and bool(a[2].flags & soicp.FLAG_STAGED_SCAN) == staged and not (b[2].flags & soicp.FLAG_STAGED_SCAN)
        _assert_same_frame(a, b, host, res, ("frame", i, "staged" if staged else "uploaded"))
    assert host.map_size() > n0, "the frames added voxels"
    assert host.timing().stage_declined == 0


def test_the_resident_entry_seeds_the_map_and_registers_against_it(gpu_slam_factory, soicp, corridor):
    sc, scans = corridor
    slam = _empty(gpu_slam_factory, sc)
    T = sc.gt_pose(0)
    d0, n0 = slam.upload_scan(scans[0])
    rc, pose, st = slam.localization_dev(False, T, d0, n0, 0.0)
    assert rc == soicp.MAP_SEEDED == 2 and pose.tobytes() == np.asarray(T, np.float64).tobytes()
    assert bytes(st) == bytes(C.sizeof(st)), "the seed zeroes the stats"
    assert slam.map_size() > 0
    d1, n1 = slam.upload_scan(scans[1])
    rc, pose, st = slam.localization_dev(True, sc.guess(1), d1, n1, 0.1)
    et, er = synth.pose_error(pose, sc.gt_pose(1))
    print(f"registered against the seeded map: rc {rc}, {et:.3e} m, {er:.3e} rad from the ground truth")
    assert rc == 0
    assert et < 0.02 and er < 0.004, (et, er)  # (the corridor's bound: tests/test_oracle_b_registration.py)


def test_without_a_device_map_the_resident_entry_is_the_host_entry(gpu_slam_factory, soicp, corridor, monkeypatch):
    sc, scans = corridor
    monkeypatch.setenv("SOICP_HOST_MAP", "1")  # read by so_icp_create
    host, res = _empty(gpu_slam_factory, sc), _empty(gpu_slam_factory, sc)
    for i in (0, 1, 2):
        T = sc.gt_pose(0) if i == 0 else sc.guess(i)
        a = host.localization(i > 0, T, scans[i], 0.1 * i)
        d, n = res.upload_scan(scans[i])
        b = res.localization_dev(i > 0, T, d, n, 0.1 * i)
        assert a[0] == (0 if i else soicp.MAP_SEEDED), (i, a[0])
        _assert_same_frame(a, b, host, res, ("SOICP_HOST_MAP=1, frame", i))
        if i:
            assert (a[2].flags & soicp.FLAG_HOST_MAP) and (b[2].flags & soicp.FLAG_HOST_MAP)


def test_a_frame_without_enough_map_gives_its_stage_slot_back(gpu_slam_factory, soicp, corridor):
    sc, scans = corridor
    slam = _empty(gpu_slam_factory, sc)
    rc, _, st0 = slam.localization(True, sc.guess(1), scans[1], 0.1)  # (plain upload)
    assert rc == soicp.NOT_ENOUGH_MAP_FEATURES
    first = slam.host_alloc_like(scans[1])
    slam.stage_scan(first)
    rc, pose, st = slam.localization(True, sc.guess(1), first, 0.1)
    assert rc == soicp.NOT_ENOUGH_MAP_FEATURES and slam.map_size() == 0
    assert st.startup_count == st0.startup_count
    bufs = [slam.host_alloc_like(scans[i]) for i in (1, 2, 3)]
    for b in bufs:  # (a slot left "in use" would leave two: the third announcement would be declined)
        slam.stage_scan(b)
    assert slam.timing().stage_declined == 0
    _load_map(slam, sc)
    rc, pose, st = slam.localization(True, sc.guess(1), bufs[0], 0.2)
    assert rc == 0 and (st.flags & soicp.FLAG_STAGED_SCAN), (rc, hex(st.flags))
