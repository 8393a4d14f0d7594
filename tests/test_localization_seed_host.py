"""so_icp_localization on a host-only context (device_id = -1): seeding the map needs no device -- initializeMapping with the
transform done on the host --, a registration does and says so.  No kernel runs here."""
import ctypes as C

import numpy as np
import pytest

from helpers import noisy_planes_cloud
from superodom_amd import synth

E_INVALID = -1
# 18 m along x: the cloud (x within +-20 m, inside the cube [-25, 25)) comes to lie across the cube face x = 25
T = np.concatenate([[18.0, -7.0, 2.0], synth.quat_from_rotvec(np.array([0.02, -0.03, 0.3]))])
IDENTITY = np.array([0, 0, 0, 0, 0, 0, 1.0])


@pytest.fixture(scope="module")
def cloud():
    return noisy_planes_cloud(2000, np.random.default_rng(5))


def _host(soicp):
    return soicp.LidarSlamGpu(device_id=-1, plane_res=0.2)


def _seed_raw(soicp, slam, pose, records, stride_bytes, time=0.5):
    """so_icp_localization(initialization = 0) called directly: records float32 [n, stride / 4] -> (rc, pose_out, the Stats handed in DIRTY)"""
    pose = np.ascontiguousarray(pose, np.float64); out = np.full(7, np.nan)
    st = soicp.Stats()
    C.memset(C.byref(st), 0xA5, C.sizeof(st))
    rc = slam.L.so_icp_localization(slam.h, 0, pose.ctypes.data_as(C.POINTER(C.c_double)), records.ctypes.data_as(C.POINTER(C.c_float)),
                                    len(records), stride_bytes, time, out.ctypes.data_as(C.POINTER(C.c_double)), C.byref(st))
    return rc, out, st


def test_seeding_needs_no_device(soicp, cloud):
    slam = _host(soicp)
    rc, pose, st = slam.localization(False, T, cloud, 0.5)
    assert rc == soicp.MAP_SEEDED and pose.tobytes() == T.tobytes()
    assert bytes(st) == bytes(C.sizeof(st))
    assert slam.map_size() > 0
    rc, pose, st = _seed_raw(soicp, _host(soicp), T, cloud, 12)
    assert rc == soicp.MAP_SEEDED and pose.tobytes() == T.tobytes()
    assert bytes(st) == bytes(C.sizeof(st)), "the seed zeroes the caller's stats"


def test_seed_with_the_identity_pose_is_set_origin_and_add_surf(soicp, cloud):
    R = synth.quat_to_R(T[3:])
    world = (cloud.astype(np.float64) @ R.T + T[:3]).astype(np.float32)  # (lies across the cube face x = 25)
    assert world[:, 0].min() < 25.0 < world[:, 0].max()
    slam, ref = _host(soicp), _host(soicp)
    rc, pose, _ = slam.localization(False, IDENTITY, world, 0.5)
    assert rc == soicp.MAP_SEEDED and pose.tobytes() == IDENTITY.tobytes()
    ref.set_origin(IDENTITY[:3])
    assert ref.add_surf_point_cloud(world) >= 0
    assert list(slam.origin()) == list(ref.origin())
    assert slam.map_size() == ref.map_size() > 0 and np.array_equal(slam.export_map(), ref.export_map())


def test_stride_32_seeds_the_same_map_and_a_stride_of_10_is_refused(soicp, cloud):
    packed, padded = _host(soicp), _host(soicp)
    assert _seed_raw(soicp, packed, T, cloud, 12)[0] == soicp.MAP_SEEDED
    rec = np.full((len(cloud), 8), 7.5e8, np.float32)
    rec[:, :3] = cloud
    assert _seed_raw(soicp, padded, T, rec, 32)[0] == soicp.MAP_SEEDED
    assert list(padded.origin()) == list(packed.origin())
    assert padded.map_size() == packed.map_size() > 0 and np.array_equal(padded.export_map(), packed.export_map())
    before = packed.export_map()
    rc, _, _ = _seed_raw(soicp, packed, T, cloud, 10)
    assert rc == E_INVALID and "stride_bytes must be a multiple of 4" in packed.last_error()
    assert np.array_equal(packed.export_map(), before)


def test_a_registration_on_a_host_only_context_fails_loudly(soicp, cloud):
    slam = _host(soicp)
    assert slam.localization(False, T, cloud, 0.5)[0] == soicp.MAP_SEEDED
    n, before = slam.map_size(), slam.export_map()
    with pytest.raises(soicp.SoIcpError, match="host-only context"):
        slam.localization(True, T, cloud, 0.6)
    assert slam.map_size() == n and np.array_equal(slam.export_map(), before)
