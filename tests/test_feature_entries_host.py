"""CPU-side check of what the six so_icp_extract_features* entries share -- the argument check in front of each -- on a host-only
context: a refused layout's message begins with the entry's own exported name, a pose count of 2^24 is refused before the buffer
is looked at, and a valid call gets as far as the device check.  No compute kernels run here."""
import ctypes as C

import numpy as np
import pytest

E_INVALID, E_HIP, E_UNSUPPORTED = -1, -2, -5
N = 64  # points of the sweep: one row


def _layout(soicp, kind, filter_point_size):
    xyzi = [("x", 0, soicp.FLOAT32, 1), ("y", 4, soicp.FLOAT32, 1), ("z", 8, soicp.FLOAT32, 1), ("intensity", 12, soicp.FLOAT32, 1)]
    if kind == "livox":
        return soicp.livox_layout(filter_point_size=filter_point_size)
    if kind == "untimed":
        return soicp.untimed_layout(xyzi, 16, 16 * N, 16, filter_point_size, 0.2)
    fields = xyzi + [("time", 16, soicp.FLOAT32, 1), ("ring", 20, soicp.UINT16, 1)]
    return soicp.sweep_layout(fields, 24, 24 * N, soicp.SENSOR_VELODYNE, filter_point_size, 0.2)


ENTRIES = [(name + suffix, kind) for name, kind in (("so_icp_extract_features", "sweep"), ("so_icp_extract_features_livox", "livox"),
                                                    ("so_icp_extract_features_untimed", "untimed")) for suffix in ("", "_dev")]


@pytest.mark.parametrize("name,kind", ENTRIES)
def test_the_shared_argument_check_of_each_entry(soicp, name, kind):
    L = soicp.load()
    host = soicp.LidarSlamGpu(device_id=-1, plane_res=0.2)
    buf = np.zeros(N * 24, np.uint8)
    poses = np.zeros((1, 8))  # one entry: a check that read 2^24 of them would leave the buffer

    def call(layout, n_poses):
        shape = (N,) if kind == "livox" else (N, 1)
        d_rec, d_surf, info = C.c_void_p(), C.c_void_p(), soicp.FeatureInfo()
        out = (C.byref(d_rec), C.byref(d_surf)) if name.endswith("_dev") else (None, None)
        pp = poses.ctypes.data_as(C.POINTER(C.c_double)) if n_poses else None
        return getattr(L, name)(host.h, buf.ctypes.data_as(C.c_void_p), *shape, C.byref(layout), 0.0, pp, n_poses, 0, None, *out, C.byref(info))

    assert call(_layout(soicp, kind, 0), 0) == E_INVALID
    msg = L.so_icp_last_error(host.h)
    assert msg.startswith(name.encode() + b": filter_point_size"), msg
    assert call(_layout(soicp, kind, 3), 1 << 24) == E_UNSUPPORTED
    msg = L.so_icp_last_error(host.h)
    assert msg.startswith(name.encode() + b": too many poses"), msg
    for n_poses in (0, 1):
        assert call(_layout(soicp, kind, 3), n_poses) == E_HIP
        assert b"host-only" in L.so_icp_last_error(host.h)
