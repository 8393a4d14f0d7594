"""CPU-side checks of so_icp_extract_features(_dev) and so_icp_prefilter_scan_dev: the symbols are exported, invalid layouts and
arguments are refused with SO_ICP_E_INVALID, a host-only context (device_id < 0) fails with SO_ICP_E_HIP, the PointField matching of
the layout helper, and known answers of the restatement (tests/feature_extraction_ref.py) itself.  No compute kernels run here."""
import ctypes as C

import numpy as np
import pytest

import feature_extraction_ref as fr

E_INVALID, E_HIP = -1, -2
NEW = ["so_icp_extract_features", "so_icp_extract_features_dev", "so_icp_prefilter_scan_dev"]


def test_symbols_are_exported(soicp):
    L = soicp.load()
    for name in NEW:
        assert hasattr(L, name) and name in soicp.EXPORTED
    assert L.so_icp_abi_version() == 4


def _call(L, h, layout, buf, width, height, poses=None, dev=False):
    n_poses = 0 if poses is None else len(poses)
    pp = None if poses is None else poses.ctypes.data_as(C.POINTER(C.c_double))
    info = fr_info()
    if dev:
        d_rec, d_surf = C.c_void_p(), C.c_void_p()
        return L.so_icp_extract_features_dev(h, None if buf is None else buf.ctypes.data_as(C.c_void_p), width, height,
                                             None if layout is None else C.byref(layout), 0.0, pp, n_poses, 0, None, C.byref(d_rec),
                                             C.byref(d_surf), C.byref(info))
    return L.so_icp_extract_features(h, None if buf is None else buf.ctypes.data_as(C.c_void_p), width, height,
                                     None if layout is None else C.byref(layout), 0.0, pp, n_poses, 0, None, None, None, C.byref(info))


def fr_info():
    from superodom_amd.binding import FeatureInfo
    return FeatureInfo()


@pytest.mark.parametrize("dev", [False, True])
def test_invalid_arguments(soicp, dev):
    L = soicp.load()
    host = soicp.LidarSlamGpu(device_id=-1, plane_res=0.2)
    buf, w, h, rs, _ = fr.velodyne_sweep(320, seed=1)
    good = fr.layout_for(fr.SENSOR_VELODYNE, 3, 0.2, row_step=rs)
    assert _call(L, None, good, buf, w, h, dev=dev) == E_INVALID                 # no context
    assert _call(L, host.h, None, buf, w, h, dev=dev) == E_INVALID               # no layout
    assert _call(L, host.h, good, None, w, h, dev=dev) == E_INVALID              # no payload
    poses = np.zeros((3, 8))
    assert (L.so_icp_extract_features(host.h, buf.ctypes.data_as(C.c_void_p), w, h, C.byref(good), 0.0, None, 3, 0, None, None, None, None)
            == E_INVALID)                                                         # n_poses without a buffer

    def bad(**kw):
        lay = fr.layout_for(fr.SENSOR_VELODYNE, 3, 0.2, row_step=rs)
        for k, v in kw.items():
            setattr(lay, k, v)
        return _call(L, host.h, lay, buf, w, h, dev=dev)
    assert bad(off_time=19) == E_INVALID          # time (4 bytes at 19) runs past point_step 22
    assert bad(off_ring=21) == E_INVALID          # ring (2 bytes) past point_step
    assert bad(off_x=22) == E_INVALID
    assert bad(off_y=-2) == E_INVALID
    assert bad(row_step=w * 22 - 1) == E_INVALID  # row_step < width * point_step
    assert bad(is_bigendian=1) == E_INVALID
    assert bad(filter_point_size=0) == E_INVALID
    assert bad(filter_point_size=-3) == E_INVALID
    assert bad(sensor=2) == E_INVALID             # SensorType::LIVOX: not a PointCloud2 sensor here
    assert bad(point_step=0, row_step=0) == E_INVALID
    assert bad(filter_point_size=0) == E_INVALID and b"filter_point_size" in L.so_icp_last_error(host.h)
    assert bad(is_bigendian=1) == E_INVALID and b"big-endian" in L.so_icp_last_error(host.h)
    # a valid call on a host-only context: E_HIP, nothing touched (the map stays empty, poses unread)
    assert _call(L, host.h, good, buf, w, h, poses=poses, dev=dev) == E_HIP
    assert b"host-only" in L.so_icp_last_error(host.h)
    assert host.export_map().size == 0


def test_prefilter_scan_dev_host_only(soicp):
    L = soicp.load()
    host = soicp.LidarSlamGpu(device_id=-1, plane_res=0.2)
    d, n = C.c_void_p(), C.c_size_t(0)
    assert L.so_icp_prefilter_scan_dev(None, None, 0, 32, 1, 0.1, 0.2, C.byref(d), C.byref(n), None) == E_INVALID
    assert L.so_icp_prefilter_scan_dev(host.h, None, 10, 32, 1, 0.1, 0.2, C.byref(d), C.byref(n), None) == E_INVALID
    assert L.so_icp_prefilter_scan_dev(host.h, C.c_void_p(4096), 10, 32, 1, 0.1, 0.2, None, C.byref(n), None) == E_INVALID
    assert L.so_icp_prefilter_scan_dev(host.h, C.c_void_p(4096), 10, 32, 1, 0.1, 0.2, C.byref(d), C.byref(n), None) == E_HIP


def test_layout_helper_matches_fields_as_pcl_does(soicp):
    b = soicp
    L = b.sweep_layout(fr.OUSTER_FIELDS, 48, 48 * 1024, b.SENSOR_OUSTER, 3, 0.2)
    assert (L.off_x, L.off_y, L.off_z, L.off_intensity, L.off_time, L.off_ring) == (0, 4, 8, 16, 20, -1)  # the Ouster point has no ring
    assert list(L.T_ouster_sensor) == [0.0, 0.0, 0.036180, 0.0, 0.0, 1.0, 0.0]
    V = b.sweep_layout(fr.VELODYNE_FIELDS, 22, 22 * 100, b.SENSOR_VELODYNE, 1, 0.2)
    assert (V.off_x, V.off_y, V.off_z, V.off_intensity, V.off_time, V.off_ring) == (0, 4, 8, 12, 18, 16)
    assert (V.point_step, V.row_step, V.filter_point_size, V.sensor) == (22, 2200, 1, b.SENSOR_VELODYNE)
    assert abs(V.min_range - 0.2) < 1e-7
    # a missing intensity and a FLOAT64 time do not match: absent (read 0); count 0 matches a single value (pcl::detail::FieldMatches);
    # count 2, a wrong datatype or a wrong name does not; the first matching field wins
    fields = [("x", 0, b.FLOAT32, 0), ("y", 4, b.FLOAT32, 2), ("z", 8, b.FLOAT64, 1), ("time", 16, b.FLOAT64, 1), ("ring", 24, b.UINT16, 1),
              ("ring", 26, b.UINT16, 1), ("Intensity", 28, b.FLOAT32, 1)]
    M = b.sweep_layout(fields, 32, 32, b.SENSOR_VELODYNE, 1, 0.2)
    assert (M.off_x, M.off_y, M.off_z, M.off_intensity, M.off_time, M.off_ring) == (0, -1, -1, -1, -1, 24)
    # the Ouster's t is UINT32 in ns: a FLOAT32 t does not match
    O = b.sweep_layout([("x", 0, b.FLOAT32, 1), ("t", 4, b.FLOAT32, 1)], 8, 8, b.SENSOR_OUSTER, 1, 0.2)
    assert (O.off_x, O.off_time) == (0, -1)
    assert b.sweep_layout(fields, 32, 32, b.SENSOR_OUSTER, 1, 0.2, is_bigendian=True).is_bigendian == 1


def test_restatement_precedence_kat():
    """a || b || (c && d): the range gate d only goes with the z test; float |d| compared with the double 1e-7"""
    r = np.float32(0.2)
    f = np.float32(1e-7)
    above, below = f, np.nextafter(f, np.float32(0))  # float32(1e-7) > 1e-7 as a double; its predecessor is below
    assert float(above) > 1e-7 > float(below)
    a = np.array([[0.05, 0.0, 0.0],        # |dx| = 0.05, inside min_range: kept (the range gate does not apply to x)
                  [0.0, 0.05, 0.0],        # same for y
                  [0.0, 0.0, 0.05],        # only |dz|, inside min_range: dropped
                  [0.0, 0.0, 5.0],         # only |dz|, outside: kept
                  [above, 0.0, 30.0],      # |dx| = float(1e-7) > 1e-7: kept
                  [below, 0.0, 30.0],      # |dx| one float below: dropped (and dz = 0)
                  [0.2, 0.0, 0.0],         # only |dz| (neighbour z = 1): x*x + y*y + z*z == 0.2f * 0.2f, not greater: dropped
                  [np.nextafter(np.float32(0.2), np.float32(1)), 0.0, 0.0],  # one float farther: kept
                  [1.0, 2.0, 3.0]], np.float32)  # NaN neighbour: every term false
    b = np.array([[0, 0, 0], [0, 0, 0], [0, 0, 0], [0, 0, 0], [0, 0, 30.0], [0, 0, 30.0], [0.2, 0, 1.0],
                  [np.nextafter(np.float32(0.2), np.float32(1)), 0, 1.0], [np.nan, 2.0, 3.0]], np.float32)
    assert (np.float32(0.2) * np.float32(0.2)) == r * r
    got = fr.surf_keep(a, b, 0.2)
    assert got.tolist() == [True, True, False, True, True, False, False, True, False]


def test_restatement_sampling_order_and_records():
    """candidates 1, 1 + s, ... against the RAW predecessor (not the last kept point); output PointXYZI records"""
    n = 10
    rec = np.zeros((n, 8), np.float32)
    rec[:, 0] = np.arange(n) * 1.0 + 1.0
    rec[:, 5] = np.arange(n) * 0.01
    rec[4, 0:3] = rec[3, 0:3]  # 4 equals its predecessor 3: dropped
    out = fr.surf_sample(rec.view(np.uint8).reshape(n, 32), 3, 0.2).view(np.float32)
    assert out[:, 0].tolist() == [2.0, 8.0]          # candidates 1, 4, 7: 4 is dropped
    assert out[:, 3].tolist() == [1.0, 1.0] and np.allclose(out[:, 4], [0.01, 0.07]) and not out[:, 5:].any()
    for k in (0, 1, 2):
        assert len(fr.surf_sample(rec[:k].view(np.uint8).reshape(k, 32), 1, 0.2)) == max(k - 1, 0)


def test_restatement_ingest_layouts():
    buf, w, h, rs, vals = fr.velodyne_sweep(160, seed=3)
    lay = fr.layout_for(fr.SENSOR_VELODYNE, 1, 0.2, row_step=rs)
    rec = fr.ingest(buf, w, h, lay)
    f = rec.view(np.float32)
    assert np.array_equal(f[:, 0].view(np.uint32), vals["x"].view(np.uint32)) and np.array_equal(f[:, 5], vals["time"])
    assert np.array_equal(rec.view(np.uint32)[:, 6], vals["ring"].astype(np.uint32)) and not rec.view(np.uint32)[:, [3, 7]].any()
    buf, w, h, rs, vals = fr.ouster_sweep(64, 8, seed=4)
    lay = fr.layout_for(fr.SENSOR_OUSTER, 1, 0.2, row_step=rs)
    f = fr.ingest(buf, w, h, lay).view(np.float32)
    assert np.array_equal(f[:, 0], -vals["x"]) and np.array_equal(f[:, 1], -vals["y"])  # R = diag(-1, -1, 1): exact
    assert np.array_equal(f[:, 2], (vals["z"].astype(np.float64) + 0.036180).astype(np.float32))
    assert np.array_equal(f[:, 5], vals["t"].astype(np.float32) * np.float32(1e-9)) and not f.view(np.uint32)[:, 6].any()
