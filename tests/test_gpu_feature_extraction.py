"""-m gpu: so_icp_extract_features(_dev) -- featureExtraction's sweep -> LaserFeature clouds on the device -- against the
restatement (tests/feature_extraction_ref.py), bit for bit: records, surf cloud, count and order.  The de-skew between the two
restated steps is the library's so_icp_deskew_scan (deskew_kernel) run on the restated ingest: the fused kernel must give its bits."""
import ctypes as C

import numpy as np
import pytest
from scipy.spatial.transform import Rotation as R

import deskew_data as dd
import feature_extraction_ref as fr
from helpers import assert_same_bits

pytestmark = pytest.mark.gpu
T0 = 1.7e9 + 0.25
T_I_L = np.concatenate([[0.05, -0.02, 0.1], R.from_rotvec([0.01, -0.02, 0.5]).as_quat()])


def _sweep(sensor, seed):
    if sensor == fr.SENSOR_OUSTER:  # os1_128-like: 1024 x 128 organised, NaNs and no-return zeros
        return fr.ouster_sweep(1024, 128, seed=seed, nan_every=997, zero_every=61)
    return fr.velodyne_sweep(28800, seed=seed, nan_every=499, zero_every=73)  # VLP-16: 28 800 points, 22-byte unaligned points


def _poses(branch, seed, rate_hz=200.0):
    if branch == "none":
        return None, False, None
    if branch == "imu":
        return dd.pose_buffer(T0, rate_hz=rate_hz, seed=seed, translate=False, flip_signs=True), True, T_I_L
    return dd.pose_buffer(T0, rate_hz=rate_hz, seed=seed, translate=True), False, None


def _want(slam, buf, w, h, layout, poses, imu, til):
    rec = fr.ingest(buf, w, h, layout)
    if poses is not None:
        rec, _ = slam.deskew_scan(rec, 20, T0, poses, imu, til)
    return rec, fr.surf_sample(rec, layout.filter_point_size, layout.min_range)


def _same(a, b):
    """bit for bit, except that a NaN coordinate only has to be a NaN: its payload and sign come from the arithmetic unit that
    produced it (the Ouster transform of a NaN point), and no consumer looks past isfinite / an ordered comparison"""
    if a.shape != b.shape:
        print("shapes", a.shape, b.shape)
        return False
    wa, wb = a.view(np.uint32).reshape(len(a), 8), b.view(np.uint32).reshape(len(b), 8)
    fa, fb = wa.view(np.float32), wb.view(np.float32)
    eq = wa == wb
    eq[:, :3] |= np.isnan(fa[:, :3]) & np.isnan(fb[:, :3])
    if eq.all():
        return True
    rows = np.nonzero(~eq.all(1))[0]
    print(f"{len(rows)} of {len(a)} records differ; first: {rows[:5].tolist()}")
    for r in rows[:5]:
        print(r, fa[r].tolist(), fb[r].tolist(), [hex(v) for v in wa[r]], [hex(v) for v in wb[r]])
    return False


@pytest.mark.parametrize("sensor", [fr.SENSOR_OUSTER, fr.SENSOR_VELODYNE])
@pytest.mark.parametrize("branch", ["imu", "vio", "none"])
@pytest.mark.parametrize("step", [1, 3, 7])
def test_extract_features_bit_for_bit(gpu_slam_factory, sensor, branch, step):
    slam = gpu_slam_factory()
    buf, w, h, rs, _ = _sweep(sensor, seed=10 + step)
    layout = fr.layout_for(sensor, step, 0.2, row_step=rs)
    poses, imu, til = _poses(branch, seed=20 + step)
    rec, surf, info = slam.extract_features(buf, w, h, layout, T0, poses, imu, til)
    want_rec, want_surf = _want(slam, buf, w, h, layout, poses, imu, til)
    assert info.n_points == w * h and info.deskewed == (poses is not None)
    assert _same(rec, want_rec), "cloud_nodistortion: the restated ingest + so_icp_deskew_scan, bit for bit"
    assert info.n_surface == len(want_surf) > 0 and _same(surf, want_surf), "cloud_surface: count, order and bits"
    bad = ~np.isfinite(rec.view(np.float32)[:, :3]).all(1)
    assert bad.sum() > 10, "the sweep carries non-finite points"
    if poses is not None:
        _, dinfo = slam.deskew_scan(fr.ingest(buf, w, h, layout), 20, T0, poses, imu, til)
        assert info.n_clamped == dinfo.n_clamped
        assert list(info.q_w_original_l) == list(dinfo.q_w_original_l) and list(info.t_w_original_l) == list(dinfo.t_w_original_l)
    else:
        assert list(info.q_w_original_l) == [0, 0, 0, 1] and list(info.t_w_original_l) == [0, 0, 0] and info.n_clamped == 0


@pytest.mark.parametrize("sensor", [fr.SENSOR_OUSTER, fr.SENSOR_VELODYNE])
def test_pose_table_in_global_memory(gpu_slam_factory, sensor):
    slam = gpu_slam_factory()
    buf, w, h, rs, _ = _sweep(sensor, seed=5)
    layout = fr.layout_for(sensor, 2, 0.2, row_step=rs)
    poses, imu, til = _poses("imu", seed=6, rate_hz=8000.0)
    assert len(poses) > 512, "this case takes the kernel's global-memory table path"
    rec, surf, info = slam.extract_features(buf, w, h, layout, T0, poses, imu, til)
    want_rec, want_surf = _want(slam, buf, w, h, layout, poses, imu, til)
    assert _same(rec, want_rec) and _same(surf, want_surf)


@pytest.mark.parametrize("axis", ["x", "z"])
def test_lidar_mounted_half_a_turn_round(gpu_slam_factory, axis):
    """T_i_l = 180 degrees about x / z under an IMU buffer: T_l_i * T_original_current of every point, and start * T_i_l, take one of
    matrix_to_quat's hand-written branches (trace <= 0) in ingest_deskew_kernel's own inlined copy of deskew_point"""
    slam = gpu_slam_factory()
    buf, w, h, rs, _ = _sweep(fr.SENSOR_VELODYNE, seed=31)
    layout = fr.layout_for(fr.SENSOR_VELODYNE, 1, 0.2, row_step=rs)
    poses, til = dd.pose_buffer(T0, seed=32, translate=False, flip_signs=True), dd.half_turn_extrinsic(axis)
    plain = fr.ingest(buf, w, h, layout)
    assert dd.half_turn_census(plain, T0, poses, axis) > 20000
    rec, surf, info = slam.extract_features(buf, w, h, layout, T0, poses, True, til)
    want_rec, want_surf = _want(slam, buf, w, h, layout, poses, True, til)
    assert _same(rec, want_rec), "cloud_nodistortion: the restated ingest + so_icp_deskew_scan, bit for bit"
    assert info.n_surface == len(want_surf) > 0 and _same(surf, want_surf), "cloud_surface: count, order and bits"
    _, dinfo = slam.deskew_scan(plain, 20, T0, poses, True, til)
    assert info.n_clamped == dinfo.n_clamped == 0
    assert list(info.q_w_original_l) == list(dinfo.q_w_original_l) and list(info.t_w_original_l) == list(dinfo.t_w_original_l)


def test_knife_edges(gpu_slam_factory):
    """|d| one float either side of 1e-7, a norm equal to 0.2f * 0.2f, the precedence of the range gate, NaN neighbours, n = 0 1 2"""
    slam = gpu_slam_factory()
    f = np.float32(1e-7)
    above, below = f, np.nextafter(f, np.float32(0))
    r_up = np.nextafter(np.float32(0.2), np.float32(1))
    pts = [[0, 0, 30], [above, 0, 30],          # 1: |dx| = float(1e-7): kept
           [0, 0, 30], [0, below, 30],          # 3: |dy| one float below: dropped
           [0, 0, 0], [0.05, 0, 0],             # 5: |dx| inside min_range: kept (the gate goes with z only)
           [0, 0, 0], [0, 0, 0.05],             # 7: only |dz|, inside min_range: dropped
           [0.2, 0, 1], [0.2, 0, 0],            # 9: only |dz|, x*x + y*y + z*z == 0.2f * 0.2f: dropped
           [r_up, 0, 1], [r_up, 0, 0],          # 11: one float farther: kept
           [np.nan, np.nan, np.nan], [5, 6, 7], # 13: NaN neighbour: dropped
           [5, 6, 7], [np.nan, 6, 8],           # 15: NaN point: dropped
           [0, 0, 40], [0, 0, np.nextafter(np.float32(40), np.float32(50))]]  # 17: |dz| one float spacing at 40 m: kept
    xyz = np.array(pts, np.float32)
    n = len(xyz)
    vals = {"x": xyz[:, 0], "y": xyz[:, 1], "z": xyz[:, 2], "intensity": np.arange(n, dtype=np.float32),
            "ring": np.arange(n) % 16, "time": np.arange(n, dtype=np.float32) * 1e-3}
    buf, w, h, rs = fr.make_payload(fr.VELODYNE_FIELDS, fr.VELODYNE_POINT_STEP, n, vals)
    layout = fr.layout_for(fr.SENSOR_VELODYNE, 1, 0.2, row_step=rs)
    rec, surf, info = slam.extract_features(buf, w, h, layout, T0)
    want_rec, want_surf = _want(slam, buf, w, h, layout, None, False, None)
    assert _same(rec, want_rec) and _same(surf, want_surf)
    kept = [int(round(t * 1e3)) for t in surf.view(np.float32)[:, 4]]
    assert [k for k in kept if k % 2 == 1] == [1, 5, 11, 17], kept
    for k in (0, 1, 2):
        b2, w2, h2, rs2 = fr.make_payload(fr.VELODYNE_FIELDS, fr.VELODYNE_POINT_STEP, k, {kk: v[:k] for kk, v in vals.items()}) if k else (np.zeros(0, np.uint8), 0, 1, 0)
        lay2 = fr.layout_for(fr.SENSOR_VELODYNE, 1, 0.2, row_step=rs2)
        rec, surf, info = slam.extract_features(b2, w2, h2, lay2, T0, dd.pose_buffer(T0, seed=3), False, None)
        want_rec, want_surf = _want(slam, b2, w2, h2, lay2, dd.pose_buffer(T0, seed=3), False, None)
        assert info.n_points == k and info.n_surface == len(want_surf) == max(k - 1, 0) and _same(rec, want_rec) and _same(surf, want_surf)


def test_unmatched_fields_read_zero(gpu_slam_factory, soicp):
    """a PointField list with no intensity and a FLOAT64 time: pcl::fromROSMsg leaves both at the point's 0"""
    slam = gpu_slam_factory()
    n = 4000
    rng = np.random.default_rng(7)
    fields = [("x", 0, soicp.FLOAT32, 1), ("y", 4, soicp.FLOAT32, 1), ("z", 8, soicp.FLOAT32, 1), ("time", 16, soicp.FLOAT64, 1),
              ("ring", 12, soicp.UINT16, 1)]
    xyz = rng.normal(0, 10, (n, 3)).astype(np.float32)
    vals = {"x": xyz[:, 0], "y": xyz[:, 1], "z": xyz[:, 2], "time": rng.uniform(0, 0.1, n), "ring": rng.integers(0, 16, n)}
    buf, w, h, rs = fr.make_payload(fields, 24, n, vals)
    layout = soicp.sweep_layout(fields, 24, rs, soicp.SENSOR_VELODYNE, 3, 0.2)
    assert layout.off_intensity == -1 and layout.off_time == -1
    rec, surf, info = slam.extract_features(buf, w, h, layout, T0, dd.pose_buffer(T0, seed=8), False, None)
    f = rec.view(np.float32)
    assert not f[:, 4].any() and not f[:, 5].any() and np.array_equal(rec.view(np.uint32)[:, 6], vals["ring"].astype(np.uint32))
    want_rec, want_surf = _want(slam, buf, w, h, layout, dd.pose_buffer(T0, seed=8), False, None)
    assert _same(rec, want_rec) and _same(surf, want_surf)


class _Hip:
    def __init__(self):
        self.h = C.CDLL("libamdhip64.so")
        self.h.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        self.h.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        self.h.hipFree.argtypes = [C.c_void_p]

    def upload(self, a):
        d = C.c_void_p()
        assert self.h.hipMalloc(C.byref(d), max(a.nbytes, 1)) == 0
        assert self.h.hipMemcpy(d, a.ctypes.data_as(C.c_void_p), a.nbytes, 1) == 0
        return d

    def download(self, d, nbytes):
        out = np.empty(nbytes, np.uint8)
        if nbytes:
            assert self.h.hipMemcpy(out.ctypes.data_as(C.c_void_p), C.c_void_p(d), nbytes, 2) == 0
        return out


def test_dev_entry_and_prefilter_on_the_device(gpu_slam_factory, soicp):
    """_dev equals the host entry; so_icp_prefilter_scan_dev on the device surf cloud equals so_icp_prefilter_scan on its host copy"""
    hip = _Hip()
    buf, w, h, rs, _ = _sweep(fr.SENSOR_OUSTER, seed=31)
    layout = fr.layout_for(fr.SENSOR_OUSTER, 3, 0.2, row_step=rs)
    poses, imu, til = _poses("imu", seed=32)
    host = gpu_slam_factory(plane_res=0.2)
    rec, surf, info = host.extract_features(buf, w, h, layout, T0, poses, imu, til)
    dev = gpu_slam_factory(plane_res=0.2)
    d_raw = hip.upload(buf)
    try:
        d_rec, d_surf, dinfo = dev.extract_features_dev(d_raw.value, w, h, layout, T0, poses, imu, til)
        assert (dinfo.n_surface, dinfo.n_clamped, dinfo.n_points) == (info.n_surface, info.n_clamped, info.n_points)
        assert np.array_equal(hip.download(d_rec, rec.nbytes), rec.reshape(-1))
        assert np.array_equal(hip.download(d_surf, surf.nbytes), surf.reshape(-1))
        for auto in (1, 0):
            dp, np_, pinfo = dev.prefilter_scan_dev(d_surf, dinfo.n_surface, 32, auto, 0.2, 0.4)
            got = dev.download_scan(dp, np_)
            hp, nh, hinfo = host.prefilter_scan(surf.view(np.float32)[:, :3], auto, 0.2, 0.4)
            want = host.download_scan(hp, nh)
            assert np_ == nh > 0 and np.array_equal(got.view(np.uint32), want.view(np.uint32))
            for k in ("average_distance", "count_far_points", "increase_blind_radius", "line_res", "plane_res", "statistic_in_input_order"):
                assert getattr(pinfo, k) == getattr(hinfo, k), k
    finally:
        hip.h.hipFree(d_raw)


def test_resident_chain_equals_the_host_chain(gpu_slam_factory):
    """sweep -> features -> prefilter_scan_dev -> localization_dev (the surf cloud never leaves the device) against the same chain
    through host buffers: same poses, statistics and map"""
    hip = _Hip()
    frames = [_sweep_shifted(k) for k in range(3)]
    res = {}
    for mode in ("host", "dev"):
        slam = gpu_slam_factory(plane_res=0.2, max_iterations=4)
        pose = np.array([0, 0, 0, 0, 0, 0, 1.0])
        out = []
        for k, (buf, w, h, rs) in enumerate(frames):
            layout = fr.layout_for(fr.SENSOR_OUSTER, 2, 0.2, row_step=rs)
            t = T0 + 0.1 * k
            poses = dd.pose_buffer(t, seed=40 + k, translate=True) * np.array([1, 0.05, 0.05, 0.05, 1, 1, 1, 1])
            if mode == "dev":
                d_raw = hip.upload(buf)
                try:
                    _, d_surf, info = slam.extract_features_dev(d_raw.value, w, h, layout, t, poses, False, None)
                    dp, n_f, pinfo = slam.prefilter_scan_dev(d_surf, info.n_surface, 32, 1, 0.2, 0.4)
                finally:
                    hip.h.hipFree(d_raw)
                rc, p, st = slam.localization_dev(k > 0, pose, dp, n_f, t)
            else:
                _, surf, info = slam.extract_features(buf, w, h, layout, t, poses, False, None)
                dp, n_f, pinfo = slam.prefilter_scan(surf.view(np.float32)[:, :3], 1, 0.2, 0.4)
                filt = slam.download_scan(dp, n_f)
                rc, p, st = slam.localization(k > 0, pose, filt, t)
            out.append((rc, p.copy(), st, n_f, pinfo.plane_res))
            pose = p
        res[mode] = (out, slam.export_map())
    (ho, hm), (do, dm) = res["host"], res["dev"]
    assert [o[0] for o in ho] == [2, 0, 0] and ho[1][2].n_iterations > 0, [o[0] for o in ho]
    for k, (a, b) in enumerate(zip(ho, do)):
        assert a[0] == b[0] and np.array_equal(a[1], b[1]) and a[3:] == b[3:]
        assert_same_bits(a[2], b[2], ("frame", k))
    assert np.array_equal(hm.view(np.uint32), dm.view(np.uint32))


def _sweep_shifted(k):
    buf, w, h, rs, _ = fr.ouster_sweep(1024, 128, seed=50 + k, nan_every=997, zero_every=61, shift=(0.3 * k, 0.1 * k, 0.0))
    return buf, w, h, rs


def test_nontrivial_ouster_transform_and_the_oracle_deskew(gpu_slam_factory, oracle):
    """a T_ouster_sensor whose rotation is not a sign flip, so the fp64 _transformVector order and its rounding are compared;
    and the de-skewed records against the C oracle's de-skew (independent of the library's deskew_setup): every point within
    one float32 spacing, nearly all bit-identical (acos / sin of slerp may differ in the last bit between host and device)"""
    slam = gpu_slam_factory()
    buf, w, h, rs, _ = _sweep(fr.SENSOR_OUSTER, seed=61)
    T = np.concatenate([[0.011, -0.023, 0.0412], R.from_rotvec([0.013, -0.021, 2.9]).as_quat()])
    layout = soicp_layout(T, rs)
    poses, imu, til = _poses("imu", seed=62)
    rec, surf, info = slam.extract_features(buf, w, h, layout, T0, poses, imu, til)
    want_rec, want_surf = _want(slam, buf, w, h, layout, poses, imu, til)
    assert _same(rec, want_rec) and _same(surf, want_surf)
    plain = fr.ingest(buf, w, h, layout)
    o, _, beyond = oracle.deskew(plain, 20, T0, poses, imu, til)
    a, b = rec.view(np.float32)[:, :3].reshape(-1), o.view(np.float32)[:, :3].reshape(-1)
    fin = np.isfinite(a) & np.isfinite(b)
    assert np.array_equal(np.isfinite(a), np.isfinite(b)) and info.n_clamped == beyond
    same = a[fin].view(np.uint32) == b[fin].view(np.uint32)
    ulp = np.spacing(np.maximum(np.abs(a[fin]), np.abs(b[fin])))
    assert same.mean() > 0.999 and (np.abs(a[fin].astype(np.float64) - b[fin]) <= ulp).all()


def soicp_layout(T, rs):
    from superodom_amd import binding
    return binding.sweep_layout(fr.OUSTER_FIELDS, fr.OUSTER_POINT_STEP, rs, binding.SENSOR_OUSTER, 3, 0.2, T_ouster_sensor=T)
