"""-m gpu: so_icp_extract_features_untimed(_dev) -- featureExtraction::assignTimeforPointCloud's sweep (no per-point time) -> LaserFeature
clouds on the device -- against the restatement (tests/untimed_ref.py), bit for bit: records, surf cloud, both counts, n_clamped and the
sweep-start pose.  As for the other sensors the de-skew between the restated ingest and the restated sampling is the library's
so_icp_deskew_scan (deskew_kernel, itself held to the oracle in test_gpu_deskew.py) on the restatement's compacted records: the fused
kernel must give its bits.  tests/test_untimed_host.py checks that every point of every sweep used here is decided (its ring does not
hang on the last bit of the float atan), and that the sweeps carry drops in every tile and the truncation cases."""
import ctypes as C

import numpy as np
import pytest
from scipy.spatial.transform import Rotation as R

import deskew_data as dd
import feature_extraction_ref as fr
import untimed_ref as ur

pytestmark = pytest.mark.gpu
T0 = 1.7e9 + 0.25
T_I_L = np.concatenate([[0.05, -0.02, 0.1], R.from_rotvec([0.01, -0.02, 0.5]).as_quat()])
EMPTY = np.zeros((0, 32), np.uint8)


def _poses(branch, seed, **kw):
    if branch == "none":
        return None, False, None
    if branch == "imu":
        return dd.pose_buffer(T0, seed=seed, translate=False, flip_signs=True, **kw), True, T_I_L
    return dd.pose_buffer(T0, seed=seed, translate=True, **kw), False, None


def _want(slam, vals, n_scans, step, min_range, poses, imu, til):
    """(records, surf cloud, DeskewInfo or None): restated ingest, so_icp_deskew_scan on its records, restated sampling"""
    rec, _ = ur.ingest(vals["x"], vals["y"], vals["z"], vals.get("intensity", np.zeros(len(vals["x"]), np.float32)), n_scans)
    dinfo = None
    if poses is not None and len(rec):
        rec, dinfo = slam.deskew_scan(rec, 20, T0, poses, imu, til)
    return rec, (fr.surf_sample(rec, step, min_range) if len(rec) else EMPTY), dinfo


def _same(a, b, what):
    if a.shape == b.shape and np.array_equal(a, b):
        return True
    print(what, "shapes", a.shape, b.shape)
    if a.shape == b.shape:
        rows = np.nonzero((a != b).any(1))[0]
        print(f"{len(rows)} of {len(a)} records differ; first: {rows[:5].tolist()}")
        for r in rows[:5]:
            print(r, a[r].view(np.float32).tolist(), b[r].view(np.float32).tolist(), a[r].view(np.uint32)[6], b[r].view(np.uint32)[6])
    return False


def _check(got, want, what):
    (rec, surf, info), (want_rec, want_surf, dinfo) = got, want
    print(what, "n_points", info.n_points, "of", "n_surface", info.n_surface, "n_clamped", info.n_clamped, "want", len(want_rec), len(want_surf))
    assert info.n_points == len(want_rec), "the number of records: in front of the first unvisited index, not dropped"
    assert _same(rec, want_rec, what + " records"), "cloud_nodistortion: the restated ingest + so_icp_deskew_scan, bit for bit"
    assert info.n_surface == len(want_surf) and _same(surf, want_surf, what + " surf"), "cloud_surface: count, order and bits"
    assert info.deskewed == (dinfo is not None)
    if dinfo is not None:
        assert info.n_clamped == dinfo.n_clamped, "only points that became records count"
        assert list(info.q_w_original_l) == list(dinfo.q_w_original_l) and list(info.t_w_original_l) == list(dinfo.t_w_original_l)
    else:
        assert list(info.q_w_original_l) == [0, 0, 0, 1] and list(info.t_w_original_l) == [0, 0, 0] and info.n_clamped == 0


def _run_and_compare(slam, soicp, vals, n_scans, step, branch, seed, what, fields=ur.XYZI, point_step=16, height=1, pad_row=0, **pose_kw):
    buf, w, h, rs = ur.payload(vals, fields, point_step, height, pad_row)
    layout = soicp.untimed_layout(fields, point_step, rs, n_scans, step, 0.2)
    poses, imu, til = _poses(branch, seed, **pose_kw)
    got = slam.extract_features_untimed(buf, w, h, layout, T0, poses, imu, til)
    want = _want(slam, vals, n_scans, step, 0.2, poses, imu, til)
    _check(got, want, what)
    return got, (buf, w, h, layout, poses, imu, til)


@pytest.mark.parametrize("n", [1, 2, 2047, 2048, 2049, 3 * 2048 + 17])
def test_sizes_around_the_tile_bit_for_bit(gpu_slam_factory, soicp, n):
    """one point, two, one short of a tile, a tile, one more, three tiles and a bit: drops in every tile, a cut-off tail at every size"""
    slam = gpu_slam_factory()
    vals = ur.gpu_sweep(f"n{n}")
    for branch in ("none", "imu", "vio"):
        (rec, surf, info), _ = _run_and_compare(slam, soicp, vals, 16, 3, branch, seed=20 + n % 7, what=f"n {n} {branch}")
    assert info.n_points < n or n <= 2


@pytest.mark.parametrize("axis", ["x", "z"])
def test_lidar_mounted_half_a_turn_round(gpu_slam_factory, soicp, axis):
    """T_i_l = 180 degrees about x / z under an IMU buffer: T_l_i * T_original_current of every record, and start * T_i_l, take one of
    matrix_to_quat's hand-written branches (trace <= 0) in untimed_ingest_deskew_kernel's own inlined copy of deskew_point.  The
    sweep is the smallest that spans two tiles."""
    slam = gpu_slam_factory()
    vals = ur.gpu_sweep("n2049")
    buf, w, h, rs = ur.payload(vals)
    layout = soicp.untimed_layout(ur.XYZI, 16, rs, 16, 3, 0.2)
    poses, til = dd.pose_buffer(T0, seed=34, translate=False, flip_signs=True), dd.half_turn_extrinsic(axis)
    plain, _ = ur.ingest(vals["x"], vals["y"], vals["z"], vals["intensity"], 16)
    assert dd.half_turn_census(plain, T0, poses, axis) > 1000
    got = slam.extract_features_untimed(buf, w, h, layout, T0, poses, True, til)
    _check(got, _want(slam, vals, 16, 3, 0.2, poses, True, til), f"half a turn about {axis}")
    assert got[2].n_clamped == 0 and got[2].n_surface > 0


def test_truncation_and_the_clamped_count(gpu_slam_factory, soicp):
    """the cut-off tail spans a tile boundary and holds would-be drops and would-be records (test_untimed_host.py); the pose buffer
    ends in the middle of the sweep, so the tail's points would all be clamped -- and must not be counted"""
    slam = gpu_slam_factory()
    n = 3 * 2048 + 17
    vals = ur.gpu_sweep(f"n{n}")
    for branch in ("imu", "vio"):
        (rec, surf, info), _ = _run_and_compare(slam, soicp, vals, 16, 1, branch, seed=31, what=f"short pose buffer {branch}", after_s=0.01)
        t = rec.view(np.float32)[:, 5]
        assert 0 < info.n_clamped < info.n_points < n and info.n_clamped >= int((t > 0.0105).sum())
    vals = ur.gpu_sweep("all_dropped")
    for branch in ("none", "vio"):
        (rec, surf, info), _ = _run_and_compare(slam, soicp, vals, 32, 3, branch, seed=32, what=f"all dropped {branch}")
        assert (info.n_points, info.n_surface, info.n_clamped, info.deskewed) == (0, 0, 0, 0) and len(rec) == 0 and len(surf) == 0


@pytest.mark.parametrize("n_scans", ur.N_SCANS)
def test_each_scan_count(gpu_slam_factory, soicp, n_scans):
    """the three ring tables and the two values without one (ring 0, nothing dropped); filter_point_size 1 and 3"""
    slam = gpu_slam_factory()
    vals = ur.gpu_sweep(f"scans{n_scans}")
    n = len(vals["x"])
    for step, branch in ((1, "none"), (3, "imu")):
        (rec, surf, info), _ = _run_and_compare(slam, soicp, vals, n_scans, step, branch, seed=40 + n_scans, what=f"N_SCANS {n_scans} step {step} {branch}")
        rings = rec.view(np.uint32)[:, 6]
        if n_scans in (4, 128):
            assert info.n_points == n and not rings.any()
        else:
            assert info.n_points < n and len(np.unique(rings)) >= 12 and rings.max() <= {16: 15, 32: 31, 64: 50}[n_scans]
        assert np.array_equal(rec.view(np.float32)[:, 4], vals["intensity"][ur.ingest(vals["x"], vals["y"], vals["z"], vals["intensity"], n_scans)[1]])


def test_look_back_past_64_workgroups(gpu_slam_factory, soicp):
    """67 tiles, and the visited prefix reaches into tile 65 (test_untimed_host.py), so the workgroup that stores the last records
    has 65 in front of it; the sweep runs past the end of the pose buffer, so n_clamped counts too"""
    slam = gpu_slam_factory()
    vals = ur.gpu_sweep("long")
    (rec, surf, info), _ = _run_and_compare(slam, soicp, vals, 16, 3, "vio", seed=51, what="67 tiles")
    assert 1000 < info.n_clamped < info.n_points < len(vals["x"])
    _run_and_compare(slam, soicp, vals, 16, 1, "none", seed=51, what="67 tiles, no de-skew")


def test_pose_table_in_global_memory(gpu_slam_factory, soicp):
    slam = gpu_slam_factory()
    vals = ur.gpu_sweep("layouts")
    poses, _, _ = _poses("imu", seed=53, rate_hz=8000.0)
    assert len(poses) > 512, "this case takes the kernel's global-memory table path"
    _run_and_compare(slam, soicp, vals, 64, 2, "imu", seed=53, what="long pose table", rate_hz=8000.0)


class _Hip:
    def __init__(self):
        self.h = C.CDLL("libamdhip64.so")
        self.h.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        self.h.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        self.h.hipFree.argtypes = [C.c_void_p]

    def upload(self, a, at=0):
        """a into a fresh allocation, starting `at` bytes in; returns (allocation, address of a[0])"""
        d = C.c_void_p()
        assert self.h.hipMalloc(C.byref(d), max(at + a.nbytes, 1)) == 0
        assert self.h.hipMemcpy(C.c_void_p(d.value + at), a.ctypes.data_as(C.c_void_p), a.nbytes, 1) == 0
        return d, d.value + at

    def download(self, d, nbytes):
        out = np.empty(nbytes, np.uint8)
        if nbytes:
            assert self.h.hipMemcpy(out.ctypes.data_as(C.c_void_p), C.c_void_p(d), nbytes, 2) == 0
        return out


def _dev_run(hip, slam, args, at=0):
    buf, w, h, layout, poses, imu, til = args
    d, addr = hip.upload(buf, at)
    try:
        d_rec, d_surf, info = slam.extract_features_untimed_dev(addr, w, h, layout, T0, poses, imu, til)
        return hip.download(d_rec, 32 * info.n_points).reshape(-1, 32), hip.download(d_surf, 32 * info.n_surface).reshape(-1, 32), info
    finally:
        hip.h.hipFree(d)


def test_layouts_and_the_resident_entry(gpu_slam_factory, soicp):
    """the driver's 16-byte point (dword loads), point_step 18 at an odd base (byte loads), no intensity field, three rows with
    row_step padding: each against the restatement, and the resident entry against the host entry, equal bytes"""
    hip = _Hip()
    slam = gpu_slam_factory()
    vals = ur.gpu_sweep("layouts")
    n = len(vals["x"])
    assert n % 3 == 0
    cases = {"xyzi 16": dict(), "step 18": dict(fields=ur.XYZI_RING_18, point_step=18), "rows": dict(height=3, pad_row=24),
             "rows, step 18": dict(fields=ur.XYZI_RING_18, point_step=18, height=3, pad_row=7)}
    first = None
    for name, kw in cases.items():
        (rec, surf, info), args = _run_and_compare(slam, soicp, vals, 64, 3, "imu", seed=61, what=name, **kw)
        first = first or (rec, surf)
        assert np.array_equal(rec, first[0]) and np.array_equal(surf, first[1]), "the layout does not change the result"
        for at in ((0, 1, 2) if "18" in name else (0,)):
            drec, dsurf, dinfo = _dev_run(hip, slam, args, at=at)
            assert np.array_equal(drec, rec) and np.array_equal(dsurf, surf), f"{name}: resident payload {at} bytes into its buffer"
            assert (dinfo.n_points, dinfo.n_surface, dinfo.n_clamped, dinfo.deskewed) == (info.n_points, info.n_surface, info.n_clamped, info.deskewed)
    no_int = {k: v for k, v in vals.items() if k != "intensity"}
    (rec, surf, info), args = _run_and_compare(slam, soicp, no_int, 64, 3, "imu", seed=61, what="no intensity", fields=ur.XYZ_ONLY, point_step=12)
    assert args[3].off_intensity == -1 and not rec.view(np.uint32)[:, 4].any() and np.array_equal(rec[:, :16], first[0][:, :16])
    drec, dsurf, _ = _dev_run(hip, slam, args)
    assert np.array_equal(drec, rec) and np.array_equal(dsurf, surf)


def test_empty_sweeps(gpu_slam_factory, soicp):
    slam = gpu_slam_factory()
    layout = soicp.untimed_layout(ur.XYZI, 16, 0, 16, 1, 0.2)
    poses = dd.pose_buffer(T0, seed=3)
    for w, h in ((0, 0), (0, 1), (0, 5)):
        rec, surf, info = slam.extract_features_untimed(np.zeros(0, np.uint8), w, h, layout, T0, poses, False, None)
        assert (info.n_points, info.n_surface, info.n_clamped, info.deskewed) == (0, 0, 0, 0) and len(rec) == 0 and len(surf) == 0
        assert list(info.q_w_original_l) == [0, 0, 0, 1]
    d_rec, d_surf, info = slam.extract_features_untimed_dev(0, 0, 1, layout, T0)
    assert info.n_points == 0 and info.n_surface == 0


def test_surf_cloud_into_the_prefilter_and_the_neighbouring_entry(gpu_slam_factory, soicp):
    """*d_surface_out into so_icp_prefilter_scan_dev gives the bits of so_icp_prefilter_scan on the host entry's surf cloud; a
    following so_icp_extract_features_dev on the same context (it shares the output buffers, as documented) gives what a fresh
    context gives, and so does the untimed entry behind it"""
    hip = _Hip()
    vals = ur.gpu_sweep("chain")
    buf, w, h, rs = ur.payload(vals)
    layout = soicp.untimed_layout(ur.XYZI, 16, rs, 16, 3, 0.2)
    poses, imu, til = _poses("vio", seed=71)
    host = gpu_slam_factory(plane_res=0.2)
    rec, surf, info = host.extract_features_untimed(buf, w, h, layout, T0, poses, imu, til)
    _check((rec, surf, info), _want(host, vals, 16, 3, 0.2, poses, imu, til), "chain")
    vbuf, vw, vh, vrs, _ = fr.velodyne_sweep(n=4800, seed=72)
    vlayout = fr.layout_for(fr.SENSOR_VELODYNE, 3, 0.2, row_step=vrs)
    vrec, vsurf, vinfo = host.extract_features(vbuf, vw, vh, vlayout, T0, poses, imu, til)
    dev = gpu_slam_factory(plane_res=0.2)
    d, addr = hip.upload(buf)
    dv, vaddr = hip.upload(vbuf)
    try:
        d_rec, d_surf, dinfo = dev.extract_features_untimed_dev(addr, w, h, layout, T0, poses, imu, til)
        assert (dinfo.n_points, dinfo.n_surface, dinfo.n_clamped) == (info.n_points, info.n_surface, info.n_clamped)
        assert np.array_equal(hip.download(d_surf, surf.nbytes), surf.reshape(-1))
        for auto in (1, 0):
            dp, n_dev, pinfo = dev.prefilter_scan_dev(d_surf, dinfo.n_surface, 32, auto, 0.2, 0.4)
            got = dev.download_scan(dp, n_dev)
            hp, n_host, hinfo = host.prefilter_scan(surf.view(np.float32)[:, :3], auto, 0.2, 0.4)
            want = host.download_scan(hp, n_host)
            assert n_dev == n_host > 0 and np.array_equal(got.view(np.uint32), want.view(np.uint32))
            for k in ("average_distance", "count_far_points", "increase_blind_radius", "line_res", "plane_res", "statistic_in_input_order"):
                assert getattr(pinfo, k) == getattr(hinfo, k), k
        assert np.array_equal(hip.download(d_rec, rec.nbytes), rec.reshape(-1)), "the pre-filter leaves the records alone"
        e_rec, e_surf, einfo = dev.extract_features_dev(vaddr, vw, vh, vlayout, T0, poses, imu, til)
        assert (einfo.n_points, einfo.n_surface, einfo.n_clamped) == (vinfo.n_points, vinfo.n_surface, vinfo.n_clamped)
        assert np.array_equal(hip.download(e_rec, vrec.nbytes), vrec.reshape(-1)) and np.array_equal(hip.download(e_surf, vsurf.nbytes), vsurf.reshape(-1))
        d_rec, d_surf, dinfo = dev.extract_features_untimed_dev(addr, w, h, layout, T0, poses, imu, til)
        assert (dinfo.n_points, dinfo.n_surface, dinfo.n_clamped) == (info.n_points, info.n_surface, info.n_clamped)
        assert np.array_equal(hip.download(d_rec, rec.nbytes), rec.reshape(-1)) and np.array_equal(hip.download(d_surf, surf.nbytes), surf.reshape(-1))
    finally:
        hip.h.hipFree(d)
        hip.h.hipFree(dv)
