"""-m gpu: so_icp_extract_features_livox(_dev) -- featureExtraction::livoxHandler's sweep -> LaserFeature clouds on the device --
against the restatement (tests/livox_ref.py), bit for bit: records, surf cloud, counts and the sweep-start pose.  As for the other
sensors (test_gpu_feature_extraction.py) the de-skew between the restated ingest and the restated sampling is the library's
so_icp_deskew_scan (deskew_kernel, itself held to the oracle in test_gpu_deskew.py): the fused kernel must give its bits.
tests/test_livox_host.py checks that every sweep used here carries rejected points, zero-record runs and division / multiplication
differences."""
import ctypes as C

import numpy as np
import pytest
from scipy.spatial.transform import Rotation as R

import deskew_data as dd
import feature_extraction_ref as fr
import livox_ref as lr
from helpers import assert_same_bits
from superodom_amd import synth

pytestmark = pytest.mark.gpu
T0 = 1.7e9 + 0.25
T_I_L = np.concatenate([[0.05, -0.02, 0.1], R.from_rotvec([0.01, -0.02, 0.5]).as_quat()])


def _poses(branch, seed, rate_hz=200.0):
    if branch == "none":
        return None, False, None
    if branch == "imu":
        return dd.pose_buffer(T0, rate_hz=rate_hz, seed=seed, translate=False, flip_signs=True), True, T_I_L
    return dd.pose_buffer(T0, rate_hz=rate_hz, seed=seed, translate=True), False, None


def _want(slam, vals, layout, poses, imu, til, time_of=lr.time_div):
    """(records, surf cloud, DeskewInfo or None): restated ingest, so_icp_deskew_scan, restated sampling"""
    rec = lr.ingest(vals, np.array(layout.R_imu_laser_gravity[:]), layout.n_scans, time_of)
    dinfo = None
    if poses is not None:
        rec, dinfo = slam.deskew_scan(rec, 20, T0, poses, imu, til)
    return rec, fr.surf_sample(rec, layout.filter_point_size, layout.min_range), dinfo


def _same(a, b, what=""):
    """bit for bit, except that a NaN coordinate only has to be a NaN (its payload and sign come from the unit that made it), as in
    test_gpu_feature_extraction.py"""
    if a.shape != b.shape:
        print(what, "shapes", a.shape, b.shape)
        return False
    wa, wb = a.view(np.uint32).reshape(len(a), 8), b.view(np.uint32).reshape(len(b), 8)
    fa, fb = wa.view(np.float32), wb.view(np.float32)
    eq = wa == wb
    eq[:, :3] |= np.isnan(fa[:, :3]) & np.isnan(fb[:, :3])
    if eq.all():
        return True
    rows = np.nonzero(~eq.all(1))[0]
    print(f"{what}: {len(rows)} of {len(a)} records differ; first: {rows[:5].tolist()}")
    for r in rows[:5]:
        print(r, fa[r].tolist(), fb[r].tolist(), [hex(v) for v in wa[r]], [hex(v) for v in wb[r]])
    return False


def _check_info(info, dinfo, n):
    assert info.n_points == n and info.deskewed == (dinfo is not None)
    if dinfo is not None:
        assert info.n_clamped == dinfo.n_clamped
        assert list(info.q_w_original_l) == list(dinfo.q_w_original_l) and list(info.t_w_original_l) == list(dinfo.t_w_original_l)
    else:
        assert list(info.q_w_original_l) == [0, 0, 0, 1] and list(info.t_w_original_l) == [0, 0, 0] and info.n_clamped == 0


def _run_and_compare(slam, vals, layout, poses, imu, til, what):
    n = len(vals["x"])
    rec, surf, info = slam.extract_features_livox(synth.livox_points(vals), n, layout, T0, poses, imu, til)
    want_rec, want_surf, dinfo = _want(slam, vals, layout, poses, imu, til)
    assert _same(rec, want_rec, what + " records"), "cloud_nodistortion: the restated ingest + so_icp_deskew_scan, bit for bit"
    assert info.n_surface == len(want_surf) > 0 and _same(surf, want_surf, what + " surf"), "cloud_surface: count, order and bits"
    _check_info(info, dinfo, n)
    return rec, surf, info


@pytest.mark.parametrize("branch", ["imu", "vio", "none"])
@pytest.mark.parametrize("step", [1, 3, 7])
def test_main_sweep_bit_for_bit(gpu_slam_factory, soicp, branch, step):
    """a non-identity R (3 degrees of roll, -2 of pitch) and, for the IMU branch, a T_i_l with a translation"""
    slam = gpu_slam_factory()
    vals = lr.gpu_sweep(f"main{step}")
    layout = soicp.livox_layout(step, 0.2, R_imu_laser_gravity=lr.R_TILT)
    poses, imu, til = _poses(branch, seed=20 + step)
    rec, surf, info = _run_and_compare(slam, vals, layout, poses, imu, til, f"{branch} step {step}")
    f = rec.view(np.float32)
    acc = lr.accepted(vals)
    assert np.array_equal(f[acc, 4], vals["reflectivity"][acc].astype(np.float32)) and np.array_equal(rec.view(np.uint32)[acc, 6], vals["line"][acc])


@pytest.mark.parametrize("axis", ["x", "z"])
def test_lidar_mounted_half_a_turn_round(gpu_slam_factory, soicp, axis):
    """T_i_l = 180 degrees about x / z under an IMU buffer: T_l_i * T_original_current of every record, and start * T_i_l, take one of
    matrix_to_quat's hand-written branches (trace <= 0) in livox_ingest_deskew_kernel's own inlined copy of deskew_point"""
    slam = gpu_slam_factory()
    vals = lr.gpu_sweep("cdr")
    layout = soicp.livox_layout(1, 0.2, R_imu_laser_gravity=lr.R_TILT)
    poses, til = dd.pose_buffer(T0, seed=33, translate=False, flip_signs=True), dd.half_turn_extrinsic(axis)
    plain = lr.ingest(vals, np.array(layout.R_imu_laser_gravity[:]), layout.n_scans, lr.time_div)
    assert dd.half_turn_census(plain, T0, poses, axis) > 2500
    _, _, info = _run_and_compare(slam, vals, layout, poses, True, til, f"half a turn about {axis}")
    assert info.n_clamped == 0


def test_zero_records(gpu_slam_factory, soicp):
    """a rejected slot is the zero record before the de-skew, goes through the de-skew like any finite point, and is a sampling
    candidate: behind a point it is kept (|dx| > 1e-7), behind another zero record it is dropped"""
    slam = gpu_slam_factory()
    vals = lr.gpu_sweep("zero")
    n = len(vals["x"])
    acc = lr.accepted(vals)
    layout = soicp.livox_layout(1, 0.2, R_imu_laser_gravity=lr.R_TILT)
    rec, surf, info = _run_and_compare(slam, vals, layout, None, False, None, "zero, no de-skew")
    assert not rec[~acc].any() and rec[acc].view(np.uint32)[:, :3].any(1).all(), "rejected: 32 zero bytes; accepted: a point"
    zero_in_surf = int((~surf.view(np.uint32)[:, :3].any(1)).sum())
    behind_point = ~acc[1:] & acc[:-1]
    assert zero_in_surf == int(behind_point.sum()) > 50, "the predicate a || b || (c && d) keeps a zero record behind a point"
    assert int((~acc[1:] & ~acc[:-1]).sum()) > 20 and info.n_surface == (n - 1) - int((~acc[1:] & ~acc[:-1]).sum()), "and drops one behind a zero record"
    poses, imu, til = _poses("vio", seed=23)
    rec2, surf2, _ = _run_and_compare(slam, vals, layout, poses, imu, til, "zero, vio")
    moved = rec2[~acc].view(np.uint32)
    assert len(np.unique(moved, axis=0)) == 1 and not moved[:, 3:].any(), "time 0: all of them through the sweep start's transform"


def test_identity_R_multiplies_too(gpu_slam_factory, soicp):
    """+inf, -inf and NaN coordinates: R * p with R = I makes the other two coordinates NaN (0 * inf), as Eigen's product does; such
    a point then stays out of the de-skew"""
    slam = gpu_slam_factory()
    vals, at = lr.special_sweep()
    layout = soicp.livox_layout(2, 0.2)
    assert list(layout.R_imu_laser_gravity) == [1, 0, 0, 0, 1, 0, 0, 0, 1]
    for branch in ("none", "imu"):
        poses, imu, til = _poses(branch, seed=29)
        rec, _, _ = _run_and_compare(slam, vals, layout, poses, imu, til, f"special {branch}")
        f = rec.view(np.float32)
        for k, i in at.items():
            ax = "xyz".index(k[0])
            others = [a for a in range(3) if a != ax]
            assert np.isnan(f[i, others]).all(), (k, f[i, :3])
            if k.endswith("inf"):
                assert f[i, ax] == (np.inf if k[1] == "+" else -np.inf), (k, f[i, :3])
            else:
                assert np.isnan(f[i, ax])
        fin = np.ones(len(f), bool); fin[list(at.values())] = False
        assert np.isfinite(f[fin, :3]).all()


def test_time_is_a_division(gpu_slam_factory, soicp):
    """time = (float)offset_time / 1e9f, correctly rounded -- and the comparison would catch the multiplication by 1e-9f"""
    slam = gpu_slam_factory()
    vals = lr.gpu_sweep("time")
    n = len(vals["x"])
    acc = lr.accepted(vals)
    differ = acc & (lr.time_div(vals["offset_time"]) != lr.time_mul(vals["offset_time"]))
    assert differ.sum() >= 1000
    layout = soicp.livox_layout(3, 0.2, R_imu_laser_gravity=lr.R_TILT)
    rec, surf, _ = _run_and_compare(slam, vals, layout, None, False, None, "time")
    assert np.array_equal(rec.view(np.float32)[acc, 5].view(np.uint32), lr.time_div(vals["offset_time"])[acc].view(np.uint32))
    wrong_rec, wrong_surf, _ = _want(slam, vals, layout, None, False, None, time_of=lr.time_mul)
    assert not np.array_equal(rec, wrong_rec) and not np.array_equal(surf, wrong_surf), "the multiply form fails this comparison"
    assert int((rec.view(np.uint32)[:, 5] != wrong_rec.view(np.uint32)[:, 5]).sum()) == int(differ.sum())


class _Hip:
    def __init__(self):
        self.h = C.CDLL("libamdhip64.so")
        self.h.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        self.h.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        self.h.hipFree.argtypes = [C.c_void_p]

    def upload(self, a, at=0, room=0):
        """a into a fresh allocation of at + len(a) + room bytes, starting `at` bytes in; returns (allocation, address of a[0])"""
        d = C.c_void_p()
        assert self.h.hipMalloc(C.byref(d), max(at + a.nbytes + room, 1)) == 0
        assert self.h.hipMemcpy(C.c_void_p(d.value + at), a.ctypes.data_as(C.c_void_p), a.nbytes, 1) == 0
        return d, d.value + at

    def download(self, d, nbytes):
        out = np.empty(nbytes, np.uint8)
        if nbytes:
            assert self.h.hipMemcpy(out.ctypes.data_as(C.c_void_p), C.c_void_p(d), nbytes, 2) == 0
        return out


def _dev_run(hip, slam, payload, n, layout, poses, imu, til, at=0):
    d, addr = hip.upload(payload, at)
    try:
        d_rec, d_surf, info = slam.extract_features_livox_dev(addr, n, layout, T0, poses, imu, til)
        return hip.download(d_rec, 32 * n).reshape(n, 32), hip.download(d_surf, 32 * info.n_surface).reshape(-1, 32), info
    finally:
        hip.h.hipFree(d)


def test_unaligned_and_packed_payloads(gpu_slam_factory, soicp):
    """_dev with the payload 0 .. 3 bytes into a device buffer (point_step 20: dword loads only at 0), and a point_step 19 packed
    payload that ends with the allocation's used bytes: all equal the aligned run and the host entry"""
    hip = _Hip()
    slam = gpu_slam_factory()
    vals = lr.gpu_sweep("loads")
    n = len(vals["x"])
    poses, imu, til = _poses("imu", seed=43)
    layout = soicp.livox_layout(3, 0.2, R_imu_laser_gravity=lr.R_TILT)
    rec, surf, info = _run_and_compare(slam, vals, layout, poses, imu, til, "loads, host entry")
    payload = synth.livox_points(vals, fill=0xA5)
    assert payload.nbytes == 20 * n - 1, "the last point has 19 bytes"
    for at in range(4):
        drec, dsurf, dinfo = _dev_run(hip, slam, payload, n, layout, poses, imu, til, at=at)
        assert np.array_equal(drec, rec) and np.array_equal(dsurf, surf), f"payload {at} bytes into the buffer"
        assert (dinfo.n_surface, dinfo.n_clamped, dinfo.n_points) == (info.n_surface, info.n_clamped, info.n_points)
    packed = synth.livox_points(vals, point_step=19)
    assert packed.nbytes == 19 * n
    lay19 = soicp.livox_layout(3, 0.2, R_imu_laser_gravity=lr.R_TILT, point_step=19)
    for at in (0, 1):
        drec, dsurf, _ = _dev_run(hip, slam, packed, n, lay19, poses, imu, til, at=at)
        assert np.array_equal(drec, rec) and np.array_equal(dsurf, surf), f"packed 19-byte points, {at} bytes into the buffer"
    hrec, hsurf, _ = slam.extract_features_livox(packed, n, lay19, T0, poses, imu, til)
    assert np.array_equal(hrec, rec) and np.array_equal(hsurf, surf)
    # fields in another order inside a 24-byte point: the offsets are data
    offs = {"line": 0, "tag": 1, "reflectivity": 2, "z": 4, "offset_time": 8, "x": 12, "y": 16}
    buf = np.full((n, 24), 0x5A, np.uint8)
    std = synth.livox_points(vals, trim_last=False).reshape(n, 20)
    for name, o in offs.items():
        w = 4 if name in ("offset_time", "x", "y", "z") else 1
        src = soicp.LIVOX_CUSTOM_POINT[name]
        buf[:, o:o + w] = std[:, src:src + w]
    lay24 = soicp.livox_layout(3, 0.2, R_imu_laser_gravity=lr.R_TILT, point_step=24, offsets=offs)
    for at in (0, 2):
        drec, dsurf, _ = _dev_run(hip, slam, buf.reshape(-1), n, lay24, poses, imu, til, at=at)
        assert np.array_equal(drec, rec) and np.array_equal(dsurf, surf)


def test_pose_table_in_global_memory(gpu_slam_factory, soicp):
    slam = gpu_slam_factory()
    vals = lr.gpu_sweep("poses")
    layout = soicp.livox_layout(2, 0.2, R_imu_laser_gravity=lr.R_TILT)
    poses, imu, til = _poses("imu", seed=53, rate_hz=8000.0)
    assert len(poses) > 512, "this case takes the kernel's global-memory table path"
    _run_and_compare(slam, vals, layout, poses, imu, til, "long pose table")


def test_deskew_equals_deskew_scan_on_the_ingested_records(gpu_slam_factory, soicp):
    """the library's own two steps: ingest alone (n_poses = 0), then so_icp_deskew_scan on those records"""
    slam = gpu_slam_factory()
    vals = lr.gpu_sweep("deskew")
    n = len(vals["x"])
    layout = soicp.livox_layout(3, 0.2, R_imu_laser_gravity=lr.R_TILT)
    payload = synth.livox_points(vals)
    plain, _, pinfo = slam.extract_features_livox(payload, n, layout, T0)
    assert pinfo.deskewed == 0 and np.array_equal(plain, lr.ingest(vals, lr.R_TILT))
    for branch in ("imu", "vio"):
        poses, imu, til = _poses(branch, seed=63)
        rec, _, info = slam.extract_features_livox(payload, n, layout, T0, poses, imu, til)
        want, dinfo = slam.deskew_scan(plain, 20, T0, poses, imu, til)
        assert np.array_equal(rec, want) and info.n_clamped == dinfo.n_clamped and info.deskewed == 1
        assert not np.array_equal(rec, plain)


def test_empty_and_tiny_sweeps(gpu_slam_factory, soicp):
    slam = gpu_slam_factory()
    layout = soicp.livox_layout(1, 0.2)
    vals = lr.gpu_sweep("cdr")
    poses = dd.pose_buffer(T0, seed=3)
    for k in (0, 1, 2):
        v = {name: a[:k] for name, a in vals.items()}
        rec, surf, info = slam.extract_features_livox(synth.livox_points(v), k, layout, T0, poses, False, None)
        want_rec, want_surf, _ = _want(slam, v, layout, poses, False, None) if k else (np.zeros((0, 32), np.uint8), np.zeros((0, 32), np.uint8), None)
        assert info.n_points == k and info.n_surface == len(want_surf) and _same(rec, want_rec) and _same(surf, want_surf)
    d_rec, d_surf, info = slam.extract_features_livox_dev(0, 0, layout, T0)
    assert info.n_points == 0 and info.n_surface == 0


def test_payload_of_a_serialised_custom_msg(gpu_slam_factory, soicp):
    """the points inside a CDR CustomMsg, handed over where they lie (point_step 20, 19 bytes for the last), give the bits of the
    same points in a bare array -- from host memory at any address and from device memory"""
    hip = _Hip()
    slam = gpu_slam_factory()
    vals = lr.gpu_sweep("cdr")
    n = len(vals["x"])
    poses, imu, til = _poses("vio", seed=73)
    layout = soicp.livox_layout(3, 0.2, R_imu_laser_gravity=lr.R_TILT)
    rec, surf, info = _run_and_compare(slam, vals, layout, poses, imu, til, "bare array")
    for frame in ("", "l", "li", "liv", "livox_frame"):
        msg = np.frombuffer(lr.encode_custom_msg(lr.custom_msg(vals, frame_id=frame)), np.uint8)
        at, point_num, count = lr.points_in_cdr(msg)
        assert point_num == count == n and len(msg) == at + 20 * n - 1
        hrec, hsurf, hinfo = slam.extract_features_livox(msg[at:], n, layout, T0, poses, imu, til)
        assert np.array_equal(hrec, rec) and np.array_equal(hsurf, surf) and hinfo.n_surface == info.n_surface
    d, addr = hip.upload(msg)  # the whole message resident, the points where the message has them
    try:
        d_rec, d_surf, dinfo = slam.extract_features_livox_dev(addr + at, n, layout, T0, poses, imu, til)
        assert np.array_equal(hip.download(d_rec, 32 * n).reshape(n, 32), rec)
        assert np.array_equal(hip.download(d_surf, 32 * dinfo.n_surface).reshape(-1, 32), surf)
    finally:
        hip.h.hipFree(d)


def test_resident_chain_equals_the_host_chain(gpu_slam_factory, soicp):
    """sweep -> so_icp_extract_features_livox_dev -> so_icp_prefilter_scan_dev -> so_icp_localization_dev against the same chain
    through host buffers, at the livox_mid360-like operating point (planeRes 0.1, 4 000 surface features) on synth's mid360_like
    scene: same poses, statistics and map"""
    hip = _Hip()
    sc = synth.Scene("mid360_like")
    frames = [lr.chain_sweep(k, sc.scan(k)) for k in range(3)]
    layout = soicp.livox_layout(3, 0.2, R_imu_laser_gravity=lr.R_TILT)
    res = {}
    for mode in ("host", "dev"):
        slam = gpu_slam_factory(plane_res=sc.plane_res, line_res=sc.plane_res / 2, max_surface_features=4000, max_iterations=4)
        slam.add_surf_point_cloud(sc.map_points)
        out = []
        for k, vals in enumerate(frames):
            n = len(vals["x"])
            t = T0 + 0.1 * k
            poses = lr.small_motion_poses(t, seed=90 + k)
            payload = synth.livox_points(vals)
            if mode == "dev":
                d, addr = hip.upload(payload)
                try:
                    _, d_surf, info = slam.extract_features_livox_dev(addr, n, layout, t, poses, False, None)
                    dp, n_f, pinfo = slam.prefilter_scan_dev(d_surf, info.n_surface, 32, 1, sc.plane_res / 2, sc.plane_res)
                finally:
                    hip.h.hipFree(d)
                rc, p, st = slam.localization_dev(True, sc.guess(k), dp, n_f, t)
            else:
                _, surf, info = slam.extract_features_livox(payload, n, layout, t, poses, False, None)
                dp, n_f, pinfo = slam.prefilter_scan(surf.view(np.float32)[:, :3], 1, sc.plane_res / 2, sc.plane_res)
                filt = slam.download_scan(dp, n_f)
                rc, p, st = slam.localization(True, sc.guess(k), filt, t)
            out.append((rc, p.copy(), st, n_f, pinfo.plane_res, int(info.n_surface)))
        res[mode] = (out, slam.export_map())
    (ho, hm), (do, dm) = res["host"], res["dev"]
    print([(o[0], o[2].n_iterations, o[3], o[5], synth.pose_error(o[1], sc.gt_pose(k))) for k, o in enumerate(ho)])
    assert [o[0] for o in ho] == [0, 0, 0] and all(o[2].n_iterations > 0 for o in ho), [o[0] for o in ho]
    for k, (a, b) in enumerate(zip(ho, do)):
        assert a[0] == b[0] and np.array_equal(a[1], b[1]) and a[3:] == b[3:]
        assert_same_bits(a[2], b[2], ("frame", k))
    assert np.array_equal(hm.view(np.uint32), dm.view(np.uint32))
