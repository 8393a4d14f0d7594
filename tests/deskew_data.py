"""Seeded inputs for the de-skew tests: a sweep of point_os::PointcloudXYZITR-like records and a pose
buffer (IMU orientations or VIO odometry) around it.  Test infrastructure only.

The second half (branch_case and what it is built from) holds the inputs of test_deskew_branches_host.py and
test_gpu_deskew_branches.py: one case per data-dependent path of deskew_math.h, each with a census -- computed here in plain
float64 numpy -- of the paths its points take, which those tests assert on."""
import functools

import numpy as np
from scipy.spatial.transform import Rotation as R


def sweep(n, stride=32, time_off=20, sweep_s=0.1, seed=0, nan_every=0):
    """records [n, stride] uint8: float x y z at 0 4 8, float time at time_off, rising over the sweep (columns share a time)."""
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    xyz = (d * rng.uniform(1.0, 80.0, (n, 1))).astype(np.float32)
    cols = max(n // 64, 1)
    t = (np.minimum(np.arange(n) // 64, cols - 1) / cols * sweep_s).astype(np.float32)
    if nan_every:
        xyz[::nan_every, rng.integers(0, 3)] = np.nan
    rec = np.zeros((n, stride // 4), np.float32)
    rec[:, 0:3] = xyz
    if stride >= 32:
        rec[:, 3] = 1.0
        rec[:, 4] = rng.uniform(0, 255, n).astype(np.float32)
    rec[:, time_off // 4] = t
    return rec.view(np.uint8).reshape(n, stride).copy()


def pose_buffer(t0, rate_hz=200.0, before_s=0.02, after_s=0.13, seed=1, translate=True, flip_signs=False):
    """[m, 8]: time, position, quaternion (x y z w) of a smooth motion: ~1 rad/s about a wobbling axis, ~2 m/s"""
    rng = np.random.default_rng(seed)
    ts = t0 - before_s + np.arange(int((before_s + after_s) * rate_hz) + 1) / rate_hz + 1.234e-4
    w = rng.normal(0, 0.8, 3)
    rot = R.from_rotvec(np.outer(ts - t0, w) + 0.02 * np.sin(np.outer(ts - t0, [7.0, 11.0, 13.0])))
    q = rot.as_quat()
    if flip_signs:
        q[1::2] *= -1.0  # q and -q are the same rotation: slerp must not take the long way round
    v = rng.normal(0, 1.5, 3)
    pos = np.outer(ts - t0, v) + 0.05 * np.sin(np.outer(ts - t0, [5.0, 3.0, 9.0])) if translate else np.zeros((len(ts), 3))
    return np.concatenate([ts[:, None], pos, q], 1)


def field(rec, off):
    return rec[:, off:off + 4].copy().view(np.float32).reshape(-1)


def xyz_of(rec):
    return np.stack([field(rec, 0), field(rec, 4), field(rec, 8)], 1)


def scipy_deskew(rec, time_off, t0, poses, imu, T_i_l=None):
    """the same computation on scipy's Rotation / Slerp (float64 throughout): returns float64 xyz [n, 3]"""
    from scipy.spatial.transform import Slerp
    xyz = xyz_of(rec).astype(np.float64)
    ts = field(rec, time_off).astype(np.float64) + t0
    rots = R.from_quat(poses[:, 4:8])
    sl = Slerp(poses[:, 0], rots)

    def at(t):
        t = np.atleast_1d(t)
        tc = np.clip(t, poses[0, 0], poses[-1, 0])
        r = sl(tc)
        p = np.stack([np.interp(tc, poses[:, 0], poses[:, 1 + k]) for k in range(3)], 1)
        return r, (np.zeros_like(p) if imu else p)
    r0, p0 = at(t0)
    rc, pc = at(ts)
    r0 = R.from_quat(np.repeat(r0.as_quat(), len(ts), 0))
    # T_original_current = T0^-1 * Tc
    roc = r0.inv() * rc
    poc = r0.inv().apply(pc - p0)
    if imu:
        til = np.array([0, 0, 0, 0, 0, 0, 1.0]) if T_i_l is None else np.asarray(T_i_l, float)
        ril, pil = R.from_quat(til[3:]), til[:3]
        rli, pli = ril.inv(), -ril.inv().apply(pil)
        # T_l_i * Toc * T_i_l
        rf = rli * roc * ril
        pf = rli.apply(roc.apply(pil) + poc) + pli
    else:
        rf, pf = roc, poc
    out = rf.apply(xyz) + pf
    bad = ~np.isfinite(xyz).all(1)
    out[bad] = xyz[bad]
    return out


def close_in_ulps(a, b):
    """(fraction of bit-identical values, largest difference in units of the float32 spacing at that magnitude)"""
    a, b = a.reshape(-1), b.reshape(-1)
    same = a.view(np.uint32) == b.view(np.uint32)
    both_nan = np.isnan(a) & np.isnan(b)
    d = np.abs(a.astype(np.float64) - b.astype(np.float64))[~(same | both_nan)]
    ulp = np.spacing(np.maximum(np.abs(a), np.abs(b)).astype(np.float32)).astype(np.float64)[~(same | both_nan)]
    return (same | both_nan).mean(), (d / ulp).max() if len(d) else 0.0


# ------------------------------------------------------------------------------------------------------------------------
# Path-directed cases: every branch of matrix_to_quat, interpolated_pose and quat_slerp, the LDS / global table switch and the
# clamped count at wavefront and workgroup edges.
# ------------------------------------------------------------------------------------------------------------------------
T0 = 1.7e9 + 0.25  # a ROS time stamp, as in the other de-skew tests
TIME_OFF = 20
N_CASE = 4096
TIL_POS = [0.05, -0.02, 0.1]
BEFORE, INTERIOR, CLAMPED = 0, 1, 2  # interpolated_pose: ts before the first entry / between two entries / at or beyond the last


def point_times(n, sweep_s=0.1):
    """a time of its own for every point, rising over the sweep (sweep() gives only n // 64 distinct ones)"""
    return (np.arange(n) / n * sweep_s).astype(np.float32)


def timed_sweep(n, seed, times=None, nan_every=300):
    """sweep()'s 32-byte records (range 1 to 80 m) with a NaN planted every nan_every points, none at the first, and the point
    times given (None: sweep()'s own, 64 points to a time)"""
    rec = sweep(n, seed=seed)
    f = rec.view(np.float32).reshape(n, 8)
    rows = np.arange(nan_every // 2, n, nan_every)
    f[rows, rows % 3] = np.nan
    if times is not None:
        f[:, TIME_OFF // 4] = np.asarray(times, np.float32)
    return rec


def poses_at(ts, t0, seed, translate=True, flip_signs=False):
    """[m, 8] the smooth motion of pose_buffer (~1 rad/s about a wobbling axis, ~2 m/s) sampled at the times given"""
    ts = np.asarray(ts, np.float64)
    rng = np.random.default_rng(seed)
    w = rng.normal(0, 0.8, 3)
    q = R.from_rotvec(np.outer(ts - t0, w) + 0.02 * np.sin(np.outer(ts - t0, [7.0, 11.0, 13.0]))).as_quat()
    if flip_signs:
        q[1::2] *= -1.0
    v = rng.normal(0, 1.5, 3)
    pos = np.outer(ts - t0, v) + 0.05 * np.sin(np.outer(ts - t0, [5.0, 3.0, 9.0])) if translate else np.zeros((len(ts), 3))
    return np.concatenate([ts[:, None], pos, q], 1)


def _imu_times(t0, before_s=0.02, n=31, rate_hz=200.0):
    return t0 - before_s + np.arange(n) / rate_hz + 1.234e-4


def quat_branch(M):
    """which branch of Eigen's matrix -> quaternion (deskew_math.h matrix_to_quat) the rotation matrices M [n, 3, 3] take:
    0 = trace > 0, else 1 + the index of the largest diagonal element (the first one on a tie)"""
    d0, d1, d2 = M[:, 0, 0], M[:, 1, 1], M[:, 2, 2]
    i = np.where(d1 > d0, 1, 0)
    i = np.where(d2 > np.where(i == 1, d1, d0), 2, i)
    return np.where(d0 + d1 + d2 > 0, 0, 1 + i)


def census(rec, time_off, t0, poses, imu, T_i_l=None):
    """The paths of deskew_math.h that the sweep start and every point take, in float64 numpy / scipy (none of the code under test):
      finite [n]            the point is de-skewed at all
      path [n], after [n]   interpolated_pose: BEFORE / INTERIOR / CLAMPED, and the index of the first entry with time > ts
      exact [n]             INTERIOR with ts equal to the time of the entry before it (ratio 0)
      lerp [n], neg [n]     INTERIOR: quat_slerp takes |dot| >= 1 - eps, and dot < 0 (the dot in the header's operation order)
      quat [n, 1 or 3]      matrix_to_quat's branch in T_w_original^-1 * T_w_current, then for an IMU buffer T_l_i * that and
                            (T_l_i * that) * T_i_l
      diag_order [n, 3]     the diagonal elements of T_l_i * T_original_current (VIO buffer: of T_original_current), largest first
      start_path, start_quat   the same for the sweep start: its path, and the branch of start * T_i_l (None for a VIO buffer)"""
    from scipy.spatial.transform import Slerp
    poses = np.asarray(poses, np.float64)
    times, n = poses[:, 0], len(poses)
    ts = field(rec, time_off).astype(np.float64) + t0

    def paths(t):
        after = np.searchsorted(times, t, side="right")  # upper_bound
        path = np.where(after == 0, BEFORE, np.where(after == n, CLAMPED, INTERIOR))
        qb, qa = poses[np.clip(after - 1, 0, n - 1), 4:8], poses[np.clip(after, 0, n - 1), 4:8]
        d = qb[:, 0] * qa[:, 0] + qb[:, 1] * qa[:, 1] + qb[:, 2] * qa[:, 2] + qb[:, 3] * qa[:, 3]
        inside = path == INTERIOR
        return dict(path=path, after=after, exact=inside & (t == times[np.clip(after - 1, 0, n - 1)]),
                    lerp=inside & (np.abs(d) >= 1.0 - np.finfo(np.float64).eps), neg=inside & (d < 0))
    out = paths(ts)
    out["finite"] = np.isfinite(xyz_of(rec)).all(1)
    sl = Slerp(times, R.from_quat(poses[:, 4:8]))
    rc = sl(np.clip(ts, times[0], times[-1]))
    r0 = sl(np.clip([t0], times[0], times[-1]))[0]
    roc = r0.inv() * rc
    mats = [roc.as_matrix()]
    out["start_path"] = int(paths(np.array([t0]))["path"][0])
    out["start_quat"] = None
    if imu:
        ril = R.from_quat([0, 0, 0, 1.0] if T_i_l is None else np.asarray(T_i_l, float)[3:])
        mats += [(ril.inv() * roc).as_matrix(), (ril.inv() * roc * ril).as_matrix()]
        out["start_quat"] = int(quat_branch((r0 * ril).as_matrix()[None])[0])
    out["quat"] = np.stack([quat_branch(m) for m in mats], 1)
    out["diag_order"] = np.argsort(-np.diagonal(mats[1 if imu else 0], axis1=1, axis2=2), axis=1)
    return out


class Case:
    """one de-skew input (the arguments of so_icp_deskew_scan) and the census of the paths it takes"""

    def __init__(self, name, rec, poses, imu, T_i_l=None):
        self.name, self.rec, self.poses, self.imu, self.T_i_l = name, rec, np.ascontiguousarray(poses, np.float64), imu, T_i_l
        self.time_off, self.t0 = TIME_OFF, T0
        self.census = census(rec, TIME_OFF, T0, self.poses, imu, T_i_l)

    @property
    def args(self):
        return self.rec, self.time_off, self.t0, self.poses, self.imu, self.T_i_l


# T_i_l rotations (x y z w) of a lidar mounted upside down or sideways; the three half turns are exact
EXTRINSICS = {
    "ext_x180": [1.0, 0, 0, 0], "ext_y180": [0, 1.0, 0, 0], "ext_z180": [0, 0, 1.0, 0],
    "ext_near_y": R.from_rotvec([0, -np.deg2rad(175.0), 0.02]).as_quat(),
    "ext_near_z": R.from_rotvec([0.01, 0, np.deg2rad(178.0)]).as_quat(),
    "ext_tie_xy": [np.sqrt(0.5), np.sqrt(0.5), 0, 0],  # half a turn about (1, 1, 0): the two largest diagonal elements tie to rounding
    "ext_111_125": R.from_rotvec(np.deg2rad(125.0) * np.ones(3) / np.sqrt(3.0)).as_quat(),
}
# 170 degrees about an axis in general position, one for each order of the three diagonal elements (the name lists them largest
# first): the two comparisons that pick matrix_to_quat's branch meet every outcome, each by a wide margin
DIAG_ORDERS = ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0))
for _o in DIAG_ORDERS:
    _axis = np.zeros(3)
    _axis[list(_o)] = [0.85, -0.5, 0.15]
    EXTRINSICS["ext_diag_%d%d%d" % _o] = R.from_rotvec(np.deg2rad(170.0) * _axis / np.linalg.norm(_axis)).as_quat()


def half_turn_extrinsic(axis):
    """T_i_l [7] of a lidar turned 180 degrees about "x", "y" or "z", with a lever arm"""
    return np.concatenate([TIL_POS, np.asarray(EXTRINSICS[f"ext_{axis}180"], np.float64)])


def half_turn_census(rec, t0, poses, axis):
    """the number of finite records whose T_l_i * T_original_current takes matrix_to_quat's hand-written branch for that axis, under an
    IMU buffer and half_turn_extrinsic(axis); asserts that all of them do, and the sweep start's start * T_i_l too"""
    q = census(rec, TIME_OFF, t0, poses, True, half_turn_extrinsic(axis))
    branch = 1 + "xyz".index(axis)
    n = int(q["finite"].sum())
    assert (q["quat"][q["finite"], 1] == branch).sum() == n and q["start_quat"] == branch
    return n


def _extrinsic_case(name):
    """IMU buffer (sign-flipped neighbours), T_i_l with a large rotation and a translation"""
    k = list(EXTRINSICS).index(name)
    til = np.concatenate([TIL_POS, np.asarray(EXTRINSICS[name], np.float64)])
    return Case(name, timed_sweep(N_CASE, 500 + k, point_times(N_CASE)), pose_buffer(T0, seed=520 + k, translate=False, flip_signs=True), True, til)


def _spin_case(name):
    """VIO buffer: 31 poses at 200 Hz turning at 40 rad/s about one axis (neighbours 0.2 rad apart) while translating; the rotation
    since the sweep start passes 120 degrees at 0.052 s"""
    k = "xyz".index(name[-1])
    ts = _imu_times(T0)
    poses = poses_at(ts, T0, 540 + k, translate=True)
    poses[:, 4:8] = R.from_rotvec(np.outer(ts - T0, 40.0 * np.eye(3)[k])).as_quat()
    return Case(name, timed_sweep(N_CASE, 530 + k, point_times(N_CASE)), poses, False)


def _exact_case(name):
    """table times = T0 + (double)t for every fourth of the sweep's own float32 point times (64 points share one), plus one entry
    before the sweep and one after it: a quarter of the points, and the sweep start, sit exactly on an entry"""
    rec = timed_sweep(N_CASE, 550)
    hit = np.unique(field(rec, TIME_OFF))[::4].astype(np.float64) + T0
    ts = np.concatenate([[T0 - 0.01], hit, [T0 + 0.11]])
    imu = name.endswith("imu")
    return Case(name, rec, poses_at(ts, T0, 551, translate=not imu, flip_signs=True), imu, np.concatenate([TIL_POS, EXTRINSICS["ext_near_y"]]) if imu else None)


def _late_case(name):
    """the buffer starts 0.03 s into the sweep: the sweep start and the early points get the first pose.  late_short ends at 0.07 s too"""
    short = name == "late_short"
    ts = T0 + 0.03 + np.arange(9 if short else 21) / 200.0 + 1.234e-4
    if short:  # IMU buffer with an extrinsic
        return Case(name, timed_sweep(N_CASE, 560, point_times(N_CASE)), poses_at(ts, T0, 561, translate=False, flip_signs=True), True,
                    np.concatenate([TIL_POS, R.from_rotvec([0.01, -0.02, 0.5]).as_quat()]))
    return Case(name, timed_sweep(N_CASE, 562, point_times(N_CASE)), poses_at(ts, T0, 563, translate=True), False)


def _edge_case(name):
    """edge511 / edge512 / edge513: a table of that many poses spans the sweep and its last entry is the first one past the sweep's
    end, so the last points have it as their "after".  tail512 / tail513: the table ends mid-sweep, so the clamped points read it."""
    n = int(name[-3:])
    ts = T0 + np.linspace(-0.002, 0.1 if name.startswith("edge") else 0.05, n)
    return Case(name, timed_sweep(N_CASE, 570 + n % 7, point_times(N_CASE)), poses_at(ts, T0, 580 + n % 7, translate=True, flip_signs=True), False)


SLERP_STEP, LERP_STEP = 1e-7, 2e-8  # rad between neighbours: dot = 1 - 1.25e-15 (slerp side), dot rounds to 1 (lerp side)


def _threshold_case(name):
    """neighbouring orientations on either side of slerp's |dot| >= 1 - eps.  Three orientations A, B = A turned by 2e-8 rad and
    C = A turned by 1e-7 rad, in a pattern of period 4 that meets both signs of the dot on each side:
      lerp   A  B -A -B      slerp   A  C -A -C      both   A  B -A  C   (lerp +, lerp -, slerp -, slerp +)"""
    kind = name.split("_")[1]
    imu = kind != "both"
    poses = _threshold_poses(_imu_times(T0), kind, 590, translate=not imu)
    return Case(name, timed_sweep(N_CASE, 591 + len(kind), point_times(N_CASE)), poses, imu, None)


def _threshold_poses(ts, kind, seed, translate):
    a = R.from_rotvec([0.3, -0.5, 0.2])
    axis = np.array([0.6, 0.0, 0.8])
    A = a.as_quat()
    B = (a * R.from_rotvec(axis * LERP_STEP)).as_quat()
    C = (a * R.from_rotvec(axis * SLERP_STEP)).as_quat()
    pattern = {"lerp": [A, B, -A, -B], "slerp": [A, C, -A, -C], "both": [A, B, -A, C]}[kind]
    poses = poses_at(ts, T0, seed, translate=translate)
    poses[:, 4:8] = [pattern[k % 4] for k in range(len(ts))]
    return poses


CLAMP_SIZES = (1, 63, 64, 65, 255, 256, 257, 4096 + 37)  # a wavefront is 64 lanes, a workgroup 256 threads


def _clamp_case(name):
    """clampN: N points against a VIO buffer that ends 0.05 s into the sweep; gone1 / gone63: against one that ends before the sweep
    starts, so that a sweep shorter than a wavefront has every finite point clamped.  These are about the count: the buffer
    translates and its orientations are threshold_lerp's, so no point meets acos / sin and host and device agree on every bit of
    a sweep too short for a share of equal values to mean anything."""
    n = int(name[5:] if name.startswith("clamp") else name[4:])
    rec = timed_sweep(n, 600 + n % 11, point_times(n), nan_every=100)
    ts = _imu_times(T0, before_s=0.2) if name.startswith("gone") else _imu_times(T0, n=15)
    return Case(name, rec, _threshold_poses(ts, "lerp", 601, translate=True), False)


_BUILDERS = {**{k: _extrinsic_case for k in EXTRINSICS}, **{f"spin_{a}": _spin_case for a in "xyz"},
             "exact_vio": _exact_case, "exact_imu": _exact_case, "late": _late_case, "late_short": _late_case,
             **{k: _edge_case for k in ("edge511", "edge512", "edge513", "tail512", "tail513")},
             **{f"threshold_{k}": _threshold_case for k in ("lerp", "slerp", "both")},
             **{f"clamp{n}": _clamp_case for n in CLAMP_SIZES}, "gone1": _clamp_case, "gone63": _clamp_case}
BRANCH_CASES = tuple(_BUILDERS)


@functools.lru_cache(maxsize=None)
def branch_case(name):
    """the Case of that name, built once; its arrays are shared, so callers leave them as they are"""
    return _BUILDERS[name](name)
