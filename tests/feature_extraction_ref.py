"""Numpy restatement of featureExtraction's per-sweep point work (src/FeatureExtraction/featureExtraction.cpp), exact in
float32 / float64, and seeded sweeps in the two sensor_msgs::PointCloud2 layouts the node ingests.  Test infrastructure only.

  ingest()       laserCloudHandler (:710-766): pcl::fromROSMsg into point_os::PointcloudXYZITR; for the Ouster
                 utils::transformOusterPoints (superodom_utils.cpp:202-209) and time = (float)t * 1e-9f
  surf_sample()  uniformFeatureExtraction (:504-525)
The de-skew between them is the library's own so_icp_deskew_scan (checked against oracle.deskew in test_gpu_deskew.py)."""
import numpy as np

from superodom_amd.binding import FLOAT32, FLOAT64, SENSOR_OUSTER, SENSOR_VELODYNE, T_OUSTER_SENSOR, UINT16, UINT32

# the driver layouts: (name, offset, datatype, count)
OUSTER_FIELDS = [("x", 0, FLOAT32, 1), ("y", 4, FLOAT32, 1), ("z", 8, FLOAT32, 1), ("intensity", 16, FLOAT32, 1), ("t", 20, UINT32, 1),
                 ("reflectivity", 24, UINT16, 1), ("ring", 26, UINT16, 1), ("ambient", 28, UINT16, 1), ("range", 32, UINT32, 1)]
OUSTER_POINT_STEP = 48   # ouster_ros os_point
VELODYNE_FIELDS = [("x", 0, FLOAT32, 1), ("y", 4, FLOAT32, 1), ("z", 8, FLOAT32, 1), ("intensity", 12, FLOAT32, 1), ("ring", 16, UINT16, 1),
                   ("time", 18, FLOAT32, 1)]
VELODYNE_POINT_STEP = 22  # velodyne_pointcloud PointXYZIRT: time at byte 18, not 4-byte aligned

_NP = {FLOAT32: np.float32, FLOAT64: np.float64, UINT16: np.uint16, UINT32: np.uint32}


def _box_ranges(dirs, half=(18.0, 11.0), floor=-1.6, ceil=3.2):
    """distance along unit rays from the sensor to the walls, floor and ceiling of a box room (planar structure to register)"""
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.full(len(dirs), np.inf)
        for ax, lim in ((0, half[0]), (1, half[1])):
            d = dirs[:, ax]
            tt = np.where(d > 0, lim / d, np.where(d < 0, -lim / d, np.inf))
            t = np.minimum(t, tt)
        d = dirs[:, 2]
        t = np.minimum(t, np.where(d > 0, ceil / d, np.where(d < 0, floor / d, np.inf)))
    return t


def make_payload(fields, point_step, n, values, row_step=None, height=1, pad_row=0, seed=0):
    """PointCloud2 data: n points, point_step bytes apart, rows of n / height points row_step bytes apart; values: name -> array"""
    width = n // height
    row_step = row_step if row_step is not None else width * point_step + pad_row
    buf = np.random.default_rng(seed).integers(0, 256, row_step * height, dtype=np.uint8)  # bytes no field covers hold garbage
    rows = np.arange(n) // width
    cols = np.arange(n) - rows * width
    base = rows * row_step + cols * point_step
    for name, off, dt, _count in fields:
        if name not in values:
            continue
        v = np.ascontiguousarray(np.asarray(values[name]).astype(_NP[dt])).view(np.uint8).reshape(n, -1)
        for b in range(v.shape[1]):
            buf[base + off + b] = v[:, b]
    return buf, width, height, row_step


def ouster_sweep(width=1024, height=128, seed=0, sweep_s=0.1, nan_every=0, zero_every=0, shift=(0.0, 0.0, 0.0)):
    """an os1-like sweep (height beams x width columns, row-major by beam) of a box room, in the Ouster frame: returns the
    PointCloud2 payload, width, height, row_step, and the field values"""
    rng = np.random.default_rng(seed)
    az = -2 * np.pi * (np.arange(width) / width)
    el = np.deg2rad(np.linspace(22.5, -22.5, height))
    A, E = np.meshgrid(az, el)
    dirs = np.stack([np.cos(E) * np.cos(A), np.cos(E) * np.sin(A), np.sin(E)], -1).reshape(-1, 3)
    r = _box_ranges(dirs) * (1 + rng.normal(0, 0.002, len(dirs)))
    xyz = (dirs * r[:, None] + np.asarray(shift)).astype(np.float32)
    xyz[:, 0] *= -1; xyz[:, 1] *= -1  # sensor -> Ouster frame (T_ouster_sensor's R is diag(-1, -1, 1))
    n = width * height
    t_ns = np.tile((np.arange(width) * (sweep_s * 1e9 / width)).astype(np.uint32), height)
    if zero_every:
        xyz[::zero_every] = 0.0  # no return: the driver writes 0 0 0
    if nan_every:
        xyz[3::nan_every, rng.integers(0, 3)] = np.nan
    vals = {"x": xyz[:, 0], "y": xyz[:, 1], "z": xyz[:, 2], "intensity": rng.uniform(0, 3000, n).astype(np.float32), "t": t_ns,
            "reflectivity": rng.integers(0, 65535, n), "ring": np.repeat(np.arange(height), width), "ambient": rng.integers(0, 65535, n),
            "range": (r * 1000).astype(np.uint32)}
    buf, w, h, rs = make_payload(OUSTER_FIELDS, OUSTER_POINT_STEP, n, vals, height=height, pad_row=16, seed=seed + 1)
    return buf, w, h, rs, vals


def velodyne_sweep(n=28800, seed=0, sweep_s=0.1, nan_every=0, zero_every=0):
    """a VLP-16-like sweep (16 rings x 1 800 firings, unorganised: height 1), firing-major as the driver packs it"""
    rng = np.random.default_rng(seed)
    rings = 16
    firings = n // rings
    az = np.repeat(2 * np.pi * np.arange(firings) / firings, rings)
    el = np.tile(np.deg2rad(np.linspace(-15, 15, rings)), firings)
    dirs = np.stack([np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el)], -1)
    r = _box_ranges(dirs) * (1 + rng.normal(0, 0.002, n))
    xyz = (dirs * r[:, None]).astype(np.float32)
    if zero_every:
        xyz[::zero_every] = 0.0
    if nan_every:
        xyz[5::nan_every, rng.integers(0, 3)] = np.nan
    time = (np.repeat(np.arange(firings), rings) * (sweep_s / firings)).astype(np.float32)
    vals = {"x": xyz[:, 0], "y": xyz[:, 1], "z": xyz[:, 2], "intensity": rng.uniform(0, 255, n).astype(np.float32),
            "ring": np.tile(np.arange(rings), firings), "time": time}
    buf, w, h, rs = make_payload(VELODYNE_FIELDS, VELODYNE_POINT_STEP, n, vals, seed=seed + 1)
    return buf, w, h, rs, vals


def _field(buf, base, off, dt):
    size = np.dtype(_NP[dt]).itemsize
    idx = (base[:, None] + off + np.arange(size)[None, :]).reshape(-1)
    return buf[idx].view(_NP[dt])


def ingest(buf, width, height, layout):
    """pcl::fromROSMsg (+ the Ouster conversion) into PointcloudXYZITR records: uint8 [n, 32]"""
    n = width * height
    rows = np.arange(n) // max(width, 1)
    base = rows * layout.row_step + (np.arange(n) - rows * width) * layout.point_step

    def get(off, dt):
        return _field(buf, base, off, dt) if off >= 0 else np.zeros(n, _NP[dt])
    x, y, z = get(layout.off_x, FLOAT32), get(layout.off_y, FLOAT32), get(layout.off_z, FLOAT32)
    inten = get(layout.off_intensity, FLOAT32)
    rec = np.zeros((n, 8), np.float32)
    if layout.sensor == SENSOR_OUSTER:
        T = np.array(layout.T_ouster_sensor[:], np.float64)
        x, y, z = ouster_transform(x, y, z, T)
        time = get(layout.off_time, UINT32).astype(np.float32) * np.float32(1e-9)
        ring = np.zeros(n, np.uint32)
    else:
        time = get(layout.off_time, FLOAT32)
        ring = get(layout.off_ring, UINT16).astype(np.uint32)
    rec[:, 0], rec[:, 1], rec[:, 2], rec[:, 4], rec[:, 5] = x, y, z, inten, time
    out = rec.view(np.uint32)
    out[:, 6] = ring
    return rec.view(np.uint8).reshape(n, 32)


def ouster_transform(x, y, z, T):
    """Eigen: Quaterniond * Vector3d (_transformVector: uv = 2 q.vec x v; v + w uv + q.vec x uv) + pos, fp64, rounded to float"""
    vx, vy, vz = x.astype(np.float64), y.astype(np.float64), z.astype(np.float64)
    qx, qy, qz, qw = T[3], T[4], T[5], T[6]
    ux, uy, uz = qy * vz - qz * vy, qz * vx - qx * vz, qx * vy - qy * vx
    ux, uy, uz = ux + ux, uy + uy, uz + uz
    ox = vx + qw * ux + (qy * uz - qz * uy)
    oy = vy + qw * uy + (qz * ux - qx * uz)
    oz = vz + qw * uz + (qx * uy - qy * ux)
    return (ox + T[0]).astype(np.float32), (oy + T[1]).astype(np.float32), (oz + T[2]).astype(np.float32)


def surf_keep(a, b, min_range):
    """uniformFeatureExtraction's predicate for candidates a against their raw predecessors b (float32 [m, 3]):
    |dx| > 1e-7 || |dy| > 1e-7 || (|dz| > 1e-7 && x*x + y*y + z*z > r*r) -- the float abs overload, compared in double; the
    squared norm and r*r in float, left to right"""
    a = np.asarray(a, np.float32); b = np.asarray(b, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        d = np.abs(a - b).astype(np.float64) > 1e-7
        r = np.float32(min_range)
        norm = (a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]) + a[:, 2] * a[:, 2]
        return d[:, 0] | d[:, 1] | (d[:, 2] & (norm > r * r))


def surf_sample(records, step, min_range):
    """cloud_surface as pcl::PointXYZI records uint8 [m, 32]: x y z, 1.0f, intensity = time, zero padding; ascending i"""
    rec = np.ascontiguousarray(records, np.uint8).reshape(-1, 32).view(np.float32)
    n = len(rec)
    idx = np.arange(1, n, step)
    keep = surf_keep(rec[idx, 0:3], rec[idx - 1, 0:3], min_range) if len(idx) else np.zeros(0, bool)
    k = idx[keep]
    out = np.zeros((len(k), 8), np.float32)
    out[:, 0:3] = rec[k, 0:3]
    out[:, 3] = 1.0
    out[:, 4] = rec[k, 5]
    return out.view(np.uint8).reshape(len(k), 32)


def layout_for(sensor, filter_point_size, min_range, fields=None, point_step=None, row_step=None):
    from superodom_amd.binding import sweep_layout
    if sensor == SENSOR_OUSTER:
        fields, point_step = fields or OUSTER_FIELDS, point_step or OUSTER_POINT_STEP
    else:
        fields, point_step = fields or VELODYNE_FIELDS, point_step or VELODYNE_POINT_STEP
    return sweep_layout(fields, point_step, row_step, sensor, filter_point_size, min_range, T_ouster_sensor=T_OUSTER_SENSOR)


__all__ = ["SENSOR_OUSTER", "SENSOR_VELODYNE", "ingest", "surf_sample", "surf_keep", "ouster_sweep", "velodyne_sweep", "make_payload",
           "layout_for", "ouster_transform"]
