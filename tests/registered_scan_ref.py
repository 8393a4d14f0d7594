"""Numpy restatement of the registered scan laserMapping::publishTopic builds (src/LaserMapping/laserMapping.cpp:464-493 with
utils::pointAssociateToMap, src/utils/superodom_utils.cpp:148-158) as so_icp_registered_scan(_dev) returns it, and the seeded inputs
of its tests.  Written from the description of the node's loop, not copied.  Test infrastructure only.

  registered_scan()  per record, float x y z at byte 0 4 8:
      near = (double)(x*x + y*y + z*z) < 0.01                 float products and sums, left to right
      (x', y', z') = near ? (x, y, z) : (float)(q * p + t)    Eigen's quaternion * vector in fp64: uv = 2 u x v, v + w uv + u x uv
      keep = (double)(x'*x' + y'*y' + z'*z') > 0.01           a NaN fails it; an infinite result passes it
  the kept records, whole, with the three floats replaced, in input order (a boolean-mask compaction)
The fp64 expressions are those of test_gpu_deskew.py::test_transform_cloud_is_the_nodes_registered_scan_bit_for_bit."""
import functools

import numpy as np

import livox_ref as lr
from superodom_amd import synth

TILE = 2048  # records per workgroup of the compaction (feature_kernels.h kSurfItems)
FAMILIES = ("scan", "livox", "nonfinite", "tiles_middle", "tiles_none", "tiles_ends")
# the sizes of tests/test_gpu_registered_scan.py: around a wavefront, a round of 256, a tile; three tiles; more than 64 workgroups
SIZES = (0, 1, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 3 * TILE, 65 * TILE + 1)


def pose(seed=0):
    """T_w_lidar = x y z, quaternion x y z w: metres of translation, a rotation with no zero component"""
    rng = np.random.default_rng(1000 + seed)
    q = synth.quat_from_rotvec(np.array([0.02, -0.03, 0.8]) + rng.normal(0, 0.1, 3))
    return np.concatenate([np.array([3.0, -4.0, 0.5]) + rng.normal(0, 1.0, 3), q])


def transform(xyz, T):
    """(x' y' z' float32 [n, 3], near [n], keep [n]) of float32 points [n, 3]"""
    p = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    x, y, z = (p[:, k].astype(np.float64) for k in range(3))
    tx, ty, tz, qx, qy, qz, qw = (float(v) for v in T)
    with np.errstate(invalid="ignore", over="ignore"):
        ux, uy, uz = qy * z - qz * y, qz * x - qx * z, qx * y - qy * x
        ux, uy, uz = ux + ux, uy + uy, uz + uz
        wx = (x + qw * ux + (qy * uz - qz * uy)) + tx
        wy = (y + qw * uy + (qz * ux - qx * uz)) + ty
        wz = (z + qw * uz + (qx * uy - qy * ux)) + tz
        near = (p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1] + p[:, 2] * p[:, 2]).astype(np.float64) < 0.01
        w = np.where(near[:, None], p, np.stack([wx, wy, wz], 1).astype(np.float32))
        keep = (w[:, 0] * w[:, 0] + w[:, 1] * w[:, 1] + w[:, 2] * w[:, 2]).astype(np.float64) > 0.01
    return w, near, keep


def registered_scan(records, T):
    """records uint8 [n, stride] -> (kept records uint8 [n_kept, stride], near [n], keep [n])"""
    rec = np.ascontiguousarray(records, np.uint8)
    n, stride = rec.shape
    w, near, keep = transform(rec[:, :12].copy().view(np.float32).reshape(n, 3), T)
    out = rec.copy()
    out[:, :12] = w.view(np.uint8).reshape(n, 12)
    return out[keep], near, keep


def registered_scan_loop(records, T):
    """the same one record at a time, in Python scalars of the two widths (the check of the vectorised form)"""
    f32, f64 = np.float32, np.float64
    t, q = [f64(v) for v in T[:3]], [f64(v) for v in T[3:]]
    out = []
    with np.errstate(invalid="ignore", over="ignore"):
        for r in np.ascontiguousarray(records, np.uint8):
            x, y, z = (f32(v) for v in r[:12].copy().view(np.float32))
            if not (f64(x * x + y * y + z * z) < 0.01):
                v = [f64(x), f64(y), f64(z)]
                uv = [q[1] * v[2] - q[2] * v[1], q[2] * v[0] - q[0] * v[2], q[0] * v[1] - q[1] * v[0]]
                uv = [a + a for a in uv]
                c = [q[1] * uv[2] - q[2] * uv[1], q[2] * uv[0] - q[0] * uv[2], q[0] * uv[1] - q[1] * uv[0]]
                x, y, z = (f32((v[k] + q[3] * uv[k] + c[k]) + t[k]) for k in range(3))
            if f64(x * x + y * y + z * z) > 0.01:
                o = r.copy()
                o[:12] = np.array([x, y, z], np.float32).view(np.uint8)
                out.append(o)
    return np.stack(out) if out else np.zeros((0, records.shape[1]), np.uint8)


# ---- the seeded inputs -------------------------------------------------------------------------------------------------------
NEAR_SENSOR_AT, NEAR_ORIGIN_AT, EVERY = 7, 31, 50  # "scan": records i % 50 == 7 lie near the sensor, i % 50 == 31 land at the world origin


def _back(T, world):
    """sensor-frame float32 points that T maps onto `world` (up to the rounding of the way there and back: micrometres)"""
    Rm = synth.quat_to_R(np.asarray(T[3:], np.float64))
    return ((np.asarray(world, np.float64) - np.asarray(T[:3], np.float64)) @ Rm).astype(np.float32)


def _payload(rng, n, stride):
    """n records of `stride` bytes whose words behind x y z are all distinct and non-zero"""
    w = np.zeros((n, stride // 4), np.uint32)
    w[:, 3:] = rng.integers(1, 2**32, (n, stride // 4 - 3), dtype=np.uint64).astype(np.uint32)
    return w


def _finish(w, xyz):
    w[:, :3] = np.ascontiguousarray(xyz, np.float32).view(np.uint32).reshape(-1, 3)
    return w.view(np.uint8).reshape(len(w), 4 * w.shape[1])


def _far(rng, n):
    """points 2 .. 60 m from the sensor"""
    d = rng.normal(0, 1, (n, 3))
    d /= np.maximum(np.linalg.norm(d, axis=1, keepdims=True), 1e-9)
    return (d * rng.uniform(2.0, 60.0, (n, 1))).astype(np.float32)


def _scan_xyz(rng, n, T):
    xyz = _far(rng, n)
    i = np.arange(n)
    a, b = i % EVERY == NEAR_SENSOR_AT, i % EVERY == NEAR_ORIGIN_AT
    d = rng.normal(0, 1, (n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True) + 1e-12
    ball = d * rng.uniform(0.0, 0.05, (n, 1))  # within 0.05 m
    xyz[a] = ball[a].astype(np.float32)
    xyz[b] = _back(T, ball[b])
    return xyz


@functools.lru_cache(maxsize=None)
def _family(name, n, stride, seed):
    rng = np.random.default_rng([seed, n, stride, FAMILIES.index(name)])
    T = pose(seed)
    if name == "livox":
        assert stride == 32
        vals = synth.livox_sweep(n=max(n, 64), seed=seed + n, reject_share=0.5)
        rec = lr.ingest({k: v[:n] for k, v in vals.items()}, lr.R_TILT)
    else:
        w = _payload(rng, n, stride)
        if name == "scan":
            xyz = _scan_xyz(rng, n, T)
        elif name == "nonfinite":
            xyz = _scan_xyz(rng, n, T)
            at = nonfinite_at(n)
            for k, i in enumerate(at):
                xyz[i, k % 3] = (np.nan, np.inf, -np.inf)[(k // 3) % 3]
        elif name == "tiles_middle":  # every record of the second tile is dropped: half zero records, half points that land at the origin
            xyz = _scan_xyz(rng, n, T)
            mid = np.arange(TILE, min(2 * TILE, n))
            xyz[mid[0::2]] = 0.0
            d = rng.uniform(-0.02, 0.02, (len(mid[1::2]), 3))
            xyz[mid[1::2]] = _back(T, d)
        elif name == "tiles_none":
            xyz = _far(rng, n)
        elif name == "tiles_ends":
            xyz = np.zeros((n, 3), np.float32)
            if n:
                xyz[[0, n - 1]] = _far(rng, 2)
        else:
            raise KeyError(name)
        rec = _finish(w, xyz)
    rec.setflags(write=False)
    want, near, keep = registered_scan(rec, T)
    for a in (want, near, keep, T):
        a.setflags(write=False)
    return rec, T, want, near, keep


def nonfinite_at(n):
    """indices of the records of "nonfinite" that carry NaN, +Inf, -Inf in x, y, z (nine of them when n allows), none of them one of
    "scan"'s special records"""
    return [i for i in (3 + 11 * k for k in range(9)) if i < n and i % EVERY not in (NEAR_SENSOR_AT, NEAR_ORIGIN_AT)]


def family(name, n, stride=32, seed=0):
    """(records uint8 [n, stride], T_w_lidar, kept records, near [n], keep [n]) -- computed once and shared: all read-only"""
    return _family(name, int(n), int(stride), int(seed))
