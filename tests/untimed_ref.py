"""Numpy restatement of featureExtraction::assignTimeforPointCloud (src/FeatureExtraction/featureExtraction.cpp:646-708), the ingest of a
sweep whose points carry x y z intensity only (provide_point_time: 0), exact in float32 / float64, and the seeded sweeps of the tests.
Written from the description of the loop, not copied.  Test infrastructure only.

  angle()           float angle = atan(z / sqrt(x*x + y*y)) * 180 / M_PI under the float-overload reading (the sum, sqrt and the
                    quotient in float; atan as float = the fp64 value rounded once; * 180 a float product; / M_PI in double) or the
                    all-double reading (everything behind the float sum in double)
  ring()            the three ring tables with int() truncating toward zero and int(NaN) = INT_MIN, and their drop tests
  time_of()         (float)(rel * scanPeriod), rel = (float)((columnTime * int(i / N) + laserTime * (i % N)) / scanPeriod)
  ingest_literal()  the loop as written: sequential, with the bound that shrinks at every drop
  ingest()          the prefix rule: D(i) = drops among [0, i); visited iff i + D(i) < n; a record iff visited and not dropped
  decided()         per point: ring and drop decision unchanged with the float atan one ulp either way and under the all-double reading
The de-skew behind it is the library's own so_icp_deskew_scan and the sampling feature_extraction_ref.surf_sample, as for the other
sensors."""
import numpy as np

import feature_extraction_ref as fr
from superodom_amd.binding import FLOAT32, UINT16

SCAN_PERIOD = 0.100859904 - 20.736e-6   # featureExtraction.h:91-93
COLUMN_TIME = 55.296e-6
LASER_TIME = 2.304e-6
INT_MIN = -2 ** 31
N_SCANS = (4, 16, 32, 64, 128)
F32 = np.float32


def angle(x, y, z, reading="float", atan_ulp=0):
    """float32 elevation in degrees; atan_ulp = -1 / +1 moves the float atan result to its neighbour (float reading only)"""
    x, y, z = (np.asarray(v, F32) for v in (x, y, z))
    with np.errstate(all="ignore"):
        s = x * x + y * y                                   # float, unfused
        if reading == "float":
            a = np.arctan((z / np.sqrt(s)).astype(np.float64)).astype(F32)
            if atan_ulp:
                a = np.nextafter(a, F32(np.inf if atan_ulp > 0 else -np.inf))
            return ((a * F32(180)).astype(np.float64) / np.pi).astype(F32)
        assert reading == "double" and not atan_ulp
        return (np.arctan(z.astype(np.float64) / np.sqrt(s.astype(np.float64))) * 180 / np.pi).astype(F32)


def _int(v):
    """int(double): toward zero; NaN -> INT_MIN (what x86-64's cvttsd2si gives)"""
    v = np.asarray(v, np.float64)
    return np.where(np.isnan(v), INT_MIN, np.trunc(np.nan_to_num(v, nan=0.0))).astype(np.int64)


def ring(ang, n_scans):
    """(scanID int64 [n], dropped bool [n]) for float32 angles"""
    ang = np.asarray(ang, F32)
    a64 = ang.astype(np.float64)
    with np.errstate(invalid="ignore"):
        if n_scans == 16:
            rid = _int(((ang + F32(15)) / F32(2)).astype(np.float64) + 0.5)
            return rid, (rid > 15) | (rid < 0)
        if n_scans == 32:
            rid = _int((a64 + 92.0 / 3.0) * 3.0 / 4.0)
            return rid, (rid > 31) | (rid < 0)
        if n_scans == 64:
            upper = _int((F32(2) - ang).astype(np.float64) * 3.0 + 0.5)
            lower = 32 + _int((-8.83 - a64) * 2.0 + 0.5)
            rid = np.where(a64 >= -8.83, upper, lower)
            return rid, (ang > F32(2)) | (a64 < -24.33) | (rid > 50) | (rid < 0)
    return np.zeros(len(ang), np.int64), np.zeros(len(ang), bool)   # "wrong scan number": ring 0, nothing dropped


def time_of(i, n_scans):
    i = np.asarray(i, np.int64)
    rel = ((COLUMN_TIME * (i // n_scans).astype(np.float64) + LASER_TIME * (i % n_scans).astype(np.float64)) / SCAN_PERIOD).astype(F32)
    return (rel.astype(np.float64) * SCAN_PERIOD).astype(F32)


def decided(x, y, z, n_scans):
    """bool [n]: the point's ring and drop decision do not hang on the last bit of the float atan, nor on the overload choice"""
    ref = ring(angle(x, y, z), n_scans)
    ok = np.ones(len(ref[0]), bool)
    for other in (angle(x, y, z, atan_ulp=-1), angle(x, y, z, atan_ulp=+1), angle(x, y, z, reading="double")):
        rid, drop = ring(other, n_scans)
        ok &= (drop == ref[1]) & (drop | (rid == ref[0]))
    return ok


def _records(x, y, z, intensity, time, rid):
    rec = np.zeros((len(x), 8), F32)
    rec[:, 0], rec[:, 1], rec[:, 2], rec[:, 4], rec[:, 5] = x, y, z, intensity, time
    rec.view(np.uint32)[:, 6] = np.asarray(rid, np.int64).astype(np.uint16).astype(np.uint32)
    return rec.view(np.uint8).reshape(len(x), 32)


def ingest_literal(x, y, z, intensity, n_scans, drop=None):
    """the loop of :655-704 as written.  drop: a bool pattern that replaces the ring test (for the tests of the bound alone).
    Returns (records uint8 [m, 32], the kept indices)."""
    x, y, z, intensity = (np.asarray(v, F32) for v in (x, y, z, intensity))
    cloud_size = len(x)
    kept, rings = [], []
    i = 0
    while i < cloud_size:
        if drop is None:
            rid, dr = ring(angle(x[i:i + 1], y[i:i + 1], z[i:i + 1]), n_scans)
            scan_id, dropped = int(rid[0]), bool(dr[0])
        else:
            scan_id, dropped = 0, bool(drop[i])
        if dropped:
            cloud_size -= 1
            i += 1
            continue
        kept.append(i); rings.append(scan_id)
        i += 1
    k = np.array(kept, np.int64)
    return _records(x[k], y[k], z[k], intensity[k], time_of(k, n_scans), np.array(rings, np.int64)), k


def kept_by_prefix_rule(drop):
    """indices that become records: visited (i + D(i) < n) and not dropped; record i sits at i - D(i)"""
    drop = np.asarray(drop, bool)
    n = len(drop)
    i = np.arange(n)
    D = np.concatenate([[0], np.cumsum(drop)[:-1]]) if n else np.zeros(0, np.int64)
    k = i[(i + D < n) & ~drop]
    assert np.array_equal(k - D[k], np.arange(len(k)))
    return k


def ingest(x, y, z, intensity, n_scans, drop=None):
    x, y, z, intensity = (np.asarray(v, F32) for v in (x, y, z, intensity))
    rid, dr = ring(angle(x, y, z), n_scans)
    if drop is not None:
        rid, dr = np.zeros(len(x), np.int64), np.asarray(drop, bool)
    k = kept_by_prefix_rule(dr)
    return _records(x[k], y[k], z[k], intensity[k], time_of(k, n_scans), rid[k]), k


# ---- the sweeps of tests/test_gpu_untimed.py (test_untimed_host.py checks what they carry) ----
XYZI = [("x", 0, FLOAT32, 1), ("y", 4, FLOAT32, 1), ("z", 8, FLOAT32, 1), ("intensity", 12, FLOAT32, 1)]                 # pcl::PointXYZI as the old driver sends it
XYZI_RING_18 = [("x", 0, FLOAT32, 1), ("y", 4, FLOAT32, 1), ("z", 8, FLOAT32, 1), ("intensity", 12, FLOAT32, 1), ("ring", 16, UINT16, 1)]  # point_step 18
XYZ_ONLY = [("x", 0, FLOAT32, 1), ("y", 4, FLOAT32, 1), ("z", 8, FLOAT32, 1)]
KEPT_ELEVATION = {4: (-30.0, 30.0), 16: (-17.5, 15.5), 32: (-30.0, 11.5), 64: (-17.5, 1.8), 128: (-30.0, 30.0)}   # inside every table's kept range


def _draw(rng, m, n_scans, drop_share):
    lo, hi = KEPT_ELEVATION[n_scans]
    el = rng.uniform(lo, hi, m)
    bad = rng.random(m) < drop_share
    el[bad] = np.where(rng.random(int(bad.sum())) < 0.5, rng.uniform(hi + 3.0, 60.0, int(bad.sum())), rng.uniform(-60.0, lo - 8.0, int(bad.sum())))
    az = rng.uniform(-np.pi, np.pi, m)
    r = rng.uniform(0.5, 40.0, m)
    e = np.deg2rad(el)
    xyz = np.stack([r * np.cos(e) * np.cos(az), r * np.cos(e) * np.sin(az), r * np.sin(e)], 1).astype(F32)
    none = bad & (rng.random(m) < 0.3)
    xyz[none] = 0.0                                          # no return: the driver writes 0 0 0 (a NaN angle)
    return xyz


def sweep(n, n_scans, seed, drop_share=0.1, all_dropped=False):
    """field values of a seeded sweep, every point decided (an undecided one is drawn again)"""
    rng = np.random.default_rng(seed)
    xyz = _draw(rng, n, n_scans, 1.0 if all_dropped else drop_share)
    for _ in range(20):
        und = ~decided(xyz[:, 0], xyz[:, 1], xyz[:, 2], n_scans)
        if not und.any():
            break
        xyz[und] = _draw(rng, int(und.sum()), n_scans, 1.0 if all_dropped else drop_share)
    assert decided(xyz[:, 0], xyz[:, 1], xyz[:, 2], n_scans).all(), "every point of a GPU data set is decided"
    return {"x": xyz[:, 0].copy(), "y": xyz[:, 1].copy(), "z": xyz[:, 2].copy(), "intensity": rng.uniform(0, 255, n).astype(F32),
            "ring": rng.integers(0, 65535, n)}


TILE = 2048
# name -> sweep() arguments; the sizes are the smallest that reach each path of the kernel (tests/test_gpu_untimed.py)
GPU_SWEEPS = {f"n{n}": dict(n=n, n_scans=16, seed=100 + k) for k, n in enumerate((1, 2, 2047, 2048, 2049, 3 * TILE + 17))}
GPU_SWEEPS.update({f"scans{s}": dict(n=2 * TILE + 301, n_scans=s, seed=200 + s) for s in N_SCANS})
# "long": few enough drops that the visited prefix reaches into tile 65 -- the workgroup with 65 in front of it still stores records
GPU_SWEEPS.update({"long": dict(n=66 * TILE + 5, n_scans=16, seed=300, drop_share=0.01), "all_dropped": dict(n=TILE + 9, n_scans=32, seed=301, all_dropped=True),
                   "layouts": dict(n=2 * TILE + 77, n_scans=64, seed=302), "chain": dict(n=3 * TILE + 5, n_scans=16, seed=303)})


def gpu_sweep(name):
    return sweep(**GPU_SWEEPS[name])


def payload(vals, fields=XYZI, point_step=16, height=1, pad_row=0, seed=0):
    """(PointCloud2 data, width, height, row_step)"""
    return fr.make_payload(fields, point_step, len(vals["x"]), vals, height=height, pad_row=pad_row, seed=seed)
