"""Numpy restatement of featureExtraction::livoxHandler's point loop (src/FeatureExtraction/featureExtraction.cpp:794-806), exact in
float32 / float64, a Python CDR codec for livox_ros_driver2/msg/CustomMsg, and the seeded sweeps of the Livox tests.  Written from the
description of the handler, not copied.  Test infrastructure only.

  ingest()   accept iff line < n_scans and (tag & 0x30) in {0x10, 0x00}; R * Vector3d(x, y, z) in fp64, each row
             (R[r][0]*x + R[r][1]*y) + R[r][2]*z, rounded to float; intensity = (float)reflectivity; time = (float)offset_time / 1e9f
             (a float32 DIVISION); ring = line; a rejected point is 32 zero bytes
The de-skew behind it is the library's own so_icp_deskew_scan and the sampling feature_extraction_ref.surf_sample, as for the other
sensors."""
import numpy as np

import cdr_py
from superodom_amd import synth
from superodom_amd.binding import LIVOX_CUSTOM_POINT, LIVOX_POINT_STEP

cdr_py.SCHEMAS.setdefault("CustomPoint", [("offset_time", "uint32"), ("x", "float32"), ("y", "float32"), ("z", "float32"),
                                          ("reflectivity", "uint8"), ("tag", "uint8"), ("line", "uint8")])
cdr_py.SCHEMAS.setdefault("CustomMsg", [("header", "Header"), ("timebase", "uint64"), ("point_num", "uint32"), ("lidar_id", "uint8"),
                                        ("rsvd", "uint8[3]"), ("points", "CustomPoint[]")])


def accepted(vals, n_scans=4):
    t = vals["tag"].astype(np.uint32) & 0x30
    return (vals["line"].astype(np.int64) < n_scans) & ((t == 0x10) | (t == 0x00))


def time_div(offset_time):
    """offset_time / float(1000000000): uint32 -> float32 (round to nearest), then a correctly rounded float32 division"""
    return np.asarray(offset_time, np.uint32).astype(np.float32) / np.float32(1e9)


def time_mul(offset_time):
    """the Ouster's form, (float)t * 1e-9f: NOT what livoxHandler does; the tests show that they can tell the two apart"""
    return np.asarray(offset_time, np.uint32).astype(np.float32) * np.float32(1e-9)


def ingest(vals, R=None, n_scans=4, time_of=time_div):
    """PointcloudXYZITR records uint8 [n, 32] of the sweep's field arrays"""
    n = len(vals["x"])
    R = np.eye(3) if R is None else np.asarray(R, np.float64).reshape(3, 3)
    x, y, z = (vals[k].astype(np.float32).astype(np.float64) for k in "xyz")
    acc = accepted(vals, n_scans)
    rec = np.zeros((n, 8), np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for r in range(3):
            rec[:, r] = ((R[r, 0] * x + R[r, 1] * y) + R[r, 2] * z).astype(np.float32)
    rec[:, 4] = vals["reflectivity"].astype(np.float32)
    rec[:, 5] = time_of(vals["offset_time"])
    rec.view(np.uint32)[:, 6] = vals["line"].astype(np.uint32)
    rec[~acc] = 0.0
    return rec.view(np.uint8).reshape(n, 32)


def values_of_points(raw, n, point_step=LIVOX_POINT_STEP, offsets=LIVOX_CUSTOM_POINT):
    """field arrays out of the bytes of n points (the inverse of synth.livox_points)"""
    raw = np.ascontiguousarray(raw, np.uint8).reshape(-1)
    base = np.arange(n) * point_step
    out = {}
    for name, dt in (("offset_time", np.uint32), ("x", np.float32), ("y", np.float32), ("z", np.float32)):
        idx = (base[:, None] + offsets[name] + np.arange(4)[None, :]).reshape(-1)
        out[name] = raw[idx].view(dt)
    for name in ("reflectivity", "tag", "line"):
        out[name] = raw[base + offsets[name]]
    return out


# ---- CDR ----
def custom_msg(vals, frame_id="livox_frame", stamp=(1700000000, 250000000), timebase=1700000000250000000, lidar_id=192):
    n = len(vals["x"])
    pts = [{"offset_time": int(vals["offset_time"][i]), "x": float(vals["x"][i]), "y": float(vals["y"][i]), "z": float(vals["z"][i]),
            "reflectivity": int(vals["reflectivity"][i]), "tag": int(vals["tag"][i]), "line": int(vals["line"][i])} for i in range(n)]
    return {"header": {"stamp": {"sec": stamp[0], "nanosec": stamp[1]}, "frame_id": frame_id}, "timebase": timebase, "point_num": n,
            "lidar_id": lidar_id, "rsvd": [0, 0, 0], "points": pts}


def encode_custom_msg(msg):
    return cdr_py.encode("CustomMsg", msg)


def decode_custom_msg(raw):
    return cdr_py.decode("CustomMsg", raw)


def points_in_cdr(raw):
    """(byte offset of points[0] inside the serialised message, point_num, number of elements) -- read with the schema codec up to
    the sequence, so the offset is where THAT reader finds the first element"""
    r = cdr_py._R(raw)
    r.value("Header")
    r.prim("uint64")
    point_num = r.prim("uint32")
    r.prim("uint8")
    r.value("uint8[3]")
    count = r.prim("uint32")
    return r.at, point_num, count


# ---- the sweeps of tests/test_gpu_livox.py (test_livox_host.py checks that none of them makes a case vacuous) ----
def sweep(seed, n=20000, **kw):
    return synth.livox_sweep(n=n, seed=seed, **kw)


def special_sweep(seed=77, n=4096):
    """+inf, -inf and NaN coordinates at known indices of accepted points"""
    vals = sweep(seed, n=n)
    acc = np.nonzero(accepted(vals))[0]
    at = {"x+inf": acc[10], "x-inf": acc[20], "xnan": acc[30], "y+inf": acc[40], "znan": acc[50], "z-inf": acc[60]}
    for k, i in at.items():
        vals[k[0]][i] = {"+inf": np.inf, "-inf": -np.inf, "nan": np.nan}[k[1:]]
    return vals, at


GPU_SWEEPS = {"main1": dict(seed=11), "main3": dict(seed=13), "main7": dict(seed=17), "zero": dict(seed=21, reject_share=0.15),
              "time": dict(seed=31), "loads": dict(seed=41, n=5003), "poses": dict(seed=51), "deskew": dict(seed=61), "cdr": dict(seed=71, n=3001),
              "special": None}


def gpu_sweep(name):
    return special_sweep()[0] if name == "special" else sweep(**GPU_SWEEPS[name])


def small_motion_poses(t0, seed, rate_hz=200.0):
    """[m, 8] pose buffer around a sweep starting at t0: millimetres and milliradians over the sweep, so that a de-skewed scan of a
    static scene still registers"""
    rng = np.random.default_rng(seed)
    ts = t0 - 0.02 + np.arange(int(0.15 * rate_hz) + 1) / rate_hz + 1.234e-4
    w, v = rng.normal(0, 0.02, 3), rng.normal(0, 0.05, 3)
    q = np.stack([synth.quat_from_rotvec((t - t0) * w) for t in ts])
    return np.concatenate([ts[:, None], np.outer(ts - t0, v), q], 1)


def chain_sweep(k, xyz=None):
    """frame k of the chain test: the scan of synth's mid360_like scene (Scene("mid360_like").scan(k), or xyz when the caller has it)
    as a Livox sweep, turned by R_TILT^T so that the ingest with R_TILT brings it back into the scene's sensor frame"""
    if xyz is None:
        cfg = synth.CONFIGS["mid360_like"]
        world = synth.World(extent=cfg["extent"], spacing=cfg["spacing"], seed=1)
        xyz = synth.raycast(world, synth.trajectory_pose(k), synth.lidar_dirs(cfg["rings"], cfg["azimuth"], cfg["fov_deg"]), seed=3 + k)
    return synth.livox_sweep(seed=80 + k, xyz=(np.asarray(xyz, np.float64) @ R_TILT).astype(np.float32))


R_TILT = synth.quat_to_R(synth.quat_from_rotvec(np.deg2rad([3.0, -2.0, 0.0])))  # imu_laser_R_Gravity: a few degrees of roll and pitch
