#!/usr/bin/env python3
"""so_icp_localization_sequence against the per-frame loop it replaces: ms per frame (registration + map insert) on os1_128_2m.
usage (GPU box): python tools/localization_sequence_rate.py [--frames 64] [--warmup 4] [--repeats 3]
  loop        so_icp_localization per frame from Python, guess_k = pose_out_(k-1) o delta_k composed in numpy (the per-frame loop)
  sequence    one so_icp_localization_sequence call over the same frames
Every run is a fresh context seeded with the same prior map, the scans in so_icp_host_alloc memory, and a warm-up run of --warmup
frames (the same in every mode) before the measured one.  Prints one JSON line per mode (best and median of --repeats runs) and a
summary line."""
import argparse, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from superodom_amd import binding, synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=64); ap.add_argument("--warmup", type=int, default=4); ap.add_argument("--repeats", type=int, default=3)
a = ap.parse_args()
sc = synth.Scene("os1_128_2m")
n = a.frames
host = [np.ascontiguousarray(sc.scan(i), dtype=np.float32) for i in range(n)]
deltas = np.zeros((n, 7)); deltas[:, 6] = 1.0
for k in range(1, n):
    deltas[k] = synth.pose_between(sc.gt_pose(k - 1), sc.guess(k))
times = 0.1 * np.arange(1, n + 1)


def context():
    slam = binding.LidarSlamGpu(device_id=0, plane_res=sc.plane_res, line_res=sc.plane_res / 2, max_iterations=5, lm_max_iterations=4,
                                max_surface_features=-1)
    slam.add_surf_point_cloud(sc.map_points)
    slam.shift_map(sc.gt_pose(0)[:3])
    return slam


def run_loop(slam, bufs, m):
    guess = sc.guess(0); poses = []
    for k in range(m):
        if k:
            guess = synth.pose_compose(poses[-1], deltas[k])
        rc, pose, _ = slam.localization(True, guess, bufs[k], times[k])
        assert rc == 0, (k, rc, slam.last_error())
        poses.append(pose)
    return np.array(poses)


def run_seq(slam, bufs, m):
    rc, poses, _, _, n_done = slam.localization_sequence(bufs[:m], sc.guess(0), deltas[:m], times[:m])
    assert rc == 0 and n_done == m, (rc, n_done, slam.last_error())
    return poses


results, ref = {}, None
for mode in ("loop", "sequence"):
    per = []
    for rep in range(a.repeats):
        slam = context()
        bufs = [slam.host_alloc_like(h) for h in host]
        fn = run_loop if mode == "loop" else run_seq
        fn(slam, bufs, a.warmup)  # (first-use allocations; the same frames in every mode, so every measured run starts from the same map)
        slam.synchronize()
        t0 = time.perf_counter()
        poses = fn(slam, bufs, n)
        slam.synchronize()  # (the last insert completes behind the call)
        per.append((time.perf_counter() - t0) * 1e3 / n)
        if ref is None:
            ref = poses
        same = bool(np.array_equal(poses, ref))
        slam.close()
    results[mode] = dict(mode=mode, frames=n, ms_per_frame_best=round(min(per), 4), ms_per_frame_median=round(float(np.median(per)), 4),
                         runs=[round(x, 4) for x in per], poses_equal_to_loop=same)
    print(json.dumps(results[mode]), flush=True)
print(json.dumps({"scene": "os1_128_2m", "frames": n, **{f"{m}_ms": results[m]["ms_per_frame_best"] for m in results}}))
