#!/usr/bin/env python3
"""so_icp_match_batch on the bench's `batch64` inputs (scene os1_128_2m: 131 072-point scans against the 2 M-point map, guesses per scan at
+-0.5 m / +-5 degrees, seeds 5000 + 64 i + h): what the change costs the existing paths, and one call for 8 / 64 / 256 poses against the
same number of so_icp_match_dev calls and against so_icp_register_batch with max_iterations = 1.
usage (GPU box): python tools/match_batch_rate.py [--mode plain|loop|match|trace] [--passes 3] [--root DIR]
  plain   so_icp_register_batch of 64, registrations/s per pass.  Needs nothing of this change: --root names another checkout whose built
          superodom_amd is measured (the parent commit's); the job alternates processes of the two builds
  loop    the staged so_icp_register loop (announce the next scan, register the current one), registrations/s per pass; --root as above
  match   per pass and scan, for 8, 64 and 256 poses: one so_icp_match_batch call with the keep switch off and on; the same number of
          so_icp_match_dev calls on a twin context, three times (its run-to-run spread); so_icp_register_batch with max_iterations = 1
  trace   one so_icp_match_batch of 64 per scan -- the run to put under rocprofv3 --kernel-trace --stats
Wall-clock times of whole calls from Python (ctypes with pre-built arguments), the queue drained before and after; the kernels' own
times come from a profiler run."""
import argparse, os, sys, time
import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--mode", default="match", choices=["plain", "loop", "match", "trace"]); ap.add_argument("--passes", type=int, default=3)
ap.add_argument("--root", default=None, help="another checkout whose built superodom_amd is measured")
a = ap.parse_args()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.abspath(a.root) if a.root else ROOT)
from superodom_amd import binding, synth  # noqa: E402

C = binding.C
REPS, B = 3, 64
sc = synth.Scene("os1_128_2m")
F32P, F64P, I32P = C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_int32)


def context(max_iterations=5):
    cx = binding.LidarSlamGpu(rank=0, world_size=1, time_kernels=0, device_id=0, plane_res=sc.plane_res, line_res=sc.plane_res / 2,
                              max_iterations=max_iterations, lm_max_iterations=4, max_surface_features=-1)
    cx.add_surf_point_cloud(sc.map_points)
    cx.shift_map(sc.gt_pose(0)[:3])
    return cx, [cx.upload_scan(np.ascontiguousarray(sc.scan(i), dtype=np.float32)) for i in range(REPS)]


def guesses(i, n):
    return np.ascontiguousarray(np.stack([synth.perturb_pose(sc.gt_pose(i), 5000 + 64 * i + h, 0.5, 5.0) for h in range(n)]))


def timed(cx, fn):
    cx.synchronize()
    t0 = time.perf_counter()
    fn()
    cx.synchronize()
    return time.perf_counter() - t0


cx, d_scans = context()
if a.mode == "plain":
    hyp = [guesses(i, B) for i in range(REPS)]
    out = np.zeros((B, 7)); rcs = np.zeros(B, np.int32); sts = (binding.Stats * B)()

    def batches():
        for i in range(REPS):
            r = cx.L.so_icp_register_batch(cx.h, None, d_scans[i][0], d_scans[i][1], 12, hyp[i].ctypes.data_as(F64P), B, out.ctypes.data_as(F64P), sts, rcs.ctypes.data_as(I32P))
            assert r >= 0, (r, cx.last_error())
    for p in range(a.passes + 1):  # (pass 0 warms up)
        t = timed(cx, batches)
        if p:
            print("[plain] pass %d: batch of 64 %.1f registrations/s (%.3f ms per batch)" % (p, REPS * B / t, 1e3 * t / REPS), flush=True)
elif a.mode == "loop":
    STEPS = 60
    scans = [cx.host_alloc_like(np.ascontiguousarray(sc.scan(i), dtype=np.float32)) for i in range(REPS)]
    gs = [sc.guess(i) for i in range(REPS)]

    def stream():
        cx.stage_scan(scans[0])
        for k in range(STEPS):
            if k + 1 < STEPS:
                cx.stage_scan(scans[(k + 1) % REPS])
            rc, _, _ = cx.register(scans[k % REPS], gs[k % REPS])
            assert rc == 0
    for p in range(a.passes + 1):
        t = timed(cx, stream)
        if p:
            print("[loop] pass %d: staged so_icp_register %.1f registrations/s (%.3f ms each)" % (p, STEPS / t, 1e3 * t / STEPS), flush=True)
else:
    SIZES = (8, 64, 256) if a.mode == "match" else (64,)
    twin, twin_scans = context()
    assert twin.keep_correspondences(True) == 0
    one, one_scans = context(max_iterations=1)
    t_stats = binding.Stats()
    for p in range(a.passes + 1):
        for i in range(REPS):
            for n_poses in SIZES:
                poses = guesses(i, n_poses)
                sts = (binding.Stats * n_poses)(); rcs = np.zeros(n_poses, np.int32); out = np.zeros((n_poses, 7))
                call = lambda: cx.L.so_icp_match_batch(cx.h, None, d_scans[i][0], d_scans[i][1], 12, poses.ctypes.data_as(F64P), n_poses, sts, rcs.ctypes.data_as(I32P))

                def once():
                    r = call()
                    assert r == n_poses, (r, cx.last_error())
                if a.mode == "trace":
                    once()
                    continue
                t = {}
                for keep in (False, True):
                    assert cx.keep_batch_correspondences(keep) == 0
                    once()  # (behind a change of the switch: the call that allocates or frees the set)
                    t[keep] = timed(cx, once)
                assert cx.keep_batch_correspondences(False) == 0

                def singles():
                    for h in range(n_poses):
                        assert twin.L.so_icp_match_dev(twin.h, twin_scans[i][0], twin_scans[i][1], poses[h].ctypes.data_as(F64P), C.byref(t_stats)) == 0
                t_loop = [timed(twin, singles) for _ in range(3)]

                def batch1():
                    r = one.L.so_icp_register_batch(one.h, None, one_scans[i][0], one_scans[i][1], 12, poses.ctypes.data_as(F64P), n_poses, out.ctypes.data_as(F64P), sts,
                                                    rcs.ctypes.data_as(I32P))
                    assert r >= 0, (r, one.last_error())
                batch1()
                t_b1 = timed(one, batch1)
                if p:
                    print("[match] pass %d scan %d, %3d poses: one so_icp_match_batch call %.3f ms (keep switch on: %.3f ms); %d so_icp_match_dev calls %.3f / %.3f / %.3f ms; "
                          "so_icp_register_batch with max_iterations = 1 %.3f ms" % (p, i, n_poses, 1e3 * t[False], 1e3 * t[True], n_poses, *[1e3 * x for x in t_loop], 1e3 * t_b1),
                          flush=True)
    if a.mode == "trace":
        print("[trace] %d x %d so_icp_match_batch calls of 64 poses" % (a.passes + 1, REPS))
    twin.close(); one.close()
cx.close()
