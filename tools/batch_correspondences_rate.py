#!/usr/bin/env python3
"""The correspondence sets of a batch's hypotheses on the bench's `batch64` inputs (scene os1_128_2m: 131 072-point scans against the
2 M-point map, 64 guesses per scan at +-0.5 m / +-5 degrees, seeds 5000 + 64 i + h): what the switch costs a batch, and one export /
sums call for 64 hypotheses against 64 calls of one hypothesis each and against the only way without these entries -- 64 twin
registrations with so_icp_keep_correspondences on, each followed by so_icp_correspondences / so_icp_correspondence_sums.
usage (GPU box): python tools/batch_correspondences_rate.py [--mode plain|keep|export|trace] [--passes 3] [--root DIR] [--lanes]
  plain   the batch of 64 with the switch off, registrations/s per pass.  Needs nothing of this change: --root names another checkout
          whose built superodom_amd is measured (the parent commit's); the job alternates processes of the two builds
  keep    per pass: the batch with the switch off and with it on (--lanes: both under SOICP_BATCH_MODE=lanes, where the switch adds the
          lanes' copies to the scan copy)
  export  per pass and scan, behind one batch with the switch on: (1) one so_icp_batch_correspondences call for the 64 hypotheses,
          records to the host and records left on the device; (2) 64 calls of n_sel = 1; (3) 64 x (so_icp_register_dev on a twin context
          + so_icp_correspondences); the same three for so_icp_batch_correspondence_sums at 1 and at 64 poses
  trace   one batch with the switch on, one export and one sums call at 64 poses per scan -- the run to put under
          rocprofv3 --kernel-trace --stats
Wall-clock times of whole calls from Python (ctypes with pre-built arguments); the kernels' own times come from a profiler run."""
import argparse, os, sys, time
import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--mode", default="export", choices=["plain", "keep", "export", "trace"]); ap.add_argument("--passes", type=int, default=3)
ap.add_argument("--root", default=None, help="another checkout whose built superodom_amd is measured")
ap.add_argument("--lanes", action="store_true", help="SOICP_BATCH_MODE=lanes: the hypotheses as concurrent registrations on worker contexts")
a = ap.parse_args()
if a.lanes:
    os.environ["SOICP_BATCH_MODE"] = "lanes"  # (read by so_icp_create)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.abspath(a.root) if a.root else ROOT)
from superodom_amd import binding, synth  # noqa: E402

C = binding.C
REPS, B = 3, 64
sc = synth.Scene("os1_128_2m")
F64P, I32P = C.POINTER(C.c_double), C.POINTER(C.c_int32)


def context():
    cx = binding.LidarSlamGpu(rank=0, world_size=1, time_kernels=0, device_id=0, plane_res=sc.plane_res, line_res=sc.plane_res / 2,
                              max_iterations=5, lm_max_iterations=4, max_surface_features=-1)
    cx.add_surf_point_cloud(sc.map_points)
    cx.shift_map(sc.gt_pose(0)[:3])
    return cx, [cx.upload_scan(np.ascontiguousarray(sc.scan(i), dtype=np.float32)) for i in range(REPS)]


cx, d_scans = context()
N_POINTS = d_scans[0][1]
hyp = [np.ascontiguousarray(np.stack([synth.perturb_pose(sc.gt_pose(i), 5000 + 64 * i + h, 0.5, 5.0) for h in range(B)])) for i in range(REPS)]
out = np.zeros((B, 7)); rcs = np.zeros(B, np.int32); sts = [(binding.Stats * B)() for _ in range(REPS)]
batch_calls = [(lambda i=i: cx.L.so_icp_register_batch(cx.h, None, d_scans[i][0], d_scans[i][1], 12, hyp[i].ctypes.data_as(F64P), B,
                                                       out.ctypes.data_as(F64P), sts[i], rcs.ctypes.data_as(I32P))) for i in range(REPS)]


def batches():
    """REPS batches of 64 -> (seconds, hypotheses that converged)"""
    cx.synchronize()
    ok = 0
    t0 = time.perf_counter()
    for i in range(REPS):
        r = batch_calls[i]()
        assert r >= 0, (r, cx.last_error())
        ok += r
    cx.synchronize()
    return time.perf_counter() - t0, ok


def timed(fn):
    cx.synchronize()
    t0 = time.perf_counter()
    fn()
    cx.synchronize()
    return time.perf_counter() - t0


N = REPS * B
if a.mode == "plain":
    for p in range(a.passes + 1):  # (pass 0 warms up)
        t, ok = batches()
        if p:
            print("[plain] pass %d: batch of 64, switch off %.1f registrations/s (%.3f ms per batch, %d of %d converged)" % (p, N / t, 1e3 * t / REPS, ok, N), flush=True)
elif a.mode == "keep":
    tag = "lanes" if a.lanes else "batched"
    for p in range(a.passes + 1):
        assert cx.keep_batch_correspondences(False) == 0  # (frees the set: an untimed pass behind it, as behind the allocation below)
        batches()
        t0, ok0 = batches()
        assert cx.keep_batch_correspondences(True) == 0
        batches()  # (the pass that allocates the set)
        t1, ok1 = batches()
        assert ok0 == ok1
        if p:
            print("[keep, %s] pass %d: switch off %.1f registrations/s (%.3f ms per batch); switch on %.1f (%.3f ms): %+.3f ms per batch"
                  % (tag, p, N / t0, 1e3 * t0 / REPS, N / t1, 1e3 * t1 / REPS, 1e3 * (t1 - t0) / REPS), flush=True)
else:
    assert cx.keep_batch_correspondences(True) == 0
    twin, twin_scans = context()
    assert twin.keep_correspondences(True) == 0
    cap = B * N_POINTS
    all_host, rec, first, info = cx.prepare_batch_correspondences(B, N_POINTS, cap)
    d_rec = C.c_void_p()
    info_dev = (binding.CorrespondenceInfo * B)(); first_dev = np.zeros(B + 1, np.uint64)
    all_dev = lambda: cx.L.so_icp_batch_correspondences(cx.h, None, B, None, None, 0, first_dev.ctypes.data_as(C.POINTER(C.c_uint64)), None, 0, C.byref(d_rec), info_dev)
    one_host = [cx.prepare_batch_correspondences(1, N_POINTS, N_POINTS, hyp=[h]) for h in range(B)]
    one_idx = [np.array([h], np.int32) for h in range(B)]
    one_info = (binding.CorrespondenceInfo * 1)(); one_first = np.zeros(2, np.uint64)
    one_dev = [(lambda h=h: cx.L.so_icp_batch_correspondences(cx.h, one_idx[h].ctypes.data_as(I32P), 1, None, None, 0, one_first.ctypes.data_as(C.POINTER(C.c_uint64)),
                                                             None, 0, C.byref(d_rec), one_info)) for h in range(B)]
    t_stats = binding.Stats(); t_pose = np.zeros(7)
    twin_host, t_rec, _, _, t_info = twin.prepare_correspondences(N_POINTS, want_points=False)
    t_dinfo = binding.CorrespondenceInfo()
    twin_dev = lambda: twin.L.so_icp_correspondences(twin.h, None, None, 0, None, None, 0, C.byref(d_rec), C.byref(t_dinfo))

    def loop(calls):
        for f in calls:
            assert f() == 0

    twin_reg = [[twin.prepare_register_dev(twin_scans[i][0], twin_scans[i][1], hyp[i][h], t_stats, t_pose) for h in range(B)] for i in range(REPS)]

    def twins(i, after):
        for h in range(B):
            assert twin_reg[i][h]() >= 0
            assert after() == 0

    if a.mode == "trace":
        for i in range(REPS):
            assert batch_calls[i]() >= 0
            assert all_dev() == 0
            poses = np.ascontiguousarray(np.stack([np.stack([synth.perturb_pose(np.array(info_dev[h].pose_eval), 9000 + j, 0.02, 0.2) for j in range(64)]) for h in range(B)]))
            assert cx.prepare_batch_correspondence_sums(poses)[0]() == 0
        print("[trace] %d x (batch of 64 with the switch on, one export of 64 hypotheses, one sums call of 64 hypotheses x 64 poses)" % REPS)
    else:
        for p in range(a.passes + 1):
            for i in range(REPS):
                assert batch_calls[i]() >= 0
                t_all, t_all_dev = timed(lambda: loop([all_host])), timed(lambda: loop([all_dev]))
                n_rec = int(first[B])
                t_one, t_one_dev = timed(lambda: loop([c[0] for c in one_host])), timed(lambda: loop(one_dev))
                t_twin, t_twin_dev, t_reg = timed(lambda: twins(i, twin_host)), timed(lambda: twins(i, twin_dev)), timed(lambda: twins(i, lambda: 0))
                line = ("[export] pass %d scan %d: %d records of 64 hypotheses.  Records to the host: one call %.3f ms, 64 calls of n_sel = 1 %.3f ms, 64 x (twin registration + "
                        "so_icp_correspondences) %.3f ms.  Records left on the device: %.3f ms, %.3f ms, %.3f ms.  (64 twin registrations alone %.3f ms)"
                        % (p, i, n_rec, 1e3 * t_all, 1e3 * t_one, 1e3 * t_twin, 1e3 * t_all_dev, 1e3 * t_one_dev, 1e3 * t_twin_dev, 1e3 * t_reg))
                if p:
                    print(line, flush=True)
                for n_poses in (1, 64):
                    poses = np.ascontiguousarray(np.stack([np.stack([synth.perturb_pose(np.array(info[h].pose_eval), 9000 + j, 0.02, 0.2) for j in range(n_poses)]) for h in range(B)]))
                    s_all = cx.prepare_batch_correspondence_sums(poses)[0]
                    s_one = [cx.prepare_batch_correspondence_sums(poses[h:h + 1], hyp=[h])[0] for h in range(B)]
                    s_twin = [twin.prepare_correspondence_sums(poses[h])[0] for h in range(B)]
                    t_s_all, t_s_one = timed(lambda: loop([s_all])), timed(lambda: loop(s_one))

                    def twin_sums():
                        for h in range(B):
                            assert twin_reg[i][h]() >= 0
                            assert s_twin[h]() == 0
                    t_s_twin = timed(twin_sums)
                    if p:
                        print("[sums] pass %d scan %d, %d poses per hypothesis: one call %.3f ms, 64 calls of n_sel = 1 %.3f ms, 64 x (twin registration + so_icp_correspondence_sums) %.3f ms"
                              % (p, i, n_poses, 1e3 * t_s_all, 1e3 * t_s_one, 1e3 * t_s_twin), flush=True)
    twin.close()
cx.close()
