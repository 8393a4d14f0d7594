#!/usr/bin/env python3
"""The correspondence sets of a run's frames on the bench's chained sequence (scene os1_128_2m: 131 072-point scans against the 2 M-point
map, three scans in rotation from pinned host buffers, delta_k = gt(k-1)^-1 o guess(k)): what the switch costs a chained run of 64
frames, and one export / sums call over all 64 frames against the only way without these entries -- 64 x (so_icp_register +
so_icp_correspondences) on a context with so_icp_keep_correspondences on.
usage (on a machine with an MI355X): python tools/sequence_correspondences_rate.py [--mode plain|keep|export|trace] [--passes 3] [--root DIR]
  plain   the run of 64 with the switch off, registrations/s per pass.  Needs nothing of this change: --root names another checkout
          whose built superodom_amd is measured (the parent commit's); the job alternates processes of the two builds
  keep    per pass: the run with the switch off and with it on (an untimed run behind either change of the switch: turning it off
          frees the set, turning it on makes the next run allocate it)
  export  per pass, behind one run with the switch on: one so_icp_sequence_correspondences call for the 64 frames, records to the host
          and records left on the device; one so_icp_sequence_correspondence_sums call at 1 pose per frame; and 64 x (so_icp_register +
          so_icp_correspondences), records to the host and left on the device, on a twin context
  trace   one run with the switch on, one export and one sums call -- the run to put under rocprofv3 --kernel-trace --stats
Wall-clock times of whole calls from Python (ctypes with pre-built arguments); the kernels' own times come from a profiler run."""
import argparse, os, sys, time
import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--mode", default="export", choices=["plain", "keep", "export", "trace"]); ap.add_argument("--passes", type=int, default=3)
ap.add_argument("--root", default=None, help="another checkout whose built superodom_amd is measured")
a = ap.parse_args()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.abspath(a.root) if a.root else ROOT)
from superodom_amd import binding, synth  # noqa: E402

C = binding.C
S, K = 3, 64
sc = synth.Scene("os1_128_2m")
guesses = [np.ascontiguousarray(sc.guess(i), dtype=np.float64) for i in range(S)]
deltas = np.zeros((K, 7)); deltas[:, 6] = 1.0
for k in range(1, K):
    deltas[k] = synth.pose_between(sc.gt_pose((k - 1) % S), guesses[k % S])


def context():
    cx = binding.LidarSlamGpu(rank=0, world_size=1, time_kernels=0, device_id=0, plane_res=sc.plane_res, line_res=sc.plane_res / 2,
                              max_iterations=5, lm_max_iterations=4, max_surface_features=-1)
    cx.add_surf_point_cloud(sc.map_points)
    cx.shift_map(sc.gt_pose(0)[:3])
    return cx, [cx.host_alloc_like(np.ascontiguousarray(sc.scan(i), dtype=np.float32)) for i in range(S)]


cx, scans = context()
N_POINTS = len(scans[0])
call, seq_out, seq_g, seq_st, seq_n, _keep = cx.prepare_register_sequence([scans[k % S] for k in range(K)], guesses[0], deltas)


def run():
    """one run of K frames -> seconds"""
    cx.synchronize()
    t0 = time.perf_counter()
    rc = call()
    cx.synchronize()
    t = time.perf_counter() - t0
    assert rc == 0 and seq_n.value == K, (rc, seq_n.value, cx.last_error())
    return t


def timed(fn, on=cx):
    on.synchronize()
    t0 = time.perf_counter()
    fn()
    on.synchronize()
    return time.perf_counter() - t0


if a.mode == "plain":
    for p in range(a.passes + 1):  # (pass 0 warms up)
        t = run()
        if p:
            print("[plain] pass %d: run of %d, switch off %.1f registrations/s (%.3f ms per frame), chained %d, chain breaks %d"
                  % (p, K, K / t, 1e3 * t / K, cx.timing().seq_chained, cx.timing().seq_chain_breaks), flush=True)
elif a.mode == "keep":
    for p in range(a.passes + 1):
        assert cx.keep_sequence_correspondences(False) == 0
        run()
        t0 = run()
        assert cx.keep_sequence_correspondences(True) == 0
        run()  # (the run that allocates the set)
        t1 = run()
        if p:
            print("[keep] pass %d: switch off %.1f registrations/s (%.3f ms per frame); switch on %.1f (%.3f ms): %+.2f us per frame"
                  % (p, K / t0, 1e3 * t0 / K, K / t1, 1e3 * t1 / K, 1e6 * (t1 - t0) / K), flush=True)
else:
    assert cx.keep_sequence_correspondences(True) == 0
    run(); run()
    guesses_out = seq_g.copy()
    exp_host, rec, first, info = cx.prepare_sequence_correspondences(K, K * N_POINTS)
    exp_dev, _, first_dev, info_dev = cx.prepare_sequence_correspondences(K, 0, want_records=False)
    assert exp_dev() == 0
    poses = np.ascontiguousarray(np.stack([np.array(info_dev[k].pose_eval) for k in range(K)]).reshape(K, 1, 7))
    sums_call = cx.prepare_sequence_correspondence_sums(poses)[0]
    if a.mode == "trace":
        run()
        assert exp_dev() == 0 and sums_call() == 0
        print("[trace] one run of %d frames with the switch on, one export (%d records left on the device), one sums call at 1 pose per frame" % (K, int(first_dev[K])))
    else:
        twin, t_scans = context()
        assert twin.keep_correspondences(True) == 0
        t_stats = binding.Stats(); t_pose = np.zeros(7); d_rec = C.c_void_p(); t_dinfo = binding.CorrespondenceInfo()
        twin_host = twin.prepare_correspondences(N_POINTS, want_points=False)[0]
        twin_dev = lambda: twin.L.so_icp_correspondences(twin.h, None, None, 0, None, None, 0, C.byref(d_rec), C.byref(t_dinfo))
        F64P = C.POINTER(C.c_double)
        regs = [(lambda k=k: twin.L.so_icp_register(twin.h, t_scans[k % S].ctypes.data_as(C.POINTER(C.c_float)), N_POINTS, 12, guesses_out[k].ctypes.data_as(F64P),
                                                   t_pose.ctypes.data_as(F64P), C.byref(t_stats))) for k in range(K)]

        def twins(after):
            for k in range(K):
                assert regs[k]() == 0
                assert after() == 0

        for p in range(a.passes + 1):
            t_run = run()
            t_host, t_dev, t_sums = timed(lambda: exp_host()), timed(lambda: exp_dev()), timed(lambda: sums_call())
            t_twin_host, t_twin_dev, t_reg = timed(lambda: twins(twin_host), twin), timed(lambda: twins(twin_dev), twin), timed(lambda: twins(lambda: 0), twin)
            if p:
                print("[export] pass %d: run of %d frames with the switch on %.3f ms; %d records.  One export call: records to the host %.3f ms, left on the device %.3f ms; "
                      "one sums call at 1 pose per frame %.3f ms.  %d x (so_icp_register + so_icp_correspondences): records to the host %.3f ms, left on the device %.3f ms "
                      "(%d registrations alone %.3f ms)" % (p, K, 1e3 * t_run, int(first[K]), 1e3 * t_host, 1e3 * t_dev, 1e3 * t_sums, K, 1e3 * t_twin_host, 1e3 * t_twin_dev,
                                                            K, 1e3 * t_reg), flush=True)
        twin.close()
cx.close()
