#!/usr/bin/env python3
"""The staged so_icp_register loop of bench.py on its own (scene os1_128_2m: 131 072-point scans against the 2 M-point map, the next
scan announced with so_icp_stage_scan while the current one registers), with the correspondence switch off or on
(so_icp_keep_correspondences) and, optionally, one so_icp_correspondences call per registration.
usage (GPU box): python tools/correspondences_rate.py [--mode plain|off|on|export|export_points] [--passes 3] [--steps 200] [--root DIR]
  plain          the switch is never touched (the only mode another checkout's build can run: --root DIR, whose
                 superodom_amd/lib/libsoicp.so must be built)
  off            turned on and off again before the loop
  on             on: every registration keeps a copy of its scan (12 n bytes, device to device)
  export         on, and one export per registration: the records only
  export_points  on, and one export per registration: records, status bytes and float residuals
One line per pass: registrations per second and, with an export, the milliseconds per export call.  Run the modes as separate
processes, interleaved; the spread between the passes of one build is the margin for comparing two builds."""
import argparse, os, sys, time
import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--mode", default="plain", choices=["plain", "off", "on", "export", "export_points"]); ap.add_argument("--passes", type=int, default=3)
ap.add_argument("--steps", type=int, default=200); ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--label", default=None)
a = ap.parse_args()
sys.path.insert(0, os.path.abspath(a.root))
from superodom_amd import binding, synth  # noqa: E402

S = 4
sc = synth.Scene("os1_128_2m")
cx = binding.LidarSlamGpu(rank=0, world_size=1, time_kernels=0, device_id=0, plane_res=sc.plane_res, line_res=sc.plane_res / 2,
                          max_iterations=5, lm_max_iterations=4, max_surface_features=-1)
cx.add_surf_point_cloud(sc.map_points)
cx.shift_map(sc.gt_pose(0)[:3])
scans = [cx.host_alloc_like(np.ascontiguousarray(sc.scan(i), dtype=np.float32)) for i in range(S)]
guesses = [np.ascontiguousarray(sc.guess(i), dtype=np.float64) for i in range(S)]
if a.mode != "plain":
    assert cx.keep_correspondences(True) == 0
    if a.mode == "off":
        assert cx.keep_correspondences(False) == 0
export = a.mode.startswith("export")
K = a.steps
stats = [binding.Stats() for _ in range(K)]; poses = [np.zeros(7) for _ in range(K)]
calls = [cx.prepare_register(scans[k % S], guesses[k % S], stats[k], poses[k]) for k in range(K)]
stage = [cx.prepare_stage_scan(scans[k % S]) for k in range(K + 1)]
if export:
    export_call, rec, status, resid, info = cx.prepare_correspondences(max(len(s_) for s_ in scans), want_points=(a.mode == "export_points"))
for p in range(a.passes + 1):  # (pass 0 warms up: allocations, the first binning ahead)
    cx.synchronize()
    t_export = 0.0
    t0 = time.perf_counter()
    stage[0]()
    for k in range(K):
        stage[k + 1]()
        assert calls[k]() == 0
        if export:
            t1 = time.perf_counter()
            assert export_call() == 0
            t_export += time.perf_counter() - t1
            assert info.valid == 1 and info.n_accepted == stats[k].iterations[stats[k].n_iterations - 1].num_surf_from_scan
    cx.synchronize()
    t = time.perf_counter() - t0
    cx.stage_cancel(scans[K % S])
    if p == 0:
        continue
    line = "[%s] pass %d: %d registrations, %.1f registrations/s (%.4f ms each)" % (a.label or a.mode, p, K, K / t, 1e3 * t / K)
    if export:
        line += ", export %.4f ms per call (%d records of %d points), %.1f registrations/s without the exports' time" % (
            1e3 * t_export / K, info.n_accepted, info.n_points, K / (t - t_export))
    print(line, flush=True)
cx.close()
