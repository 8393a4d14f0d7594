#!/usr/bin/env python3
"""The staged so_icp_register loop of bench.py on its own (scene os1_128_2m: 131 072-point scans against the 2 M-point map, the next
scan announced with so_icp_stage_scan while the current one registers), with the geometry switch
(so_icp_keep_correspondence_geometry) never touched, off or on and, optionally, one so_icp_correspondence_geometry call per
registration.
usage (GPU box): python tools/correspondence_geometry_rate.py [--mode MODE] [--passes 3] [--steps 200] [--root DIR]
  plain          neither switch is ever touched (the only mode another checkout's build can run: --root DIR, whose
                 superodom_amd/lib/libsoicp.so must be built)
  off            both switches turned on and off again before the loop
  corr           so_icp_keep_correspondences on, the geometry switch off: the base line of the snapshot's cost
  on             both on: every registration also snapshots its neighbours (one launch, 81 n bytes written at most)
  export_counts  both on, and one export per registration with no host output: the kernel, the counts' copy and the wait
  export         ... with the records copied to the host (192 bytes each)
  export_points  ... with the records and the 3 n label bytes
One line per pass: registrations per second and, with an export, the milliseconds per export call.  The snapshot's cost per
registration is `on` against `corr`; the export's copy is `export` against `export_counts`.  Run the modes as separate processes,
interleaved; the spread between the processes of one build is the margin for comparing two builds."""
import argparse, os, sys, time
import numpy as np

MODES = ["plain", "off", "corr", "on", "export_counts", "export", "export_points"]
ap = argparse.ArgumentParser()
ap.add_argument("--mode", default="plain", choices=MODES); ap.add_argument("--passes", type=int, default=3)
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
    if a.mode != "corr":
        assert cx.keep_correspondence_geometry(True) == 0
    if a.mode == "off":
        assert cx.keep_correspondence_geometry(False) == 0 and cx.keep_correspondences(False) == 0
export = a.mode.startswith("export")
K = a.steps
stats = [binding.Stats() for _ in range(K)]; poses = [np.zeros(7) for _ in range(K)]
calls = [cx.prepare_register(scans[k % S], guesses[k % S], stats[k], poses[k]) for k in range(K)]
stage = [cx.prepare_stage_scan(scans[k % S]) for k in range(K + 1)]
if export:
    cap = max(len(s_) for s_ in scans)
    export_call, rec, labels, info = cx.prepare_correspondence_geometry(0 if a.mode == "export_counts" else cap, want_points=False)
    if a.mode == "export_points":
        export_call, rec, labels, info = cx.prepare_correspondence_geometry(cap, want_points=True)
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
            last = stats[k].iterations[stats[k].n_iterations - 1]
            assert info.valid == 1 and info.n_accepted == last.num_surf_from_scan and list(info.obs_hist) == list(last.obs_hist)
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
