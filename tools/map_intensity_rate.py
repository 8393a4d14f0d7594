#!/usr/bin/env python3
"""The `localization` block of bench.py on its own, with the intensity switch off or on (so_icp_set_cloud_intensity): wall time per frame
of back-to-back Localization() frames at BASELINE sizes, every map insert included.
usage (GPU box): python tools/map_intensity_rate.py [--intensity off|on] [--runs 3] [--frames 48] [--root DIR]
  raw_sweep   the 131 072-point scans themselves, the next one announced ahead (so_icp_stage_scan), so_icp_localization
  node_order  so_icp_prefilter_scan (VoxelGrid at planeRes) + so_icp_localization_dev on the filtered cloud
  --intensity on   the scans are 32-byte records with a seeded intensity at byte 16 and the switch is on (off: packed xyz, as bench.py)
  --root DIR       measure the package of another checkout (its superodom_amd/lib/libsoicp.so must be built); with --intensity off only
                   entries that every version has are called
One line per run; the spread between the runs of one build is the margin for comparing two builds."""
import argparse, os, sys, time
import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--intensity", default="off", choices=["off", "on"]); ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--frames", type=int, default=48); ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
a = ap.parse_args()
sys.path.insert(0, os.path.abspath(a.root))
from superodom_amd import binding, synth  # noqa: E402

on = a.intensity == "on"
sc = synth.Scene("os1_128_2m")
scans = [np.ascontiguousarray(sc.scan(i), np.float32) for i in range(4)]
guesses = [sc.guess(i) for i in range(4)]
if on:  # pcl::PointXYZI records: x y z, pad, intensity, pad
    rng = np.random.default_rng(1)
    recs = []
    for s in scans:
        r = np.zeros((len(s), 8), np.float32)
        r[:, :3] = s; r[:, 4] = rng.uniform(0, 255, len(s))
        recs.append(r)
    scans = recs
for run in range(a.runs):
    ls = binding.LidarSlamGpu(device_id=0, plane_res=sc.plane_res, line_res=sc.plane_res / 2, max_iterations=5, lm_max_iterations=4,
                              max_surface_features=-1, time_kernels=0)
    if on:
        assert ls.set_cloud_intensity(16) == 0
    ls.add_surf_point_cloud(sc.map_points)
    ls.shift_map(sc.gt_pose(0)[:3])
    bufs = [ls.host_alloc_like(x) for x in scans]

    def frames(node_order):
        for k in range(a.frames + 4):
            if k == 4:
                ls.map_size()  # (settles the insert in flight: the clock starts on an idle device)
                t_all = time.perf_counter()
            i = k % 4
            if node_order:
                if on:
                    d_f, n_f, _ = ls.prefilter_scan_records(bufs[i], False, sc.plane_res / 2, sc.plane_res)
                else:
                    d_f, n_f, _ = ls.prefilter_scan(bufs[i], False, sc.plane_res / 2, sc.plane_res)
                rc, _, _ = ls.localization_dev(True, guesses[i], d_f, n_f, 0.1 * k)
            elif on:
                if k == 0:
                    ls.stage_scan_records(bufs[0])
                ls.stage_scan_records(bufs[(k + 1) % 4])
                rc, _, _ = ls.localization_records(True, guesses[i], bufs[i], 0.1 * k)
            else:
                if k == 0:
                    ls.stage_scan(bufs[0])
                ls.stage_scan(bufs[(k + 1) % 4])
                rc, _, _ = ls.localization(True, guesses[i], bufs[i], 0.1 * k)
            assert rc == 0
        ls.map_size()  # (the last insert included)
        return 1e3 * (time.perf_counter() - t_all) / a.frames
    raw, node = frames(False), frames(True)
    print("[intensity %s] run %d: raw_sweep_ms_per_frame %.4f node_order_ms_per_frame %.4f | map %d points | inserts laid out by the device / handed back %s"
          % (a.intensity, run, raw, node, ls.map_size(), ls.map_insert_stats()), flush=True)
    ls.close()
