#!/usr/bin/env python3
"""Seam C on the workload scan (scene os1_128_2m: 131 072-point scans against the 2 M-point map): per-call times of so_icp_match and of
so_icp_correspondence_sums at 1 and at 64 poses, the same evaluation done from the records (so_icp_correspondences + a host sum in
numpy), and the registration rate of the host loop (tests/seam_c_ref.register_through_seam's schedule with pre-built calls) beside
the staged so_icp_register loop of bench.py.
usage (GPU box): python tools/seam_c_rate.py [--mode calls|loop|sums1|sums64] [--passes 3] [--steps 100]
  calls   per-call times: match, sums x 1, sums x 64, records + host sum
  loop    registrations/s: staged so_icp_register, then the host loop on the same scans and guesses
  sums1 / sums64   nothing but one match and `steps` sums calls at 1 / 64 poses (the run to put under rocprofv3 --kernel-trace --stats)
Wall-clock times of whole calls from Python (ctypes with pre-built arguments); the kernels' own times come from a profiler run."""
import argparse, os, sys, time
import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--mode", default="calls", choices=["calls", "loop", "sums1", "sums64"]); ap.add_argument("--passes", type=int, default=3)
ap.add_argument("--steps", type=int, default=100)
a = ap.parse_args()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
from superodom_amd import binding, synth  # noqa: E402
import correspondences_ref as cref  # noqa: E402

S = 4
sc = synth.Scene("os1_128_2m")
cx = binding.LidarSlamGpu(rank=0, world_size=1, time_kernels=0, device_id=0, plane_res=sc.plane_res, line_res=sc.plane_res / 2,
                          max_iterations=5, lm_max_iterations=4, max_surface_features=-1)
cx.add_surf_point_cloud(sc.map_points)
cx.shift_map(sc.gt_pose(0)[:3])
scans = [cx.host_alloc_like(np.ascontiguousarray(sc.scan(i), dtype=np.float32)) for i in range(S)]
guesses = [np.ascontiguousarray(sc.guess(i), dtype=np.float64) for i in range(S)]
assert cx.keep_correspondences(True) == 0
K = a.steps


def timed(fn, reps):
    cx.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    cx.synchronize()
    return 1e3 * (time.perf_counter() - t0) / reps


def poses_near(pose, k):
    return np.ascontiguousarray(np.stack([np.array(pose)] + [synth.perturb_pose(pose, 50 + j, 0.02, 0.2) for j in range(1, k)]))


if a.mode in ("sums1", "sums64"):
    k = 1 if a.mode == "sums1" else 64
    assert cx.match(scans[0], guesses[0])[0] == 0
    call, _, out = cx.prepare_correspondence_sums(poses_near(guesses[0], k))
    for _ in range(K):
        assert call() == 0
    print("[%s] %d calls at %d poses, count %d" % (a.mode, K, k, int(out[0].count)))
elif a.mode == "calls":
    st = binding.Stats()
    n = len(scans[0])
    match = lambda: cx.L.so_icp_match(cx.h, binding._p(scans[0], binding.C.c_float), n, 12, binding._p(guesses[0], binding.C.c_double), binding.C.byref(st))
    call1, _, out1 = cx.prepare_correspondence_sums(poses_near(guesses[0], 1))
    call64, _, out64 = cx.prepare_correspondence_sums(poses_near(guesses[0], 64))
    export_call, rec, _, _, info = cx.prepare_correspondences(n, want_points=False)

    def records_and_host_sum():
        assert export_call() == 0
        r = rec[:info.n_accepted]
        cref.normal_equations(r["p"], r["n"], r["residual"], r["weight"], np.array(info.pose_eval))

    for p in range(a.passes + 1):
        t_match = timed(match, K)
        assert st.n_iterations == 1
        t1, t64 = timed(call1, K), timed(call64, K)
        t_exp, t_host = timed(export_call, K), timed(records_and_host_sum, max(K // 10, 3))
        if p == 0:
            continue
        print("[calls] pass %d: so_icp_match %.4f ms; so_icp_correspondence_sums %.4f ms at 1 pose, %.4f ms at 64 poses (%.5f ms per pose); "
              "so_icp_correspondences records only %.4f ms, records + numpy sum %.3f ms; %d accepted of %d points"
              % (p, t_match, t1, t64, t64 / 64, t_exp, t_host, int(out1[0].count), n), flush=True)
else:
    stats = [binding.Stats() for _ in range(K)]; poses = [np.zeros(7) for _ in range(K)]
    calls = [cx.prepare_register(scans[k % S], guesses[k % S], stats[k], poses[k]) for k in range(K)]
    stage = [cx.prepare_stage_scan(scans[k % S]) for k in range(K + 1)]
    import seam_c_ref  # noqa: E402
    for p in range(a.passes + 1):
        cx.synchronize()
        t0 = time.perf_counter()
        stage[0]()
        for k in range(K):
            stage[k + 1]()
            assert calls[k]() == 0
        cx.synchronize()
        t_reg = time.perf_counter() - t0
        cx.stage_cancel(scans[K % S])
        n_loop = max(K // 4, 4)
        n_sums = 0
        t0 = time.perf_counter()
        for k in range(n_loop):
            res = seam_c_ref.register_through_seam(lambda T: seam_c_ref.sums_of_match(cx.match(scans[k % S], T)[1]),
                                                   lambda T: cx.correspondence_sums(T)[0], guesses[k % S], max_outer=5, lm_max=4)
            n_sums += res.n_sums_calls
        cx.synchronize()
        t_loop = time.perf_counter() - t0
        if p == 0:
            continue
        print("[loop] pass %d: staged so_icp_register %.1f registrations/s (%.4f ms each); host loop through so_icp_match / so_icp_correspondence_sums "
              "%.1f registrations/s (%.4f ms each, %.1f sums calls per registration, Python between the calls included)"
              % (p, K / t_reg, 1e3 * t_reg / K, n_loop / t_loop, 1e3 * t_loop / n_loop, n_sums / n_loop), flush=True)
cx.close()
