#!/usr/bin/env python3
"""The absolute pose prior on the workload scan (scene os1_128_2m: 131 072-point scans against the 2 M-point map): the staged
so_icp_register loop of bench.py with a prior set before every call beside the same loop without one, and the same prior through the
Seam C host loop (so_icp_match, so_icp_correspondence_sums and so_icp_pose_prior_sums around so_icp_lm_begin / _feed).
usage (GPU box): python tools/pose_prior_rate.py [--mode register|loop|solve] [--passes 3] [--steps 200] [--root DIR]
  register  registrations/s and ms each: no prior ever set; so_icp_set_pose_prior before every call with U = 0 (the same registration to the
            bit: what the mechanism costs); the same with the reference's form on the guess (another problem: the LM iterations are printed)
  loop      the host loop with the prior added to every Sums, registrations/s (tests/seam_c_ref.register_through_seam's schedule)
  solve     nothing but `steps` staged registrations without and `steps` with a prior (U = 0: the same passes) -- the run to put under
            rocprofv3 --kernel-trace --stats: solve_kernel beside solve_kernel_prior
Wall-clock times of whole calls from Python (ctypes with pre-built arguments); the kernels' own times come from a profiler run."""
import argparse, os, sys, time
import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--mode", default="register", choices=["register", "loop", "solve"]); ap.add_argument("--passes", type=int, default=3)
ap.add_argument("--steps", type=int, default=200)
ap.add_argument("--root", default=None, help="another checkout whose built superodom_amd is measured (e.g. one built with -DSO_PRIOR_OVERLAP=0)")
a = ap.parse_args()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.abspath(a.root) if a.root else ROOT)
from superodom_amd import binding, synth  # noqa: E402
import pose_prior_ref as ppr  # noqa: E402

S = 4
sc = synth.Scene("os1_128_2m")
cx = binding.LidarSlamGpu(rank=0, world_size=1, time_kernels=0, device_id=0, plane_res=sc.plane_res, line_res=sc.plane_res / 2,
                          max_iterations=5, lm_max_iterations=4, max_surface_features=-1)
cx.add_surf_point_cloud(sc.map_points)
cx.shift_map(sc.gt_pose(0)[:3])
scans = [cx.host_alloc_like(np.ascontiguousarray(sc.scan(i), dtype=np.float32)) for i in range(S)]
guesses = [np.ascontiguousarray(sc.guess(i), dtype=np.float64) for i in range(S)]
priors = [ppr.reference_prior(guesses[i], [0.2, 0.4, 0.1], 0.9) for i in range(S)]
zero_priors = [binding.pose_prior(guesses[i], np.zeros((6, 6)), ppr.REFERENCE_FLOOR, ppr.REFERENCE_FRACTION) for i in range(S)]
K = a.steps
stats = [binding.Stats() for _ in range(K)]; poses = [np.zeros(7) for _ in range(K)]
calls = [cx.prepare_register(scans[k % S], guesses[k % S], stats[k], poses[k]) for k in range(K)]
stage = [cx.prepare_stage_scan(scans[k % S]) for k in range(K + 1)]
set_prior = {"reference": [(lambda p=priors[i]: cx.L.so_icp_set_pose_prior(cx.h, binding.C.byref(p))) for i in range(S)],
             "zero": [(lambda p=zero_priors[i]: cx.L.so_icp_set_pose_prior(cx.h, binding.C.byref(p))) for i in range(S)]}


def evaluations():
    """evaluation passes per registration: one per outer iteration and one per LM iteration"""
    return sum(sum(1 + s.iterations[i].lm_iterations for i in range(s.n_iterations)) for s in stats) / K


def staged_loop(with_prior):
    cx.synchronize()
    t0 = time.perf_counter()
    stage[0]()
    for k in range(K):
        stage[k + 1]()
        if with_prior:
            assert set_prior[with_prior][k % S]() == 0
        assert calls[k]() == 0
    cx.synchronize()
    t = time.perf_counter() - t0
    cx.stage_cancel(scans[K % S])
    assert all(bool(s.flags & binding.FLAG_POSE_PRIOR) == bool(with_prior) for s in stats)
    return t


if a.mode == "solve":
    staged_loop(None)  # (solve_kernel beside solve_kernel_prior in the same trace)
    staged_loop("zero")
    print("[solve] %d staged registrations with a prior (U = 0), %.2f outer iterations and %.2f evaluations each" % (K, sum(s.n_iterations for s in stats) / K, evaluations()))
elif a.mode == "register":
    for p in range(a.passes + 1):  # (pass 0 warms up)
        t_plain, ev_plain = staged_loop(None), evaluations()
        t_zero, ev_zero = staged_loop("zero"), evaluations()
        t_ref, ev_ref = staged_loop("reference"), evaluations()
        if p:
            print("[register] pass %d: no prior %.1f registrations/s (%.4f ms each, %.2f evaluations); a prior with U = 0 before every call %.1f "
                  "(%.4f ms, %.2f evaluations): %+.4f ms; the reference's prior on the guess %.1f (%.4f ms, %.2f evaluations): %+.4f ms"
                  % (p, K / t_plain, 1e3 * t_plain / K, ev_plain, K / t_zero, 1e3 * t_zero / K, ev_zero, 1e3 * (t_zero - t_plain) / K,
                     K / t_ref, 1e3 * t_ref / K, ev_ref, 1e3 * (t_ref - t_plain) / K), flush=True)
else:
    import seam_c_ref  # noqa: E402
    assert cx.keep_correspondences(True) == 0
    n_loop = max(K // 4, 4)
    for p in range(a.passes + 1):
        n_sums = 0
        cx.synchronize()
        t0 = time.perf_counter()
        for k in range(n_loop):
            prior = priors[k % S]
            res = seam_c_ref.register_through_seam(ppr.with_prior(lambda T: seam_c_ref.sums_of_match(cx.match(scans[k % S], T)[1]), prior),
                                                   ppr.with_prior(lambda T: cx.correspondence_sums(T)[0], prior), guesses[k % S], max_outer=5, lm_max=4)
            n_sums += res.n_sums_calls
        cx.synchronize()
        t_loop = time.perf_counter() - t0
        if p:
            print("[loop] pass %d: host loop with so_icp_pose_prior_sums behind every match and sums call %.1f registrations/s (%.4f ms each, %.1f sums calls "
                  "per registration, Python between the calls included)" % (p, n_loop / t_loop, 1e3 * t_loop / n_loop, n_sums / n_loop), flush=True)
cx.close()
