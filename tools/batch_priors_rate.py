#!/usr/bin/env python3
"""One pose prior per hypothesis of a batch on the bench's `batch64` inputs (scene os1_128_2m: 131 072-point scans against the 2 M-point
map, 64 guesses per scan at +-0.5 m / +-5 degrees, seeds 5000 + 64 i + h): the batch of 64 without priors, with a prior on every
hypothesis (so_icp_set_batch_priors), and the only way to register 64 hypotheses of the regularised problem without that entry:
64 x (so_icp_set_pose_prior + so_icp_register_dev) on the resident scan.
usage (GPU box): python tools/batch_priors_rate.py [--mode plain|prior|loop|solve] [--passes 3] [--root DIR]
  plain   the batch of 64 without priors, registrations/s per pass.  Needs nothing of this change: --root names another checkout
          whose built superodom_amd is measured (the parent commit's); the job alternates processes of the two builds
  prior   per pass: the batch without priors, the batch with the reference's diagonal form measured at every hypothesis' guess
          (SO_ICP_PRIOR_AT_GUESS, the uncertainty terms at 0), the batch with U = 0 on every hypothesis, and the loop of single
          registrations with the reference's form on the guess
  loop    that loop alone (runs on the parent's build too: --root)
  solve   nothing but one batch without priors and one with a prior on every hypothesis per scan -- the run to put under
          rocprofv3 --kernel-trace --stats: solve_kernel<.., true> and solve_kernel_batch_prior in one trace
Wall-clock times of whole calls from Python (ctypes with pre-built arguments); the kernels' own times come from a profiler run."""
import argparse, os, sys, time
import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--mode", default="prior", choices=["plain", "prior", "loop", "solve"]); ap.add_argument("--passes", type=int, default=3)
ap.add_argument("--root", default=None, help="another checkout whose built superodom_amd is measured")
a = ap.parse_args()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.abspath(a.root) if a.root else ROOT)
from superodom_amd import binding, synth  # noqa: E402
import pose_prior_ref as ppr  # noqa: E402

C = binding.C
REPS, B = 3, 64
sc = synth.Scene("os1_128_2m")
cx = binding.LidarSlamGpu(rank=0, world_size=1, time_kernels=0, device_id=0, plane_res=sc.plane_res, line_res=sc.plane_res / 2,
                          max_iterations=5, lm_max_iterations=4, max_surface_features=-1)
cx.add_surf_point_cloud(sc.map_points)
cx.shift_map(sc.gt_pose(0)[:3])
d_scans = [cx.upload_scan(np.ascontiguousarray(sc.scan(i), dtype=np.float32)) for i in range(REPS)]
hyp = [np.ascontiguousarray(np.stack([synth.perturb_pose(sc.gt_pose(i), 5000 + 64 * i + h, 0.5, 5.0) for h in range(B)])) for i in range(REPS)]
UNCERTAINTY, CONFIDENCE = [0.0, 0.0, 0.0], 0.9
F64P, I32P = C.POINTER(C.c_double), C.POINTER(C.c_int32)


def evaluations(stats):
    """evaluation passes per registration: one per outer iteration and one per LM iteration"""
    return sum(sum(1 + s.iterations[i].lm_iterations for i in range(s.n_iterations)) for s in stats) / len(stats)


out = np.zeros((B, 7)); rcs = np.zeros(B, np.int32); sts = [(binding.Stats * B)() for _ in range(REPS)]
batch_calls = [(lambda i=i: cx.L.so_icp_register_batch(cx.h, None, d_scans[i][0], d_scans[i][1], 12, hyp[i].ctypes.data_as(F64P), B,
                                                       out.ctypes.data_as(F64P), sts[i], rcs.ctypes.data_as(I32P))) for i in range(REPS)]


def batch_priors(kind):
    """-> per scan, the call that sets the 64 priors of its batch"""
    ident = [0, 0, 0, 0, 0, 0, 1.0]
    if kind == "reference":
        p, mode = ppr.reference_prior(ident, UNCERTAINTY, CONFIDENCE), binding.PRIOR_AT_GUESS
    else:
        p, mode = binding.pose_prior(ident, np.zeros((6, 6)), ppr.REFERENCE_FLOOR, ppr.REFERENCE_FRACTION), binding.PRIOR_GIVEN
    arr = (binding.PosePrior * B)(*([p] * B)); modes = (C.c_uint8 * B)(*([mode] * B))
    return lambda: cx.L.so_icp_set_batch_priors(cx.h, B, arr, modes)


def batches(set_priors=None):
    """REPS batches of 64 -> (seconds, hypotheses that converged, evaluations per registration)"""
    cx.synchronize()
    ok = 0
    t0 = time.perf_counter()
    for i in range(REPS):
        if set_priors:
            assert set_priors() == 0
        r = batch_calls[i]()
        assert r >= 0, (r, cx.last_error())
        ok += r
    cx.synchronize()
    t = time.perf_counter() - t0
    every = [s for per_scan in sts for s in per_scan]
    assert all(bool(s.flags & binding.FLAG_POSE_PRIOR) == bool(set_priors) for s in every)
    return t, ok, evaluations(every)


def loop_setup():
    stats = [[binding.Stats() for _ in range(B)] for _ in range(REPS)]; poses = [[np.zeros(7) for _ in range(B)] for _ in range(REPS)]
    calls = [[cx.prepare_register_dev(d_scans[i][0], d_scans[i][1], hyp[i][h], stats[i][h], poses[i][h]) for h in range(B)] for i in range(REPS)]
    priors = [[ppr.reference_prior(hyp[i][h], UNCERTAINTY, CONFIDENCE) for h in range(B)] for i in range(REPS)]
    set_prior = [[(lambda p=priors[i][h]: cx.L.so_icp_set_pose_prior(cx.h, C.byref(p))) for h in range(B)] for i in range(REPS)]

    def loop():
        cx.synchronize()
        t0 = time.perf_counter()
        for i in range(REPS):
            for h in range(B):
                assert set_prior[i][h]() == 0
                assert calls[i][h]() >= 0
        cx.synchronize()
        t = time.perf_counter() - t0
        assert all(s.flags & binding.FLAG_POSE_PRIOR for row in stats for s in row)
        return t, evaluations([s for row in stats for s in row])
    return loop


N = REPS * B
if a.mode == "plain":
    for p in range(a.passes + 1):  # (pass 0 warms up)
        t, ok, ev = batches()
        if p:
            print("[plain] pass %d: batch of 64, no priors %.1f registrations/s (%.3f ms per batch, %.2f evaluations each, %d of %d converged)" % (p, N / t, 1e3 * t / REPS, ev, ok, N), flush=True)
elif a.mode == "loop":
    loop = loop_setup()
    for p in range(a.passes + 1):
        t, ev = loop()
        if p:
            print("[loop] pass %d: 64 x (so_icp_set_pose_prior on the guess + so_icp_register_dev) %.1f registrations/s (%.4f ms each, %.2f evaluations)" % (p, N / t, 1e3 * t / N, ev), flush=True)
elif a.mode == "prior":
    loop = loop_setup()
    reference, zero = batch_priors("reference"), batch_priors("zero")
    for p in range(a.passes + 1):
        t0, ok0, ev0 = batches()
        t1, ok1, ev1 = batches(reference)
        tz, okz, evz = batches(zero)
        t2, ev2 = loop()
        if p:
            print("[prior] pass %d: batch of 64, no priors %.1f registrations/s (%.3f ms per batch, %.2f evaluations); a prior at every hypothesis' guess %.1f "
                  "(%.3f ms, %.2f evaluations): %+.3f ms per batch; U = 0 on every hypothesis %.1f (%.3f ms, %.2f evaluations): %+.3f ms; 64 x (so_icp_set_pose_prior + "
                  "so_icp_register_dev) %.1f (%.4f ms each, %.2f evaluations): the batch with priors is %.2f times that"
                  % (p, N / t0, 1e3 * t0 / REPS, ev0, N / t1, 1e3 * t1 / REPS, ev1, 1e3 * (t1 - t0) / REPS, N / tz, 1e3 * tz / REPS, evz, 1e3 * (tz - t0) / REPS,
                     N / t2, 1e3 * t2 / N, ev2, t2 / t1), flush=True)
else:
    batches()
    _, _, ev0 = batches()
    _, _, ev1 = batches(batch_priors("zero"))
    print("[solve] %d batches of 64 per kind: no priors (%.2f evaluations each); U = 0 on every hypothesis (%.2f evaluations each: the same passes through the other kernel)" % (REPS, ev0, ev1))
cx.close()
