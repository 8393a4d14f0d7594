#!/usr/bin/env python3
"""Per-frame pose priors in the chained sequence on the workload scan (scene os1_128_2m: 131 072-point scans against the 2 M-point
map): `steps` registrations as ONE so_icp_register_sequence call, as bench.py's `chained` entry runs them, without priors and with a
prior measured at every frame's own guess (so_icp_set_sequence_priors, SO_ICP_PRIOR_AT_GUESS), beside the only way to put that prior
on every frame without this entry: so_icp_set_pose_prior on the guess before every call of the staged so_icp_register loop.
usage (GPU box): python tools/sequence_priors_rate.py [--mode chain|prior|staged|solve] [--passes 3] [--steps 200] [--root DIR]
  chain   the chained sequence without priors, registrations/s per pass.  Needs nothing of this change: --root names another checkout
          whose built superodom_amd is measured (the parent commit's); the job alternates processes of the two builds
  prior   per pass: the chained sequence without priors, with an AT_GUESS prior on every frame (the reference's form, the uncertainty
          terms at 0), and the staged loop with so_icp_set_pose_prior(the same form on the guess) before every so_icp_register
  staged  that staged loop alone (runs on the parent's build too: --root)
  solve   nothing but one chained call without priors, one with GIVEN priors and one with AT_GUESS priors -- the run to put under
          rocprofv3 --kernel-trace --stats: solve_kernel, solve_kernel_prior and solve_kernel_prior_at_guess in one trace
Wall-clock times of whole calls from Python (ctypes with pre-built arguments); the kernels' own times come from a profiler run."""
import argparse, os, sys, time
import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--mode", default="prior", choices=["chain", "prior", "staged", "solve"]); ap.add_argument("--passes", type=int, default=3)
ap.add_argument("--steps", type=int, default=200)
ap.add_argument("--root", default=None, help="another checkout whose built superodom_amd is measured")
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
K = a.steps
UNCERTAINTY, CONFIDENCE = [0.0, 0.0, 0.0], 0.9


def seq_args(steps):
    """bench.py's chained entry: scan k % S, delta_k = gt(k - 1)^-1 o guess(k)"""
    d = np.zeros((steps, 7)); d[:, 6] = 1.0
    for k in range(1, steps):
        d[k] = synth.pose_between(sc.gt_pose((k - 1) % S), guesses[k % S])
    return [scans[k % S] for k in range(steps)], d


seq_scans, seq_d = seq_args(K)
call_seq, seq_out, seq_g, seq_st, seq_n, _keep = cx.prepare_register_sequence(seq_scans, guesses[0], seq_d)


def evaluations(stats):
    """evaluation passes per registration: one per outer iteration and one per LM iteration"""
    return sum(sum(1 + s.iterations[i].lm_iterations for i in range(s.n_iterations)) for s in stats) / len(stats)


def chained(set_priors=None):
    """one call over K scans -> (seconds, chained registrations, chain breaks)"""
    cx.reset_timing()
    cx.synchronize()
    if set_priors:
        assert set_priors() == 0
    t0 = time.perf_counter()
    rc = call_seq()
    cx.synchronize()
    t = time.perf_counter() - t0
    assert rc == 0 and seq_n.value == K, (rc, seq_n.value, cx.last_error())
    st = list(seq_st)[:K]
    assert all(bool(s.flags & binding.FLAG_POSE_PRIOR) == bool(set_priors) for s in st)
    tm = cx.timing()
    return t, int(tm.seq_chained), int(tm.seq_chain_breaks), evaluations(st)


def staged_setup():
    stats = [binding.Stats() for _ in range(K)]; poses = [np.zeros(7) for _ in range(K)]
    calls = [cx.prepare_register(scans[k % S], guesses[k % S], stats[k], poses[k]) for k in range(K)]
    stage = [cx.prepare_stage_scan(scans[k % S]) for k in range(K + 1)]
    priors = [ppr.reference_prior(guesses[i], UNCERTAINTY, CONFIDENCE) for i in range(S)]
    set_prior = [(lambda p=priors[i]: cx.L.so_icp_set_pose_prior(cx.h, binding.C.byref(p))) for i in range(S)]

    def loop():
        cx.synchronize()
        t0 = time.perf_counter()
        stage[0]()
        for k in range(K):
            stage[k + 1]()
            assert set_prior[k % S]() == 0
            assert calls[k]() == 0
        cx.synchronize()
        t = time.perf_counter() - t0
        cx.stage_cancel(scans[K % S])
        assert all(s.flags & binding.FLAG_POSE_PRIOR for s in stats)
        return t, evaluations(stats)
    return loop


def run_priors(mode):
    ident = [0, 0, 0, 0, 0, 0, 1.0]
    ps = [ppr.reference_prior(guesses[k % S] if mode == binding.PRIOR_GIVEN else ident, UNCERTAINTY, CONFIDENCE) for k in range(K)]
    arr = (binding.PosePrior * K)(*ps)
    modes = (binding.C.c_uint8 * K)(*([mode] * K))
    return lambda: cx.L.so_icp_set_sequence_priors(cx.h, K, arr, modes)


if a.mode == "chain":
    for p in range(a.passes + 1):  # (pass 0 warms up)
        t, n_ch, n_br, ev = chained()
        if p:
            print("[chain] pass %d: %.1f registrations/s (%.4f ms each, %.2f evaluations; %d chained, %d chain breaks)" % (p, K / t, 1e3 * t / K, ev, n_ch, n_br), flush=True)
elif a.mode == "staged":
    loop = staged_setup()
    for p in range(a.passes + 1):
        t, ev = loop()
        if p:
            print("[staged] pass %d: so_icp_set_pose_prior on the guess before every so_icp_register %.1f registrations/s (%.4f ms each, %.2f evaluations)" % (p, K / t, 1e3 * t / K, ev), flush=True)
elif a.mode == "prior":
    loop = staged_setup()
    at_guess = run_priors(binding.PRIOR_AT_GUESS)
    for p in range(a.passes + 1):
        t0, ch0, br0, ev0 = chained()
        t1, ch1, br1, ev1 = chained(at_guess)
        t2, ev2 = loop()
        if p:
            print("[prior] pass %d: chained, no priors %.1f registrations/s (%.4f ms each, %.2f evaluations, %d chained, %d breaks); chained, a prior at every "
                  "frame's guess %.1f (%.4f ms, %.2f evaluations, %d chained, %d breaks): %+.4f ms; staged so_icp_set_pose_prior + so_icp_register %.1f "
                  "(%.4f ms, %.2f evaluations): the chained run with priors is %.3f times that"
                  % (p, K / t0, 1e3 * t0 / K, ev0, ch0, br0, K / t1, 1e3 * t1 / K, ev1, ch1, br1, 1e3 * (t1 - t0) / K, K / t2, 1e3 * t2 / K, ev2, t2 / t1), flush=True)
else:
    chained()
    _, ch1, _, ev1 = chained(run_priors(binding.PRIOR_GIVEN))
    _, ch2, _, ev2 = chained(run_priors(binding.PRIOR_AT_GUESS))
    print("[solve] %d registrations per call: no priors; GIVEN priors on the guesses of the staged loop (%d chained, %.2f evaluations each); AT_GUESS priors (%d chained, "
          "%.2f evaluations each)" % (K, ch1, ev1, ch2, ev2))
cx.close()
