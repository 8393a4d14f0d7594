"""-m gpu: the end of a solve in the persistent launch -- the state block kept in LDS and written out once, the mirror published
without fences, and the evaluation pass that is not run when the proposed step is within the parameter tolerance.  None of it may
change a bit: every case is compared with the per-evaluation launches (SOICP_PERSISTENT=0: the one-thread controller, lm_solver.h's
protocol step for step, publish_state_to) and held to the oracle's counts and codes."""
import os

import numpy as np
import pytest

import pose_prior_ref as ppr
from helpers import assert_follows_oracle, assert_same_bits, chain_deltas, scene_with_oracle

pytestmark = pytest.mark.gpu

MK = dict(max_surface_features=-1, max_iterations=5)
PROF_ENDGAME = str(128 | 131072)  # SOICP_ABLATE: the instrumented solve, dbg[8..15] = the end-game record (kernels.hip eval_pass)
PASSES_WORD = 15                  # passes the solve launch ran

# The registration whose first solve ends on the parameter tolerance, fixed by the oracle on the CPU: `small`, scan 2, from a guess 2 cm
# and 0.2 degrees off.  Oracle: (lm_iterations, successful steps, termination) = (3, 2, 2) then (2, 1, 1).
PTOL_SCENE, PTOL_SCAN, PTOL_GUESS = "small", 2, dict(dt=0.02, dth_deg=0.2)


def _make_with_env(make, env, **kw):
    """a context created under `env` (read by so_icp_create)"""
    for k, v in env.items():
        os.environ[k] = v
    try:
        return make(**kw)
    finally:
        for k in env:
            del os.environ[k]


def _codes(st):
    it = st.iterations if hasattr(st, "iterations") else st.iters
    return [(it[k].lm_iterations, it[k].num_successful_steps, it[k].termination) for k in range(st.n_iterations)]


@pytest.fixture(scope="module")
def tiny(oracle, gpu_slam_factory):
    """`tiny` with its oracle map, a context as built and one with per-evaluation launches; the oracle's registrations of scans 0 and 1"""
    sc, slam, om = scene_with_oracle("tiny", oracle, gpu_slam_factory, max_iterations=5)
    per_eval = _make_with_env(gpu_slam_factory, {"SOICP_PERSISTENT": "0"}, plane_res=sc.plane_res, line_res=sc.plane_res / 2, **MK)
    per_eval.add_surf_point_cloud(sc.map_points)
    refs = {i: om.register(sc.scan(i), sc.guess(i), oracle.default_config(max_iterations=5)) for i in (0, 1)}
    assert [refs[i][2].n_iterations for i in (0, 1)] == [2, 3], "the oracle's outer iteration counts of tiny scans 0 and 1"
    yield sc, slam, per_eval, refs
    slam.close(); per_eval.close()


@pytest.mark.parametrize("scan", [0, 1])
def test_single_registration(tiny, scan):
    sc, slam, per_eval, refs = tiny
    rc, pose, st = slam.register(sc.scan(scan), sc.guess(scan))
    rc2, pose2, st2 = per_eval.register(sc.scan(scan), sc.guess(scan))
    orc, opose, ost, _ = refs[scan]
    assert rc == rc2 == orc == 0
    assert_follows_oracle(st, ost, ("tiny", scan), pose=pose, opose=opose)
    assert np.array_equal(pose, pose2), pose - pose2
    assert_same_bits(st, st2, ("persistent vs per-evaluation launches", scan))  # (equal call histories: uncertainty included)


def test_registration_with_a_pose_prior(tiny):
    sc, slam, per_eval, _ = tiny
    prior = ppr.reference_prior(sc.guess(1), [0.2, 0.4, 0.1], 0.9)
    out = []
    for s in (slam, per_eval):
        s.set_pose_prior(prior)
        rc, pose, st = s.register(sc.scan(1), sc.guess(1))
        assert rc == 0
        out.append((pose, st))
    assert out[0][1].n_iterations >= 2
    assert np.array_equal(out[0][0], out[1][0]), out[0][0] - out[1][0]
    assert_same_bits(out[0][1], out[1][1], "pose prior: persistent vs per-evaluation launches")


def test_chained_sequence(gpu_slam_factory):
    """Eight chained scans: the solves that do not end a registration leave their report to the sweep behind them, the last solve of
    every registration publishes itself; both as built and with per-evaluation launches, and each equal to the single call from the
    guess the sequence reports."""
    from superodom_amd import synth
    sc = synth.Scene("tiny")
    mk = dict(plane_res=sc.plane_res, line_res=sc.plane_res / 2, **MK)
    seq, plain = gpu_slam_factory(**mk), gpu_slam_factory(**mk)
    seq0 = _make_with_env(gpu_slam_factory, {"SOICP_PERSISTENT": "0"}, **mk)
    for s in (seq, plain, seq0):
        s.add_surf_point_cloud(sc.map_points)
    ids = list(range(8))
    deltas = chain_deltas(sc, ids)
    res = []
    for s in (seq, seq0):
        scans = [s.host_alloc_like(np.ascontiguousarray(sc.scan(i), dtype=np.float32)) for i in ids]
        rc, poses, guesses, stats, n_done = s.register_sequence(scans, sc.guess(0), deltas)
        assert rc == 0 and n_done == len(ids), (rc, n_done, s.last_error())
        res.append((poses, guesses, stats))
    (poses, guesses, stats), (poses0, guesses0, stats0) = res
    assert max(st.n_iterations for st in stats) >= 2, "no solve of the sequence deferred its report"
    for k in ids:
        assert np.array_equal(poses[k], poses0[k]) and np.array_equal(guesses[k], guesses0[k]), k
        assert_same_bits(stats[k], stats0[k], ("sequence: persistent vs per-evaluation launches", k))
        prc, ppose, pst = plain.register(sc.scan(k), guesses[k])
        assert prc == 0 and np.array_equal(ppose, poses[k]), (k, ppose - poses[k])
        assert_same_bits(pst, stats[k], ("sequence vs single call", k))
    seq.close(); plain.close(); seq0.close()


@pytest.fixture(scope="module")
def ptol(oracle, gpu_slam_factory):
    """PTOL_SCENE with its oracle map and, for max_iterations 1 and 5, an instrumented context, and for 1 also one as built and one with
    per-evaluation launches"""
    sc, prof1, om = _make_with_env(lambda **kw: scene_with_oracle(PTOL_SCENE, oracle, gpu_slam_factory, **kw), {"SOICP_ABLATE": PROF_ENDGAME}, max_iterations=1)
    ctxs = {"prof1": prof1}
    for name, env, iters in (("prof5", {"SOICP_ABLATE": PROF_ENDGAME}, 5), ("built1", {}, 1), ("per_eval1", {"SOICP_PERSISTENT": "0"}, 1)):
        ctxs[name] = _make_with_env(gpu_slam_factory, env, plane_res=sc.plane_res, line_res=sc.plane_res / 2, max_surface_features=-1, max_iterations=iters)
        ctxs[name].add_surf_point_cloud(sc.map_points)
    yield sc, om, ctxs
    for s in ctxs.values():
        s.close()


def test_parameter_tolerance_skips_the_pass(ptol, oracle):
    sc, om, ctxs = ptol
    scan, guess = sc.scan(PTOL_SCAN), sc.guess(PTOL_SCAN, **PTOL_GUESS)
    orc, opose, ost, _ = om.register(scan, guess, oracle.default_config(max_iterations=1))
    assert orc == 0 and _codes(ost) == [(3, 2, 2)], f"the oracle no longer ends this solve on the parameter tolerance: {_codes(ost)}"
    got = {}
    for name in ("prof1", "built1", "per_eval1"):
        rc, pose, st = ctxs[name].register(scan, guess)
        assert rc == 0, (name, rc)
        assert _codes(st) == _codes(ost), (name, _codes(st))
        assert_follows_oracle(st, ost, name, pose=pose, opose=opose)
        got[name] = (pose, st)
    for name in ("prof1", "built1"):
        assert np.array_equal(got[name][0], got["per_eval1"][0]), name
        assert_same_bits(got[name][1], got["per_eval1"][1], (name, "vs per-evaluation launches"))
    passes = int(ctxs["prof1"].debug_stamps()[PASSES_WORD])
    print("termination 2: lm_iterations", ost.iters[0].lm_iterations, "passes run", passes)
    assert passes == ost.iters[0].lm_iterations == 3, "the solve that ends on the parameter tolerance runs one pass fewer than 1 + lm_iterations"


def test_whole_registration_after_the_skipped_pass(ptol, oracle):
    """the same registration to its end: the solve behind the one that ended on the parameter tolerance stops on the function tolerance"""
    sc, om, ctxs = ptol
    scan, guess = sc.scan(PTOL_SCAN), sc.guess(PTOL_SCAN, **PTOL_GUESS)
    orc, opose, ost, _ = om.register(scan, guess, oracle.default_config(max_iterations=5))
    assert orc == 0 and _codes(ost) == [(3, 2, 2), (2, 1, 1)], _codes(ost)
    rc, pose, st = ctxs["prof5"].register(scan, guess)
    assert rc == 0 and _codes(st) == _codes(ost), _codes(st)
    assert_follows_oracle(st, ost, "prof5", pose=pose, opose=opose)
    assert int(ctxs["prof5"].debug_stamps()[PASSES_WORD]) == 1 + ost.iters[1].lm_iterations


def test_function_tolerance_runs_every_pass(tiny, oracle, gpu_slam_factory):
    """tiny scan 0 held to one outer iteration: (3, 2, 1) by the oracle, and the instrumented solve counts 1 + 3 passes"""
    sc, _, _, refs = tiny
    assert _codes(refs[0][2])[0] == (3, 2, 1), _codes(refs[0][2])
    prof = _make_with_env(gpu_slam_factory, {"SOICP_ABLATE": PROF_ENDGAME}, plane_res=sc.plane_res, line_res=sc.plane_res / 2, max_surface_features=-1, max_iterations=1)
    prof.add_surf_point_cloud(sc.map_points)
    rc, pose, st = prof.register(sc.scan(0), sc.guess(0))
    assert rc == 0 and _codes(st) == [(3, 2, 1)], _codes(st)
    passes = int(prof.debug_stamps()[PASSES_WORD])
    prof.close()
    print("termination 1: lm_iterations 3, passes run", passes)
    assert passes == 1 + 3, "a solve that ends on the function tolerance runs exactly 1 + lm_iterations passes"
