"""-m gpu: what the sweep and solve kernels do at entry -- the lines of the kernel arguments and of the state block that their first
statements read are requested together, before the "already converged?" / "predecessor over?" tests.  Nothing of it may change a
result: every case is held to the oracle, and to the bit against a path with another entry (per-evaluation launches, no speculated
launches, the ordinary entry point, single registrations).  The sizes walk the persistent solve through every number of queries a
thread can own, where an entry-time request for a thread's first query pair (built, measured, not kept: profiles/launch_entry)
has its guards."""
import os

import numpy as np
import pytest

from helpers import CARRIED_OVER_FIELDS, assert_follows_oracle, assert_same_bits, chain_deltas, scene_with_oracle
from superodom_amd import synth

pytestmark = pytest.mark.gpu

SCAN = 3          # scan of the `small` scene whose first n points are registered
WORKGROUPS = 16   # 4 096 solve threads: a thread owns 0, 1, 2 or 4 queries over the sizes below
SIZES = [1, 255, 256, 257, 4095, 4096, 4097, 8191, 8192, 8193, 16384]


def _make_with_env(make, env, **kw):
    """a context created under `env` (read by so_icp_create)"""
    for k, v in env.items():
        os.environ[k] = v
    try:
        return make(**kw)
    finally:
        for k in env:
            del os.environ[k]


@pytest.fixture(scope="module")
def small(oracle, gpu_slam_factory):
    """the `small` scene with its oracle map and three contexts: 16 solve workgroups, the same with per-evaluation launches, default grid"""
    sc, few, om = scene_with_oracle("small", oracle, gpu_slam_factory, max_iterations=5, solve_workgroups=WORKGROUPS)
    mk = dict(plane_res=sc.plane_res, line_res=sc.plane_res / 2, max_surface_features=-1, max_iterations=5)
    per_eval = _make_with_env(gpu_slam_factory, {"SOICP_PERSISTENT": "0"}, solve_workgroups=WORKGROUPS, **mk)
    full = gpu_slam_factory(**mk)
    for s in (per_eval, full):
        s.add_surf_point_cloud(sc.map_points)
    refs = {}

    def oracle_of(n):  # one oracle registration per size, shared by the cases that need it
        if n not in refs:
            refs[n] = om.register(np.ascontiguousarray(sc.scan(SCAN)[:n]), sc.guess(SCAN), oracle.default_config(max_iterations=5))
        return refs[n]
    yield sc, few, per_eval, full, oracle_of
    for s in (few, per_eval, full):
        s.close()


def _follows(rc, pose, st, ref, tag):
    orc, opose, ost, _ = ref
    assert rc == orc, (tag, rc, orc)
    if rc == 0:
        assert_follows_oracle(st, ost, tag, pose=pose, opose=opose)
    else:  # so few points do not register: equal return codes and equal statistics
        assert_follows_oracle(st, ost, tag)


@pytest.mark.parametrize("n", SIZES)
def test_solve_entry_at_every_ownership_count(small, n):
    sc, few, per_eval, _, oracle_of = small
    scan, guess = np.ascontiguousarray(sc.scan(SCAN)[:n]), sc.guess(SCAN)
    rc, pose, st = few.register(scan, guess)
    _follows(rc, pose, st, oracle_of(n), ("16 workgroups", n))
    if n <= 256 * WORKGROUPS:  # one query per thread at the most: the sums do not depend on the grid
        rc2, pose2, st2 = per_eval.register(scan, guess)
        assert rc2 == rc and np.array_equal(pose, pose2), (n, rc, rc2)
        assert_same_bits(st, st2, ("persistent vs per-evaluation launches", n), omit=CARRIED_OVER_FIELDS)


@pytest.mark.parametrize("n", [257, 16384])
def test_solve_entry_at_the_default_grid(small, n):
    sc, _, _, full, oracle_of = small
    rc, pose, st = full.register(np.ascontiguousarray(sc.scan(SCAN)[:n]), sc.guess(SCAN))
    _follows(rc, pose, st, oracle_of(n), ("default grid", n))


@pytest.mark.parametrize("scene", ["tiny", "small"])  # (tiny: the wavefront-per-query sweep; small: the chunked sweep)
def test_launches_that_return_at_entry(oracle, gpu_slam_factory, scene):
    """A registration that converges in fewer outer iterations than were enqueued ahead: the speculated launches behind it return at
    entry, after the requests the entry code makes.  Same bits as without speculation."""
    sc, spec, _ = scene_with_oracle(scene, oracle, gpu_slam_factory, oracle_too=False, max_iterations=5)
    mk = dict(plane_res=sc.plane_res, line_res=sc.plane_res / 2, max_surface_features=-1, max_iterations=5)
    plain = _make_with_env(gpu_slam_factory, {"SOICP_SPECULATE": "0"}, **mk)
    plain.add_surf_point_cloud(sc.map_points)
    scan, guess = sc.scan(1), sc.guess(1)
    rc1, p1, s1 = spec.register(scan, guess)
    rc2, p2, s2 = plain.register(scan, guess)
    assert rc1 == rc2 == 0
    assert s1.n_iterations < 5, f"the registration used every enqueued iteration ({s1.n_iterations}): no launch returned at entry"
    assert np.array_equal(p1, p2), p1 - p2
    assert_same_bits(s1, s2, ("speculation on vs off", scene))
    spec.close(); plain.close()


def test_chain_break_launches_return_on_done_count(gpu_slam_factory):
    """so_icp_register_sequence over five tiny scans, the third 0.45 m / 4 degrees off its prediction: it needs more outer iterations
    than were enqueued, the launches of the registration behind it return on done_count.  Every registration is the one
    so_icp_register performs from the guess the call reports."""
    sc = synth.Scene("tiny")
    mk = dict(plane_res=sc.plane_res, line_res=sc.plane_res / 2, max_surface_features=-1, max_iterations=5)
    slam, plain = gpu_slam_factory(**mk), gpu_slam_factory(**mk)
    for s in (slam, plain):
        s.add_surf_point_cloud(sc.map_points)
    ids = [0, 1, 2, 3, 4]
    scans = [slam.host_alloc_like(np.ascontiguousarray(sc.scan(i), dtype=np.float32)) for i in ids]
    deltas = chain_deltas(sc, ids, off={2: (0.45, 4.0)})
    rc, poses, guesses, stats, n_done = slam.register_sequence(scans, sc.guess(0), deltas)
    assert rc == 0 and n_done == len(ids), (rc, n_done, slam.last_error())
    t = slam.timing()
    print("outer iterations", [st.n_iterations for st in stats], "| chained", t.seq_chained, "| chain breaks", t.seq_chain_breaks)
    assert t.seq_chain_breaks >= 1, ([st.n_iterations for st in stats], t.seq_chain_breaks)
    for k in range(len(ids)):
        prc, ppose, pst = plain.register(scans[k], guesses[k])
        assert prc == 0 and np.array_equal(ppose, poses[k]), (k, ppose - poses[k])
        assert_same_bits(pst, stats[k], ("scan", k))
    slam.close(); plain.close()


def test_batch_entry_order(gpu_slam_factory, oracle):
    """three hypotheses of one tiny scan: the BATCH instantiations find their state block through bv.active before they warm it"""
    sc, slam, _ = scene_with_oracle("tiny", oracle, gpu_slam_factory, oracle_too=False, max_iterations=5)
    scan = sc.scan(2)
    poses = np.stack([synth.perturb_pose(sc.gt_pose(2), 9100 + h, 0.05 + 0.2 * h, 0.5 + 2.0 * h) for h in range(3)])
    ok, rcs, out, sts = slam.register_batch(scan, poses)
    assert ok == 3 and (rcs == 0).all(), (ok, rcs)
    for h in range(3):
        rc, ph, sh = slam.register(scan, poses[h])
        assert rc == 0 and np.array_equal(ph, out[h]), (h, ph - out[h])
        assert_same_bits(sts[h], sh, ("batch vs single", h), omit=("uncertainty",))  # (from the call before: the single ones advance it)
    slam.close()
