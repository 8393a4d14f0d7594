"""-m gpu: so_icp_register_sequence -- the pose under which the NEXT scan is binned ahead and its map window placed.  The host forms it
while registration k still runs: exact_guess(k) o delta_(k+1), anchored on the last collected result (reg_plan.h: predicted_guess).
Composed from the prediction of k's guess instead it is dead-reckoned through the whole call and gathers every frame's correction.

The run here makes that visible on the smallest scene: every guess lies 0.1 m BELOW its ground truth (no rotation), so every
registration corrects + 0.1 m in z and a dead-reckoned prediction sinks 0.1 m per frame -- z = -24 m at frame 240, within the 1 m
margin of the cube face at -25 m, where cube_stable() refuses the chained start of one frame (the actual guesses never leave
z ~ -0.1 m).  Anchored, the prediction stays 0.1 m off for ever.  Results never depended on the prediction: every frame is the
registration so_icp_register runs from guesses_out[k], bit for bit."""
import numpy as np
import pytest

from helpers import assert_same_bits
from sequence_prediction_data import ROTATION, biased_deltas, biased_guess
from superodom_amd import synth
from test_gpu_sequence import _check_run

pytestmark = pytest.mark.gpu

FRAMES = 300


def _contexts(gpu_slam_factory, sc, n=2):
    mk = dict(plane_res=sc.plane_res, line_res=sc.plane_res / 2, max_surface_features=-1, max_iterations=5)
    out = [gpu_slam_factory(**mk) for _ in range(n)]
    for s in out:
        s.add_surf_point_cloud(sc.map_points)
    return out


@pytest.fixture(scope="module")
def biased_run(soicp, gpu_slam_factory):
    """300 frames of `tiny` in ONE call, scans 0..3 in rotation; computed once, read by (a) and (b)"""
    sc = synth.Scene("tiny")
    slam, plain = _contexts(gpu_slam_factory, sc)
    rot = [slam.host_alloc_like(np.ascontiguousarray(sc.scan(i), dtype=np.float32)) for i in range(ROTATION)]
    scans = [rot[k % ROTATION] for k in range(FRAMES)]
    pose0 = biased_guess(sc, 0); deltas = biased_deltas(sc, FRAMES)
    res = slam.register_sequence(scans, pose0, deltas)
    breaks = slam.timing().seq_chain_breaks
    yield dict(sc=sc, slam=slam, plain=plain, scans=scans, pose0=pose0, deltas=deltas, res=res, breaks=breaks)
    slam.close(); plain.close()


def test_a_constant_bias_does_not_break_the_chain(soicp, biased_run):
    """(a) Unchained frames: frame 0, and one restart per registration that needed more outer iterations than were enqueued ahead
    (seq_chain_breaks) -- nothing else.  With the prediction dead-reckoned, frame 240 is a further one (run once on that build:
    unchained frames [0, 240], no chain break counted, every registration two outer iterations)."""
    rc, poses, guesses, stats, n_done = biased_run["res"]
    assert rc == 0 and n_done == FRAMES, (rc, n_done, biased_run["slam"].last_error())
    unchained = [k for k, st in enumerate(stats) if not st.flags & soicp.FLAG_CHAINED]
    iters = [st.n_iterations for st in stats]
    print("unchained frames", unchained, "| chain breaks", biased_run["breaks"], "| outer iterations min / max", min(iters), max(iters),
          "| guess z min / max %.3f %.3f" % (guesses[:, 2].min(), guesses[:, 2].max()))
    assert unchained[0] == 0
    assert len(unchained) == 1 + biased_run["breaks"], (unchained, biased_run["breaks"])
    assert np.all(np.abs(guesses[:, 2] - np.array([biased_guess(biased_run["sc"], k)[2] for k in range(FRAMES)])) < 0.05)  # (the actual guesses stay where the deltas put them)


def test_every_frame_is_the_single_registration_from_its_guess(biased_run):
    """(b) pose and statistics of so_icp_register from guesses_out[k], and guesses_out[k] == pose_compose(pose_after of k - 1, delta_k),
    bit for bit -- at frames 0, 1, 2, 120, 238 - 242 and 299, and at every frame between them: the plain context registers the frames in
    the run's order, so that what a context carries over from the call before (uncertainty, startup_count) is compared as well."""
    r = biased_run
    _check_run(r["slam"], r["plain"], r["scans"], r["pose0"], r["deltas"], r["res"])


@pytest.mark.parametrize("scene", ["tiny", "small"])
def test_the_announced_scan_under_the_anchored_prediction(soicp, gpu_slam_factory, scene):
    """(c) 12 frames in two calls of 6, the scan that starts the second call announced before the first: staged beside the first call's
    last registration under exact_guess(5) o delta_6.  All 12 frames equal the one-call run bit for bit.  A scan of `tiny` (4 096 points)
    is swept by query waves and has no work list, so it arrives staged but cannot carry FLAG_BINNED_AHEAD; `small`, the scene of
    test_a_run_worked_off_in_two_calls_with_the_next_scan_announced, is binned ahead and carries it."""
    sc = synth.Scene(scene)
    slam, plain = _contexts(gpu_slam_factory, sc)
    rot = [slam.host_alloc_like(np.ascontiguousarray(sc.scan(i), dtype=np.float32)) for i in range(ROTATION)]
    scans = [rot[k % ROTATION] for k in range(12)]
    pose0 = biased_guess(sc, 0); deltas = biased_deltas(sc, 12)
    whole = plain.register_sequence(scans, pose0, deltas)
    assert whole[0] == 0 and whole[4] == 12
    slam.sequence_announce_next(scans[6], deltas[6])
    a = slam.register_sequence(scans[:6], pose0, deltas[:6])
    assert a[0] == 0 and a[4] == 6 and np.array_equal(a[1], whole[1][:6]) and np.array_equal(a[2], whole[2][:6])
    last = a[3][5].iterations[a[3][5].n_iterations - 1]
    g6 = synth.pose_compose(np.array(last.pose_after), deltas[6])
    d2 = deltas[6:].copy(); d2[0] = [0, 0, 0, 0, 0, 0, 1]
    b = slam.register_sequence(scans[6:], g6, d2)
    assert b[0] == 0 and b[4] == 6 and np.array_equal(b[1], whole[1][6:]) and np.array_equal(b[2], whole[2][6:])
    for k, (x, y) in enumerate(zip(list(a[3]) + list(b[3]), whole[3])):
        assert_same_bits(x, y, ("two calls", scene, k))
    f0 = b[3][0].flags
    print(scene, "frame 0 of the second call: flags", hex(f0))
    assert f0 & soicp.FLAG_STAGED_SCAN
    assert bool(f0 & soicp.FLAG_BINNED_AHEAD) == (not f0 & soicp.FLAG_QUERY_WAVES), hex(f0)
    if scene == "small":
        assert f0 & soicp.FLAG_BINNED_AHEAD
    slam.close(); plain.close()
