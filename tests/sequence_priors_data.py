"""The runs of tests/test_gpu_sequence_priors.py (so_icp_set_sequence_priors) and what can be said about them without a device: scenes
and sizes are those of tests/test_gpu_sequence.py, every frame gets a prior and a mode, and the host schedule of
so_icp_register_sequence's chained path (superodom_amd/csrc/sequence.cpp) is restated on outer-iteration counts, so that the CPU suite
can show -- with the Seam C host loop on the oracle, the prior in every Sums -- that the chosen priors make the runs take the paths the
GPU tests need: chained frames that measure at their guess, a chain that breaks."""
import numpy as np

import pose_prior_ref as ppr
import seam_c_ref
from helpers import chain_deltas
from superodom_amd import binding, synth

NONE, GIVEN, AT_GUESS = binding.PRIOR_NONE, binding.PRIOR_GIVEN, binding.PRIOR_AT_GUESS
MAX_OUTER, LM_MAX = 5, 4
SEQ_DEPTH_0 = 2  # so_icp_ctx::seq_depth of a fresh context (ctx.h): outer iterations the first registration gets enqueued ahead

# name -> scene, max_surface_features, scan ids, chain_deltas' off=, the modes' rule
RUNS = {
    "small_chunked": dict(scene="small", max_feat=-1, ids=[0, 1, 2, 3, 4, 5, 6], off=None, modes="cycle"),      # swept in chunks, binned ahead
    "small_sampled": dict(scene="small", max_feat=3000, ids=[2, 3, 4, 5], off=None, modes="cycle"),            # query waves
    "tiny": dict(scene="tiny", max_feat=-1, ids=[0, 1, 2, 3, 4, 5], off=None, modes="cycle"),                   # query waves
    # test_a_registration_that_needs_more_iterations_breaks_the_chain_not_the_results' run, a prior at the guess on every frame
    "broken": dict(scene="small", max_feat=-1, ids=[0, 1, 2, 3, 4, 5, 6, 7], off={3: (0.45, 4.0), 6: (0.45, 4.0)}, modes="at_guess"),
}
U_KINDS = ("dense", "zero_row")


def modes_of(run):
    n = len(RUNS[run]["ids"])
    if RUNS[run]["modes"] == "at_guess":
        return [AT_GUESS] * n
    return [(GIVEN, NONE, AT_GUESS, AT_GUESS)[k % 4] for k in range(n)]


def prior_u(kind, seed):
    """-> (U [6, 6], count_floor, count_fraction): a dense upper triangle, U as given; the reference's diagonal form -- its last row
    zero (LidarSlam.cpp:294), rows scaled by the feature count"""
    if kind == "dense":
        return np.triu(np.random.default_rng(seed).standard_normal((6, 6)) * 4.0), None, None
    assert kind == "zero_row"
    v = np.sqrt(0.9)
    return np.diag([v, v, v, v, v, 0.0]), ppr.REFERENCE_FLOOR, ppr.REFERENCE_FRACTION


def run_inputs(run, kind):
    """-> (scene, scans, pose0, deltas, priors, modes).  A GIVEN frame measures 2 cm / 0.2 degrees from the ground truth; the T_meas of
    the other frames is not read, and is poisoned to show it."""
    r = RUNS[run]
    sc = synth.Scene(r["scene"])
    ids = r["ids"]
    scans = [np.ascontiguousarray(sc.scan(i), dtype=np.float32) for i in ids]
    modes = modes_of(run)
    priors = []
    for k, i in enumerate(ids):
        U, floor, fraction = prior_u(kind, 100 + i)
        T_meas = synth.perturb_pose(sc.gt_pose(i), 900 + i, 0.02, 0.2) if modes[k] == GIVEN else np.full(7, np.nan)
        priors.append(binding.pose_prior(T_meas, U, floor, fraction))
    return sc, scans, sc.guess(ids[0]), chain_deltas(sc, ids, off=r["off"]), priors, modes


def frame_prior(priors, modes, k, guess):
    """P_k of the contract: priors[k], T_meas := the frame's guess where the mode says so; None for a frame without a prior"""
    if modes[k] == NONE:
        return None
    p = priors[k]
    T_meas = guess if modes[k] == AT_GUESS else p.T_meas[:]
    return binding.pose_prior(T_meas, np.array(p.sqrt_information[:]).reshape(6, 6), p.count_floor[:], p.count_fraction[:])


class SampledOracleSeam(seam_c_ref.OracleSeam):
    """seam_c_ref.OracleSeam with the sampling rule of max_surface_features in the match"""

    def __init__(self, om, oracle, scan, plane_res, max_feat):
        super().__init__(om, oracle, scan, plane_res)
        self.max_feat = max_feat

    def match(self, pose):
        self.om.shift(np.asarray(pose, np.float64)[:3])
        self.corrs = self.om.plane_match(pose, self.scan, self.oracle.default_config(tukey_variant=self.variant, max_surface_features=self.max_feat))
        self.hist = seam_c_ref.hist_of(self.corrs)
        self.statuses.append(self.corrs["status"].astype(np.uint8))
        return self.sums(pose)


def oracle_iterations(oracle, run, kind):
    """the run through the host loop on the oracle, guesses chained as so_icp_register_sequence chains them -> outer iterations per frame"""
    sc, scans, pose0, deltas, priors, modes = run_inputs(run, kind)
    om = oracle.OracleMap(plane_res=sc.plane_res)
    om.add_surf(sc.map_points)
    guess, iters = np.asarray(pose0, float), []
    for k, scan in enumerate(scans):
        seam = SampledOracleSeam(om, oracle, scan, sc.plane_res, RUNS[run]["max_feat"])
        P = frame_prior(priors, modes, k, guess)
        match, sums = (seam.match, seam.sums) if P is None else (ppr.with_prior(seam.match, P), ppr.with_prior(seam.sums, P))
        res = seam_c_ref.register_through_seam(match, sums, guess, max_outer=MAX_OUTER, lm_max=LM_MAX)
        iters.append(res.n_iterations)
        if k + 1 < len(scans):
            guess = synth.pose_compose(res.iters[-1].pose_after, deltas[k + 1])
    return iters


def schedule(iters, depth=SEQ_DEPTH_0, max_outer=MAX_OUTER):
    """SequenceCall::run_chained on outer-iteration counts, every frame startable: frame k gets min(depth, max_outer) iterations
    enqueued, depth being what the last COLLECTED frame needed; frame k + 1 is enqueued behind them, chained, before k is collected; a
    frame that needs more than it got breaks the chain, and the frame behind it starts again, unchained, once it is collected.
    -> (chained flag per frame, chain breaks)"""
    n = len(iters)
    chained, breaks = [False] * n, 0
    enq = [0] * n
    enq[0] = max(1, min(depth, max_outer))
    for k in range(n):
        if k + 1 < n:
            chained[k + 1] = True
            enq[k + 1] = max(1, min(depth, max_outer))
        if iters[k] > enq[k] and k + 1 < n:
            chained[k + 1] = False
            breaks += 1
        depth = max(1, iters[k])
        if k + 1 < n and not chained[k + 1]:
            enq[k + 1] = max(1, min(depth, max_outer))
    return chained, breaks
