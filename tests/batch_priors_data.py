"""The batches of tests/test_gpu_batch_priors.py (so_icp_set_batch_priors) and what can be said about them without a device: scenes,
sizes and guesses are those of test_gpu_configs.py::test_batched_hypotheses_equal_single_registrations_bit_for_bit, every hypothesis
gets a prior and a mode, and the hypotheses can be run through the Seam C host loop on the oracle -- the prior in every Sums -- so that
the CPU suite shows that the chosen priors move the results and leave the hypotheses in the rounds for different numbers of them."""
import numpy as np

import pose_prior_ref as ppr
import seam_c_ref
import sequence_priors_data as spd
from superodom_amd import binding, synth

NONE, GIVEN, AT_GUESS = binding.PRIOR_NONE, binding.PRIOR_GIVEN, binding.PRIOR_AT_GUESS
MAX_OUTER, LM_MAX = 5, 4
SCAN_ID = 2
U_KINDS = spd.U_KINDS

# name -> scene, hypotheses, max_surface_features.  tiny: a 16-workgroup grid, query waves for the single registration; five hypotheses
# get workgroups per hypothesis that do not divide the grid, 70 cross the 64-hypothesis group
CASES = {"tiny5": ("tiny", 5, None), "tiny70": ("tiny", 70, None), "small9": ("small", 9, 1500)}


def modes_of(n_hyp):
    return [(GIVEN, NONE, AT_GUESS, AT_GUESS)[h % 4] for h in range(n_hyp)]


def guesses(sc, n_hyp, i=SCAN_ID):
    return np.stack([synth.perturb_pose(sc.gt_pose(i), 7000 + 64 * i + h, 0.02 + 0.5 * (h % 7) / 6.0, 0.2 + 5.0 * (h % 5) / 4.0) for h in range(n_hyp)])


def priors_for(sc, n_hyp, kind, modes=None, i=SCAN_ID):
    """one prior per hypothesis, seeded by the hypothesis (h and 64 + h differ).  A GIVEN hypothesis measures 2 cm / 0.2 degrees from
    the ground truth; the T_meas of the others is not read, and is poisoned to show it."""
    modes = modes_of(n_hyp) if modes is None else modes
    out = []
    for h in range(n_hyp):
        U, floor, fraction = spd.prior_u(kind, 100 + h)
        T_meas = synth.perturb_pose(sc.gt_pose(i), 900 + h, 0.02, 0.2) if modes[h] == GIVEN else np.full(7, np.nan)
        out.append(binding.pose_prior(T_meas, U, floor, fraction))
    return out


def batch_inputs(case, kind):
    """-> (scene, scan, guesses [n_hyp, 7], priors, modes, max_surface_features or None)"""
    scene, n_hyp, sub = CASES[case]
    sc = synth.Scene(scene)
    modes = modes_of(n_hyp)
    return sc, np.ascontiguousarray(sc.scan(SCAN_ID), dtype=np.float32), guesses(sc, n_hyp), priors_for(sc, n_hyp, kind, modes), modes, sub


hypothesis_prior = spd.frame_prior  # P_h of the contract: priors[h], T_meas := poses_in[h] where the mode says so; None without a prior


def oracle_hypotheses(oracle, case, kind, n_first):
    """the first n_first hypotheses of the case through the host loop on the oracle, with their priors and without
    -> [(mode, outer iterations, final pose, outer iterations of the plain registration, its final pose)]"""
    sc, scan, poses, priors, modes, sub = batch_inputs(case, kind)
    om = oracle.OracleMap(plane_res=sc.plane_res)
    om.add_surf(sc.map_points)
    out = []
    for h in range(min(n_first, len(poses))):
        seam = spd.SampledOracleSeam(om, oracle, scan, sc.plane_res, -1 if sub is None else sub)
        plain = seam_c_ref.register_through_seam(seam.match, seam.sums, poses[h], max_outer=MAX_OUTER, lm_max=LM_MAX)
        P = hypothesis_prior(priors, modes, h, poses[h])
        res = plain
        if P is not None:
            seam = spd.SampledOracleSeam(om, oracle, scan, sc.plane_res, -1 if sub is None else sub)
            res = seam_c_ref.register_through_seam(ppr.with_prior(seam.match, P), ppr.with_prior(seam.sums, P), poses[h], max_outer=MAX_OUTER, lm_max=LM_MAX)
        out.append((modes[h], res.n_iterations, np.array(res.iters[-1].pose_after), plain.n_iterations, np.array(plain.iters[-1].pose_after)))
    return out
