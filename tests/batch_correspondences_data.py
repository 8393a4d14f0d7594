"""The batches of tests/test_gpu_batch_correspondences.py (so_icp_keep_batch_correspondences, so_icp_batch_correspondences,
so_icp_batch_correspondence_sums) and what can be said about them without a device: scenes, sizes and guesses are those of
tests/batch_priors_data.py (no priors unless a test asks for them), and the hypotheses can be run through the Seam C host loop on the
oracle, so that the CPU suite shows that the chosen guesses give the export something to tell apart: every hypothesis accepts points,
the hypotheses end in different outer iterations, and at least two of them accept different points."""
import numpy as np

import batch_priors_data as bpd
import seam_c_ref
import sequence_priors_data as spd
from superodom_amd import synth

MAX_OUTER, LM_MAX, SCAN_ID = bpd.MAX_OUTER, bpd.LM_MAX, bpd.SCAN_ID
CASES = bpd.CASES          # "tiny5", "tiny70" (crosses the group of 64), "small9" (sub-sampled to 1500: status 254)
ADEQUACY_CASES = ("tiny5", "small9")
TILE = 1024                # corr_kernels.h kCorrTile
SIZES = [0, 1, 63, 64, 65, 255, 256, 257, TILE - 1, TILE, TILE + 1, 4096]
SUMS_SIZES = [1, 255, TILE, TILE + 1, 4096]
SUMS_POSES = [1, 2, 64]


def batch_inputs(case):
    """-> (scene, scan, guesses [n_hyp, 7], max_surface_features or None)"""
    scene, n_hyp, sub = CASES[case]
    sc = synth.Scene(scene)
    return sc, np.ascontiguousarray(sc.scan(SCAN_ID), dtype=np.float32), bpd.guesses(sc, n_hyp), sub


def poses_near(pose, n_poses, seed):
    """n_poses evaluation poses within 5 cm / 0.5 degrees of `pose`, the first one `pose` itself"""
    return np.stack([np.asarray(pose, np.float64)] + [synth.perturb_pose(pose, seed + j, 0.05, 0.5) for j in range(1, n_poses)])


def oracle_sets(oracle, case):
    """every hypothesis of the case through the host loop on the oracle -> [(outer iterations, positions of the accepted points of its
    last match)]"""
    sc, scan, poses, sub = batch_inputs(case)
    om = oracle.OracleMap(plane_res=sc.plane_res)
    om.add_surf(sc.map_points)
    out = []
    for h in range(len(poses)):
        seam = spd.SampledOracleSeam(om, oracle, scan, sc.plane_res, -1 if sub is None else sub)
        res = seam_c_ref.register_through_seam(seam.match, seam.sums, poses[h], max_outer=MAX_OUTER, lm_max=LM_MAX)
        out.append((res.n_iterations, np.flatnonzero(seam.statuses[-1] == 0)))
    return out
