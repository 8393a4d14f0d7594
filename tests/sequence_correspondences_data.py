"""The runs of tests/test_gpu_sequence_correspondences.py (so_icp_keep_sequence_correspondences, so_icp_sequence_correspondences,
so_icp_sequence_correspondence_sums) and what can be said about them without a device.  The runs are those of
tests/sequence_priors_data.py: `small_chunked`, `small_sampled` and `tiny` without priors, `broken` with a prior at every guess (the
run that file shows to break its chain), and `sizes` and `sizes_chained`, whose frames are prefixes of the tiny scene's scans.  The frames can be run
through the Seam C host loop on the oracle, chained as so_icp_register_sequence chains them, so that the CPU suite shows that the
frames of a run accept different point sets and end in different outer iterations, that the chunked run has chained frames and that
the broken run breaks its chain."""
import numpy as np

import pose_prior_ref as ppr
import seam_c_ref
import sequence_priors_data as spd
from helpers import chain_deltas
from superodom_amd import synth

MAX_OUTER, LM_MAX = spd.MAX_OUTER, spd.LM_MAX
TILE = 1024  # corr_kernels.h kCorrTile
PLAIN_RUNS = ("small_chunked", "small_sampled", "tiny")
PRIOR_KIND = "dense"
# points per frame of the run `sizes`: around wavefront, workgroup and tile; an empty frame (it takes the per-frame entry) between
# frames of three and of two tiles, so that a selection in run order has a zero-tile entry in its middle
SIZES = [2049, 0, 1025, 1, 63, 64, 65, 255, 256, 257, TILE - 1, TILE]
SIZES_IDS = [0, 1, 2, 3, 4, 5, 0, 1, 2, 3, 4, 5]
# `sizes` runs with SOICP_SEQ_CHAIN=0, one registration after the other: on the chained path a run that holds frames of a handful of
# points ends with "registration state was not published by the device" -- with the switch off as well, so before this feature (seen
# on an MI355X for five orders of SIZES, at another frame each time).  `sizes_chained`: unequal frames that the chained path does run --
# every frame starts a scan or more away from its prediction, so the chain also breaks
SIZES_CHAINED = [2049, 1025, 64, 65, 255]
SIZES_CHAINED_IDS = [0, 3, 5, 0, 1]
SUMS_FRAMES = [SIZES.index(n) for n in (1, 255, TILE, TILE + 1, 2049)]  # five sizes around wavefront, workgroup and tile
SUMS_POSES = [1, 2, 64]
# name -> scene, max_surface_features, scan ids: sequence_priors_data's runs without their priors; `small_sampled` starts two scans
# earlier than there, at the frame whose neighbour needs a third outer iteration (the CPU suite holds every run to that)
RUNS = {
    "small_chunked": dict(scene="small", max_feat=-1, ids=[0, 1, 2, 3, 4, 5, 6]),   # swept in chunks, binned ahead
    "small_sampled": dict(scene="small", max_feat=3000, ids=[0, 1, 2, 3, 4]),      # query waves
    "tiny": dict(scene="tiny", max_feat=-1, ids=[0, 1, 2, 3, 4, 5]),               # query waves
    "broken": dict(scene="small", max_feat=-1, ids=spd.RUNS["broken"]["ids"]),     # a prior at every guess, a chain that breaks
    "sizes": dict(scene="tiny", max_feat=-1, ids=SIZES_IDS),
    "sizes_chained": dict(scene="tiny", max_feat=-1, ids=SIZES_CHAINED_IDS),
}
RUN_SCENE = {r: RUNS[r]["scene"] for r in RUNS}
RUN_MAX_FEAT = {r: RUNS[r]["max_feat"] for r in RUNS}


def run_inputs(run):
    """-> (scene, scans, pose0, deltas, priors or None, modes or None)"""
    if run == "broken":
        return spd.run_inputs(run, PRIOR_KIND)
    sc, ids = synth.Scene(RUNS[run]["scene"]), RUNS[run]["ids"]
    sizes = dict(sizes=SIZES, sizes_chained=SIZES_CHAINED).get(run, [None] * len(ids))
    scans = [np.ascontiguousarray(sc.scan(i)[:n], dtype=np.float32) for i, n in zip(ids, sizes)]
    # (sizes_chained: the predictions of scans 0, 3, 5, 6, 7 of a walk through the scene's six scans, applied to these five)
    deltas = chain_deltas(sc, SIZES_IDS)[[0, 3, 5, 6, 7]] if run == "sizes_chained" else chain_deltas(sc, ids)
    return sc, scans, sc.guess(ids[0]), deltas, None, None


def poses_near(pose, n_poses, seed):
    """n_poses evaluation poses within 5 cm / 0.5 degrees of `pose`, the first one `pose` itself"""
    return np.stack([np.asarray(pose, np.float64)] + [synth.perturb_pose(pose, seed + j, 0.05, 0.5) for j in range(1, n_poses)])


def tile_first(ns):
    """the prefix table of the entries' tile counts (reg_plan.h: selection_tile_table)"""
    return np.concatenate([[0], np.cumsum([(n + TILE - 1) // TILE for n in ns])]).astype(np.uint32)


def ticket_ref(t, first):
    """(entry, tile) of ticket t by a plain scan of the table: the entry whose range of tickets holds t"""
    for e in range(len(first) - 1):
        if first[e] <= t < first[e + 1]:
            return e, t - int(first[e])
    raise AssertionError((t, list(first)))


def oracle_frames(oracle, run):
    """the run through the host loop on the oracle, guesses chained as so_icp_register_sequence chains them (as
    sequence_priors_data.oracle_iterations runs it, here with the accepted sets) -> [(outer iterations, positions of the accepted points
    of the frame's last match)]"""
    sc, scans, pose0, deltas, priors, modes = run_inputs(run)
    om = oracle.OracleMap(plane_res=sc.plane_res)
    om.add_surf(sc.map_points)
    guess, out = np.asarray(pose0, float), []
    for k, scan in enumerate(scans):
        seam = spd.SampledOracleSeam(om, oracle, scan, sc.plane_res, RUN_MAX_FEAT[run])
        P = spd.frame_prior(priors, modes, k, guess) if priors is not None else None
        match, sums = (seam.match, seam.sums) if P is None else (ppr.with_prior(seam.match, P), ppr.with_prior(seam.sums, P))
        res = seam_c_ref.register_through_seam(match, sums, guess, max_outer=MAX_OUTER, lm_max=LM_MAX)
        out.append((res.n_iterations, np.flatnonzero(seam.statuses[-1] == 0)))
        if k + 1 < len(scans):
            guess = synth.pose_compose(res.iters[-1].pose_after, deltas[k + 1])
    return out
