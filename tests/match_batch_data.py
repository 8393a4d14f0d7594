"""The inputs of tests/test_gpu_match_batch.py (so_icp_match_batch) and what can be said about them without a device.  Scenes, sizes and
guesses are those of tests/batch_priors_data.py; tiny5 and small9 get three more poses behind the guesses:

    REPEAT  pose 0 once more (two hypotheses of one launch on the same pose: their slices, records and counters are their own)
    LOST    the ground truth of the scan with z + 10 m: every point is judged and none accepted
    SHIFTED the ground truth with x + 5 m: a fraction of the points accepted

The CPU suite (tests/test_match_batch_host.py) holds on the oracle that these poses are what they are named and that all poses of a
case lie in one map block, which is what so_icp_match_batch's bit-for-bit statement needs."""
import numpy as np

import batch_correspondences_data as bcd
import batch_priors_data as bpd
import sequence_priors_data as spd
from superodom_amd import synth

CASES = bpd.CASES          # "tiny5", "tiny70" (crosses the group of 64), "small9" (sub-sampled to 1500: status 254)
WITH_EXTRAS = ("tiny5", "small9")
SCAN_ID = bpd.SCAN_ID
SIZES = bcd.SIZES
REPEAT, LOST, SHIFTED = -3, -2, -1   # where the extras stand in a case that has them
# accepted points at full sampling (max_surface_features = -1) on the oracle: the five guesses of tiny5, then SHIFTED on tiny
TINY5_ACCEPTED = [3637, 3664, 3617, 3361, 3267]
TINY_SHIFTED_ACCEPTED = 1586


def extras(sc, pose0, i=SCAN_ID):
    gt = np.asarray(sc.gt_pose(i), np.float64)
    lost, shifted = gt.copy(), gt.copy()
    lost[2] += 10.0
    shifted[0] += 5.0
    return np.stack([np.asarray(pose0, np.float64), lost, shifted])


def inputs(case):
    """-> (scene, scan, poses [n_poses, 7], max_surface_features or None)"""
    scene, n_hyp, sub = CASES[case]
    sc = synth.Scene(scene)
    poses = bpd.guesses(sc, n_hyp)
    if case in WITH_EXTRAS:
        poses = np.concatenate([poses, extras(sc, poses[0])])
    return sc, np.ascontiguousarray(sc.scan(SCAN_ID), dtype=np.float32), np.ascontiguousarray(poses), sub


def three_poses(sc):
    """a guess, the repeat of it and the lost pose: the poses of the size tests"""
    g = bpd.guesses(sc, 1)
    return np.ascontiguousarray(np.concatenate([g, extras(sc, g[0])[:2]]))


def oracle_matches(oracle, case, max_feat=-1):
    """every pose of the case matched on the oracle -> [(pos_in_localmap, accepted, status bytes (255: not sampled), Sums or None)]
    max_feat < 0: full sampling, through SampledOracleSeam.match (orc_plane_match judges every point it is given).  max_feat >= 0: the
    sampling rule is orc_register's, so the match is the first half of a registration of ONE outer iteration -- its correspondences
    are those formed at the guess, whatever its solve does afterwards."""
    sc, scan, poses, sub = inputs(case)
    om = oracle.OracleMap(plane_res=sc.plane_res)
    om.add_surf(sc.map_points)
    out = []
    for pose in poses:
        if max_feat < 0:
            pos = list(om.shift(np.asarray(pose, np.float64)[:3]))
            seam = spd.SampledOracleSeam(om, oracle, scan, sc.plane_res, -1)
            s = seam.match(pose)
            out.append((pos, int(s.count), seam.statuses[-1].copy(), s))
        else:
            rc, _, st, corrs = om.register(scan, pose, oracle.default_config(max_iterations=1, max_surface_features=max_feat), want_corrs=True)
            assert rc == 0
            status = corrs["status"].astype(np.uint8)
            out.append((list(st.pos_in_map), int((status == 0).sum()), status, None))
    return out
