"""Seam C (include/so_icp.h: so_icp_match, so_icp_correspondence_sums): the reference's registration loop (LidarSlam.cpp:119-148) run
on the HOST around a match function and a sums function -- what a caller that keeps its own solver writes -- and the oracle-backed
pair of functions that lets the loop itself be checked without a GPU.

    match_fn(pose) -> binding.Sums      one pass of extractFeaturesConstraints at `pose`: the set is formed and summed at `pose`
                                        (hist = reject_hist | obs_hist of that pass)
    sums_fn(pose)  -> binding.Sums      the set the last match formed, summed at `pose`

The solver in between is the library's own host state machine (so_icp_lm_begin / so_icp_lm_feed, lm_solver.h), so the loop differs from
so_icp_register only in where the sums come from."""
from types import SimpleNamespace

import numpy as np

import correspondences_ref as cref
from superodom_amd import binding


# The scans the loop is held on, (scene, scan): the first four seeded scans of both scenes.  A scan whose status bytes differ between the
# host loop and the registration it is compared with sits on a gate edge (two fp64 summations of the normal equations that differ in
# the last bits move the pose of the second match by ~1e-15 m, and a point that close to a gate's threshold changes its verdict): such
# a scan is named in GATE_EDGE and left out -- at most one in eight.  None of these is one.
LOOP_SCANS = [("tiny", 0), ("tiny", 1), ("tiny", 2), ("tiny", 3), ("small", 0), ("small", 1), ("small", 2), ("small", 3)]
GATE_EDGE = []
KEPT_SCANS = [s for s in LOOP_SCANS if s not in GATE_EDGE]
assert len(GATE_EDGE) * 8 <= len(LOOP_SCANS)


def register_through_seam(match_fn, sums_fn, guess, max_outer=4, lm_max=4):
    """LidarSlam.cpp:119-148: per outer iteration match at the current pose, solve (so_icp_lm_begin on the match's sums, one sums_fn per
    candidate -> so_icp_lm_feed until the solver is done), adopt the solver's pose; stop at num_successful_steps == 1 or the last
    iteration.  -> namespace(pose, n_iterations, iters[...], JtJ [6, 6], Jtr [6]) with the oracle's field names (iters[k].num_surf,
    .lm_iterations, .num_successful_steps, .termination, .initial_cost, .final_cost, .reject_hist, .obs_hist, .pose_after), so that
    helpers.assert_follows_oracle takes it on either side."""
    T = np.array(guess, np.float64)
    res = SimpleNamespace(pose=T.copy(), n_iterations=0, iters=[], JtJ=np.zeros((6, 6)), Jtr=np.zeros(6), n_sums_calls=0)
    for it in range(max_outer):
        at_x = match_fn(T)
        drv = binding.LmDriver()
        more, nxt = drv.begin(T, at_x, lm_max)
        while more:
            s = sums_fn(nxt)
            res.n_sums_calls += 1
            accepted_before = drv.result()[1].num_successful_steps
            more, nxt = drv.feed(s)
            if drv.result()[1].num_successful_steps > accepted_before:
                at_x = s  # (the solver adopted the candidate: these are the sums at its pose)
        x, ist = drv.result()
        res.iters.append(SimpleNamespace(num_surf=int(at_x.count), lm_iterations=ist.lm_iterations, num_successful_steps=ist.num_successful_steps,
                                         termination=ist.termination, initial_cost=ist.initial_cost, final_cost=ist.final_cost,
                                         reject_hist=[int(v) for v in at_x.hist[:7]], obs_hist=[int(v) for v in at_x.hist[7:16]],
                                         pose_after=x.copy()))
        res.n_iterations = it + 1
        T = x
        if ist.num_successful_steps == 1 or it == max_outer - 1:  # LidarSlam.cpp:141
            break
    res.pose = T.copy()
    if at_x.count >= 1.0:  # (the normal equations at the returned pose, as so_icp_stats carries them)
        k = 0
        for i in range(6):
            for j in range(i, 6):
                res.JtJ[i, j] = res.JtJ[j, i] = at_x.JtJ[k]; k += 1
        res.Jtr[:] = at_x.Jtr[:]
    return res


def sums_from_fields(p, n, d, coeff, pose, a2, variant, hist):
    """binding.Sums of accepted correspondences (p float or double [N, 3], n, d, coeff) at `pose`: residual and loss in fp64 as
    correspondences_ref states them, the 29 sums in longdouble.  Also returns the sums of the terms' magnitudes for sum_bound:
    (Sums, cost_abs, JtJ_abs [6, 6], Jtr_abs [6])."""
    pose = np.asarray(pose, np.float64)
    if not len(p):
        return binding.LmDriver.sums(0.0, 0.0, np.zeros(6), np.zeros((6, 6)), hist), 0.0, np.zeros((6, 6)), np.zeros(6)
    r = cref.residuals(p, n, d, pose)
    term, w = cref.loss(r, coeff, a2, variant)
    JtJ, Jtr, JtJ_abs, Jtr_abs = cref.normal_equations(p, np.asarray(n, np.longdouble), np.asarray(r, np.longdouble), np.asarray(w, np.longdouble), pose)
    assert JtJ.dtype == np.longdouble and Jtr.dtype == np.longdouble
    cost = float(np.asarray(term, np.longdouble).sum())
    s = binding.LmDriver.sums(cost, float(len(p)), Jtr.astype(np.float64), JtJ.astype(np.float64), hist)
    return s, float(np.abs(term).sum()), JtJ_abs.astype(np.float64), Jtr_abs.astype(np.float64)


def hist_of(corrs):
    """reject_hist[7] | obs_hist[9] of oracle correspondences (so_oracle.c orc_register: every judged point's status; the three labels of
    every accepted one)"""
    h = np.zeros(16, np.int64)
    st = corrs["status"]
    h[:7] = np.bincount(st[st >= 0], minlength=7)[:7]
    acc = corrs["obs"][st == 0][:, :3].ravel()
    h[7:] = np.bincount(acc, minlength=9)[:9]
    return h


class OracleSeam:
    """match_fn / sums_fn on the CPU oracle: orc_plane_match per point (no sub-sampling: max_surface_features = -1), the sums in
    longdouble numpy.  statuses[k]: the status bytes of the k-th match (gate-edge diagnosis)."""

    def __init__(self, om, oracle, scan, plane_res, variant=0):
        self.om, self.oracle, self.scan = om, oracle, np.ascontiguousarray(scan, np.float32)
        self.a2, self.variant = cref.tukey_a2(plane_res), variant
        self.corrs, self.hist, self.statuses = None, None, []

    def match(self, pose):
        self.om.shift(np.asarray(pose, np.float64)[:3])  # LidarSlam.cpp:363
        self.corrs = self.om.plane_match(pose, self.scan, self.oracle.default_config(tukey_variant=self.variant))
        self.hist = hist_of(self.corrs)
        self.statuses.append(self.corrs["status"].astype(np.uint8))
        return self.sums(pose)

    def sums(self, pose):
        c = self.corrs[self.corrs["status"] == 0]
        return sums_from_fields(c["p"], c["n"], c["d"], c["coeff"], pose, self.a2, self.variant, self.hist)[0]


def sums_of_match(st):
    """the so_icp_stats of a so_icp_match as the binding.Sums at its pose: cost, count, JtJ / Jtr and both histograms of iterations[0]"""
    it = st.iterations[0]
    return binding.LmDriver.sums(it.initial_cost, float(it.num_surf_from_scan), list(st.Jtr), np.array(st.JtJ).reshape(6, 6),
                                 list(it.reject_hist) + list(it.obs_hist))


class DeviceSeam:
    """match_fn / sums_fn on a product context (keep_correspondences on): so_icp_match, so_icp_correspondence_sums"""

    def __init__(self, slam, scan):
        self.slam, self.scan, self.statuses = slam, np.ascontiguousarray(scan, np.float32), []

    def match(self, pose):
        rc, st = self.slam.match(self.scan, pose)
        assert rc == 0, rc
        self.statuses.append(self.slam.match_status(len(self.scan)))
        return sums_of_match(st)

    def sums(self, pose):
        return self.slam.correspondence_sums(pose)[0]
