"""The absolute pose prior (include/so_icp.h: so_icp_pose_prior, so_icp_pose_prior_sums; superodom_amd/csrc/pose_prior.h) restated in
numpy.longdouble, with the sum of the magnitudes of every output's terms beside it (the yardstick of a rounding bound).

    e[0..2] = t - t_m,  qe = conj(q_m) (x) q,  e[3..5] = 2 vec(qe)
    B = blockdiag(I3, w' I3 + [v']x),  (v', w') = qe negated when qe.w < 0
    d_i = sqrt(max(count_floor[i], trunc(count * count_fraction[i]))) where count_floor[i] > 0, else 1
    r = D U e,  J = D U B,  cost = r'r / 2,  Jtr = J'r,  JtJ = J'J

Also the pieces the tests build priors and poses from."""
from types import SimpleNamespace

import numpy as np

from superodom_amd import binding

LD = np.longdouble
EPS = 2.0 ** -53


def quat_mul(a, b):
    """Hamilton product, x y z w (so_math.h quat_mul) in the operands' dtype -> (product, sum of the magnitudes of each component's terms)"""
    ax, ay, az, aw = a; bx, by, bz, bw = b
    rows = [(aw * bx, ax * bw, ay * bz, -az * by), (aw * by, ay * bw, az * bx, -ax * bz), (aw * bz, az * bw, ax * by, -ay * bx),
            (aw * bw, -ax * bx, -ay * by, -az * bz)]
    return np.array([sum(r) for r in rows], dtype=LD), np.array([sum(abs(t) for t in r) for r in rows], dtype=LD)


def skew(v):
    return np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]], dtype=LD)


def row_scale(count, floor, fraction):
    """d[6] in longdouble; the products count * fraction are formed in fp64, as std::max(50, int(good_feature_num * 0.1)) forms them"""
    d = np.ones(6, LD)
    for i in range(6):
        if floor[i] > 0:
            d[i] = np.sqrt(LD(max(float(floor[i]), float(np.trunc(np.float64(count) * np.float64(fraction[i]))))))
    return d


def residual_and_jacobian(prior, pose, count):
    """prior: binding.PosePrior.  -> namespace(e, B, d, r, J and e_abs, B_abs, r_abs, J_abs: the same with every term by its magnitude)"""
    Tm = np.array(prior.T_meas[:], LD); U = np.array(prior.sqrt_information[:], LD).reshape(6, 6)
    pose = np.array(pose, LD)
    qc = np.array([-Tm[3], -Tm[4], -Tm[5], Tm[6]], LD)
    qe, qe_abs = quat_mul(qc, pose[3:])
    e = np.concatenate([pose[:3] - Tm[:3], 2 * qe[:3]])
    e_abs = np.concatenate([np.abs(pose[:3]) + np.abs(Tm[:3]), 2 * qe_abs[:3]])
    m, m_abs = (-qe, qe_abs) if qe[3] < 0 else (qe, qe_abs)
    B = np.zeros((6, 6), LD); B[:3, :3] = np.eye(3); B[3:, 3:] = m[3] * np.eye(3, dtype=LD) + skew(m[:3])
    B_abs = np.zeros((6, 6), LD); B_abs[:3, :3] = np.eye(3); B_abs[3:, 3:] = m_abs[3] * np.eye(3, dtype=LD) + np.abs(skew(m_abs[:3]))
    d = row_scale(count, prior.count_floor[:], prior.count_fraction[:])
    D = np.diag(d)
    return SimpleNamespace(e=e, B=B, d=d, r=D @ U @ e, J=D @ U @ B, e_abs=e_abs, B_abs=B_abs, r_abs=D @ np.abs(U) @ e_abs, J_abs=D @ np.abs(U) @ B_abs)


def contribution(prior, pose, count):
    """-> namespace(cost, Jtr [6], JtJ [6, 6] in longdouble; cost_abs, Jtr_abs, JtJ_abs: the sums of the magnitudes of their terms)"""
    f = residual_and_jacobian(prior, pose, count)
    return SimpleNamespace(cost=f.r @ f.r / 2, Jtr=f.J.T @ f.r, JtJ=f.J.T @ f.J,
                           cost_abs=f.r_abs @ f.r_abs / 2, Jtr_abs=f.J_abs.T @ f.r_abs, JtJ_abs=f.J_abs.T @ f.J_abs, parts=f)


def words(c):
    """the 28 words a contribution adds, in so_icp_sums order without count: cost, Jtr[6], JtJ upper triangle -> (values, magnitudes)"""
    iu = np.triu_indices(6)
    return (np.concatenate([[c.cost], c.Jtr, c.JtJ[iu]]), np.concatenate([[c.cost_abs], c.Jtr_abs, c.JtJ_abs[iu]]))


def sums_words(s):
    """the same 28 words of a binding.Sums, fp64"""
    return np.concatenate([[s.cost], s.Jtr[:], s.JtJ[:]])


def empty_sums(count=0.0, hist=None):
    return binding.LmDriver.sums(0.0, float(count), np.zeros(6), np.zeros((6, 6)), hist)


def host_prior_sums(prior, pose, count):
    """so_icp_pose_prior_sums on sums that hold nothing but `count`: the contribution itself (0 + v = v)"""
    return binding.pose_prior_sums(prior, pose, empty_sums(count))


def with_prior(seam_fn, prior):
    """a seam_c_ref match / sums function whose Sums carry the prior at the pose they were formed at"""
    return lambda pose: binding.pose_prior_sums(prior, pose, seam_fn(pose))


def quat_from_rotvec(rv):
    rv = np.asarray(rv, float)
    a = np.linalg.norm(rv)
    if a == 0:
        return np.array([0, 0, 0, 1.0])
    return np.concatenate([np.sin(a / 2) * rv / a, [np.cos(a / 2)]])


def pose_of(t, rv):
    return np.concatenate([np.asarray(t, float), quat_from_rotvec(rv)])


def plus(pose, delta):
    """PoseLocalParameterization::Plus: p += dp, q = normalize(q (x) [dtheta / 2, 1]) in fp64"""
    pose, delta = np.asarray(pose, float), np.asarray(delta, float)
    q, _ = quat_mul(np.array(pose[3:], LD), np.array([delta[3] / 2, delta[4] / 2, delta[5] / 2, 1.0], LD))
    q = np.array(q, float)
    return np.concatenate([pose[:3] + delta[:3], q / np.linalg.norm(q)])


# the reference's prior (LidarSlam.cpp:285-297): U = diag(sqrt((1 - uncertainty_xyz) V), sqrt(V), sqrt(V), 0) and the count scaling
REFERENCE_FLOOR = [50, 50, 50, 10, 10, 5]
REFERENCE_FRACTION = [0.1, 0.1, 0.1, 0.01, 0.01, 0.001]


def reference_prior(T_meas, uncertainty_xyz, visual_confidence):
    V = float(visual_confidence)
    diag = [np.sqrt((1 - uncertainty_xyz[0]) * V), np.sqrt((1 - uncertainty_xyz[1]) * V), np.sqrt((1 - uncertainty_xyz[2]) * V), np.sqrt(V), np.sqrt(V), 0.0]
    return binding.pose_prior(T_meas, np.diag(diag), REFERENCE_FLOOR, REFERENCE_FRACTION)
