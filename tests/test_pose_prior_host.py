"""CPU: the absolute pose prior (so_icp_pose_prior_from_information, so_icp_pose_prior_sums, so_icp_set_pose_prior) -- what can be held
without a device: the arithmetic of superodom_amd/csrc/pose_prior.h against tests/pose_prior_ref.py, its Jacobian against central
differences, the LLT, the Seam C host loop on the oracle with the prior in every Sums, and the ABI.  tests/test_gpu_pose_prior.py then
holds the device solve to this arithmetic."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import pose_prior_ref as ppr
import seam_c_ref
from helpers import DEGENERATE_OBSERVABLE, DegenerateScene, pose_delta6
from superodom_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNTS = [0, 499, 500, 501, 4999, 5000, 10 ** 5]  # fraction 0.1 crosses floor 50 at 500, 0.01 crosses 10 at 1 000 .. (far sides too)


def dense_upper(rng, scale=3.0):
    return np.triu(rng.standard_normal((6, 6)) * scale)


def prior_cases(soicp):
    """(tag, PosePrior, pose) -- every case the arithmetic branches on"""
    rng = np.random.default_rng(20260)
    Tm = ppr.pose_of([1.5, -2.25, 0.75], [0.1, -0.2, 0.3])
    near = ppr.plus(Tm, [0.05, -0.02, 0.03, 0.01, -0.02, 0.015])
    far = np.concatenate([Tm[:3] + [0.2, 0.1, -0.3], np.array(ppr.quat_mul(np.array(Tm[3:], ppr.LD), np.array(ppr.quat_from_rotvec(np.deg2rad(170.0) * np.array([0.6, 0.0, 0.8])), ppr.LD))[0], float)])
    far[3:] /= -np.linalg.norm(far[3:])  # the same rotation, 170 degrees from q_m, by the quaternion whose product with conj(q_m) has w = -cos(85 deg)
    Tm_neg = Tm.copy(); Tm_neg[3:] = -Tm_neg[3:]
    ident = np.array([0, 0, 0, 0, 0, 0, 1.0])
    U_dense = dense_upper(rng)
    U_zero_row = np.diag([2.0, 3.0, 0.5, 1.5, 0.0, 4.0])
    cases = [("dense U, near", soicp.pose_prior(Tm, U_dense), near),
             ("dense U, 170 degrees apart (qe.w < 0)", soicp.pose_prior(Tm, U_dense), far),
             ("dense U, -q_m", soicp.pose_prior(Tm_neg, U_dense), near),
             ("identity pose on identity measurement", soicp.pose_prior(ident, U_dense), ident),
             ("diagonal U with a zero row", soicp.pose_prior(Tm, U_zero_row), near),
             ("U = 0", soicp.pose_prior(Tm, np.zeros((6, 6))), near),
             ("reference form", ppr.reference_prior(Tm, [0.25, 0.5, 1.0], 0.8), near),
             ("dense U with count scaling", soicp.pose_prior(Tm, U_dense, ppr.REFERENCE_FLOOR, ppr.REFERENCE_FRACTION), far)]
    for k in range(4):  # seeded
        T = ppr.pose_of(rng.standard_normal(3) * 5, rng.standard_normal(3))
        cases.append((f"seeded {k}", soicp.pose_prior(T, dense_upper(rng), ppr.REFERENCE_FLOOR if k % 2 else None, ppr.REFERENCE_FRACTION if k % 2 else None),
                      ppr.pose_of(T[:3] + rng.standard_normal(3), rng.standard_normal(3))))
    return cases


def test_the_170_degree_case_takes_the_negated_branch(soicp):
    tags = {t: (p, x) for t, p, x in prior_cases(soicp)}
    for tag, neg in (("dense U, 170 degrees apart (qe.w < 0)", True), ("dense U, -q_m", True), ("dense U, near", False)):
        p, x = tags[tag]
        qe, _ = ppr.quat_mul(np.array([-p.T_meas[3], -p.T_meas[4], -p.T_meas[5], p.T_meas[6]], ppr.LD), np.array(x[3:], ppr.LD))
        assert (qe[3] < 0) == neg, (tag, float(qe[3]))


def test_prior_sums_against_the_restatement(soicp):
    """so_icp_pose_prior_sums on sums that hold only `count` against pose_prior_ref, word by word: |got - want| <= 64 * 2^-53 * sum|terms|
    (the deepest chain -- a JtJ word of a rotation column: 3 products of the rotation block over 4-term quaternion sums, the row scale,
    6 products -- is under twenty roundings).  Then on sums that hold something: the plane sum joins the terms."""
    worst = 0.0
    for tag, prior, pose in prior_cases(soicp):
        for count in COUNTS:
            got = ppr.sums_words(ppr.host_prior_sums(prior, pose, count))
            want, mag = ppr.words(ppr.contribution(prior, pose, count))
            err, bound = np.abs(np.asarray(got, ppr.LD) - want), 64 * ppr.EPS * mag
            assert np.all(err <= bound), (tag, count, np.argmax(err - bound), float(np.max(err)), got, want)
            worst = max(worst, float(np.max(err / np.maximum(bound, ppr.LD(1e-300)))))
    print(f"largest |difference| / bound over {len(prior_cases(soicp))} priors x {len(COUNTS)} counts: {worst:.4f}")
    rng = np.random.default_rng(5)
    tag, prior, pose = prior_cases(soicp)[7]
    A = rng.standard_normal((6, 6)); base = soicp.LmDriver.sums(12.5, 4999.0, rng.standard_normal(6), A @ A.T, list(range(16)))
    before = ppr.sums_words(base)
    after = soicp.pose_prior_sums(prior, pose, base)
    want, mag = ppr.words(ppr.contribution(prior, pose, 4999.0))
    assert np.all(np.abs(np.asarray(ppr.sums_words(after), ppr.LD) - (np.asarray(before, ppr.LD) + want)) <= 64 * ppr.EPS * (mag + np.abs(before)))
    assert after.count == 4999.0 and list(after.hist[:]) == [float(v) for v in range(16)], "count and hist stay"


def test_count_scaling_crosses_where_the_reference_does(soicp):
    """row scale: sqrt(max(50, int(count * 0.1))) and its kin; between 499 and 501 the floor of row 0 gives way, the others hold"""
    Tm = np.array([0, 0, 0, 0, 0, 0, 1.0]); pose = np.array([1.0, 1.0, 1.0, 0, 0, 0, 1.0])
    prior = soicp.pose_prior(Tm, np.eye(6), ppr.REFERENCE_FLOOR, ppr.REFERENCE_FRACTION)
    for count, want in ((0, 50), (499, 50), (500, 50), (501, 50), (509, 50), (510, 51), (4999, 499), (5000, 500), (10 ** 5, 10 ** 4)):
        s = ppr.host_prior_sums(prior, pose, count)
        assert abs(s.JtJ[0] - want) <= 4 * ppr.EPS * want, (count, s.JtJ[0])  # J = D: JtJ[0][0] = d_0^2, a square root squared
    s = ppr.host_prior_sums(prior, pose, 10 ** 5)
    assert abs(s.JtJ[15] - 1000.0) <= 1e-9 and abs(s.JtJ[20] - 100.0) <= 1e-9  # rows 3 and 5: int(1e5 * 0.01), int(1e5 * 0.001)


def library_jacobian(soicp, prior, pose):
    """J out of so_icp_pose_prior_sums: with row k of U alone, cost = r_k^2 / 2 and Jtr = J[k, :] r_k; the sign of r_k is the
    restatement's.  None where a row's residual is zero (nothing to divide by)."""
    U = np.array(prior.sqrt_information[:]).reshape(6, 6)
    J = np.zeros((6, 6))
    for k in range(6):
        if not U[k].any():
            continue
        one = soicp.pose_prior(prior.T_meas[:], np.where(np.arange(6)[:, None] == k, U, 0.0))
        s = ppr.host_prior_sums(one, pose, 0)
        rk = float(ppr.residual_and_jacobian(one, pose, 0).r[k])
        if rk == 0.0:
            return None
        assert abs(rk * rk / 2 - s.cost) <= 1e-12 * s.cost, (k, rk, s.cost)
        J[k] = np.array(s.Jtr[:]) / rk
    return J


def central_difference_jacobian(prior, pose, delta=1e-6):
    J = np.zeros((6, 6))
    for i in range(6):
        d = np.zeros(6); d[i] = delta
        rp = np.array(ppr.residual_and_jacobian(prior, ppr.plus(pose, d), 0).r, float)
        rm = np.array(ppr.residual_and_jacobian(prior, ppr.plus(pose, -d), 0).r, float)
        J[:, i] = (rp - rm) / (2 * delta)
    return J


def test_jacobian_against_central_differences(soicp):
    """through Plus (q (x) [1, dtheta / 2] normalised, delta = 1e-6): |J_fd - J| <= 1e-6 |J| where qe.w > 0.1; on a qe.w < 0 pose J = -J_fd
    in the rotation columns' block -- the sign inconsistency that is restated, not repaired (the residual takes qe as it is, the Jacobian negates
    it) -- while the translation columns, which do not see qe, agree."""
    n_checked = 0
    for tag, prior, pose in prior_cases(soicp):
        if not np.any(np.array(prior.sqrt_information[:])):
            continue
        qe_w = float(ppr.quat_mul(np.array([-prior.T_meas[3], -prior.T_meas[4], -prior.T_meas[5], prior.T_meas[6]], ppr.LD), np.array(pose[3:], ppr.LD))[0][3])
        unscaled = soicp.pose_prior(prior.T_meas[:], np.array(prior.sqrt_information[:]).reshape(6, 6))
        J = library_jacobian(soicp, unscaled, pose)
        if J is None:
            continue
        J_ref = np.array(ppr.residual_and_jacobian(unscaled, pose, 0).J, float)
        assert np.linalg.norm(J - J_ref) <= 1e-9 * np.linalg.norm(J_ref), tag  # the library's J is the restatement's
        J_fd = central_difference_jacobian(unscaled, pose)
        if qe_w > 0.1:
            assert np.linalg.norm(J_fd - J) <= 1e-6 * np.linalg.norm(J), (tag, np.linalg.norm(J_fd - J), np.linalg.norm(J))
            n_checked += 1
        elif qe_w < 0:
            assert np.linalg.norm(J_fd[:, :3] - J[:, :3]) <= 1e-6 * np.linalg.norm(J), tag
            assert np.linalg.norm(J_fd[:, 3:] + J[:, 3:]) <= 1e-6 * np.linalg.norm(J), (tag, "the rotation block is minus the derivative")
            assert np.linalg.norm(J[:, 3:]) > 1e-3 * np.linalg.norm(J)
            n_checked += 100
    assert n_checked % 100 >= 6 and n_checked // 100 >= 2, n_checked


def test_from_information(soicp):
    rng = np.random.default_rng(11)
    Tm = ppr.pose_of([1, 2, 3], [0.3, 0.2, 0.1])
    for k in range(8):
        A = rng.standard_normal((6, 6)); info = A @ A.T + 0.1 * np.eye(6)
        rc, p = soicp.pose_prior_from_information(info, Tm)
        assert rc == 0
        U = np.array(p.sqrt_information[:]).reshape(6, 6); want = np.linalg.cholesky(info).T
        assert np.linalg.norm(U - want) <= 16 * ppr.EPS * np.linalg.norm(want), (k, np.linalg.norm(U - want))
        assert list(p.T_meas[:]) == list(Tm) and not any(p.count_floor[:]) and not any(p.count_fraction[:])
        assert np.allclose(U.T @ U, info, rtol=1e-12, atol=1e-12)
    # the reference's diagonal: information(5,5) = 0 (LidarSlam.cpp:294)
    diag = np.array([37.5, 25.0, 0.0, 8.0, 8.0, 0.0])
    rc, p = soicp.pose_prior_from_information(np.diag(diag), Tm)
    U = np.array(p.sqrt_information[:]).reshape(6, 6)
    assert rc == 0 and np.all(np.isfinite(U)) and not U[5].any() and not U[2].any() and np.array_equal(U, np.diag(np.sqrt(diag)))
    # a singular positive semi-definite matrix whose zero pivot has a zero column below it
    v = np.array([1.0, 2.0, 0, 0, 0, 0]); rc, p = soicp.pose_prior_from_information(np.outer(v, v), Tm)
    assert rc == 0 and np.all(np.isfinite(p.sqrt_information[:]))
    indefinite = np.eye(6); indefinite[1, 1] = -1.0
    assert soicp.pose_prior_from_information(indefinite, Tm)[0] == -1
    indefinite = np.eye(6); indefinite[0, 1] = indefinite[1, 0] = 2.0
    assert soicp.pose_prior_from_information(indefinite, Tm)[0] == -1
    off_zero_pivot = np.zeros((6, 6)); off_zero_pivot[1, 0] = off_zero_pivot[0, 1] = 1.0
    assert soicp.pose_prior_from_information(off_zero_pivot, Tm)[0] == -1
    nan = np.eye(6); nan[3, 3] = np.nan
    assert soicp.pose_prior_from_information(nan, Tm)[0] == -1
    L = soicp.load()
    assert L.so_icp_pose_prior_from_information(None, None, None) == -1


# ---- the host loop on the oracle -----------------------------------------------------------------------------------------------------
_scenes = {}


def scene_and_map(oracle, name):
    if name not in _scenes:
        sc = DegenerateScene(name) if name in DEGENERATE_OBSERVABLE else synth.Scene(name)
        om = oracle.OracleMap(plane_res=sc.plane_res)
        om.add_surf(sc.map_points)
        _scenes[name] = (sc, om)
    return _scenes[name]


def loop(oracle, name, i, prior, max_outer=5):
    sc, om = scene_and_map(oracle, name)
    scan, guess = np.ascontiguousarray(sc.scan(i), np.float32), sc.guess(i)
    seam = seam_c_ref.OracleSeam(om, oracle, scan, sc.plane_res)
    if prior is None:
        return seam_c_ref.register_through_seam(seam.match, seam.sums, guess, max_outer=max_outer, lm_max=4)
    return seam_c_ref.register_through_seam(ppr.with_prior(seam.match, prior), ppr.with_prior(seam.sums, prior), guess, max_outer=max_outer, lm_max=4)


def result_bits(res):
    return (res.n_iterations, res.pose.tobytes(), res.JtJ.tobytes(), res.Jtr.tobytes(),
            tuple((it.lm_iterations, it.num_successful_steps, it.termination, it.num_surf, np.float64(it.initial_cost).tobytes(),
                   np.float64(it.final_cost).tobytes(), it.pose_after.tobytes()) for it in res.iters))


def test_host_loop_with_a_zero_prior_is_the_plain_loop(soicp, oracle):
    sc, _ = scene_and_map(oracle, "tiny")
    zero = soicp.pose_prior(sc.gt_pose(0), np.zeros((6, 6)), ppr.REFERENCE_FLOOR, ppr.REFERENCE_FRACTION)
    assert result_bits(loop(oracle, "tiny", 0, zero)) == result_bits(loop(oracle, "tiny", 0, None))


def test_host_loop_with_a_stiff_translation_prior_ends_on_it(soicp, oracle):
    sc, _ = scene_and_map(oracle, "tiny")
    T_meas = np.array(sc.gt_pose(0)); T_meas[:3] += [0.05, -0.04, 0.03]
    info = np.zeros((6, 6)); info[:3, :3] = 1e12 * np.eye(3)
    rc, prior = soicp.pose_prior_from_information(info, T_meas)
    assert rc == 0
    res = loop(oracle, "tiny", 0, prior)
    print("stiff translation prior: |t - t_meas| =", np.abs(res.pose[:3] - T_meas[:3]))
    assert np.all(np.abs(res.pose[:3] - T_meas[:3]) <= 1e-6), res.pose[:3] - T_meas[:3]


def test_host_loop_on_the_open_corridor_takes_the_free_axis_from_the_prior(soicp, oracle):
    """open_corridor leaves the translation along x to chance (DEGENERATE_OBSERVABLE lacks row 0): without a prior scan 0 ends 5.1 cm from
    the ground truth's x.  Information 1e4 on x alone, measured 4 cm beside the ground truth, puts the result on the prior's x to 1e-3 m.
    The five observable coordinates do NOT stay within assert_follows_oracle's pose_tol (1e-8) of the no-prior run: a pose 5 cm further
    along the corridor matches other map points to the same planes, whose 1 cm noise moves the rest by some 1e-5.  The run of this test
    on the CPU oracle loop, from which the committed bound (helpers.TOL_T = TOL_R = 1e-4, the tolerance of record) was taken:

        open_corridor: x - x_meas = -2.014e-05 m (no prior: -5.112e-02 m); the other five coordinates against the no-prior run:
        [ 1.864e-05  5.956e-05  1.519e-05 -3.021e-06  2.357e-06]"""
    name = "open_corridor"
    sc, _ = scene_and_map(oracle, name)
    free = [a for a in range(6) if a not in DEGENERATE_OBSERVABLE[name]]
    assert free == [0]
    plain = loop(oracle, name, 0, None)
    T_meas = np.array(sc.gt_pose(0)); T_meas[0] += 0.04
    info = np.zeros((6, 6)); info[0, 0] = 1e4
    rc, prior = soicp.pose_prior_from_information(info, T_meas)
    assert rc == 0
    res = loop(oracle, name, 0, prior)
    d = pose_delta6(plain.pose, res.pose)
    print(f"open_corridor: x - x_meas = {res.pose[0] - T_meas[0]:.3e} m (no prior: {plain.pose[0] - T_meas[0]:.3e} m); "
          f"the other five coordinates against the no-prior run: {np.array2string(d[1:], precision=3)}")
    assert abs(res.pose[0] - T_meas[0]) <= 1e-3
    assert np.all(np.abs(d[1:]) <= OPEN_CORRIDOR_OTHER_FIVE), d[1:]


OPEN_CORRIDOR_OTHER_FIVE = 1e-4  # helpers.TOL_T / TOL_R; measured 6.0e-5 at most, see the docstring


# ---- ABI ---------------------------------------------------------------------------------------------------------------------------------
def test_struct_and_symbols(soicp):
    L = soicp.load()
    assert C.sizeof(soicp.PosePrior) == 55 * 8
    for sym in ("so_icp_pose_prior_from_information", "so_icp_pose_prior_sums", "so_icp_set_pose_prior"):
        assert sym in soicp.EXPORTED and getattr(L, sym)
    assert L.so_icp_abi_version() == 4 and soicp.FLAG_POSE_PRIOR == 0x800
    header = open(os.path.join(ROOT, "include", "so_icp.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} so_icp_pose_prior;", header).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [(n, int(k)) for n, k in re.findall(r"(\w+)\[(\d+)\]", body)]
    assert fields == [(n, C.sizeof(t) // 8) for n, t in soicp.PosePrior._fields_], fields
    assert "#define SO_ICP_FLAG_POSE_PRIOR 0x800u" in header


def test_host_only_context_and_bad_arguments(soicp):
    L = soicp.load()
    host = soicp.LidarSlamGpu(device_id=-1, plane_res=0.2)
    prior = soicp.pose_prior([0, 0, 0, 0, 0, 0, 1.0], np.eye(6))
    assert L.so_icp_set_pose_prior(None, C.byref(prior)) == -1
    assert L.so_icp_set_pose_prior(host.h, C.byref(prior)) == -2 and b"no CPU fallback" in L.so_icp_last_error(host.h)
    assert L.so_icp_set_pose_prior(host.h, None) == -2
    with pytest.raises(soicp.SoIcpError, match="no CPU fallback"):
        host.set_pose_prior(prior)
    host.close()
    pose = np.array([0, 0, 0, 0, 0, 0, 1.0]); s = ppr.empty_sums()
    f64p = C.POINTER(C.c_double)
    assert L.so_icp_pose_prior_sums(None, pose.ctypes.data_as(f64p), C.byref(s)) == -1
    assert L.so_icp_pose_prior_sums(C.byref(prior), None, C.byref(s)) == -1
    assert L.so_icp_pose_prior_sums(C.byref(prior), pose.ctypes.data_as(f64p), None) == -1
