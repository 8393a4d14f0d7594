"""What so_icp_correspondence_geometry (include/so_icp.h) must give, stated from the oracle's own correspondences (oracle_py CORR_DTYPE:
nbr, d2, eig, obs) and from the host build of the function the export kernel calls (plane_fit.h plane_fit5_geometry, built by
host_fit() below from tests/native/corr_geometry_host.cpp).  Shared by tests/test_correspondence_geometry_host.py (CPU) and
tests/test_gpu_correspondence_geometry.py (GPU)."""
import ctypes as C
import os
import subprocess

import numpy as np

import correspondences_ref as cref

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "native", "corr_geometry_host.cpp")
LIB = os.path.join(HERE, "native", "libcorr_geometry_host.so")
HDR = os.path.join(ROOT, "superodom_amd", "csrc")

RECORD_DTYPE = np.dtype([("index", "<u4"), ("nbr_index", "<u4", 5), ("obs", "u1", 3), ("reserved", "u1"), ("nbr", "<f4", 15), ("d2", "<f4", 5),
                         ("pad", "<u4"), ("pw", "<f8", 3), ("eig", "<f8", 3), ("pca_normal", "<f8", 3), ("mean_abs_dist", "<f8")])
assert RECORD_DTYPE.itemsize == 192

# (scene, scans): the inputs of the CPU checks and of the GPU tests -- those of tests/test_plane_fit_host.py
SCENES = [("tiny", (0, 1, 2)), ("small", (0, 5))]

# ---- measured tolerances ---------------------------------------------------------------------------------------------------------
# The largest differences between the HOST build of plane_fit5_geometry and the oracle (cyclic Jacobi eigen-solver, column-pivoted
# Householder plane; oracle/so_oracle.c orc_plane_match) over every accepted correspondence of SCENES, registered with
# max_iterations=5, at the pose the last outer iteration was formed at -- 37 854 points; measured by
# test_correspondence_geometry_host.py::test_measured_tolerances, which prints them and holds them to these constants (the
# constants are the measured values rounded up to two digits):
#   eig            max |eig - oracle eig| / oracle eig[2]
#   pca_normal     max |pca_normal - oracle normal| (both flipped towards pw by the same rule, LidarSlam.cpp:553-561)
#   mean_abs_dist  max |mean_abs_dist - oracle mean |n.p_j + d||
EIG_REL_MEASURED = 4.8e-14   # measured 4.751e-14 (tiny scan 1)
NORMAL_MEASURED = 1.6e-15    # measured 1.554e-15 (small scan 0)
MEAN_ABS_MEASURED = 7.2e-15  # measured 7.105e-15 (small scan 5)


def gpu_tolerance(measured):
    """10 x the measured host-against-oracle difference and not below 1e-12: the device's fit_div / fit_rsqrt may round differently
    from the host's division and 1 / sqrt, and that margin is unmeasured on the host"""
    return max(10.0 * measured, 1e-12)


def pw_bound(p, pose):
    """|pw - numpy's R(q) p + t|: the rotation is some twenty fp64 operations on terms of size |p|, the sum one more on |t|"""
    return 64 * cref.EPS * (np.linalg.norm(np.asarray(p, np.float64), axis=1) + np.linalg.norm(np.asarray(pose, float)[:3]) + 1.0)


def world(pose, p):
    pose = np.asarray(pose, np.float64)
    return cref.rotate(pose[3:], np.asarray(p, np.float64)) + pose[:3]


def host_fit():
    """fit(nb [N, 15] f32, pw [N, 3] f64, pose [7], plane_res, geometry=True) -> dict(status, nd, coeff, obs[, eig, normal, mean_abs]):
    plane_fit5_geometry (geometry=True) or plane_fit5 of the host build"""
    deps = [SRC, os.path.join(HDR, "plane_fit.h"), os.path.join(HDR, "so_math.h")]
    if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-I", HDR, SRC, "-o", LIB])
    L = C.CDLL(LIB)
    f32p, f64p, i32p = C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_int)
    L.cg_fit_geometry.argtypes = [f32p, f64p, f64p, C.c_float, C.c_double, C.c_int, f64p, f64p, i32p, i32p, f64p, f64p, f64p]
    L.cg_fit_plain.argtypes = [f32p, f64p, f64p, C.c_float, C.c_double, C.c_int, f64p, f64p, i32p, i32p]

    def fit(nb, pw, pose, plane_res, geometry=True):
        nb = np.ascontiguousarray(nb, np.float32).reshape(-1, 15); pw = np.ascontiguousarray(pw, np.float64).reshape(-1, 3)
        pose = np.ascontiguousarray(pose, np.float64)
        n = len(nb)
        nd = np.zeros((n, 4)); co = np.zeros(n); st = np.zeros(n, np.int32); ob = np.zeros((n, 3), np.int32)
        pr = np.float32(plane_res)
        head = (nb.ctypes.data_as(f32p), pw.ctypes.data_as(f64p), pose.ctypes.data_as(f64p), np.float32(3) * pr, float(pr) / 2.0, n)
        out = (nd.ctypes.data_as(f64p), co.ctypes.data_as(f64p), st.ctypes.data_as(i32p), ob.ctypes.data_as(i32p))
        res = dict(status=st, nd=nd, coeff=co, obs=ob)
        if not geometry:
            L.cg_fit_plain(*head, *out)
            return res
        ev = np.zeros((n, 3)); nrm = np.zeros((n, 3)); ma = np.zeros(n)
        L.cg_fit_geometry(*head, *out, ev.ctypes.data_as(f64p), nrm.ctypes.data_as(f64p), ma.ctypes.data_as(f64p))
        res.update(eig=ev, normal=nrm, mean_abs=ma)
        return res
    return fit


def pose_fit_of(st, guess):
    """the pose the LAST outer iteration of a registration formed its correspondences at, from oracle Stats (.iters) or so_icp_stats
    (.iterations): the guess when there was one iteration, else pose_after of the iteration before the last"""
    its = st.iters if hasattr(st, "iters") else st.iterations
    return np.asarray(guess, np.float64) if st.n_iterations <= 1 else np.array(its[st.n_iterations - 2].pose_after)


def oracle_geometry(oracle, corrs, pose_fit):
    """(pw, eig, normal, mean_abs) of ACCEPTED oracle correspondences `corrs` by orc_plane_match's own statements (so_oracle.c): eig as
    it stored them; the normal = the first eigenvector of orc_eig3_sym on the scatter summed in its order, flipped towards pw; the
    mean absolute distance of the five neighbours from its plane (n, d), summed in its order"""
    L = oracle.lib()
    L.orc_eig3_sym.restype = None
    f64p = C.POINTER(C.c_double)
    n = len(corrs)
    nbr = np.asarray(corrs["nbr"], np.float64).reshape(n, 5, 3)
    pw = world(pose_fit, corrs["p"])
    mean = np.zeros((n, 3))
    for j in range(5):
        mean += nbr[:, j]
    mean /= 5.0
    S = np.zeros((n, 3, 3))
    for j in range(5):
        c = nbr[:, j] - mean
        S += c[:, :, None] * c[:, None, :]
    normal = np.zeros((n, 3)); ev = np.zeros(3); V = np.zeros(9)
    for t in range(n):
        L.orc_eig3_sym(np.ascontiguousarray(S[t]).ctypes.data_as(f64p), ev.ctypes.data_as(f64p), V.ctypes.data_as(f64p))
        normal[t] = V[:3]
    flip = np.einsum("ij,ij->i", pw, normal) < 0
    normal[flip] = -normal[flip]
    pn, pd = np.asarray(corrs["n"]), np.asarray(corrs["d"])
    total = np.zeros(n)
    for j in range(5):
        total += np.abs(pn[:, 0] * nbr[:, j, 0] + pn[:, 1] * nbr[:, j, 1] + pn[:, 2] * nbr[:, j, 2] + pd)
    return pw, np.asarray(corrs["eig"]), normal, total / 5.0


def differences(got_eig, got_normal, got_mean_abs, o_eig, o_normal, o_mean_abs):
    """(eig relative to eig[2], normal, mean_abs): the three figures the tolerances are stated in"""
    if not len(got_eig):
        return 0.0, 0.0, 0.0
    return (float(np.max(np.abs(got_eig - o_eig) / o_eig[:, 2:3])), float(np.max(np.abs(got_normal - o_normal))),
            float(np.max(np.abs(got_mean_abs - o_mean_abs))))


def hist_of(obs):
    """obs_hist[9] of labels [N, 3]"""
    return np.bincount(np.asarray(obs, np.int64).ravel(), minlength=9)[:9]
