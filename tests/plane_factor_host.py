"""The host build of superodom_amd/csrc/plane_factor.h (tests/native/plane_factor_host.cpp: g++ -O2 -ffp-contract=off, the flags of the
device build) behind one function, for tests/test_plane_factor_host.py (CPU) and the bit comparison of tests/test_gpu_correspondences.py."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "plane_factor_host.cpp")
LIB = os.path.join(HERE, "native", "libplane_factor_host.so")
HDR = os.path.join(os.path.dirname(HERE), "superodom_amd", "csrc")
N_SUMS = 29  # cost, count, Jtr[6], JtJ[21]
_lib = None


def _load():
    global _lib
    if _lib is None:
        deps = [SRC, os.path.join(HDR, "plane_factor.h"), os.path.join(HDR, "so_math.h")]
        if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in deps):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-I", HDR, SRC, "-o", LIB])
        _lib = C.CDLL(LIB)
        f32p, f64p = C.POINTER(C.c_float), C.POINTER(C.c_double)
        _lib.pfac_evaluate.argtypes = [f32p, f64p, f64p, f64p, C.c_int, f64p, C.c_double, C.c_int, f64p, f64p, f64p, f64p]
        _lib.pfac_evaluate.restype = None
    return _lib


def evaluate(p, n, d, coeff, pose, a2, variant):
    """(residual [N], weight [N], cost term [N], the 29 sums added in index order) of the correspondences (p float32 [N, 3], n [N, 3],
    d, coeff) at `pose` under TukeyLoss(a2, variant), by plane_factor.h on the host"""
    L = _load()
    p = np.ascontiguousarray(p, np.float32).reshape(-1, 3)
    n, d, coeff = (np.ascontiguousarray(a, np.float64) for a in (n, d, coeff))
    pose = np.ascontiguousarray(pose, np.float64)
    N = len(p)
    assert n.shape == (N, 3) and d.shape == (N,) and coeff.shape == (N,) and pose.shape == (7,)
    r, w, term, sums = np.zeros(N), np.zeros(N), np.zeros(N), np.zeros(N_SUMS)
    f32p, f64p = C.POINTER(C.c_float), C.POINTER(C.c_double)
    L.pfac_evaluate(p.ctypes.data_as(f32p), n.ctypes.data_as(f64p), d.ctypes.data_as(f64p), coeff.ctypes.data_as(f64p), N, pose.ctypes.data_as(f64p),
                    float(a2), int(variant), r.ctypes.data_as(f64p), w.ctypes.data_as(f64p), term.ctypes.data_as(f64p), sums.ctypes.data_as(f64p))
    return r, w, term, sums


def displaced(pose):
    """`pose` moved 1 m up and turned a little: on the synthetic scenes part of a scan's correspondences then lies outside the loss's
    window (the callers assert it)"""
    o = np.array(pose, np.float64)
    o[:3] += (0.3, -0.2, 1.0)
    o[3:] += (0.01, -0.02, 0.015, 0.0)
    o[3:] /= np.linalg.norm(o[3:])
    return o
