"""The host build of superodom_amd/csrc/deskew_math.h (tests/native/deskew_host.cpp: g++ -O2 -ffp-contract=off, the flags of the device
build) behind one function with so_icp_deskew_scan's arguments, for tests/test_deskew_branches_host.py (CPU) and the bit comparison
of tests/test_gpu_deskew_branches.py."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "deskew_host.cpp")
LIB = os.path.join(HERE, "native", "libdeskew_host.so")
HDR = os.path.join(os.path.dirname(HERE), "superodom_amd", "csrc")
_lib = None


def _load():
    global _lib
    if _lib is None:
        deps = [SRC, os.path.join(HDR, "deskew_math.h"), os.path.join(HDR, "so_math.h")]
        if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in deps):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-I", HDR, SRC, "-o", LIB])
        _lib = C.CDLL(LIB)
        f64p = C.POINTER(C.c_double)
        _lib.dsk_host_deskew.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_double, f64p, C.c_size_t, C.c_int, f64p, f64p]
        _lib.dsk_host_deskew.restype = C.c_longlong
    return _lib


def deskew(records, time_off, t0, poses, imu, T_i_l=None):
    """records uint8 [n, stride] (float x y z at 0 4 8, float time at time_off), poses [n_poses, 8] = time, position, quaternion x y z w
    -> (rewritten records, start frame[7] = t_w_original_l + q_w_original_l, clamped count), by deskew_setup and deskew_point on the
    host; ValueError for a table whose times do not increase strictly"""
    L = _load()
    rec = np.ascontiguousarray(records, np.uint8).copy()
    poses = np.ascontiguousarray(poses, np.float64).reshape(-1, 8)
    til = None if T_i_l is None else np.ascontiguousarray(T_i_l, np.float64)
    assert rec.ndim == 2 and rec.shape[1] >= 12 and 0 <= time_off <= rec.shape[1] - 4 and len(poses) >= 1 and (til is None or til.shape == (7,))
    start = np.zeros(7)
    f64p = C.POINTER(C.c_double)
    n = L.dsk_host_deskew(rec.ctypes.data_as(C.c_void_p), rec.shape[0], rec.shape[1], int(time_off), float(t0), poses.ctypes.data_as(f64p),
                          len(poses), int(bool(imu)), None if til is None else til.ctypes.data_as(f64p), start.ctypes.data_as(f64p))
    if n < 0:
        raise ValueError("the pose times do not increase strictly")
    return rec, start, int(n)
