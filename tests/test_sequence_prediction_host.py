"""CPU: the pose so_icp_register_sequence bins the next scan under and places its window for (reg_plan.h: predicted_guess) -- it is
pose_compose(exact guess of the registration in flight, next delta) to the bit, and over the biased run of
tests/test_gpu_sequence_prediction.py it never comes within cube_stable's margin of a cube face, where the prediction composed from the
prediction before it does, at frame 240."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import sequence_prediction_data as sqd
from superodom_amd import synth

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "native", "sequence_prediction_host.cpp")
LIB = os.path.join(HERE, "native", "libsequence_prediction_host.so")
HDR = os.path.join(ROOT, "superodom_amd", "csrc")
F64P, I32P = C.POINTER(C.c_double), C.POINTER(C.c_int)

ORIGIN, DIMS, MARGIN = (10, 10, 5), (21, 21, 11), 1.0  # the default window (LocalMap.h:131-144) and the margin sequence.cpp passes
FRAMES = 600


class Trajectory:  # (what the data module needs of a synth.Scene, without its map)
    gt_pose = staticmethod(synth.trajectory_pose)


@pytest.fixture(scope="module")
def native():
    deps = [SRC] + [os.path.join(HDR, h) for h in ("reg_plan.h", "so_math.h")]
    if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-fPIC", "-shared", "-I", HDR, SRC, "-o", LIB])
    L = C.CDLL(LIB)
    L.sq_predicted_guess.argtypes = [F64P, F64P, F64P]; L.sq_predicted_guess.restype = None
    L.sq_pose_compose.argtypes = [F64P, F64P, F64P]; L.sq_pose_compose.restype = None
    L.sq_cube_stable.argtypes = [I32P, I32P, F64P, C.c_double]
    return L


def _call(fn, a, d):
    a, d, o = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(d, np.float64), np.zeros(7)
    fn(a.ctypes.data_as(F64P), d.ctypes.data_as(F64P), o.ctypes.data_as(F64P))
    return o


def _stable(native, pose):
    t = np.ascontiguousarray(pose[:3], np.float64)
    return bool(native.sq_cube_stable((C.c_int * 3)(*ORIGIN), (C.c_int * 3)(*DIMS), t.ctypes.data_as(F64P), MARGIN))


def _exact_guess(sc, deltas, k):
    """of frame k, with registration k - 1 taken to end on its ground truth (it ends within millimetres of it)"""
    return sqd.biased_guess(sc, 0) if k == 0 else synth.pose_compose(sc.gt_pose((k - 1) % sqd.ROTATION), deltas[k])


def test_the_rule_is_pose_compose_of_the_exact_guess_and_the_next_delta(native):
    sc = Trajectory()
    deltas = sqd.biased_deltas(sc, 400)
    for k in (0, 317):  # pose0, and a later frame
        exact = _exact_guess(sc, deltas, k)
        got = _call(native.sq_predicted_guess, exact, deltas[k + 1])
        assert got.tobytes() == _call(native.sq_pose_compose, exact, deltas[k + 1]).tobytes()
        assert got.tobytes() == synth.pose_compose(exact, deltas[k + 1]).tobytes()  # (the arithmetic the GPU tests hold guesses_out to)


def test_the_anchored_prediction_stays_clear_of_the_cube_faces(native):
    sc = Trajectory()
    deltas = sqd.biased_deltas(sc, FRAMES + 1)
    worst = 0.0
    dead = sqd.biased_guess(sc, 0)  # the prediction composed from the prediction before it, for comparison
    dead_refused = []
    for k in range(FRAMES):
        pred = _call(native.sq_predicted_guess, _exact_guess(sc, deltas, k), deltas[k + 1])
        assert _stable(native, pred), (k, pred[:3])
        worst = max(worst, float(np.linalg.norm(pred[:3] - sqd.biased_guess(sc, k + 1)[:3])))
        dead = _call(native.sq_pose_compose, dead, deltas[k + 1])
        if not _stable(native, dead):
            dead_refused.append(k + 1)
            dead = _exact_guess(sc, deltas, k + 1)  # (the frame is started from its exact guess instead: the chain begins again there)
    print("anchored: worst distance from the actual guess %.3f m | dead-reckoned: refused at frames %s" % (worst, dead_refused))
    assert worst < 0.11  # one frame's correction: the 0.1 m bias
    assert dead_refused and 235 <= dead_refused[0] <= 245, dead_refused  # (0.1 m per frame from z ~ 0 to within 1 m of the face at -25)
