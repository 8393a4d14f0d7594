"""The run of tests/test_gpu_sequence_prediction.py and tests/test_sequence_prediction_host.py: scans 0..3 of a scene in rotation, every
guess 0.1 m below its ground truth (no rotation), delta_k = gt(k-1)^-1 o guess_k.  Every registration then corrects + 0.1 m in z: a
prediction composed from the prediction before it sinks 0.1 m per frame, one anchored on the last exact guess stays 0.1 m off."""
import numpy as np

from superodom_amd import synth

ROTATION = 4
BIAS = np.array([0.0, 0.0, -0.1])


def biased_guess(sc, k):
    g = np.array(sc.gt_pose(k % ROTATION), float)
    g[:3] += BIAS
    return g


def biased_deltas(sc, count):
    d = np.zeros((count, 7)); d[:, 6] = 1.0
    for k in range(1, count):
        d[k] = synth.pose_between(sc.gt_pose((k - 1) % ROTATION), biased_guess(sc, k))
    return d
