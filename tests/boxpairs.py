"""Seeded (prediction, target) pairs for the gradient tests of csrc/boxgrad.hip: what a rotated-IoU regression loss sees
in the middle of training -- targets from the detection cloud, predictions jittered in all seven numbers, every eighth
prediction contained in its target, and a second prediction table in which every fourth pair is disjoint (the pairs only
a penalty moves)."""
import numpy as np

import boxscenes


def pairs(seed, n):
    """(targets, predictions, predictions_far), fp32 [n, 7] each.  predictions: centre +-1 m, z +-0.4, sizes x [0.7,
    1.3], heading +-0.4; every eighth: sizes x 0.4, the target's centre, heading + 0.2.  predictions_far: the same with
    every fourth moved 8 m in x."""
    target = boxscenes.cloud(seed, n, 1)[0]
    rng = np.random.default_rng(seed + 1)
    pred = target.astype(np.float64)
    pred[:, 0:2] += rng.random((n, 2)) * 2.0 - 1.0
    pred[:, 2] += rng.random(n) * 0.8 - 0.4
    pred[:, 3:6] *= 0.7 + rng.random((n, 3)) * 0.6
    pred[:, 6] += rng.random(n) * 0.8 - 0.4
    inside = np.arange(7, n, 8)
    pred[inside] = target[inside]
    pred[inside, 3:6] *= 0.4
    pred[inside, 6] += 0.2
    far = pred.copy()
    far[np.arange(2, n, 4), 0] += 8.0
    return target, pred.astype(np.float32), far.astype(np.float32)
