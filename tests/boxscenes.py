"""Seeded box clouds for the rotated-box tests (csrc/box.hip): what a detection head emits -- boxes of car size spread
over a 40 m x 40 m field, every fourth a jittered copy of its neighbour, some with parallel edges, some exact duplicates
-- and a jittered lattice for the counts at which the NMS reduce changes its instance."""
import numpy as np


def cloud(seed, n, B):
    """(boxes fp32 [n, 7], batch ids int32 [n], scores fp32 [n])."""
    rng = np.random.default_rng(seed); b = np.zeros((n, 7), np.float32)
    b[:, 0] = rng.random(n) * 40.0;  b[:, 1] = rng.random(n) * 40.0 - 20.0;  b[:, 2] = rng.random(n) * 2.0 - 1.0
    b[:, 3] = 3.0 + rng.random(n) * 2.0;  b[:, 4] = 1.5 + rng.random(n) * 0.8;  b[:, 5] = 1.4 + rng.random(n) * 0.6
    b[:, 6] = rng.random(n) * 6.0 - 3.0
    j = np.arange(3, n, 4); b[j] = b[j - 1]                     # jittered copies: what a head emits
    b[j, :2] += (rng.random((len(j), 2)).astype(np.float32) - 0.5) * 1.0
    b[j, 6] += (rng.random(len(j)).astype(np.float32) - 0.5) * 0.3
    k = np.arange(7, n, 16); b[k, 6] = b[k - 2, 6]              # parallel edges
    d = np.arange(11, n, 32); b[d] = b[d - 4]                   # exact duplicates
    bid = rng.integers(0, B, n).astype(np.int32); score = rng.random(n).astype(np.float32)
    score[d] = score[d - 4]; bid[j] = bid[j - 1]; bid[d] = bid[d - 4]
    return b, bid, score


def lattice(seed, n, pitch=0.9):
    """n boxes of 2 x 1 on a jittered lattice: each overlaps a handful of others.  (boxes, scores)."""
    rng = np.random.default_rng(seed)
    side = int(np.ceil(np.sqrt(n)))
    i = np.arange(n)
    b = np.zeros((n, 7), np.float32)
    b[:, 0] = (i % side) * pitch + rng.random(n) * 0.4
    b[:, 1] = (i // side) * pitch + rng.random(n) * 0.4
    b[:, 3], b[:, 4], b[:, 5] = 2.0, 1.0, 1.5
    b[:, 6] = rng.random(n) * 3.0 - 1.5
    return b, rng.random(n).astype(np.float32)


def corners64(boxes):
    """The corners of boxes_to_corners from float64 trigonometry, rounded to fp32: (bev [n, 4, 2], zrange [n, 2])."""
    b = boxes.astype(np.float64)
    c, s = np.cos(b[:, 6]), np.sin(b[:, 6])
    sx = np.array([1.0, -1.0, -1.0, 1.0]); sy = np.array([1.0, 1.0, -1.0, -1.0])
    lx, ly = sx[None] * b[:, 3:4] * 0.5, sy[None] * b[:, 4:5] * 0.5
    bev = np.stack([b[:, 0:1] + (lx * c[:, None] - ly * s[:, None]), b[:, 1:2] + (lx * s[:, None] + ly * c[:, None])], -1)
    z = np.stack([b[:, 2] - b[:, 5] * 0.5, b[:, 2] + b[:, 5] * 0.5], -1)
    return bev.astype(np.float32), z.astype(np.float32)
