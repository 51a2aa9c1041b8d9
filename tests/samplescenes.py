"""The clouds that test_refsample.py (CPU: the conditions) and test_gpu_sample.py (GPU: the kernels) share.  Everything
is generated from fixed seeds; references are computed once per process and never modified."""
import functools

import numpy as np

import refsample as rs

B, N_SCENE, M, M_FAR = 2, 2000, 600, 150
RADIUS, NSAMPLE = 1.0, 16


@functools.lru_cache(maxsize=None)
def base():
    """2 scenes x 2000 points uniform in [0, 8)^3 (4 columns: xyz + an intensity), scene-contiguous; 600 queries, the
    last 150 in [12, 16)^3 (no point within the radius), with random scenes"""
    rng = np.random.default_rng(0)
    pts = np.concatenate([rng.random((B * N_SCENE, 3)) * 8.0, rng.random((B * N_SCENE, 1))], axis=1).astype(np.float32)
    p_bid = np.repeat(np.arange(B, dtype=np.int32), N_SCENE)
    q = rng.random((M, 3)) * 8.0
    q[M - M_FAR:] = 12.0 + rng.random((M_FAR, 3)) * 4.0
    q = q.astype(np.float32)
    q_bid = rng.integers(0, B, M).astype(np.int32)
    for a in (pts, p_bid, q, q_bid):
        a.setflags(write=False)
    return pts, p_bid, q, q_bid


@functools.lru_cache(maxsize=None)
def base_ball(nsample=NSAMPLE, pad="none"):
    pts, p_bid, q, q_bid = base()
    return rs.ball_query(q, q_bid, None, pts, p_bid, None, B, RADIUS, nsample, 3, pad)


def interleaved(pts, bid, seed=2):
    """the rows in a random interleave of the scenes that keeps the order inside every scene: (pts, bid, new row of
    every old row)"""
    order = np.argsort(np.random.default_rng(seed).random(len(bid)), kind="stable")      # a random permutation ...
    for b in np.unique(bid):                                        # ... whose slots per scene are refilled in order
        slots = np.nonzero(bid[order] == b)[0]
        order[slots] = np.sort(order[slots])
    new_row = np.empty(len(bid), dtype=np.int64)
    new_row[order] = np.arange(len(bid))
    return np.ascontiguousarray(pts[order]), np.ascontiguousarray(bid[order]), new_row


# integer-lattice clouds: float32 arithmetic is exact on them
# FPS from (0, 0, 0): four points at squared distance 4 tie at every step and go in ascending index; the point at
# squared distance 1 is last
TIE_POINTS = np.array([[0, 0, 0], [1, 0, 0], [0, 2, 0], [2, 0, 0], [0, -2, 0], [-2, 0, 0]], dtype=np.float32)
TIE_ORDER = [0, 2, 3, 4, 5, 1]
# a query at the origin with radius 2: squared distance 4 is NOT inside (strict <), 3 is
EDGE_POINTS = np.array([[2, 0, 0], [1, 1, 1], [0, 0, 2], [0, 0, 0], [0, -2, 0], [-1, 1, -1], [1, 1, 2]], dtype=np.float32)
EDGE_HITS = [1, 3, 5]
DUPLICATES = np.tile(np.array([[3, -1, 2]], dtype=np.float32), (10, 1))
