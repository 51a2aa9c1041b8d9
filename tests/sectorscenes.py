"""The clouds and boxes that test_refsector.py (CPU: the conditions) and test_gpu_sector.py (GPU: the kernels) share.
Everything is generated from fixed seeds and never modified."""
import functools

import numpy as np

B, N_SCENE = 3, 2000
CENTER = (1.5, -2.25)
RADIUS = 1.6
BOX_COUNTS = ((0, 1, 40), (129, 40, 1))            # boxes per scene: none, one, some, and one past a staged tile of 128


@functools.lru_cache(maxsize=None)
def base():
    """3 scenes x 2000 points, x / y uniform in [-40, 40), z in [-2, 2), plus an intensity column; scene-contiguous"""
    rng = np.random.default_rng(0)
    n = B * N_SCENE
    pts = np.concatenate([rng.random((n, 2)) * 80.0 - 40.0, rng.random((n, 1)) * 4.0 - 2.0, rng.random((n, 1))],
                         axis=1).astype(np.float32)
    bid = np.repeat(np.arange(B, dtype=np.int32), N_SCENE)
    pts.setflags(write=False)
    bid.setflags(write=False)
    return pts, bid


@functools.lru_cache(maxsize=None)
def boxes(counts, seed=1):
    """sum(counts) OpenPCDet boxes (8 columns: the 7-vector and a score), counts[b] of them in scene b, in a random
    order across scenes: centres over the cloud, sizes about (4, 2, 1.6)"""
    rng = np.random.default_rng(seed)
    m = int(sum(counts))
    out = np.concatenate([rng.random((m, 2)) * 80.0 - 40.0, rng.random((m, 1)) * 2.0 - 1.0,
                          np.array([3.0, 1.5, 1.2]) + rng.random((m, 3)) * np.array([2.0, 1.0, 0.8]),
                          rng.random((m, 1)) * 6.28 - 3.14, rng.random((m, 1))], axis=1).astype(np.float32)
    bid = np.repeat(np.arange(len(counts), dtype=np.int32), counts)[rng.permutation(m)]
    out.setflags(write=False)
    bid.setflags(write=False)
    return out, bid


# About the centre c (its coordinates are exact in float32): points on the four axes, with either zero, the centre itself,
# and points a float32 step to either side of the negative x axis.  SPECIAL_SECTORS[S] are their sectors, by hand: the
# direction the rule looks at is (a, b) = c - p, the angle theta of it in [0, 2 pi), the sector floor(theta / (2 pi / S)).
def special(center=CENTER):
    cx, cy = np.float32(center[0]), np.float32(center[1])
    one = np.float32(1.0)
    up, down = np.nextafter(cy, np.float32(np.inf)), np.nextafter(cy, np.float32(-np.inf))
    xy = [(cx - one, cy),          # 0: theta = 0 (west of the centre: OpenPCDet's atan2 = pi, its dropped index S)
          (cx, cy - one),          # 1: theta = pi / 2
          (cx + one, cy),          # 2: theta = pi
          (cx, cy + one),          # 3: theta = 3 pi / 2
          (cx, cy),                # 4: the centre
          (cx - one, down),        # 5: just above theta = 0
          (cx - one, up)]          # 6: just below theta = 2 pi
    pts = np.zeros((len(xy), 4), dtype=np.float32)
    pts[:, :2] = np.array(xy, dtype=np.float32)
    return pts


SPECIAL_SECTORS = {
    1: [0, 0, 0, 0, 0, 0, 0],
    2: [0, 0, 1, 1, 0, 0, 1],
    3: [0, 0, 1, 2, 0, 0, 2],
    4: [0, 1, 2, 3, 0, 0, 3],
    6: [0, 1, 3, 4, 0, 0, 5],
    64: [0, 16, 32, 48, 0, 0, 63],
}
