"""The fixtures of the centre-head target tests (numpy only): ground-truth boxes and the rows of a sparse 2-D level over
a 40 x 56 map (W != H catches swapped axes) of 3 scenes and 3 classes, at voxel 0.1 and a stride of 1, 2 or 4, so radii
run from the min_radius clamp up to about 15.

  scene 0   TILE + 2 random boxes (more than one staged tile), more than MAX_OBJS: the last ones have no slot
  scene 1   no box at all
  scene 2   boxes on the four borders and corners, centres outside the range (clamped), two boxes of one class in one
            cell, two classes in one cell, overlapping windows, spoiled rows (NaN, Inf, sizes 0 and negative), classes
            -1 and C, a box far outside the lower-left corner (centre (0, 0) exactly: equidistant from the rows at cells
            (1, 0) and (0, 1) -- an exact tie in any precision)
  others    foreign batch ids (-1 and B), and boxes behind the device count
The boxes of all scenes are shuffled together.  The rows: random cells per scene in shuffled order with the scenes mixed,
rows outside the grid, foreign batch ids, dead rows behind the device count; ``rows(..., without=2)`` leaves scene 2
without a row."""
import numpy as np

W, H, B, C = 40, 56, 3, 3
VOXEL = (0.1, 0.1)
MAX_OBJS = 100
STRIDES = (1, 2, 4)


def params(stride, **kw):
    p = dict(grid_size=(W, H), voxel_size=VOXEL, range_min=(-2.0 * stride, -2.8 * stride), stride=stride, num_classes=C,
             max_objs=MAX_OBJS, min_overlap=0.1, min_radius=2)
    p.update(kw)
    return p


def _random_boxes(rng, n, stride, extra):
    x0, y0 = -2.0 * stride, -2.8 * stride
    b = np.zeros((n, 7 + extra), np.float32)
    b[:, 0] = x0 + rng.uniform(0.013, 0.987, n) * W * 0.1 * stride
    b[:, 1] = y0 + rng.uniform(0.013, 0.987, n) * H * 0.1 * stride
    b[:, 2] = rng.uniform(-1.5, 0.5, n)
    b[:, 3] = rng.uniform(0.3, 5.3, n)
    b[:, 4] = rng.uniform(0.3, 2.3, n)
    b[:, 5] = rng.uniform(0.5, 2.5, n)
    b[:, 6] = rng.uniform(-3.1, 3.1, n)
    if extra:
        b[:, 7:] = rng.uniform(-2.0, 2.0, (n, extra))
    return b


def boxes(stride, tile, seed=0, extra=2):
    """(boxes f32 [M, 7 + extra], batch ids i32 [M], class ids i64 [M], n_boxes): the device count is below M"""
    rng = np.random.default_rng(1000 * stride + seed)
    s = float(stride)
    x0, y0 = -2.0 * s, -2.8 * s
    xe, ye = x0 + W * 0.1 * s, y0 + H * 0.1 * s
    cell = 0.1 * s
    parts, bid, cls = [], [], []

    def add(b, scene, c):
        parts.append(np.atleast_2d(b).astype(np.float32))
        n = parts[-1].shape[0]
        bid.extend([scene] * n if np.isscalar(scene) else list(scene))
        cls.extend([c] * n if np.isscalar(c) else list(c))

    n0 = tile + 2
    add(_random_boxes(rng, n0, stride, extra), 0, rng.integers(0, C, n0))
    special = _random_boxes(rng, 26, stride, extra)
    k = 0
    for px, py in ((x0 + 0.31 * cell, y0 + 20.4 * cell), (xe - 0.27 * cell, y0 + 31.6 * cell),      # four borders
                   (x0 + 17.3 * cell, y0 + 0.42 * cell), (x0 + 23.7 * cell, ye - 0.36 * cell),
                   (x0 + 0.4 * cell, y0 + 0.3 * cell), (xe - 0.3 * cell, y0 + 0.6 * cell),           # four corners
                   (x0 + 0.7 * cell, ye - 0.2 * cell), (xe - 0.6 * cell, ye - 0.7 * cell),
                   (x0 - 3.3, y0 + 11.3 * cell), (xe + 5.1, y0 + 40.7 * cell),                       # outside: clamped
                   (x0 + 30.2 * cell, y0 - 7.7), (x0 + 9.6 * cell, ye + 2.9),
                   (x0 - 50.0, y0 - 50.0)):                                                          # centre (0, 0)
        special[k, 0], special[k, 1] = px, py
        k += 1
    tie_box = k - 1
    for j in (k, k + 1, k + 2, k + 3):                    # four boxes in one cell: twice class 1, then classes 0 and 2
        special[j, 0], special[j, 1] = x0 + 12.0 * cell + (0.21 + 0.13 * (j - k)) * cell, y0 + 33.0 * cell + 0.55 * cell
    special[k + 1, 3:5] = (4.9, 2.1)                      # (a larger window over a smaller one)
    special[k + 4, 0], special[k + 4, 1] = x0 + 14.4 * cell, y0 + 34.6 * cell      # an overlapping window next to them
    special[k + 5, 0] = np.nan
    special[k + 6, 6] = np.inf
    special[k + 7, 3] = 0.0
    special[k + 8, 4] = -1.0
    special[k + 9, 5] = 0.0
    special[k + 10, 2] = -np.inf
    sc = rng.integers(0, C, 26)
    sc[k:k + 4] = (1, 1, 0, 2)
    sc[k + 4] = 1
    sc[k + 11], sc[k + 12] = -1, C                        # classes of another head / out of range: slot kept, mask 0
    sc[tie_box] = 0
    add(special, 2, sc)
    add(_random_boxes(rng, 4, stride, extra), [-1, B, -7, B + 5], rng.integers(0, C, 4))
    all_boxes, bid, cls = np.concatenate(parts), np.asarray(bid, np.int32), np.asarray(cls, np.int64)
    order = rng.permutation(all_boxes.shape[0])
    all_boxes, bid, cls = all_boxes[order], bid[order], cls[order]
    tail = _random_boxes(rng, 9, stride, extra)           # behind the device count: they do not exist
    n_boxes = all_boxes.shape[0]
    all_boxes = np.concatenate([all_boxes, tail])
    bid = np.concatenate([bid, rng.integers(0, B, 9).astype(np.int32)])
    cls = np.concatenate([cls, rng.integers(0, C, 9)])
    return np.ascontiguousarray(all_boxes), bid, cls, n_boxes


def second_boxes(stride, tile):
    """another box set of the same shape with a smaller device count (the replay of a captured graph)"""
    b, bid, cls, n = boxes(stride, tile, seed=7)
    return b, bid, cls, n - 31


def rows(seed=0, without=None):
    """(indices i32 [N, 3] = (b, y, x), n_live): shuffled, scenes mixed; scene 2 holds the cells (1, 0) and (0, 1) and
    not the cell (0, 0)"""
    rng = np.random.default_rng(77 + seed)
    parts = []
    for b, n in ((0, 420), (1, 150), (2, 260)):
        if b == without:
            continue
        ys, xs = rng.integers(0, H, n), rng.integers(0, W, n)
        if b == 2:
            keep = (xs + ys) > 1
            ys, xs = np.concatenate([ys[keep], [0, 1]]), np.concatenate([xs[keep], [1, 0]])
        parts.append(np.stack([np.full(len(ys), b), ys, xs], 1))
    bad = np.array([[0, -1, 5], [0, 3, W], [1, H, 2], [2, 4, -2], [-1, 5, 5], [B, 6, 6], [0, H + 7, W + 3]])
    idx = np.concatenate(parts + [bad]).astype(np.int32)
    idx = idx[rng.permutation(idx.shape[0])]
    dead = np.stack([rng.integers(0, B, 37), rng.integers(0, H, 37), rng.integers(0, W, 37)], 1).astype(np.int32)
    n_live = idx.shape[0]
    return np.ascontiguousarray(np.concatenate([idx, dead])), n_live
