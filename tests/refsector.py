"""A plain numpy restatement of sectorised keypoint sampling (csrc/sample.hip: spx_sector_ids, spx_fps_quota,
spx_fps_segments), for the tests: the sector rule, the RoI filter, the quotas and the packed sampling, in numpy float32
arrays whose every subtract, multiply, add and square root is a ufunc call of its own (each rounded on its own, which is
the contract; numpy contracts nothing into an FMA, and its float32 sqrt is correctly rounded).  The sampling inside a
segment is refsample.fps_scene.  Nothing here is fast."""
import numpy as np

import refsample as rs

f32 = np.float32
AXES = ((1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.0, -1.0))


def table(S):
    """float32 [S, 2]: (cos, sin)(2 pi k / S) computed in float64 and rounded, exact where 4 k % S == 0"""
    out = np.zeros((S, 2), dtype=f32)
    for k in range(S):
        if 4 * k % S == 0:
            out[k] = AXES[4 * k // S]
        else:
            t = 2.0 * np.pi * float(k) / float(S)
            out[k] = (f32(np.cos(t)), f32(np.sin(t)))
    return out


def sectors(x, y, S, center=(0.0, 0.0)):
    """the sector of every (x, y) (float32 arrays) about the centre: int64 [n]"""
    x, y = np.asarray(x, dtype=f32), np.asarray(y, dtype=f32)
    tab = table(S)
    with np.errstate(all="ignore"):
        a = -(x - f32(center[0]))
        b = -(y - f32(center[1]))
        half = np.where((b > 0) | ((b == 0) & (a > 0)), 0, 1)
        past = np.zeros(len(x), dtype=np.int64)
        for k in range(S):
            hk = 1 if 2 * k >= S else 0
            cross = tab[k, 0] * b - tab[k, 1] * a
            past += (half > hk) | ((half == hk) & (cross >= 0))
    sector = np.maximum(past - 1, 0)
    return np.where((a == 0) & (b == 0), 0, sector)


def valid_boxes(boxes, batch_ids, batch, n_boxes=None):
    """per scene the indices (ascending) of its valid boxes: below the count, id in range, seven finite values, sizes > 0"""
    boxes = np.asarray(boxes)
    index = rs.scenes(batch_ids, len(boxes), batch, n_boxes)
    out = []
    for s in index:
        if len(s):
            v = boxes[s, :7].astype(f32)
            s = s[np.isfinite(v).all(axis=1) & (v[:, 3:6] > 0).all(axis=1)]
        out.append(s)
    return out


def roi_keep(xyz, boxes, radius):
    """of the points xyz (float32 [n, 3], valid) of ONE scene and its valid boxes (float32 [m, >= 7]): kept or not"""
    n = len(xyz)
    if len(boxes) == 0 or n == 0:
        return np.zeros(n, dtype=bool)
    with np.errstate(all="ignore"):
        c = np.ascontiguousarray(boxes[:, :3], dtype=f32)
        d0 = c[None, :, 0] - xyz[:, None, 0]
        d1 = c[None, :, 1] - xyz[:, None, 1]
        d2 = c[None, :, 2] - xyz[:, None, 2]
        s = d0 * d0 + d1 * d1
        s = s + d2 * d2
        near = np.argmin(s, axis=1)                          # the first of equal minima: the lowest box index
        best = s[np.arange(n), near]
        h = f32(0.5) * np.ascontiguousarray(boxes[:, 3:6], dtype=f32)
        r2 = rs.dist2(h)
        return (best < f32(np.inf)) & (np.sqrt(best) < np.sqrt(r2[near]) + f32(radius))


def sector_ids(points, batch_ids, batch, S, center=(0.0, 0.0), rois=None, roi_batch_ids=None, roi_radius=None,
               n_points=None, n_rois=None, ndim=3):
    """seg int32 [N]: b * S + sector, or -1"""
    points = np.asarray(points)
    seg = np.full(len(points), -1, dtype=np.int32)
    boxes = None if rois is None else valid_boxes(rois, roi_batch_ids, batch, n_rois)
    for b, index in enumerate(rs.scenes(batch_ids, len(points), batch, n_points)):
        index = rs.valid_points(points, index, ndim)
        if len(index) == 0:
            continue
        xyz = np.ascontiguousarray(points[index, :ndim], dtype=f32)
        if rois is not None:
            keep = roi_keep(xyz, np.asarray(rois)[boxes[b]], roi_radius)
            index, xyz = index[keep], xyz[keep]
        seg[index] = b * S + sectors(xyz[:, 0], xyz[:, 1], S, center)
    return seg


def quotas(sizes, batch, S, K):
    """from the sizes of the batch * S segments: quota, slot int32 [batch * S], count int32 [batch], in exact integers"""
    sizes = [int(v) for v in sizes]
    quota, slot, count = [], [], []
    for b in range(batch):
        nk = sizes[b * S:(b + 1) * S]
        n, at = sum(nk), 0
        for v in nk:
            q = 0 if n == 0 else min(v, (v * K + n - 1) // n)
            quota.append(q)
            slot.append(at)
            at += q
        count.append(at)
    return np.array(quota, dtype=np.int32), np.array(slot, dtype=np.int32), np.array(count, dtype=np.int32)


def segments(ids, groups):
    """the point indices of every group, ascending (ids outside [0, groups) are in none)"""
    ids = np.asarray(ids)
    return [np.nonzero(ids == g)[0] for g in range(groups)]


def fps_segments(points, index, quota, max_samples, ndim=3):
    """idx int32 [G, max_samples] (-1 at or beyond count), count int32 [G]: group g = the point indices index[g]"""
    points = np.asarray(points)
    G = len(index)
    idx = np.full((G, max_samples), -1, dtype=np.int32)
    count = np.zeros(G, dtype=np.int32)
    for g in range(G):
        k = min(max(int(quota[g]), 0), max_samples)
        valid = rs.valid_points(points, np.asarray(index[g], dtype=np.int64), ndim)
        if k == 0 or len(valid) == 0:
            continue
        picks, _ = rs.fps_scene(np.ascontiguousarray(points[valid, :ndim], dtype=f32), k)
        idx[g, :len(picks)] = valid[picks]
        count[g] = len(picks)
    return idx, count


def sector_fps(points, batch_ids, batch, K, S, ndim=3, **kw):
    """idx int32 [batch, K + S - 1] packed sector by sector, count int32 [batch], seg int32 [N], quota int32 [batch * S]"""
    seg = sector_ids(points, batch_ids, batch, S, ndim=ndim, **kw)
    index = segments(seg, batch * S)
    quota, slot, count = quotas([len(s) for s in index], batch, S, K)
    per, _ = fps_segments(points, index, quota, K, ndim)
    idx = np.full((batch, K + S - 1), -1, dtype=np.int32)
    for g in range(batch * S):
        idx[g // S, slot[g]:slot[g] + quota[g]] = per[g, :quota[g]]
    return idx, count, seg, quota
