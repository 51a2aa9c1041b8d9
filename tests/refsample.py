"""A plain numpy restatement of farthest-point sampling and the ball query over raw points (csrc/sample.hip), for the
tests: a loop over the steps of a scene / over the queries, the points of the scene side by side in numpy float32 arrays
whose every subtract, multiply and add is a ufunc call of its own (each rounded on its own, which is the contract; numpy
contracts nothing into an FMA).  Nothing here is fast.  The gather and the gradient are refquery's."""
import numpy as np

f32 = np.float32


def scenes(batch_ids, n, batch, n_points=None):
    """the point indices of every scene, ascending: rows at or beyond n_points and ids outside [0, batch) are in none"""
    ids = np.zeros(n, dtype=np.int64) if batch_ids is None else np.asarray(batch_ids).astype(np.int64)
    live = n if n_points is None else max(min(int(n_points), n), 0)
    ids = np.where(np.arange(n) < live, ids, -1)
    return [np.nonzero(ids == b)[0] for b in range(batch)]


def valid_points(points, index, ndim):
    """of the point indices `index`, those whose first ndim coordinates are all finite"""
    return index[np.isfinite(points[index, :ndim].astype(f32)).all(axis=1)] if len(index) else index


def dist2(d):
    """(d0 * d0 + d1 * d1) + d2 * d2 (ndim 2: d0 * d0 + d1 * d1) over the rows of d, one rounding per operation"""
    s = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]
    if d.shape[1] == 3:
        s = s + d[:, 2] * d[:, 2]
    return s


def fps_scene(xyz, K):
    """positions (into xyz, float32 [n, ndim], all valid) of min(n, K) samples, and the t of every step's pick"""
    n = len(xyz)
    picks, dists = [], []
    if n == 0:
        return picks, dists
    with np.errstate(all="ignore"):
        t = np.full(n, np.inf, dtype=f32)
        c = 0                                               # slot 0: the lowest valid point index
        picks.append(c)
        dists.append(f32(np.inf))
        for _ in range(1, min(n, K)):
            d2 = dist2(xyz - xyz[c])
            t = np.where(d2 < t, d2, t)
            t[c] = f32(-1)                                  # a chosen point stops being a candidate
            c = int(np.argmax(t))                           # the first of equal maxima: the lowest point index
            picks.append(c)
            dists.append(t[c])
    return picks, dists


def fps(points, batch_ids, batch, K, ndim=3, n_points=None):
    """idx int32 [batch, K] (-1 at or beyond count), count int32 [batch]"""
    points = np.asarray(points)
    idx = np.full((batch, K), -1, dtype=np.int32)
    count = np.zeros(batch, dtype=np.int32)
    for b, index in enumerate(scenes(batch_ids, len(points), batch, n_points)):
        index = valid_points(points, index, ndim)
        picks, _ = fps_scene(np.ascontiguousarray(points[index, :ndim], dtype=f32), K)
        idx[b, :len(picks)] = index[picks]
        count[b] = len(picks)
    return idx, count


def ball_query(queries, q_batch_ids, n_queries, points, p_batch_ids, n_points, batch, radius, nsample, ndim=3, pad="none"):
    """rows int32 [M, nsample], count int32 [M], offsets float32 [M, nsample, ndim], and hits [M]: the hits of the whole
    scene, before the cut at nsample (a diagnostic the kernel does not return)"""
    import refquery
    queries, points = np.asarray(queries), np.asarray(points)
    M = len(queries)
    rows = np.full((M, nsample), -1, dtype=np.int32)
    count = np.zeros(M, dtype=np.int32)
    offsets = np.zeros((M, nsample, ndim), dtype=f32)
    hits = np.zeros(M, dtype=np.int64)
    index = [valid_points(points, s, ndim) for s in scenes(p_batch_ids, len(points), batch, n_points)]
    xyz = [np.ascontiguousarray(points[s, :ndim], dtype=f32) for s in index]
    nq = M if n_queries is None else max(min(int(n_queries), M), 0)
    with np.errstate(all="ignore"):
        r2 = f32(radius) * f32(radius)
        for m in range(nq):
            b = 0 if q_batch_ids is None else int(q_batch_ids[m])
            q = queries[m, :ndim].astype(f32)
            if not 0 <= b < batch or np.isnan(q).any():
                continue
            d = xyz[b] - q
            hit = np.nonzero(dist2(d) < r2)[0]              # ascending position = ascending point index
            hits[m] = len(hit)
            k = min(len(hit), nsample)
            rows[m, :k] = index[b][hit[:k]]
            offsets[m, :k] = d[hit[:k]]
            count[m] = k
    if pad == "first":
        rows, offsets = refquery.pad_first(rows, count, offsets)
    return rows, count, offsets, hits
