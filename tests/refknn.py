"""A plain numpy restatement of the k-nearest-neighbour query with inverse-distance weights over raw points
(csrc/knn.hip), for the tests: a loop over the queries, the points of the query's scene side by side in numpy float32
arrays whose every subtract, multiply, add, square root and divide is a ufunc call of its own (each rounded on its own,
which is the contract; numpy contracts nothing into an FMA and its float32 sqrt and divide are correctly rounded).
Nothing here is fast.  Scenes, the validity of a point and the distance are refsample's; the blend and its gradient are
refinterp's, the gather and its gradient refquery's."""
import numpy as np

from refsample import dist2, scenes, valid_points

f32 = np.float32


def weights_of(d2, eps):
    """r_s = 1 / (sqrt(d2_s) + eps), norm = ((r_0 + r_1) + r_2) ..., w_s = r_s / norm over the float32 vector d2"""
    r = f32(1) / (np.sqrt(d2) + f32(eps))
    norm = r[0]
    for s in range(1, len(r)):
        norm = norm + r[s]                                  # (ascending slot, one rounding per addition)
    return r / norm


def knn_query(queries, q_batch_ids, n_queries, points, p_batch_ids, n_points, batch, k, ndim=3, width=None, pad="none",
              eps=1e-8):
    """rows int32 [M, width], count int32 [M], dist2 / weights float32 [M, width], offsets float32 [M, width, ndim]"""
    queries, points = np.asarray(queries), np.asarray(points)
    M, width = len(queries), k if width is None else width
    assert width >= k
    rows = np.full((M, width), -1, dtype=np.int32)
    count = np.zeros(M, dtype=np.int32)
    d2o = np.zeros((M, width), dtype=f32)
    weights = np.zeros((M, width), dtype=f32)
    offsets = np.zeros((M, width, ndim), dtype=f32)
    index = [valid_points(points, s, ndim) for s in scenes(p_batch_ids, len(points), batch, n_points)]
    xyz = [np.ascontiguousarray(points[s, :ndim], dtype=f32) for s in index]
    nq = M if n_queries is None else max(min(int(n_queries), M), 0)
    with np.errstate(all="ignore"):
        for m in range(nq):
            b = 0 if q_batch_ids is None else int(q_batch_ids[m])
            q = queries[m, :ndim].astype(f32)
            if not 0 <= b < batch or not np.isfinite(q).all() or len(index[b]) == 0:
                continue
            d = xyz[b] - q
            d2 = dist2(d)
            order = np.lexsort((index[b], d2))[:k]          # the total order (d2, point index)
            c = len(order)
            rows[m, :c], count[m] = index[b][order], c
            d2o[m, :c], offsets[m, :c] = d2[order], d[order]
            weights[m, :c] = weights_of(d2[order], eps)
            if pad == "first":                              # slot 0 again, with weight 0
                rows[m, c:k], d2o[m, c:k], offsets[m, c:k] = rows[m, 0], d2o[m, 0], offsets[m, 0]
    return rows, count, d2o, weights, offsets

