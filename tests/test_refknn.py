"""CPU: the numpy restatement tests/refknn.py (what tests/test_gpu_knn.py holds the kernel of csrc/knn.hip to, bit for
bit) against independent formulations: float64 distances over the whole scene sorted by (distance, index), the float64
weight formula, and integer-lattice clouds on which float32 arithmetic is exact."""
import functools

import numpy as np
import pytest

import refknn as rk
import samplescenes as ss

KS = (1, 3, 16, 64)
U = 2.0 ** -24                                              # half an ulp of a float32 in [1, 2): one rounding


@functools.lru_cache(maxsize=None)
def base_knn(k):
    pts, p_bid, q, q_bid = ss.base()
    return rk.knn_query(q, q_bid, None, pts, p_bid, None, ss.B, k)


@functools.lru_cache(maxsize=None)
def base_f64(k):
    """per query of the base scene: the first k + 1 point indices by float64 (distance, index) and their distances"""
    pts, p_bid, q, q_bid = ss.base()
    idx = np.zeros((ss.M, k + 1), dtype=np.int64)
    dist = np.zeros((ss.M, k + 1))
    for m in range(ss.M):
        scene = np.nonzero(p_bid == q_bid[m])[0]
        d = np.sqrt(((pts[scene, :3].astype(np.float64) - q[m].astype(np.float64)) ** 2).sum(axis=1))
        order = np.lexsort((scene, d))[:k + 1]
        idx[m], dist[m] = scene[order], d[order]
    return idx, dist


@pytest.mark.parametrize("k", KS)
def test_neighbours_equal_the_float64_order_where_it_is_decided(k):
    """a query is left out when two adjacent float64 distances among its first k + 1 differ by less than 1e-6 relative
    (float32 rounding may order them either way); at most 1 % of the queries may be left out"""
    rows, count, d2, _, offsets = base_knn(k)
    idx, dist = base_f64(k)
    close = (np.diff(dist, axis=1) < 1e-6 * dist[:, 1:]).any(axis=1)
    print(f"k = {k}: {int(close.sum())} of {ss.M} queries left out")
    assert close.sum() <= ss.M // 100
    assert (count == k).all() and (rows >= 0).all()
    keep = ~close
    np.testing.assert_array_equal(rows[keep], idx[keep, :k])
    np.testing.assert_allclose(np.sqrt(d2.astype(np.float64))[keep], dist[keep, :k], rtol=1e-6)
    pts, _, q, _ = ss.base()
    np.testing.assert_array_equal(offsets, pts[rows, :3] - q[:, None, :])
    assert (np.diff(d2, axis=1) >= 0).all()                 # written in ascending distance


@pytest.mark.parametrize("k", KS)
def test_weights_equal_the_float64_formula(k):
    """within 1e-6 relative: eight roundings of 2^-24 (the square root, + eps, 1 / x, the division by the norm, and
    what the additions of the norm leave of their k - 1 roundings: its terms are positive, so every addition's error is
    2^-24 of a partial sum that is no larger than the norm, and the errors of a sum of k terms of mixed sign of
    rounding stay far below their worst case (k - 1) * 2^-24); and a live query's weights sum to 1 within 4 * 2^-24 * k"""
    rows, count, d2, w, _ = base_knn(k)
    r = 1.0 / (np.sqrt(d2.astype(np.float64)) + np.float64(np.float32(1e-8)))
    want = r / r.sum(axis=1, keepdims=True)
    np.testing.assert_allclose(w, want, rtol=1e-6)
    assert (np.abs(w.astype(np.float64).sum(axis=1) - 1.0) <= 4 * U * k).all()
    assert (w > 0).all() and (np.diff(w, axis=1) <= 0).all()             # the nearest point weighs most


def test_equal_distances_go_to_the_lowest_index():
    zero = np.zeros((1, 3), dtype=np.float32)
    # from the origin: squared distances 4, 4, 1, 4, 4 (and 0 at index 6)
    pts = np.array([[2, 0, 0], [0, 2, 0], [1, 0, 0], [0, 0, -2], [-2, 0, 0], [5, 5, 5], [0, 0, 0]], dtype=np.float32)
    rows, count, d2, w, off = rk.knn_query(zero, None, None, pts, None, None, 1, 4)
    assert rows[0].tolist() == [6, 2, 0, 1] and count[0] == 4 and d2[0].tolist() == [0, 1, 4, 4]
    rows, count, _, _, _ = rk.knn_query(zero, None, None, pts[::-1].copy(), None, None, 1, 4)
    assert rows[0].tolist() == [0, 4, 2, 3]                 # the same points renumbered: 0 <- 6, 4 <- 2, then 2 < 3 < 5 < 6
    rows, count, d2, _, _ = rk.knn_query(zero[:, :2], None, None, np.ascontiguousarray(pts[:, :2]), None, None, 1, 3, ndim=2)
    assert rows[0].tolist() == [3, 6, 2] and d2[0].tolist() == [0, 0, 1]          # (0, 0, -2) projects onto the query


def test_an_all_duplicates_scene_yields_ascending_distinct_indices():
    q = np.array([[1, 1, 1]], dtype=np.float32)
    rows, count, d2, w, _ = rk.knn_query(q, None, None, ss.DUPLICATES, None, None, 1, 6)
    assert rows[0].tolist() == [0, 1, 2, 3, 4, 5] and count[0] == 6 and (d2[0] == d2[0, 0]).all()
    assert np.abs(w[0] - np.float32(1 / 6)).max() <= 2 * U
    rows, count, _, w, _ = rk.knn_query(q, None, None, ss.DUPLICATES, None, None, 1, 16, pad="first")
    assert rows[0].tolist() == list(range(10)) + [0] * 6 and count[0] == 10 and (w[0, 10:] == 0).all()
    rows, count, _, _, _ = rk.knn_query(q, None, None, ss.DUPLICATES, None, None, 1, 12, width=16)
    assert rows[0].tolist() == list(range(10)) + [-1] * 6 and count[0] == 10


def test_a_coincident_point_gets_almost_all_the_weight_and_no_nan():
    pts = np.array([[3, -1, 2], [4, -1, 2], [3, 1, 2]], dtype=np.float32)
    rows, count, d2, w, _ = rk.knn_query(pts[:1], None, None, pts, None, None, 1, 3, width=4)
    assert rows[0].tolist() == [0, 1, 2, -1] and d2[0].tolist() == [0, 1, 4, 0]
    r = np.array([np.float32(1) / np.float32(1e-8), 1 / (1 + np.float32(1e-8)), 1 / (2 + np.float32(1e-8))], dtype=np.float32)
    norm = (r[0] + r[1]) + r[2]
    assert np.isfinite(w).all() and w[0, 3] == 0
    np.testing.assert_array_equal(w[0, :3], r / norm)       # weight 1e8 / norm
    assert w[0, 0] > 0.9999999 and w[0, 1] < 2e-8


def test_invalid_queries_points_and_device_counts():
    pts, p_bid, q, q_bid = ss.base()
    q, q_bid, pts, p_bid = q[:60].copy(), q_bid[:60].copy(), pts.copy(), p_bid.copy()
    q[1, 0], q[2, 1], q[3, 2] = np.nan, np.inf, -np.inf
    q_bid[4], q_bid[5] = -1, ss.B
    near = rk.knn_query(q, q_bid, None, pts, p_bid, None, ss.B, 3)[0]
    pts[near[0, 0], 0], pts[near[0, 1], 2] = np.nan, np.inf                      # query 0 loses its two nearest points
    rows, count, d2, w, off = rk.knn_query(q, q_bid, 50, pts, p_bid, 3000, ss.B, 3, width=4)
    assert count[1:6].tolist() == [0] * 5 and (count[50:] == 0).all() and (rows[count == 0] == -1).all()
    assert (w[count == 0] == 0).all() and (d2[count == 0] == 0).all() and (off[count == 0] == 0).all()
    assert rows[0, 0] == near[0, 2] and rows.max() < 3000 and (rows[:, 3] == -1).all()
    assert (count[q_bid == 1][:5] == 3).sum() >= 1          # scene 1 keeps its 1000 rows below the device count
