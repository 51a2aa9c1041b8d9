"""CPU: the numpy restatement tests/refsample.py -- what the kernels of csrc/sample.hip are held to bit for bit -- against
independent formulations: the ball query against float64 distances over all points (filtered, index-sorted, truncated),
farthest-point sampling against the property that defines every step (a chain in float64 would diverge at the first
near-tie), and integer-lattice clouds on which float32 is exact."""
import numpy as np

import refsample as rs
import samplescenes as ss


def test_ball_query_against_float64_distances():
    pts, p_bid, q, q_bid = ss.base()
    rows, count, offsets, hits = ss.base_ball()
    r2 = float(np.float32(ss.RADIUS) * np.float32(ss.RADIUS))
    ambiguous = 0
    for m in range(ss.M):
        d2 = ((pts[:, :3].astype(np.float64) - q[m].astype(np.float64)) ** 2).sum(axis=1)
        d2[p_bid != q_bid[m]] = np.inf
        if (np.abs(d2 - r2) <= 1e-6 * r2).any():
            ambiguous += 1
            continue
        want = np.nonzero(d2 < r2)[0]                               # ascending point index
        assert hits[m] == len(want)
        k = min(len(want), ss.NSAMPLE)
        assert count[m] == k
        np.testing.assert_array_equal(rows[m, :k], want[:k])
        assert (rows[m, k:] == -1).all() and (offsets[m, k:] == 0).all()
        np.testing.assert_allclose(offsets[m, :k], pts[want[:k], :3].astype(np.float64) - q[m], rtol=0, atol=1e-6)
    assert ambiguous <= ss.M // 100, ambiguous                      # the cap is a condition
    truncated, partial, empty = (hits > ss.NSAMPLE).sum(), ((hits > 0) & (hits <= ss.NSAMPLE)).sum(), (hits == 0).sum()
    assert min(truncated, partial, empty) >= 100, (truncated, partial, empty)
    assert (hits[ss.M - ss.M_FAR:] == 0).all()


def test_ball_query_padding_and_invalid_queries():
    pts, p_bid, q, q_bid = ss.base()
    rows, count, offsets, _ = ss.base_ball()
    prow, pcount, poff, _ = ss.base_ball(pad="first")
    np.testing.assert_array_equal(pcount, count)
    for m in range(ss.M):
        k = count[m]
        np.testing.assert_array_equal(prow[m, :k], rows[m, :k])
        if k:
            assert (prow[m, k:] == rows[m, 0]).all() and (poff[m, k:] == offsets[m, 0]).all()
        else:
            assert (prow[m] == -1).all() and (poff[m] == 0).all()
    bad_q = q.copy()
    bad_q[::3, 1] = np.nan
    bad_bid = q_bid.copy()
    bad_bid[1::3] = ss.B
    bad_bid[4::6] = -1
    r = rs.ball_query(bad_q, bad_bid, 500, pts, p_bid, None, ss.B, ss.RADIUS, ss.NSAMPLE)
    dead = np.isnan(bad_q).any(axis=1) | (bad_bid < 0) | (bad_bid >= ss.B) | (np.arange(ss.M) >= 500)
    assert (r[1][dead] == 0).all() and (r[0][dead] == -1).all()
    np.testing.assert_array_equal(r[0][~dead], rows[~dead])
    # points behind a count, with bad ids or coordinates are never hits
    bad_pts = pts.copy()
    bad_pts[5::7, 2] = np.inf
    bad_pts[6::7, 0] = np.nan
    bad_pid = p_bid.copy()
    bad_pid[3::7] = -1
    r = rs.ball_query(q, q_bid, None, bad_pts, bad_pid, 3500, ss.B, ss.RADIUS, ss.NSAMPLE)
    got = r[0][r[0] >= 0]
    assert len(got) > 1000 and got.max() < 3500
    assert np.isfinite(bad_pts[got, :3]).all() and (bad_pid[got] >= 0).all()


def test_fps_every_step_takes_a_farthest_point():
    pts, p_bid, _, _ = ss.base()
    K = 256
    idx, count = rs.fps(pts, p_bid, ss.B, K)
    assert (count == K).all()
    xyz = pts[:ss.N_SCENE, :3].astype(np.float64)
    chosen = idx[0]
    assert chosen[0] == 0 and len(set(chosen.tolist())) == K and chosen.max() < ss.N_SCENE
    shortfall = 0.0
    mind = np.full(ss.N_SCENE, np.inf)
    for s in range(1, K):
        mind = np.minimum(mind, np.sqrt(((xyz - xyz[chosen[s - 1]]) ** 2).sum(axis=1)))
        rest = np.ones(ss.N_SCENE, dtype=bool)
        rest[chosen[:s]] = False
        assert rest[chosen[s]]                                      # not chosen before
        best = mind[rest].max()
        assert mind[chosen[s]] >= (1 - 1e-5) * best, (s, mind[chosen[s]], best)
        shortfall = max(shortfall, 1.0 - mind[chosen[s]] / best)
    print("largest shortfall over", K - 1, "steps:", shortfall)
    assert (idx[1] >= ss.N_SCENE).all() and len(set(idx[1].tolist())) == K


def test_fps_scenes_counts_and_invalid_points():
    pts, p_bid, _, _ = ss.base()
    # a scene is its points in ascending index: an order-preserving interleave leaves the sampled POINTS unchanged
    new_pts, new_bid, _ = ss.interleaved(pts, p_bid)
    assert (np.diff(new_bid) != 0).sum() > 1000
    a, ca = rs.fps(pts, p_bid, ss.B, 64)
    b, cb = rs.fps(new_pts, new_bid, ss.B, 64)
    np.testing.assert_array_equal(ca, cb)
    np.testing.assert_array_equal(pts[a.reshape(-1)], new_pts[b.reshape(-1)])
    # K beyond the valid points, bad ids, bad coordinates, a count
    few = pts[:40].copy()
    bid = np.zeros(40, dtype=np.int32)
    bid[10:20] = 1
    bid[3], bid[4] = -1, 2
    few[0, 0], few[5, 2] = np.nan, np.inf
    idx, count = rs.fps(few, bid, 2, 32, n_points=30)
    assert count.tolist() == [30 - 10 - 4, 10]
    assert idx[0, 0] == 1 and not set(idx[0, :16].tolist()) & {0, 3, 4, 5} and (idx[0, 16:] == -1).all()
    assert sorted(idx[1, :10].tolist()) == list(range(10, 20)) and idx[1, 0] == 10


def test_exact_lattice_cases():
    idx, count = rs.fps(ss.TIE_POINTS, None, 1, 6)
    assert idx[0].tolist() == ss.TIE_ORDER and count[0] == 6       # ties: the lowest index
    idx, count = rs.fps(ss.TIE_POINTS[:, :2], None, 1, 8, ndim=2)
    assert idx[0].tolist() == ss.TIE_ORDER + [-1, -1] and count[0] == 6
    rows, count, offsets, hits = rs.ball_query(np.zeros((1, 3), dtype=np.float32), None, None, ss.EDGE_POINTS, None, None,
                                               1, 2.0, 8)
    assert rows[0, :3].tolist() == ss.EDGE_HITS and count[0] == 3 and hits[0] == 3     # d2 == r2 is outside
    np.testing.assert_array_equal(offsets[0, :3], ss.EDGE_POINTS[ss.EDGE_HITS])
    idx, count = rs.fps(ss.DUPLICATES, None, 1, 6)
    assert idx[0].tolist() == [0, 1, 2, 3, 4, 5] and count[0] == 6 # duplicates: distinct, ascending indices
    idx, count = rs.fps(ss.DUPLICATES, None, 1, 16)
    assert idx[0].tolist() == list(range(10)) + [-1] * 6 and count[0] == 10
