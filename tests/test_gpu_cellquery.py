"""Cell-indexed ball query and radius-limited k-NN (csrc/cellquery.hip, ``F.point_cell_index`` / ``F.ball_query_cells`` /
``F.knn_query_cells``): every table equals a numpy float32 loop over all points -- every operation rounded on its own,
the ball / k-NN rule, points outside the range excluded -- exactly.  Coordinates sit on a lattice of multiples of 0.125
with index radius 0.5 (cell edge 0.5078125, exact), so d2 == r2 is hit on purpose and is not a hit.  Where every point
lies inside the range the tables also equal ``F.ball_query`` / ``F.knn_query`` on the device."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

R, V, RNG = 0.5, 0.5 * (1 + 2.0 ** -6), [0, 0, 0, 4, 4, 4]
f32 = np.float32


def reference(pts, pb, qs, qb, B, radius, n, knn, pad, n_points=None, n_queries=None, eps=1e-8, rng=RNG):
    """(rows, count, offsets, dist2, weights) of all queries by an all-points loop in float32"""
    p, q, N, M = pts[:, :3].astype(f32), qs[:, :3].astype(f32), len(pts), len(qs)
    r2, eps = f32(radius) * f32(radius), f32(eps)
    with np.errstate(invalid="ignore"):
        take = ((p >= f32(rng[:3])) & (p < f32(rng[3:]))).all(1)                  # (false for NaN, Inf is outside)
    take &= (np.arange(N) < (N if n_points is None else n_points)) & (pb >= 0) & (pb < B)
    rows, count = np.full((M, n), -1, np.int32), np.zeros(M, np.int32)
    off, dist2, wts = np.zeros((M, n, 3), f32), np.zeros((M, n), f32), np.zeros((M, n), f32)
    for m in range(M if n_queries is None else n_queries):
        ok = np.isfinite(q[m]).all() if knn else not np.isnan(q[m]).any()
        if not (ok and 0 <= qb[m] < B):
            continue
        with np.errstate(invalid="ignore", over="ignore"):
            d = p - q[m]
            s = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]                             # every operation rounded on its own
            s = s + d[:, 2] * d[:, 2]
            hit = np.flatnonzero(take & (pb == qb[m]) & (s < r2))                 # ascending index
        if knn:
            hit = hit[np.lexsort((hit, s[hit]))]                                  # the total order (d2, index)
        hit = hit[:n]
        c = count[m] = len(hit)
        rows[m, :c], off[m, :c], dist2[m, :c] = hit, d[hit], s[hit]
        if knn and c:
            r = f32(1) / (np.sqrt(s[hit]) + eps)
            norm = r[0]
            for v in r[1:]:
                norm = norm + v                                                   # ascending slot
            wts[m, :c] = r / norm
        if pad == "first" and c:
            rows[m, c:], off[m, c:], dist2[m, c:] = rows[m, 0], off[m, 0], dist2[m, 0]
    return rows, count, off, dist2, wts


def dev(cuda, a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def same(got, want, knn):
    rows, count, off, dist2, wts = want
    np.testing.assert_array_equal(got.rows.cpu().numpy(), rows)
    np.testing.assert_array_equal(got.count.cpu().numpy(), count)
    np.testing.assert_array_equal(got.offsets.cpu().numpy().view(np.uint32), off.view(np.uint32))
    if knn:
        np.testing.assert_array_equal(got.dist2.cpu().numpy().view(np.uint32), dist2.view(np.uint32))
        np.testing.assert_array_equal(got.weights.cpu().numpy().view(np.uint32), wts.view(np.uint32))


def check(cuda, pts, pb, qs, qb, B, radius, n, k, pad, n_points=None, n_queries=None, brute=False):
    """both queries over one index of radius R against the reference (and the brute-force kernels); the counts"""
    from spconv_amd.pytorch import functional as F
    count = lambda v: None if v is None else torch.tensor([v], dtype=torch.int32, device=cuda)
    P, PB, Q, QB, npd, nqd = dev(cuda, pts), dev(cuda, pb), dev(cuda, qs), dev(cuda, qb), count(n_points), count(n_queries)
    index = F.point_cell_index(P, PB, B, R, RNG, n_points=npd)
    ball = F.ball_query_cells(Q, QB, index, radius, n, pad=pad, with_offsets=True, n_queries=nqd)
    knn = F.knn_query_cells(Q, QB, index, k, radius, pad=pad, with_offsets=True, n_queries=nqd)
    want_ball = reference(pts, pb, qs, qb, B, radius, n, False, pad, n_points, n_queries)
    want_knn = reference(pts, pb, qs, qb, B, radius, k, True, pad, n_points, n_queries)
    same(ball, want_ball, False)
    same(knn, want_knn, True)
    if brute:           # every point inside the range: the brute-force kernels give the same tables
        b = F.ball_query(Q, QB, P, PB, B, radius, n, pad=pad, with_offsets=True, n_queries=nqd, n_points=npd)
        assert torch.equal(b.rows, ball.rows) and torch.equal(b.count, ball.count) and torch.equal(b.offsets, ball.offsets)
        kb = F.knn_query(Q, QB, P, PB, B, k, with_offsets=True, n_queries=nqd, n_points=npd)
        inside = (kb.dist2 < np.float32(radius) ** 2) & (kb.rows >= 0)            # the leading entries inside the radius
        if pad == "none":
            assert torch.equal(torch.where(inside, kb.rows, -1), knn.rows) and torch.equal(inside.sum(1).int(), knn.count)
    return want_ball[1], want_knn[1]


def test_stencil_edges(cuda):
    """scene s < 27: a query near the faces of cell (3, 3, 3) that direction s crosses, a partner in the neighbour cell
    inside the radius and one two cells away; scene 27: points one ulp round a cell boundary, d2 == r2, and queries
    outside the range by less than r, in a corner cell, and by more than a cell"""
    pts, pb, qs, qb = [], [], [], []
    near, step = {-1: 1.625, 0: 1.75, 1: 2.0}, {-1: -0.25, 0: 0.0, 1: 0.25}      # cell 3 = [1.5234375, 2.03125)
    for s, dirs in enumerate(np.ndindex(3, 3, 3)):
        dirs = [v - 1 for v in dirs]
        q = [near[v] for v in dirs]
        assert all(int(f32(v) / f32(V)) == 3 for v in q)
        qs.append(q)
        pts += [[a + step[v] for a, v in zip(q, dirs)], [a + 1.125 * v for a, v in zip(q, dirs)]]
        pb += [s, s]
        qb.append(s)
    edge = f32(4 * V)                                                             # 2.03125: cells 3 | 4
    for axis in range(3):
        for x in (np.nextafter(edge, f32(0)), edge, np.nextafter(edge, f32(9))):
            p = [1.75, 1.75, 1.75]
            p[axis] = x
            pts.append(p)
        for x in (edge - f32(0.375), edge + f32(0.375), edge - f32(0.5), edge + f32(0.5)):
            q = [1.75, 1.75, 1.75]
            q[axis] = x
            qs.append(q)
    pts += [[0.125, 1.75, 1.75], [3.875, 3.875, 3.875], [3.875, 0.0, 0.0], [0.75, 3.0, 3.0], [1.5, 3.0, 3.0]]
    qs += [[-0.25, 1.75, 1.75], [-1.0, 1.75, 1.75], [4.125, 4.125, 4.125], [4.25, 3.875, 3.875], [4.25, -0.125, -0.125],
           [100.0, 100.0, 100.0], [-100.0, 1.75, 1.75], [1.25, 3.0, 3.0]]         # (the last: d2 == r2 on one side)
    pb += [27] * (len(pts) - len(pb))
    qb += [27] * (len(qs) - len(qb))
    pts, qs, pb, qb = np.array(pts, f32), np.array(qs, f32), np.array(pb, np.int32), np.array(qb, np.int32)
    cb, ck = check(cuda, pts, pb, qs, qb, 28, R, 4, 4, "none", brute=True)
    want = np.where(np.arange(27) == 13, 2, 1)               # the partner, never the far point (direction 0: both are q)
    assert (cb[:27] == want).all() and (ck[:27] == want).all()
    assert list(cb[-8:]) == [1, 0, 1, 1, 1, 0, 0, 1]


@pytest.mark.parametrize("pad", ["none", "first"])
@pytest.mark.parametrize("n,k", [(1, 1), (16, 16), (128, 64)])
def test_selection(cuda, n, k, pad):
    """300 points (64 places: duplicates) of one cell in shuffled index order, 16 on one place elsewhere, a few round
    them: runs longer than a step and than the incoming half, so several compactions and the gate run; the hits of the
    three queries exceed, equal (16) and fall short of nsample"""
    gen = np.random.default_rng(5)
    pts = np.concatenate([1.625 + 0.125 * gen.integers(0, 4, (300, 3)), np.full((16, 3), 3.5),
                          1.0 + 0.125 * gen.integers(0, 16, (40, 3))]).astype(f32)
    pts = pts[gen.permutation(len(pts))]
    qs = np.array([[1.75, 1.75, 1.75], [3.625, 3.5, 3.5], [2.375, 2.0, 2.0], [0.25, 0.25, 0.25]], f32)
    zeros = lambda a: np.zeros(len(a), np.int32)
    cb, ck = check(cuda, pts, zeros(pts), qs, zeros(qs), 1, R, n, k, pad, brute=True)
    assert cb[0] == n and ck[0] == k and cb[1] == min(n, 16) and cb[3] == 0


@pytest.mark.parametrize("radius", [0.5, 0.25])
def test_wave_mix(cuda, radius):
    """70 queries (no multiple of 4 or 16) over 2000 points in 3 scenes, a dense blob among them: the groups of a wave
    get runs of 0 to hundreds of records; foreign and negative batch ids, NaN / Inf points and queries, points outside
    the range, device counts below the sizes, a query radius under the index's"""
    gen = np.random.default_rng(11)
    pts = (0.125 * gen.integers(-4, 36, (2000, 3))).astype(f32)
    pts[:500] = (1.0 + 0.125 * gen.integers(0, 5, (500, 3))).astype(f32)
    pb = gen.integers(0, 3, 2000).astype(np.int32)
    pb[gen.integers(0, 2000, 40)] = gen.choice([-1, 3, 7], 40)
    pts[gen.integers(0, 2000, 20), gen.integers(0, 3, 20)] = gen.choice([np.nan, np.inf, -np.inf], 20)
    qs = (0.125 * gen.integers(-6, 38, (70, 3))).astype(f32)
    qs[:12] = (1.0 + 0.125 * gen.integers(0, 5, (12, 3))).astype(f32)
    qb = gen.integers(0, 3, 70).astype(np.int32)
    qb[[5, 30]], qs[7, 1], qs[8, 0], qs[9, 2] = [-2, 3], np.nan, np.inf, -np.inf
    order = gen.permutation(2000)
    cb, _ = check(cuda, pts[order], pb[order], qs, qb, 3, radius, 32, 16, "first", n_points=1900, n_queries=66)
    assert cb.max() == 32 and (cb == 0).sum() >= 6 and len(set(cb)) > 6


def test_capture_replays(cuda):
    """index build, both queries and group_voxels captured once; replayed with a second cloud and smaller device counts"""
    from spconv_amd.pytorch import functional as F
    N, M, n, k, gen = 1500, 50, 16, 8, np.random.default_rng(3)
    clouds = [(0.125 * gen.integers(0, 32, (N, 3))).astype(f32) for _ in range(2)]
    queries = [(0.125 * gen.integers(-2, 34, (M, 3))).astype(f32) for _ in range(2)]
    feat = gen.standard_normal((N, 5)).astype(f32)
    plan = F.cluster_plan(R, RNG, 1)
    buf = F.cell_index_buffers(N, plan, cuda)
    i32 = dict(dtype=torch.int32, device=cuda)
    pts, qs, feats = torch.zeros((N, 3), device=cuda), torch.zeros((M, 3), device=cuda), dev(cuda, feat)
    n_dev, m_dev = torch.zeros((1,), **i32), torch.zeros((1,), **i32)
    rows, cnt, krows, kcnt = torch.empty((M, n), **i32), torch.empty((M,), **i32), torch.empty((M, k), **i32), torch.empty((M,), **i32)
    off, kd2 = torch.empty((M, n, 3), device=cuda), torch.empty((M, k), device=cuda)
    r2 = np.float32(R) ** 2

    def run():
        index = F.point_cell_index_into(pts, None, n_dev, plan, buf)
        F.ball_query_cells_into(qs, None, m_dev, index, n, r2, False, rows, cnt, off)
        F.knn_query_cells_into(qs, None, m_dev, index, k, r2, 1e-8, False, krows, kcnt, kd2)
        return F.group_voxels(feats, F.VoxelNeighbors(rows, cnt, off, None, N, m_dev, n_dev))
    run()                                                          # (modules loaded before the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        grouped = run()
    zeros = lambda a: np.zeros(len(a), np.int32)
    for cloud, query, np_, nq in zip(clouds, queries, (N, N - 211), (M, M - 7)):
        pts.copy_(dev(cuda, cloud))
        qs.copy_(dev(cuda, query))
        n_dev.fill_(np_)
        m_dev.fill_(nq)
        graph.replay()
        torch.cuda.synchronize()
        want = reference(cloud, zeros(cloud), query, zeros(query), 1, R, n, False, "none", np_, nq)
        kwant = reference(cloud, zeros(cloud), query, zeros(query), 1, R, k, True, "none", np_, nq)
        np.testing.assert_array_equal(rows.cpu().numpy(), want[0])
        np.testing.assert_array_equal(cnt.cpu().numpy(), want[1])
        np.testing.assert_array_equal(off.cpu().numpy(), want[2])
        np.testing.assert_array_equal(krows.cpu().numpy(), kwant[0])
        np.testing.assert_array_equal(kd2.cpu().numpy(), kwant[3])
        np.testing.assert_array_equal(grouped.cpu().numpy(), np.where(want[0][..., None] >= 0, feat[want[0]], 0))


def test_modules_take_the_cell_path(cuda):
    """BallQueryAndGroup / KNNQueryAndGroup with coors_range_xyz equal the brute-force modules inside the range"""
    import spconv_amd.pytorch as spconv
    gen = np.random.default_rng(9)
    pts = dev(cuda, (1.0 + 0.125 * gen.integers(0, 16, (2000, 3))).astype(f32))
    qs = dev(cuda, (1.5 + 0.125 * gen.integers(0, 9, (41, 3))).astype(f32))
    pb, qb = dev(cuda, gen.integers(0, 2, 2000).astype(np.int32)), dev(cuda, gen.integers(0, 2, 41).astype(np.int32))
    feats = dev(cuda, gen.standard_normal((2000, 6)).astype(f32))
    out, count = spconv.BallQueryAndGroup(R, 16, coors_range_xyz=RNG)(pts, pb, feats, qs, qb, 2)
    want, wcount = spconv.BallQueryAndGroup(R, 16)(pts, pb, feats, qs, qb, 2)
    assert torch.equal(out, want) and torch.equal(count, wcount) and int(count.max()) == 16
    # 125 points per unit of volume and every query half a unit inside the cloud: the 4 nearest lie inside the radius
    out, count = spconv.KNNQueryAndGroup(4, radius=R, coors_range_xyz=RNG)(pts, pb, feats, qs, qb, 2)
    want, wcount = spconv.KNNQueryAndGroup(4)(pts, pb, feats, qs, qb, 2)
    assert torch.equal(out, want) and torch.equal(count, wcount) and int(count.min()) == 4
