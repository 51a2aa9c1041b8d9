"""Farthest-point sampling and ball query over raw points on the kernels of csrc/sample.hip (spconv_amd/pytorch/_sample.py,
spatial.FarthestPointSample / BallQueryAndGroup) against the numpy restatement tests/refsample.py, over the clouds of
tests/samplescenes.py (whose conditions test_refsample.py asserts on the CPU).

Every comparison is bit for bit: indices and counts are integers, the offsets float32 arithmetic in which numpy rounds
every operation on its own (the contract), the gather moves rows unchanged, and the gradient is a sequential float32 sum
in ascending entry that numpy reproduces.  The one tolerance is gradcheck's own, in float64."""
import numpy as np
import pytest
import torch

import refquery as rq
import refsample as rs
import samplescenes as ss

pytestmark = pytest.mark.gpu

DTYPES = {"f16": torch.float16, "f32": torch.float32}


def bits(t):
    t = t.detach().cpu().contiguous()
    return t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()]).numpy()


def dev(cuda, a):
    return None if a is None else torch.from_numpy(np.array(a, order="C")).to(cuda)


def count_of(cuda, n):
    return None if n is None else torch.tensor([n], dtype=torch.int32, device=cuda)


def cloud(sizes, seed, extent=4.0, nfeat=4):
    """scene-contiguous uniform points in [0, extent)^3 with `sizes` points per scene"""
    rng = np.random.default_rng(seed)
    n = int(sum(sizes))
    pts = (rng.random((n, nfeat)) * extent).astype(np.float32)
    bid = np.repeat(np.arange(len(sizes), dtype=np.int32), sizes)
    return pts, bid


def run_fps(cuda, pts, bid, B, K, ndim=3, n_points=None):
    from spconv_amd import _lib
    from spconv_amd.pytorch import functional as F
    before = _lib.load().spx_launch_count(b"sample/fps")
    s = F.farthest_point_sample(dev(cuda, pts), dev(cuda, bid), B, K, ndim=ndim, n_points=count_of(cuda, n_points))
    assert _lib.load().spx_launch_count(b"sample/fps") == before + 1
    assert s.idx.dtype == torch.int32 and tuple(s.idx.shape) == (B, K) and tuple(s.count.shape) == (B,)
    np.testing.assert_array_equal(s.batch_ids.cpu().numpy(), np.repeat(np.arange(B, dtype=np.int32), K))
    return s


def assert_fps(s, want):
    np.testing.assert_array_equal(s.count.cpu().numpy(), want[1])
    np.testing.assert_array_equal(s.idx.cpu().numpy(), want[0])


# ------------------------------------------------------------------------------------------------ farthest-point sampling

@pytest.mark.parametrize("K", [1, 2, 64, 257])
@pytest.mark.parametrize("valid", [(0, 1, 2), (63, 64, 65), (1023, 1024, 1025), (65, 0, 1024)])
def test_fps_three_scenes_bit_for_bit(cuda, valid, K):
    """three scenes in one call; every scene with points carries three invalid ones as well (NaN, +inf, -inf), so the
    valid counts are the listed ones and K exceeds some of them"""
    sizes = [v + 3 if v else 0 for v in valid]
    pts, bid = cloud(sizes, 100 + sum(valid))
    start = 0
    for n in sizes:
        if n:
            pts[start + 1, 0], pts[start + n // 2, 2], pts[start + n - 1, 1] = np.nan, np.inf, -np.inf
        start += n
    want = rs.fps(pts, bid, 3, K)
    assert want[1].tolist() == [min(v, K) for v in valid]
    assert_fps(run_fps(cuda, pts, bid, 3, K), want)


@pytest.mark.parametrize("ndim", [3, 2])
def test_fps_both_tiers_and_the_boundary(cuda, ndim):
    """a scene of exactly resident_points() points stays in registers, one of a point more streams staged records"""
    from spconv_amd.pytorch import _sample
    R = _sample.resident_points()
    pts, bid = cloud([R, R + 1, 7], 7 + ndim, extent=50.0, nfeat=ndim + 1)
    pts[5, 0], pts[R + 9, 1] = np.nan, np.inf
    want = rs.fps(pts, bid, 3, 64, ndim)
    assert want[1].tolist() == [64, 64, 7]
    s = run_fps(cuda, pts, bid, 3, 64, ndim)
    assert_fps(s, want)
    again = run_fps(cuda, pts, bid, 3, 64, ndim)
    assert torch.equal(s.idx, again.idx) and torch.equal(s.count, again.count)


def test_fps_interleaved_scenes_equal_the_contiguous_cloud(cuda):
    pts, bid, _, _ = ss.base()
    new_pts, new_bid, new_row = ss.interleaved(pts, bid)
    a = run_fps(cuda, pts, bid, ss.B, 128)
    assert_fps(a, rs.fps(pts, bid, ss.B, 128))
    b = run_fps(cuda, new_pts, new_bid, ss.B, 128)
    np.testing.assert_array_equal(b.idx.cpu().numpy(), new_row[a.idx.cpu().numpy()])
    again = run_fps(cuda, pts, bid, ss.B, 128)
    assert torch.equal(a.idx, again.idx) and torch.equal(a.count, again.count)       # identical run to run


def test_fps_never_samples_what_is_no_point(cuda):
    pts, bid, _, _ = ss.base()
    pts, bid = pts.copy(), bid.copy()
    live = len(pts) - 300                                            # 300 plausible rows behind the device count
    bid[3::11], bid[4::11] = -1, ss.B
    pts[5::11, 0], pts[6::11, 2], pts[0, 1] = np.nan, np.inf, -np.inf
    want = rs.fps(pts, bid, ss.B, 200, n_points=live)
    s = run_fps(cuda, pts, bid, ss.B, 200, n_points=live)
    assert_fps(s, want)
    got = s.idx.cpu().numpy().reshape(-1)
    assert got.min() >= 1 and got.max() < live and np.isfinite(pts[got, :3]).all()
    assert (np.repeat(np.arange(ss.B), 200) == bid[got]).all()
    # a scene whose points are all invalid, and no batch ids at all
    bad = pts[:50].copy()
    bad[:, 1] = np.nan
    assert_fps(run_fps(cuda, bad, None, 1, 8), (np.full((1, 8), -1, dtype=np.int32), np.zeros(1, dtype=np.int32)))
    assert_fps(run_fps(cuda, pts[:500], None, 1, 33), rs.fps(pts[:500], None, 1, 33))


def test_fps_exact_lattice_cases(cuda):
    s = run_fps(cuda, ss.TIE_POINTS, None, 1, 6)
    assert s.idx.cpu().numpy()[0].tolist() == ss.TIE_ORDER and int(s.count[0]) == 6
    s = run_fps(cuda, np.ascontiguousarray(ss.TIE_POINTS[:, :2]), None, 1, 8, ndim=2)
    assert s.idx.cpu().numpy()[0].tolist() == ss.TIE_ORDER + [-1, -1] and int(s.count[0]) == 6
    s = run_fps(cuda, ss.DUPLICATES, None, 1, 6)
    assert s.idx.cpu().numpy()[0].tolist() == [0, 1, 2, 3, 4, 5] and int(s.count[0]) == 6
    s = run_fps(cuda, ss.DUPLICATES, None, 1, 16)
    assert s.idx.cpu().numpy()[0].tolist() == list(range(10)) + [-1] * 6 and int(s.count[0]) == 10


def test_gather_samples_fills_dead_slots_with_nan(cuda):
    from spconv_amd.pytorch import functional as F
    pts, bid = cloud([5, 0, 40], 3)
    s = run_fps(cuda, pts, bid, 3, 8)
    rows = F.gather_samples(dev(cuda, pts), s)
    idx = s.idx.cpu().numpy().reshape(-1)
    want = np.where((idx >= 0)[:, None], pts[np.clip(idx, 0, None)], np.float32(np.nan))
    assert tuple(rows.shape) == (24, 4) and int((idx < 0).sum()) == 3 + 8
    np.testing.assert_array_equal(bits(rows)[idx >= 0], want.view(np.int32)[idx >= 0])
    assert bool(torch.isnan(rows[torch.from_numpy(idx < 0).to(cuda)]).all())


# ------------------------------------------------------------------------------------------------ ball query

def run_ball(cuda, q, q_bid, pts, p_bid, B, radius, nsample, ndim=3, pad="none", with_offsets=True, n_queries=None,
             n_points=None, with_groups=False):
    from spconv_amd import _lib
    from spconv_amd.pytorch import functional as F
    before = _lib.load().spx_launch_count(b"sample/ball_query")
    nb = F.ball_query(dev(cuda, q), dev(cuda, q_bid), dev(cuda, pts), dev(cuda, p_bid), B, radius, nsample, ndim=ndim,
                      pad=pad, with_offsets=with_offsets, n_queries=count_of(cuda, n_queries),
                      n_points=count_of(cuda, n_points), with_groups=with_groups)
    assert _lib.load().spx_launch_count(b"sample/ball_query") == before + (1 if len(q) else 0)
    assert nb.num_voxels == len(pts) and tuple(nb.rows.shape) == (len(q), nsample)
    return nb


def assert_neighbors(nb, want):
    rows, count, offsets = want[:3]
    assert nb.rows.dtype == torch.int32 and nb.count.dtype == torch.int32
    np.testing.assert_array_equal(nb.count.cpu().numpy(), count)
    np.testing.assert_array_equal(nb.rows.cpu().numpy(), rows)
    if nb.offsets is not None:
        assert nb.offsets.dtype == torch.float32 and tuple(nb.offsets.shape) == offsets.shape
        np.testing.assert_array_equal(bits(nb.offsets), offsets.view(np.int32))


@pytest.mark.parametrize("with_offsets", [True, False])
@pytest.mark.parametrize("pad", ["none", "first"])
@pytest.mark.parametrize("nsample", [1, 16, 128])
def test_ball_query_base_scene_bit_for_bit(cuda, nsample, pad, with_offsets):
    pts, p_bid, q, q_bid = ss.base()
    nb = run_ball(cuda, q, q_bid, pts, p_bid, ss.B, ss.RADIUS, nsample, pad=pad, with_offsets=with_offsets)
    assert (nb.offsets is not None) == with_offsets and nb.groups is None
    assert_neighbors(nb, ss.base_ball(nsample, pad))


def test_ball_query_scene_sizes_around_the_tile(cuda):
    """scenes whose last tile is partial, that fit one tile exactly-but-one, and that span several tiles"""
    sizes = [1, 63, 64, 65, 1023, 1025, 4097]
    pts, p_bid = cloud(sizes, 11)
    rng = np.random.default_rng(12)
    q_bid = np.sort(rng.integers(0, len(sizes), 700)).astype(np.int32)
    q = (rng.random((700, 3)) * 4.0).astype(np.float32)
    first = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    q[::5] = pts[first[q_bid[::5]], :3] + np.float32(0.01)          # (near a point of its scene: the small scenes hit too)
    want = rs.ball_query(q, q_bid, None, pts, p_bid, None, len(sizes), 0.5, 16)
    hit_scenes = set(q_bid[want[1] > 0].tolist())
    assert hit_scenes == set(range(len(sizes))) and (want[3] > 16).sum() > 50 and (want[1] == 0).sum() > 50
    nb = run_ball(cuda, q, q_bid, pts, p_bid, len(sizes), 0.5, 16)
    assert_neighbors(nb, want)
    # the last point of every scene is found from itself: a partial tile is read to its end
    last = (np.cumsum(sizes) - 1).astype(np.int64)
    scene = np.arange(len(sizes), dtype=np.int32)
    want = rs.ball_query(pts[last, :3], scene, None, pts, p_bid, None, len(sizes), 0.5, 128)
    assert all(last[b] in want[0][b] for b in range(len(sizes)))
    assert_neighbors(run_ball(cuda, pts[last, :3], scene, pts, p_bid, len(sizes), 0.5, 128), want)


def test_ball_query_does_not_depend_on_the_order_across_scenes(cuda):
    pts, p_bid, q, q_bid = ss.base()
    want = ss.base_ball(ss.NSAMPLE, "first")
    order = np.argsort(q_bid, kind="stable")                        # scene-contiguous queries
    nb = run_ball(cuda, q[order], q_bid[order], pts, p_bid, ss.B, ss.RADIUS, ss.NSAMPLE, pad="first")
    assert_neighbors(nb, tuple(w[order] for w in want[:3]))
    perm = np.random.default_rng(5).permutation(ss.M)               # shuffled queries
    nb = run_ball(cuda, q[perm], q_bid[perm], pts, p_bid, ss.B, ss.RADIUS, ss.NSAMPLE, pad="first")
    assert_neighbors(nb, tuple(w[perm] for w in want[:3]))
    new_pts, new_bid, new_row = ss.interleaved(pts, p_bid)          # interleaved points: the same points, renumbered
    nb = run_ball(cuda, q, q_bid, new_pts, new_bid, ss.B, ss.RADIUS, ss.NSAMPLE, pad="first")
    rows = np.where(want[0] >= 0, new_row[np.clip(want[0], 0, None)], -1).astype(np.int32)
    assert_neighbors(nb, (rows, want[1], want[2]))


def test_ball_query_device_counts_and_invalid_rows(cuda):
    pts, p_bid, q, q_bid = ss.base()
    bad_q, bad_bid = q.copy(), q_bid.copy()
    bad_q[::3, 1] = np.nan
    bad_q[1::11, 0], bad_q[2::11, 2], bad_q[3::11] = np.inf, -np.inf, np.inf     # (the reference turns down NaN only)
    bad_bid[1::7], bad_bid[4::9] = ss.B, -1
    bad_pts, bad_pid = pts.copy(), p_bid.copy()
    bad_pts[5::7, 2], bad_pts[6::7, 0] = np.inf, np.nan
    bad_pid[3::7], bad_pid[2::13] = -1, ss.B
    want = rs.ball_query(bad_q, bad_bid, 500, bad_pts, bad_pid, 3500, ss.B, ss.RADIUS, ss.NSAMPLE, 3, "first")
    nb = run_ball(cuda, bad_q, bad_bid, bad_pts, bad_pid, ss.B, ss.RADIUS, ss.NSAMPLE, pad="first", n_queries=500,
                  n_points=3500)
    assert_neighbors(nb, want)
    assert nb.n_queries is not None and nb.n_live is not None
    dead = ~np.isfinite(bad_q[:, :3]).all(axis=1) | (bad_bid < 0) | (bad_bid >= ss.B) | (np.arange(ss.M) >= 500)
    assert dead.sum() > 300 and bool((nb.count[torch.from_numpy(dead).to(cuda)] == 0).all())
    assert int(nb.rows.max()) < 3500 and int((nb.count > 0).sum()) > 100
    # an infinite radius: a query with an infinite coordinate still finds nothing (its d2 is +inf or NaN, never < r2)
    want = rs.ball_query(bad_q, bad_bid, 500, bad_pts, bad_pid, 3500, ss.B, float("inf"), ss.NSAMPLE, 3, "first")
    nb = run_ball(cuda, bad_q, bad_bid, bad_pts, bad_pid, ss.B, float("inf"), ss.NSAMPLE, pad="first", n_queries=500,
                  n_points=3500)
    assert_neighbors(nb, want)
    assert bool((nb.count[torch.from_numpy(dead).to(cuda)] == 0).all()) and int((nb.count > 0).sum()) > 100


def test_ball_query_exact_lattice_and_empty_cases(cuda):
    from spconv_amd.pytorch import functional as F
    zero = np.zeros((1, 3), dtype=np.float32)
    nb = run_ball(cuda, zero, None, ss.EDGE_POINTS, None, 1, 2.0, 8)
    assert nb.rows.cpu().numpy()[0, :3].tolist() == ss.EDGE_HITS and int(nb.count[0]) == 3      # d2 == r2 is outside
    assert_neighbors(nb, rs.ball_query(zero, None, None, ss.EDGE_POINTS, None, None, 1, 2.0, 8))
    nb = run_ball(cuda, zero[:, :2], None, np.ascontiguousarray(ss.EDGE_POINTS[:, :2]), None, 1, 2.0, 8, ndim=2)
    assert_neighbors(nb, rs.ball_query(zero[:, :2], None, None, ss.EDGE_POINTS[:, :2], None, None, 1, 2.0, 8, 2))
    pts, p_bid, q, q_bid = ss.base()
    none = run_ball(cuda, q[:0], q_bid[:0], pts, p_bid, ss.B, ss.RADIUS, 16, with_groups=True)          # M = 0
    assert tuple(none.rows.shape) == (0, 16) and tuple(none.count.shape) == (0,) and none.groups is None
    assert tuple(F.group_voxels(dev(cuda, pts), none).shape) == (0, 16, 4)
    # an empty scene between two others: its queries find nothing, the others are unchanged
    three = np.where(p_bid == 1, 2, 0).astype(np.int32)
    q3 = np.where(q_bid == 1, 2, 0).astype(np.int32)
    q3[::4] = 1
    want = rs.ball_query(q, q3, None, pts, three, None, 3, ss.RADIUS, 16)
    assert (want[1][q3 == 1] == 0).all() and (want[1][q3 != 1] > 0).sum() > 100
    assert_neighbors(run_ball(cuda, q, q3, pts, three, 3, ss.RADIUS, 16), want)
    nb = run_ball(cuda, q, None, pts[:0], None, 1, ss.RADIUS, 16)                                       # no points at all
    assert bool((nb.rows == -1).all()) and bool((nb.count == 0).all()) and bool((nb.offsets == 0).all())


# ------------------------------------------------------------------------------------------------ grouping

@pytest.fixture(scope="module")
def main(cuda):
    """the base scene on the device, empty slots left at -1, groups built (shared, never modified)"""
    pts, p_bid, q, q_bid = ss.base()
    nb = run_ball(cuda, q, q_bid, pts, p_bid, ss.B, ss.RADIUS, ss.NSAMPLE, with_groups=True)
    want = ss.base_ball()
    assert_neighbors(nb, want)
    return nb, want[0], len(pts)


def features(n, C, name, seed, cuda):
    g = torch.Generator().manual_seed(seed)
    host = torch.randn((n, C), generator=g, dtype=torch.float64).to(DTYPES[name])
    return host, host.to(cuda)


@pytest.mark.parametrize("C,name", [(3, "f16"), (3, "f32"), (64, "f16"), (64, "f32")])
def test_group_point_features_forward_and_backward(cuda, main, C, name):
    from spconv_amd.pytorch import functional as F
    nb, rows, n = main
    host, feat = features(n, C, name, 100 + C, cuda)
    got = F.group_voxels(feat, nb)
    assert got.dtype == DTYPES[name] and tuple(got.shape) == (ss.M, ss.NSAMPLE, C)
    assert np.array_equal(bits(got), rq.group(bits(host), rows))
    dhost, ddout = features(ss.M * ss.NSAMPLE, C, name, 200 + C, cuda)
    want = torch.from_numpy(rq.group_backward(dhost.float().numpy(), rows, n)).to(DTYPES[name])
    feat.requires_grad_(True)
    grads = []
    for _ in range(2):
        out = F.group_voxels(feat, nb)
        grads.append(torch.autograd.grad(out, feat, ddout.view(ss.M, ss.NSAMPLE, C))[0])
    np.testing.assert_array_equal(bits(grads[0]), bits(want))
    np.testing.assert_array_equal(bits(grads[0]), bits(grads[1]))
    assert int((grads[0] != 0).any(dim=1).sum()) > 1000


def test_gradcheck_over_a_ball_query(cuda):
    from spconv_amd.pytorch import functional as F
    pts, bid = cloud([30, 25], 21, extent=2.0)
    rng = np.random.default_rng(22)
    q, q_bid = (rng.random((40, 3)) * 2.0).astype(np.float32), rng.integers(0, 2, 40).astype(np.int32)
    feat = (torch.randperm(55 * 3, generator=torch.Generator().manual_seed(5)).double().reshape(55, 3) * 0.01).to(cuda)
    for pad in ("none", "first"):
        nb = run_ball(cuda, q, q_bid, pts, bid, 2, 0.7, 6, pad=pad, with_groups=True)
        assert int((nb.rows >= 0).sum()) > 100 and int((nb.count < 6).sum()) > 5
        assert torch.autograd.gradcheck(lambda f: F.group_voxels(f, nb), (feat.clone().requires_grad_(True),))


def test_ball_query_and_group_module(cuda):
    import spconv_amd.pytorch as spconv
    pts, p_bid, q, q_bid = ss.base()
    rows, count, offsets, _ = ss.base_ball(ss.NSAMPLE, "first")
    host, feat = features(len(pts), 16, "f16", 31, cuda)
    feat.requires_grad_(True)
    dp, dpb, dq, dqb = dev(cuda, pts), dev(cuda, p_bid), dev(cuda, q), dev(cuda, q_bid)
    out, got_count = spconv.BallQueryAndGroup(ss.RADIUS, ss.NSAMPLE)(dp, dpb, feat, dq, dqb, ss.B)
    assert tuple(out.shape) == (ss.M, ss.NSAMPLE, 3 + 16) and out.dtype == torch.float16
    nb = spconv.functional.ball_query(dq, dqb, dp, dpb, ss.B, ss.RADIUS, ss.NSAMPLE, pad="first", with_offsets=True)
    parts = torch.cat([nb.offsets.to(torch.float16), spconv.functional.group_voxels(feat.detach(), nb)], dim=2)
    assert torch.equal(out.view(torch.int16), parts.view(torch.int16))
    np.testing.assert_array_equal(got_count.cpu().numpy(), count)
    want = np.concatenate([bits(torch.from_numpy(offsets).to(torch.float16)), rq.group(bits(host), rows)], axis=2)
    assert np.array_equal(bits(out), want)
    (grad,) = torch.autograd.grad(out, feat, torch.ones_like(out))                  # every entry counts one per column
    sizes = np.diff(rq.transposed(rows, len(pts))[0]).astype(np.float32)
    np.testing.assert_array_equal(grad.float().cpu().numpy(),
                                  torch.from_numpy(np.repeat(sizes[:, None], 16, axis=1)).half().float().numpy())
    plain, _ = spconv.BallQueryAndGroup(ss.RADIUS, ss.NSAMPLE, False)(dp, dpb, feat.detach(), dq, dqb, ss.B)
    assert torch.equal(plain.view(torch.int16), parts[:, :, 3:].contiguous().view(torch.int16))
    s = spconv.FarthestPointSample(32)(dp, dpb, ss.B)
    assert_fps(s, rs.fps(pts, p_bid, ss.B, 32))


# ------------------------------------------------------------------------------------------------ capture

def test_capture_sampling_query_and_grouping_in_one_graph(cuda):
    """scene groups -> FPS -> gather_samples -> ball_query (with the transposed list) -> group -> group_bwd on ONE
    stream in one graph, replayed on a second cloud with another device point count copied into the static buffers.  The
    backward is the call GroupFunction.backward makes (group_bwd), issued by the capturing thread."""
    from spconv_amd.pytorch import _query
    from spconv_amd.pytorch import functional as F
    base_pts, base_bid, _, _ = ss.base()
    other_pts, other_bid, _ = ss.interleaved(base_pts * np.float32(0.97), base_bid, seed=9)
    sets = [(base_pts, base_bid, len(base_pts)), (other_pts, other_bid, len(base_pts) - 700)]
    N, K, C, S = len(base_pts), 96, 16, 16
    points = torch.empty((N, 4), dtype=torch.float32, device=cuda)
    bid = torch.empty((N,), dtype=torch.int32, device=cuda)
    n_points = torch.empty((1,), dtype=torch.int32, device=cuda)
    feat = features(N, C, "f16", 41, cuda)[1]
    dout = features(ss.B * K * S, C, "f16", 42, cuda)[1].view(ss.B * K, S, C)

    def step():
        groups = F.scene_groups(bid, N, ss.B, n_points)
        s = F.farthest_point_sample(points, bid, ss.B, K, n_points=n_points, groups=groups)
        keys = F.gather_samples(points, s)
        nb = F.ball_query(keys, s.batch_ids, points, bid, ss.B, 1.1, S, pad="first", with_offsets=True,
                          n_points=n_points, with_groups=True, groups=groups)
        return s.idx, s.count, keys, nb.rows, nb.count, nb.offsets, _query.group_voxels(feat, nb), _query.group_bwd(dout, nb)

    def load(k):
        points.copy_(dev(cuda, sets[k][0]))
        bid.copy_(dev(cuda, sets[k][1]))
        n_points.fill_(sets[k][2])
    eager = []
    for k in (0, 1):
        load(k)
        got = [t.clone() for t in step()]
        pts_k, bid_k, live = sets[k]
        idx, cnt = rs.fps(pts_k, bid_k, ss.B, K, n_points=live)
        np.testing.assert_array_equal(got[0].cpu().numpy(), idx)
        keys = pts_k[idx.reshape(-1)]
        want = rs.ball_query(keys[:, :3], np.repeat(np.arange(ss.B, dtype=np.int32), K), None, pts_k, bid_k, live, ss.B,
                             1.1, S, 3, "first")
        np.testing.assert_array_equal(got[3].cpu().numpy(), want[0])
        np.testing.assert_array_equal(bits(got[5]), want[2].view(np.int32))
        assert int(got[3].max()) < live and int((got[4] == S).sum()) > 50 and int((got[4] < S).sum()) > 50
        eager.append(got)
    assert not torch.equal(eager[0][0], eager[1][0])
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = step()
    for k in (1, 0, 1):
        load(k)
        graph.replay()
        torch.cuda.synchronize()
        for got, want in zip(outs, eager[k]):
            np.testing.assert_array_equal(bits(got), bits(want))
