"""The k-nearest-neighbour query and the inverse-distance interpolation on the kernel of csrc/knn.hip
(spconv_amd/pytorch/_knn.py, spatial.KNNInterpolate / KNNQueryAndGroup) against the numpy restatement tests/refknn.py
(whose conditions test_refknn.py asserts on the CPU), over clouds of its own and those of tests/samplescenes.py.

Every comparison is bit for bit: indices and counts are integers; squared distances, weights and offsets are float32
arithmetic in which numpy rounds every operation on its own (the contract: its float32 sqrt and divide are correctly
rounded); the blend and its gradient are sequential float32 sums in a fixed order that refinterp reproduces; the gather
moves rows unchanged.  The one tolerance is gradcheck's own, in float64."""
import functools

import numpy as np
import pytest
import torch

import refinterp as ri
import refknn as rk
import refquery as rq
import samplescenes as ss

pytestmark = pytest.mark.gpu

DTYPES = {"f16": torch.float16, "f32": torch.float32}
SCENE_SETS = [(0, 1, 2), (3, 4, 63), (64, 65, 1023), (1024, 1025, 2049)]
KS = [1, 3, 4, 5, 16, 17, 64]


def bits(t):
    t = t.detach().cpu().contiguous()
    return t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()]).numpy()


def dev(cuda, a):
    return None if a is None else torch.from_numpy(np.array(a, order="C")).to(cuda)


def count_of(cuda, n):
    return None if n is None else torch.tensor([n], dtype=torch.int32, device=cuda)


def run_knn(cuda, q, q_bid, pts, p_bid, B, k, n_queries=None, n_points=None, **kw):
    from spconv_amd import _lib
    from spconv_amd.pytorch import functional as F
    before = _lib.load().spx_launch_count(b"sample/knn_query")
    got = F.knn_query(dev(cuda, q), dev(cuda, q_bid), dev(cuda, pts), dev(cuda, p_bid), B, k,
                      n_queries=count_of(cuda, n_queries), n_points=count_of(cuda, n_points), **kw)
    assert _lib.load().spx_launch_count(b"sample/knn_query") == before + (1 if len(q) else 0)
    width = kw.get("width") or k
    assert got.k == k and got.num_points == len(pts) and tuple(got.rows.shape) == (len(q), width)
    assert got.rows.dtype == torch.int32 and got.count.dtype == torch.int32 and tuple(got.count.shape) == (len(q),)
    return got


def assert_knn(got, want):
    """want: refknn's (rows, count, dist2, weights, offsets); a table the call was not asked for is None"""
    rows, count, d2, w, off = want
    np.testing.assert_array_equal(got.count.cpu().numpy(), count)
    np.testing.assert_array_equal(got.rows.cpu().numpy(), rows)
    for name, have, ref in (("dist2", got.dist2, d2), ("weights", got.weights, w), ("offsets", got.offsets, off)):
        if have is not None:
            assert have.dtype == torch.float32 and tuple(have.shape) == ref.shape, name
            np.testing.assert_array_equal(bits(have), ref.view(np.int32), err_msg=name)


@functools.lru_cache(maxsize=None)
def sized_cloud(valid, M=257):
    """three scenes with `valid` valid points each and, where a scene has any, three invalid ones (NaN, +inf, -inf);
    M queries in shuffled scene order, a fifth of them ON a point of their scene"""
    sizes = [v + 3 if v else 0 for v in valid]
    rng = np.random.default_rng(300 + sum(valid))
    pts = (rng.random((int(sum(sizes)), 4)) * 4.0).astype(np.float32)
    bid = np.repeat(np.arange(3, dtype=np.int32), sizes)
    start = 0
    for n in sizes:
        if n:
            pts[start + 1, 0], pts[start + n // 2, 2], pts[start + n - 1, 1] = np.nan, np.inf, -np.inf
        start += n
    q = (rng.random((M, 3)) * 4.0).astype(np.float32)
    q_bid = rng.integers(0, 3, M).astype(np.int32)
    first = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    on = np.nonzero(np.asarray(sizes)[q_bid[::5]] > 0)[0] * 5
    q[on] = pts[first[q_bid[on]], :3]
    for a in (pts, bid, q, q_bid):
        a.setflags(write=False)
    return pts, bid, q, q_bid


@functools.lru_cache(maxsize=None)
def sized_ref(valid, k):
    pts, bid, q, q_bid = sized_cloud(valid)
    return rk.knn_query(q, q_bid, None, pts, bid, None, 3, k)


@functools.lru_cache(maxsize=None)
def base_ref(k, width=None, pad="none"):
    pts, p_bid, q, q_bid = ss.base()
    return rk.knn_query(q, q_bid, None, pts, p_bid, None, ss.B, k, width=width, pad=pad)


# ------------------------------------------------------------------------------------------------ the query

@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("valid", SCENE_SETS)
def test_scene_sizes_across_the_tile_and_every_tier(cuda, valid, k):
    """valid counts on both sides of the 8-point batch, the 1024-point tile and k; k at and just past the edge of every
    list size (4, 16, 64); 257 queries of three scenes mixed inside the workgroups"""
    pts, bid, q, q_bid = sized_cloud(valid)
    want = sized_ref(valid, k)
    for b, v in enumerate(valid):
        assert (want[1][q_bid == b] == min(v, k)).all()
    got = run_knn(cuda, q, q_bid, pts, bid, 3, k, with_weights=True, with_offsets=True)
    assert_knn(got, want)
    live = got.rows[got.rows >= 0].cpu().numpy()
    assert np.isfinite(pts[live, :3]).all()


@pytest.mark.parametrize("M", [0, 1, 255, 256, 257])
def test_query_counts_around_the_workgroup(cuda, M):
    pts, bid, q, q_bid = sized_cloud((64, 65, 1023))
    want = rk.knn_query(q[:M], q_bid[:M], None, pts, bid, None, 3, 3, width=4)
    got = run_knn(cuda, q[:M], q_bid[:M], pts, bid, 3, 3, width=4, with_weights=True, with_offsets=True, with_groups=True)
    assert_knn(got, want)
    assert (got.groups is None) == (M == 0)
    if M == 0:
        from spconv_amd.pytorch import functional as F
        assert tuple(F.knn_interpolate(dev(cuda, pts), got).shape) == (0, 4)


def test_result_does_not_depend_on_the_order_across_scenes(cuda):
    pts, p_bid, q, q_bid = ss.base()
    want = base_ref(16)
    a = run_knn(cuda, q, q_bid, pts, p_bid, ss.B, 16, with_weights=True, with_offsets=True)
    assert_knn(a, want)
    again = run_knn(cuda, q, q_bid, pts, p_bid, ss.B, 16, with_weights=True, with_offsets=True)
    for x, y in zip(a[:5], again[:5]):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))                 # identical run to run
    order = np.argsort(q_bid, kind="stable")                        # scene-contiguous queries
    got = run_knn(cuda, q[order], q_bid[order], pts, p_bid, ss.B, 16, with_weights=True, with_offsets=True)
    assert_knn(got, tuple(w[order] for w in want))
    perm = np.random.default_rng(5).permutation(ss.M)               # shuffled queries
    got = run_knn(cuda, q[perm], q_bid[perm], pts, p_bid, ss.B, 16, with_weights=True, with_offsets=True)
    assert_knn(got, tuple(w[perm] for w in want))
    new_pts, new_bid, new_row = ss.interleaved(pts, p_bid)          # interleaved points: the same points, renumbered
    got = run_knn(cuda, q, q_bid, new_pts, new_bid, ss.B, 16, with_weights=True, with_offsets=True)
    assert_knn(got, (new_row[want[0]].astype(np.int32),) + want[1:])         # (an order-keeping renumbering: ties too)


def test_device_counts_and_invalid_rows(cuda):
    pts, p_bid, q, q_bid = ss.base()
    bad_q, bad_bid = q.copy(), q_bid.copy()
    bad_q[::5, 1], bad_q[1::10, 0], bad_q[2::10, 2] = np.nan, np.inf, -np.inf
    bad_bid[3::7], bad_bid[4::9] = ss.B, -1
    bad_pts, bad_pid = pts.copy(), p_bid.copy()
    bad_pts[5::7, 2], bad_pts[6::7, 0], bad_pts[0, 1] = np.inf, np.nan, -np.inf
    bad_pid[3::7], bad_pid[2::13] = -1, ss.B
    want = rk.knn_query(bad_q, bad_bid, 500, bad_pts, bad_pid, 3500, ss.B, 5, width=8, pad="first")
    got = run_knn(cuda, bad_q, bad_bid, bad_pts, bad_pid, ss.B, 5, n_queries=500, n_points=3500, width=8, pad="first",
                  with_weights=True, with_offsets=True)
    assert_knn(got, want)
    assert got.n_queries is not None and got.n_points is not None
    dead = ~np.isfinite(bad_q).all(axis=1) | (bad_bid < 0) | (bad_bid >= ss.B) | (np.arange(ss.M) >= 500)
    assert dead.sum() > 250 and bool((got.count[torch.from_numpy(dead).to(cuda)] == 0).all())
    assert bool((got.count[torch.from_numpy(~dead).to(cuda)] == 5).all()) and (~dead).sum() > 100
    live = got.rows[got.rows >= 0].cpu().numpy()
    assert live.max() < 3500 and np.isfinite(bad_pts[live, :3]).all() and ((bad_pid[live] >= 0) & (bad_pid[live] < ss.B)).all()
    # a cloud whose points are all invalid, no batch ids at all, and no points at all
    nowhere = pts[:50].copy()
    nowhere[:, 1] = np.nan
    for cloud in (nowhere, pts[:0]):
        got = run_knn(cuda, q[:40], None, cloud, None, 1, 3, width=4, pad="first", with_weights=True, with_offsets=True)
        assert bool((got.rows == -1).all()) and bool((got.count == 0).all())
        assert all(bool((t == 0).all()) for t in (got.dist2, got.weights, got.offsets))
    assert_knn(run_knn(cuda, q[:40], None, pts[:500], None, 1, 17, with_weights=True),
               rk.knn_query(q[:40], None, None, pts[:500], None, None, 1, 17)[:4] + (None,))


@pytest.mark.parametrize("with_offsets", [True, False])
@pytest.mark.parametrize("pad", ["none", "first"])
@pytest.mark.parametrize("k,width", [(3, 4), (3, 8), (5, 8), (5, 5)])
def test_tables_widths_padding_and_optional_outputs(cuda, k, width, pad, with_offsets):
    """scenes of 2, 4 and 65 valid points: counts below k get -1 / 0 or slot 0 again with weight 0, slots in [k, width)
    always -1 / 0; every optional table on and off"""
    pts, bid, q, q_bid = sized_cloud((2, 4, 65), 64)
    want = rk.knn_query(q, q_bid, None, pts, bid, None, 3, k, width=width, pad=pad)
    assert (want[1] < k).sum() > 10 and (want[1] == k).sum() > 10
    got = run_knn(cuda, q, q_bid, pts, bid, 3, k, width=width, pad=pad, with_weights=True, with_offsets=with_offsets)
    assert (got.offsets is not None) == with_offsets and got.dist2 is not None and got.weights is not None
    assert_knn(got, want)
    bare = run_knn(cuda, q, q_bid, pts, bid, 3, k, width=width, pad=pad, with_dist2=False, with_offsets=with_offsets)
    assert bare.dist2 is None and bare.weights is None and bare.groups is None
    assert_knn(bare, want)
    if width in (4, 8):
        c = got.corners()
        assert c.rows is got.rows and c.weights is got.weights and c.num_voxels == len(pts)
    if width == k:
        nb = got.neighbors()
        assert nb.rows is got.rows and nb.offsets is got.offsets and nb.num_voxels == len(pts)


def test_exact_lattice_and_duplicate_cases(cuda):
    zero = np.zeros((1, 3), dtype=np.float32)
    pts = np.array([[2, 0, 0], [0, 2, 0], [1, 0, 0], [0, 0, -2], [-2, 0, 0], [5, 5, 5], [0, 0, 0]], dtype=np.float32)
    got = run_knn(cuda, zero, None, pts, None, 1, 4, with_weights=True, with_offsets=True)
    assert got.rows.cpu().numpy()[0].tolist() == [6, 2, 0, 1] and got.dist2.cpu().numpy()[0].tolist() == [0, 1, 4, 4]
    assert_knn(got, rk.knn_query(zero, None, None, pts, None, None, 1, 4))
    assert bool(torch.isfinite(got.weights).all()) and float(got.weights[0, 0]) > 0.9999999      # d2 = 0: 1e8 / norm
    got = run_knn(cuda, zero, None, pts[::-1].copy(), None, 1, 4)
    assert got.rows.cpu().numpy()[0].tolist() == [0, 4, 2, 3]                   # equal distances: the lowest index
    got = run_knn(cuda, zero[:, :2], None, np.ascontiguousarray(pts[:, :2]), None, 1, 3, ndim=2, with_weights=True,
                  with_offsets=True)
    assert got.rows.cpu().numpy()[0].tolist() == [3, 6, 2]
    assert_knn(got, rk.knn_query(zero[:, :2], None, None, pts[:, :2], None, None, 1, 3, ndim=2))
    q = np.array([[1, 1, 1]], dtype=np.float32)
    for k, width, pad, rows in ((6, None, "none", [0, 1, 2, 3, 4, 5]), (16, None, "first", list(range(10)) + [0] * 6),
                                (12, 16, "none", list(range(10)) + [-1] * 6), (64, None, "none", list(range(10)) + [-1] * 54)):
        got = run_knn(cuda, q, None, ss.DUPLICATES, None, 1, k, width=width, pad=pad, with_weights=True)
        assert got.rows.cpu().numpy()[0].tolist() == rows and int(got.count[0]) == min(k, 10)
        assert_knn(got, rk.knn_query(q, None, None, ss.DUPLICATES, None, None, 1, k, width=width, pad=pad)[:4] + (None,))


def test_two_dimensions_bit_for_bit(cuda):
    pts, bid, q, q_bid = sized_cloud((64, 65, 1023))
    pts2, q2 = np.ascontiguousarray(pts[:, :3]), np.ascontiguousarray(q[:, :2])       # (the third column is not a coordinate)
    for k in (3, 16, 33):
        want = rk.knn_query(q2, q_bid, None, pts2, bid, None, 3, k, ndim=2)
        assert_knn(run_knn(cuda, q2, q_bid, pts2, bid, 3, k, ndim=2, with_weights=True, with_offsets=True), want)


# ------------------------------------------------------------------------------------------------ interpolation, grouping

@pytest.fixture(scope="module")
def three(cuda):
    """three_nn of the base queries over the base points, groups built (shared, never modified)"""
    from spconv_amd.pytorch import functional as F
    pts, p_bid, q, q_bid = ss.base()
    knn = F.three_nn(dev(cuda, q), dev(cuda, q_bid), dev(cuda, pts), dev(cuda, p_bid), ss.B, with_groups=True)
    want = base_ref(3, 4)
    assert_knn(knn, want)
    assert knn.groups is not None and knn.offsets is None
    return knn, want[0], want[3], len(pts)


def features(n, C, name, seed, cuda):
    g = torch.Generator().manual_seed(seed)
    host = torch.randn((n, C), generator=g, dtype=torch.float64).to(DTYPES[name])
    return host, host.to(cuda)


@pytest.mark.parametrize("C,name", [(3, "f16"), (3, "f32"), (64, "f16"), (64, "f32")])
def test_knn_interpolate_forward_and_backward(cuda, three, C, name):
    from spconv_amd.pytorch import functional as F
    knn, rows, weights, n = three
    host, feat = features(n, C, name, 300 + C, cuda)
    got = F.knn_interpolate(feat, knn)
    assert got.dtype == DTYPES[name] and tuple(got.shape) == (ss.M, C)
    want = torch.from_numpy(ri.forward(host.float().numpy(), rows, weights)).to(DTYPES[name])
    np.testing.assert_array_equal(bits(got), bits(want))
    dhost, ddout = features(ss.M, C, name, 400 + C, cuda)
    dwant = torch.from_numpy(ri.backward(dhost.float().numpy(), rows, weights, n)).to(DTYPES[name])
    feat.requires_grad_(True)
    grads = []
    for _ in range(2):
        grads.append(torch.autograd.grad(F.knn_interpolate(feat, knn), feat, ddout)[0])
    np.testing.assert_array_equal(bits(grads[0]), bits(dwant))
    np.testing.assert_array_equal(bits(grads[0]), bits(grads[1]))
    assert int((grads[0] != 0).any(dim=1).sum()) > 500


def test_gradcheck_of_the_interpolation_module(cuda):
    import spconv_amd.pytorch as spconv
    rng = np.random.default_rng(23)
    known = (rng.random((40, 3)) * 2.0).astype(np.float32)
    k_bid = np.repeat(np.arange(2, dtype=np.int32), [22, 18])
    unknown, u_bid = (rng.random((25, 3)) * 2.0).astype(np.float32), rng.integers(0, 2, 25).astype(np.int32)
    feat = (torch.randperm(40 * 3, generator=torch.Generator().manual_seed(5)).double().reshape(40, 3) * 0.01).to(cuda)
    args = (dev(cuda, known), dev(cuda, k_bid))
    rest = (dev(cuda, unknown), dev(cuda, u_bid), 2)
    for k in (3, 5):
        module = spconv.KNNInterpolate(k)
        assert torch.autograd.gradcheck(lambda f: module(*args, f, *rest), (feat.clone().requires_grad_(True),))
    out = spconv.KNNInterpolate()(*args, feat, *rest)
    want = rk.knn_query(unknown, u_bid, None, known, k_bid, None, 2, 3, width=4)
    ref = ri.forward(feat.cpu().numpy(), want[0], want[3], acc=np.float64)
    np.testing.assert_allclose(out.cpu().numpy(), ref, rtol=1e-12)       # (float64, positive terms: a few roundings of 2^-53)


def test_knn_query_and_group_module(cuda):
    import spconv_amd.pytorch as spconv
    pts, p_bid, q, q_bid = ss.base()
    rows, count, _, _, offsets = base_ref(16, None, "first")
    host, feat = features(len(pts), 16, "f16", 31, cuda)
    feat.requires_grad_(True)
    dp, dpb, dq, dqb = dev(cuda, pts), dev(cuda, p_bid), dev(cuda, q), dev(cuda, q_bid)
    out, got_count = spconv.KNNQueryAndGroup(16)(dp, dpb, feat, dq, dqb, ss.B)
    assert tuple(out.shape) == (ss.M, 16, 3 + 16) and out.dtype == torch.float16
    knn = spconv.functional.knn_query(dq, dqb, dp, dpb, ss.B, 16, pad="first", with_offsets=True)
    parts = torch.cat([knn.offsets.to(torch.float16), spconv.functional.group_voxels(feat.detach(), knn.neighbors())], dim=2)
    assert torch.equal(out.view(torch.int16), parts.view(torch.int16))
    np.testing.assert_array_equal(got_count.cpu().numpy(), count)
    want = np.concatenate([bits(torch.from_numpy(offsets).to(torch.float16)), rq.group(bits(host), rows)], axis=2)
    assert np.array_equal(bits(out), want)
    (grad,) = torch.autograd.grad(out, feat, torch.ones_like(out))                  # every entry counts one per column
    sizes = np.diff(rq.transposed(rows, len(pts))[0]).astype(np.float32)
    np.testing.assert_array_equal(grad.float().cpu().numpy(),
                                  torch.from_numpy(np.repeat(sizes[:, None], 16, axis=1)).half().float().numpy())
    plain, _ = spconv.KNNQueryAndGroup(16, False)(dp, dpb, feat.detach(), dq, dqb, ss.B)
    assert torch.equal(plain.view(torch.int16), parts[:, :, 3:].contiguous().view(torch.int16))


# ------------------------------------------------------------------------------------------------ capture

def test_capture_query_blend_and_gradient_in_one_graph(cuda):
    """scene groups -> knn_query_into -> the transposed list -> blend -> its gradient on ONE stream in one graph,
    replayed on a second cloud with other device counts copied into the static buffers.  The backward is the call
    TrilinearFunction.backward makes (interp_bwd), issued by the capturing thread."""
    from spconv_amd.pytorch import _interp
    from spconv_amd.pytorch import functional as F
    from spconv_amd.pytorch._level import flat_groups
    base_pts, base_bid, base_q, base_qbid = ss.base()
    other_pts, other_bid, _ = ss.interleaved(base_pts * np.float32(0.97), base_bid, seed=9)
    other_q, other_qbid = np.ascontiguousarray(base_q[::-1] * np.float32(1.01)), np.ascontiguousarray(base_qbid[::-1])
    sets = [(base_pts, base_bid, len(base_pts), base_q, base_qbid, ss.M),
            (other_pts, other_bid, len(base_pts) - 700, other_q, other_qbid, ss.M - 90)]
    N, M, C = len(base_pts), ss.M, 16
    known = torch.empty((N, 4), dtype=torch.float32, device=cuda)
    k_bid = torch.empty((N,), dtype=torch.int32, device=cuda)
    unknown = torch.empty((M, 3), dtype=torch.float32, device=cuda)
    u_bid = torch.empty((M,), dtype=torch.int32, device=cuda)
    n_known = torch.empty((1,), dtype=torch.int32, device=cuda)
    n_unknown = torch.empty((1,), dtype=torch.int32, device=cuda)
    rows = torch.empty((M, 4), dtype=torch.int32, device=cuda)
    count = torch.empty((M,), dtype=torch.int32, device=cuda)
    dist2 = torch.empty((M, 4), dtype=torch.float32, device=cuda)
    weights = torch.empty((M, 4), dtype=torch.float32, device=cuda)
    host_feat, feat = features(N, C, "f16", 41, cuda)
    host_dout, dout = features(M, C, "f16", 42, cuda)

    def step():
        groups = F.scene_groups(k_bid, N, ss.B, n_known)
        F.knn_query_into(unknown, u_bid, n_unknown, known, groups, 3, 3, 1e-8, False, rows, count, dist2, weights)
        corners = F.PointCorners(rows, weights, flat_groups(rows, N, n_known), N, n_unknown, n_known)
        return rows, count, dist2, weights, _interp.interp_fwd(feat, corners), _interp.interp_bwd(dout, corners)

    def load(s):
        known.copy_(dev(cuda, sets[s][0]))
        k_bid.copy_(dev(cuda, sets[s][1]))
        n_known.fill_(sets[s][2])
        unknown.copy_(dev(cuda, sets[s][3]))
        u_bid.copy_(dev(cuda, sets[s][4]))
        n_unknown.fill_(sets[s][5])
    eager = []
    for s in (0, 1):
        load(s)
        got = [t.clone() for t in step()]
        pts_s, bid_s, live, q_s, qbid_s, nq = sets[s]
        want = rk.knn_query(q_s, qbid_s, nq, pts_s, bid_s, live, ss.B, 3, width=4)
        for have, ref in zip(got[:4], want[:4]):
            np.testing.assert_array_equal(bits(have), ref.view(np.int32))
        np.testing.assert_array_equal(bits(got[4]), bits(torch.from_numpy(
            ri.forward(host_feat.float().numpy(), want[0], want[3])).half()))
        np.testing.assert_array_equal(bits(got[5]), bits(torch.from_numpy(
            ri.backward(host_dout.float().numpy(), want[0], want[3], N, live)).half()))
        assert int(got[0].max()) < live and int((got[1] == 3).sum()) == nq
        eager.append(got)
    assert not torch.equal(eager[0][0], eager[1][0])
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = step()
    for s in (1, 0, 1):
        load(s)
        graph.replay()
        torch.cuda.synchronize()
        for got, want in zip(outs, eager[s]):
            np.testing.assert_array_equal(bits(got), bits(want))
