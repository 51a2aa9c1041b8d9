"""GPU: SparseConvTensor.dense() / ToDense / dense_static / from_dense on the kernels of csrc/dense.hip.

A conversion copies: every comparison is torch.equal against a reference built here with plain torch indexing from
unique, in-range rows.  Shapes sit where the tiling can go wrong: 105 cells with an odd innermost extent, a single
cell, 1 to 4 spatial dimensions, and one grid larger than a workgroup's tile (256 cells x 64 bytes of channels) in
every direction."""
import numpy as np
import pytest
import torch

from spconv_amd import _lib

pytestmark = pytest.mark.gpu

GRIDS = [(2, [3, 5, 7]), (1, [1, 1, 1]), (2, [37]), (2, [9, 11]), (1, [3, 4, 5, 6])]
BIG = (3, [5, 33, 70])
CHANNELS = [1, 3, 5, 8, 64, 130]
DTYPES = [torch.int8, torch.float16, torch.bfloat16, torch.float32, torch.float64]


def _rows(n, C, dtype, dev, seed):
    g = torch.Generator().manual_seed(seed)
    if dtype == torch.int8:
        return torch.randint(-127, 128, (n, C), generator=g, dtype=torch.int8).to(dev)
    return (torch.randn((n, C), generator=g, dtype=torch.float64) + 3.0).to(dtype).to(dev)      # (no zeros)


def _coords(B, spatial, n, dev, seed):
    """n distinct cells of the grid in random order: int32 [n, ndim + 1]"""
    cells = B * int(np.prod(spatial))
    rng = np.random.default_rng(seed)
    pick = rng.permutation(cells)[:n]
    idx = np.stack(np.unravel_index(pick, [B] + list(spatial)), 1).astype(np.int32)
    return torch.from_numpy(idx).to(dev)


def _ref_dense(f, idx, B, spatial, channels_first, fill=0):
    out = torch.full([B] + list(spatial) + [f.shape[1]], fill, dtype=f.dtype, device=f.device)
    out[tuple(idx[:, i].long() for i in range(idx.shape[1]))] = f
    if not channels_first:
        return out
    nd = len(spatial)
    return out.permute(0, nd + 1, *range(1, nd + 1)).contiguous()


def _tensor(f, idx, B, spatial):
    import spconv_amd.pytorch as spconv
    return spconv.SparseConvTensor(f, idx, spatial, B)


def _bits(t):
    return t.contiguous().view({1: torch.int8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


@pytest.mark.parametrize("channels_first", [True, False])
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).replace("torch.", ""))
def test_dense_equals_indexing(cuda, dtype, channels_first):
    for gi, (B, spatial) in enumerate(GRIDS):
        cells = B * int(np.prod(spatial))
        for C in CHANNELS:
            n = max(1, (2 * cells) // 5)
            f, idx = _rows(n, C, dtype, cuda, gi * 10 + C), _coords(B, spatial, n, cuda, gi)
            got = _tensor(f, idx, B, spatial).dense(channels_first)
            assert got.is_contiguous() and got.dtype == dtype
            assert torch.equal(got, _ref_dense(f, idx, B, spatial, channels_first)), (B, spatial, C)


@pytest.mark.parametrize("channels_first", [True, False])
@pytest.mark.parametrize("dtype", [torch.int8, torch.float16, torch.float64], ids=lambda d: str(d).replace("torch.", ""))
def test_grid_larger_than_a_tile(cuda, dtype, channels_first):
    B, spatial = BIG
    n = (B * int(np.prod(spatial))) // 10
    for C in (130, 5):
        f, idx = _rows(n, C, dtype, cuda, C), _coords(B, spatial, n, cuda, 7)
        got = _tensor(f, idx, B, spatial).dense(channels_first)
        assert torch.equal(got, _ref_dense(f, idx, B, spatial, channels_first))


@pytest.mark.parametrize("channels_first", [True, False])
def test_empty_full_and_single_row(cuda, channels_first):
    B, spatial, C = 2, [3, 5, 7], 5
    cells = B * 105
    for n in (0, 1, cells):
        f, idx = _rows(n, C, torch.float32, cuda, n), _coords(B, spatial, n, cuda, n)
        got = _tensor(f, idx, B, spatial).dense(channels_first)
        assert torch.equal(got, _ref_dense(f, idx, B, spatial, channels_first)), n
    # an all-empty tile next to live ones (batch item 2 of the large grid holds nothing)
    B, spatial = BIG
    idx = _coords(2, spatial, 3000, cuda, 1)
    f = _rows(3000, 64, torch.float16, cuda, 1)
    assert torch.equal(_tensor(f, idx, B, spatial).dense(channels_first), _ref_dense(f, idx, B, spatial, channels_first))


@pytest.mark.parametrize("channels_first", [True, False])
def test_column_slice_of_features(cuda, channels_first):
    B, spatial = 2, [3, 5, 7]
    idx = _coords(B, spatial, 60, cuda, 3)
    for dtype, lo, hi in ((torch.float16, 3, 11), (torch.float32, 4, 12), (torch.int8, 1, 6)):
        wide = _rows(60, 16, dtype, cuda, 5)
        f = wide[:, lo:hi]
        assert not f.is_contiguous()
        got = _tensor(f, idx, B, spatial).dense(channels_first)
        assert torch.equal(got, _ref_dense(f.contiguous(), idx, B, spatial, channels_first))


@pytest.mark.parametrize("channels_first", [True, False])
def test_duplicate_coordinates_highest_row_wins(cuda, channels_first):
    B, spatial, C = 2, [3, 5, 7], 8
    idx = _coords(B, spatial, 50, cuda, 11)
    f = _rows(50, C, torch.float16, cuda, 11)
    idx[[4, 20, 33]] = idx[4].clone()                    # one coordinate on three rows
    x = _tensor(f, idx, B, spatial)
    keep = torch.tensor([i for i in range(50) if i not in (4, 20)], device=cuda)
    want = _ref_dense(f[keep], idx[keep], B, spatial, channels_first)
    a, b = x.dense(channels_first), x.dense(channels_first)
    assert torch.equal(a, want) and torch.equal(b, want)


def _with_stray_rows(B, spatial, C, dev, dtype=torch.float32):
    """40 good rows with dead / out-of-range rows mixed in: (features, indices, mask of the good rows)"""
    good = _coords(B, spatial, 40, dev, 21)
    stray = torch.tensor([[-1, 0, 0, 0], [B, 1, 1, 1], [0, -1, 2, 2], [1, 0, spatial[1], 0], [0, 1, 1, spatial[2]],
                          [-1, -1, -1, -1]], dtype=torch.int32, device=dev)
    idx = torch.cat([good[:10], stray[:3], good[10:], stray[3:]])
    mask = torch.ones(idx.shape[0], dtype=torch.bool, device=dev)
    mask[10:13] = False
    mask[-3:] = False
    return _rows(idx.shape[0], C, dtype, dev, 22), idx, mask


@pytest.mark.parametrize("channels_first", [True, False])
def test_dead_and_out_of_range_rows_are_ignored(cuda, channels_first):
    B, spatial, C = 2, [3, 5, 7], 5
    f, idx, good = _with_stray_rows(B, spatial, C, cuda)
    got = _tensor(f, idx, B, spatial).dense(channels_first)
    torch.cuda.synchronize()
    assert torch.equal(got, _ref_dense(f[good], idx[good], B, spatial, channels_first))


@pytest.mark.parametrize("channels_first", [True, False])
def test_rows_past_n_live_are_ignored(cuda, channels_first):
    from spconv_amd.pytorch.static import dense_static
    B, spatial, C, n, k = 2, [3, 5, 7], 8, 60, 23
    f, idx = _rows(n, C, torch.float16, cuda, 31), _coords(B, spatial, n, cuda, 31)
    x = _tensor(f, idx, B, spatial)
    x.n_live_dev = torch.tensor([k], dtype=torch.int32, device=cuda)
    want = _ref_dense(f[:k], idx[:k], B, spatial, channels_first)
    assert torch.equal(x.dense(channels_first), want)
    assert torch.equal(dense_static(x, channels_first), want)


@pytest.mark.parametrize("channels_first", [True, False])
@pytest.mark.parametrize("dtype", [torch.float16, torch.float32, torch.float64], ids=lambda d: str(d).replace("torch.", ""))
def test_backward_equals_autograd_of_indexing(cuda, dtype, channels_first):
    for (B, spatial), C in ((GRIDS[0], 5), (GRIDS[4], 8), (BIG, 130), (BIG, 3)):
        n = (B * int(np.prod(spatial))) // 3
        idx = _coords(B, spatial, n, cuda, 41)
        f = _rows(n, C, dtype, cuda, 41).requires_grad_(True)
        fr = f.detach().clone().requires_grad_(True)
        out = _tensor(f, idx, B, spatial).dense(channels_first)
        g = _rows(out.numel(), 1, dtype, cuda, 42).view(out.shape)
        out.backward(g)
        _ref_dense(fr, idx, B, spatial, channels_first).backward(g)
        assert torch.equal(f.grad, fr.grad), (B, spatial, C)
    # a gradient that is not contiguous in the layout the forward produced
    B, spatial = GRIDS[0]
    idx = _coords(B, spatial, 50, cuda, 43)
    f = _rows(50, 5, dtype, cuda, 43).requires_grad_(True)
    fr = f.detach().clone().requires_grad_(True)
    out = _tensor(f, idx, B, spatial).dense(channels_first)
    g = _rows(out.numel(), 1, dtype, cuda, 44).view(out.shape[::-1]).permute(*range(out.dim() - 1, -1, -1))
    assert g.shape == out.shape and not g.is_contiguous()
    out.backward(g)
    _ref_dense(fr, idx, B, spatial, channels_first).backward(g)
    assert torch.equal(f.grad, fr.grad)


@pytest.mark.parametrize("channels_first", [True, False])
def test_backward_gives_zero_to_rows_without_a_cell(cuda, channels_first):
    B, spatial, C = 2, [3, 5, 7], 5
    f, idx, good = _with_stray_rows(B, spatial, C, cuda)
    idx[[2, 30]] = idx[35].clone()                       # rows 2 and 30 lose to row 35
    good[[2, 30]] = False
    f.requires_grad_(True)
    out = _tensor(f, idx, B, spatial).dense(channels_first)
    g = _rows(out.numel(), 1, torch.float32, cuda, 45).view(out.shape)
    out.backward(g)
    fr = f.detach()[good].clone().requires_grad_(True)
    _ref_dense(fr, idx[good], B, spatial, channels_first).backward(g)
    assert torch.equal(f.grad[good], fr.grad)
    assert int((f.grad[~good] != 0).sum()) == 0 and int((~good).sum()) == 8


def test_gradcheck_float64(cuda):
    B, spatial, C = 2, [2, 3, 3], 3
    idx = _coords(B, spatial, 14, cuda, 51)
    f = _rows(14, C, torch.float64, cuda, 51).requires_grad_(True)
    for channels_first in (True, False):
        assert torch.autograd.gradcheck(lambda t: _tensor(t, idx, B, spatial).dense(channels_first), (f,))


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32, torch.float64, torch.int8],
                         ids=lambda d: str(d).replace("torch.", ""))
def test_from_dense_equals_to_sparse(cuda, dtype):
    import spconv_amd.pytorch as spconv
    for (B, spatial), C in ((GRIDS[0], 5), (GRIDS[1], 1), (GRIDS[2], 8), (GRIDS[3], 3), (GRIDS[4], 64), (BIG, 130)):
        cells = B * int(np.prod(spatial))
        n = max(1, cells // 4)
        idx = _coords(B, spatial, n, cuda, 61)
        d = _ref_dense(_rows(n, C, dtype, cuda, 61), idx, B, spatial, False)
        flat = d.view(cells, C)
        if dtype != torch.int8 and cells > 8:
            empty = (flat == 0).all(1).nonzero().flatten()
            flat[empty[0]] = -0.0                              # a cell of negative zeros only: inactive
            flat[empty[1], C - 1] = float("nan")               # a NaN in an otherwise empty cell: active
        sp = d.to_sparse(d.dim() - 1)
        x = spconv.SparseConvTensor.from_dense(d)
        assert x.indices.dtype == torch.int32 and x.batch_size == B and list(x.spatial_shape) == list(spatial)
        assert torch.equal(x.indices, sp.indices().T.int()), (B, spatial, C)
        assert torch.equal(_bits(x.features), _bits(sp.values()))
        if dtype != torch.int8 and cells > 8:
            assert bool(torch.isnan(x.features.float()).any()) and x.features.shape[0] == n + 1


@pytest.mark.parametrize("dtype", [torch.int8, torch.float16], ids=lambda d: str(d).replace("torch.", ""))
@pytest.mark.parametrize("spatial", [[257, 16, 16], [128, 128, 128], [129, 128, 128]], ids=lambda s: "x".join(map(str, s)))
def test_from_dense_across_scan_boundary(cuda, spatial, dtype):
    """from_dense counts per 256-cell block and one workgroup scans the counts (scan_kernel of csrc/scan.h), len =
    cells / 256 of them: 257 (one pass, two items per thread, the last threads hold none), 8192 (the last one-pass
    length, every thread holds 32 items) and 8256 (the loop form, 256 items per round).  Occupied with 1 .. 5 cells each:
    the first and the last block and the two blocks either side of every 32nd block boundary -- the ends of a thread's
    run in the one-pass form at each of these lengths, and the ends of a round of the loop form; a few thousand cells
    anywhere besides.  One channel; coordinates, row order and features exactly as torch's to_sparse."""
    import spconv_amd.pytorch as spconv
    cells = int(np.prod(spatial))
    nblk = cells // 256
    assert cells % 256 == 0 and nblk in (257, 8192, 8256)
    rng = np.random.default_rng(91)
    edge = np.arange(0, nblk, 2 if nblk == 257 else 32)
    blocks = np.unique(np.concatenate([[0, nblk - 1], edge, edge[1:] - 1]))
    pick = [rng.integers(0, cells, 3000)]
    for b in blocks:
        pick.append(b * 256 + rng.choice(256, size=1 + int(b) % 5, replace=False))
    pick = np.unique(np.concatenate(pick))
    flat = torch.zeros((cells, 1), dtype=dtype, device=cuda)
    vals = _rows(pick.size, 1, dtype, cuda, 92)
    vals[vals == 0] = 1
    flat[torch.from_numpy(pick).to(cuda)] = vals
    d = flat.view([1] + list(spatial) + [1])
    sp = d.to_sparse(d.dim() - 1)
    x = spconv.SparseConvTensor.from_dense(d)
    assert x.features.shape[0] == pick.size
    assert torch.equal(x.indices, sp.indices().T.int())
    assert torch.equal(_bits(x.features), _bits(sp.values()))


def test_from_dense_round_trip_and_gradient(cuda):
    import spconv_amd.pytorch as spconv
    B, spatial, C = 2, [3, 5, 7], 5
    idx = _coords(B, spatial, 70, cuda, 71)
    d = _ref_dense(_rows(70, C, torch.float32, cuda, 71), idx, B, spatial, False)
    assert torch.equal(spconv.SparseConvTensor.from_dense(d).dense(channels_first=False), d)
    empty = torch.zeros_like(d)
    x = spconv.SparseConvTensor.from_dense(empty)
    assert x.features.shape == (0, C) and x.indices.shape == (0, 4)
    assert torch.equal(x.dense(channels_first=False), empty)
    a = d.clone().requires_grad_(True)
    b = d.clone().requires_grad_(True)
    feats = spconv.SparseConvTensor.from_dense(a).features
    g = _rows(feats.shape[0], C, torch.float32, cuda, 72)
    feats.backward(g)
    b.to_sparse(b.dim() - 1).values().backward(g)
    want = b.grad.to_dense() if b.grad.is_sparse else b.grad
    assert torch.equal(a.grad, want)


@pytest.mark.parametrize("channels_first", [True, False])
def test_quantised_features(cuda, channels_first):
    B, spatial, C = 2, [3, 5, 7], 8
    idx = _coords(B, spatial, 60, cuda, 81)
    f = (_rows(60, C, torch.float32, cuda, 81) - 3.0)
    q = torch.quantize_per_tensor(f, 0.05, 3, torch.qint8)
    x = _tensor(f, idx, B, spatial).replace_feature(q)
    got = x.dense(channels_first)
    assert got.dtype == torch.qint8 and got.q_scale() == 0.05 and got.q_zero_point() == 3
    assert torch.equal(got.int_repr(), _ref_dense(q.int_repr(), idx, B, spatial, channels_first, fill=3))
    assert torch.equal(got.dequantize(), _ref_dense(q.dequantize(), idx, B, spatial, channels_first))


def test_dense_of_a_static_tensor_inside_a_captured_graph(cuda):
    B, spatial, C, cap = 2, [5, 9, 13], 16, 400
    feats = torch.zeros((cap, C), dtype=torch.float16, device=cuda)
    inds = torch.full((cap, 4), -1, dtype=torch.int32, device=cuda)
    n_live = torch.zeros((1,), dtype=torch.int32, device=cuda)

    def load(n, seed):
        f, idx = _rows(n, C, torch.float16, cuda, seed), _coords(B, spatial, n, cuda, seed)
        feats.zero_()
        inds.fill_(-1)
        feats[:n].copy_(f)
        inds[:n].copy_(idx)
        feats[n:n + 5].fill_(7.0)                       # stale rows behind the live count keep old coordinates
        inds[n:n + 5].copy_(idx[:5])
        n_live.fill_(n)
        return f, idx

    x = _tensor(feats, inds, B, spatial)
    x.n_live_dev = n_live
    load(300, 91)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), torch.no_grad():
        x.dense()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.no_grad(), torch.cuda.graph(graph):
        out = x.dense()
    for n, seed in ((300, 91), (121, 92), (395, 93)):
        f, idx = load(n, seed)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, _ref_dense(f, idx, B, spatial, True)), n


def test_cuda_dense_dispatches_the_new_kernels(cuda):
    L = _lib.load()
    keys = [b"dense/map", b"dense/scatter_cf", b"dense/scatter_cl", b"dense/gather_cf", b"dense/gather_cl",
            b"dense/compact"]
    count = lambda: {k: int(L.spx_launch_count(k)) for k in keys}
    B, spatial, C = 2, [3, 5, 7], 8
    idx = _coords(B, spatial, 50, cuda, 95)
    f = _rows(50, C, torch.float16, cuda, 95).requires_grad_(True)
    c0 = count()
    out = _tensor(f, idx, B, spatial).dense()
    c1 = count()
    assert c1[b"dense/map"] == c0[b"dense/map"] + 1 and c1[b"dense/scatter_cf"] == c0[b"dense/scatter_cf"] + 1
    out.backward(torch.ones_like(out))
    c2 = count()
    assert c2[b"dense/gather_cf"] == c1[b"dense/gather_cf"] + 1 and c2[b"dense/map"] == c1[b"dense/map"]
    out = _tensor(f, idx, B, spatial).dense(channels_first=False)
    out.backward(torch.ones_like(out))
    c3 = count()
    assert c3[b"dense/scatter_cl"] == c2[b"dense/scatter_cl"] + 1 and c3[b"dense/gather_cl"] == c2[b"dense/gather_cl"] + 1
    import spconv_amd.pytorch as spconv
    spconv.SparseConvTensor.from_dense(out.detach())
    assert count()[b"dense/compact"] == c3[b"dense/compact"] + 2          # the count pass and the fill pass
