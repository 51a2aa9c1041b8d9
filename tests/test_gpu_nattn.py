"""Neighbour attention and aggregation on the kernels of csrc/nattn.hip (spconv_amd/pytorch/_nattn.py) against a
float64 restatement in torch -- index gather, einsum, masked softmax, einsum -- over a synthetic table (M = 77 queries
over n = 53 rows, 50 of them live) with holes, a query without a key, a query of one row, dead rows, an unnamed row and
one row that more than 300 entries name.

Criteria.  16-bit forward: |out - ref| <= 4 u max|v| over the query's key rows per (query, head), u = 2^-11 / 2^-8 (out
is a convex combination of those rows, rounded once).  float32 forward and every gradient: max|got - ref| <= 2
max|composite - ref| + u max|ref|, the composite being the same torch ops in the input dtype with a float32 softmax and
u the unit roundoff of the tensor's own dtype."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

M, N, LIVE, UNNAMED, HOT = 77, 53, 50, 7, 3
DTYPES = {"f16": (torch.float16, 2.0 ** -11), "bf16": (torch.bfloat16, 2.0 ** -8), "f32": (torch.float32, 2.0 ** -24)}
HEADS = [(1, 8), (3, 16), (2, 64), (1, 128)]


def bits(t):
    t = t.detach().contiguous()
    return t.view({2: torch.int16, 4: torch.int32}[t.element_size()]).cpu().numpy()


@functools.lru_cache(maxsize=None)
def host_rows(S):
    g = np.random.default_rng(S)
    rows = g.integers(0, N, size=(M, S)).astype(np.int32)       # (rows 50 .. 52 among them: no keys)
    rows[g.random((M, S)) < 0.4] = HOT
    rows[rows == UNNAMED] = HOT
    rows[g.random((M, S)) < 0.2] = -1                           # holes anywhere in a row
    rows[5], rows[6], rows[8] = -1, 11, 51                      # no key; one row in every slot; dead rows only
    rows[9, 0], rows[9, S // 2], rows[9, -1] = 52, -1, -1
    assert S < 16 or (rows == HOT).sum() > 300
    return rows


def table(cuda, S, groups=True):
    from spconv_amd.pytorch import functional as F
    from spconv_amd.pytorch._level import flat_groups
    rows = torch.from_numpy(host_rows(S)).to(cuda)
    live = torch.tensor([LIVE], dtype=torch.int32, device=cuda)
    count = (rows >= 0).sum(1).to(torch.int32)
    return F.VoxelNeighbors(rows, count, None, flat_groups(rows, N, live) if groups else None, N, None, live)


def keys_of(nb, live):
    return (nb.rows >= 0) & (nb.rows < live)


def attention(q, k, v, nb, live, H, scale, bias, dtype):
    """the restatement: gather, einsum, masked softmax (float64, or float32 for a composite), einsum"""
    (Mq, S), D = nb.rows.shape, q.shape[1] // H
    key, idx = keys_of(nb, live), nb.rows.clamp(0, k.shape[0] - 1).long()
    hole = ~key[:, :, None, None]
    kg = k.to(dtype)[idx].view(Mq, S, H, D).masked_fill(hole, 0)
    vg = v.to(dtype)[idx].view(Mq, S, H, D).masked_fill(hole, 0)
    soft = torch.float64 if dtype == torch.float64 else torch.float32
    x = torch.einsum("mhd,mshd->msh", q.to(dtype).view(Mq, H, D), kg).to(soft) * scale
    if bias is not None:
        x = x + bias.to(soft)
    x = x.masked_fill(~key[:, :, None], -torch.inf)
    x = x.masked_fill(~key.any(1)[:, None, None], 0)            # (a query without a key: P is masked below)
    P = torch.softmax(x, dim=1).masked_fill(~key[:, :, None], 0).to(dtype)
    return torch.einsum("msh,mshd->mhd", P, vg).reshape(Mq, H * D)


def aggregate(w, v, nb, live, dtype):
    (Mq, S), G = nb.rows.shape, w.shape[2]
    key, idx = keys_of(nb, live), nb.rows.clamp(0, v.shape[0] - 1).long()
    vg = v.to(dtype)[idx].view(Mq, S, G, -1).masked_fill(~key[:, :, None, None], 0)
    return torch.einsum("msg,msgd->mgd", w.to(dtype).masked_fill(~key[:, :, None], 0), vg).reshape(Mq, -1)


def inputs(cuda, name, H, D, S, with_bias, seed=0, Mq=M, n=N):
    g = torch.Generator().manual_seed(1000 * S + 10 * D + H + seed)
    dtype = DTYPES[name][0]
    q, k, v = (torch.randn((r, H * D), generator=g).to(dtype).to(cuda) for r in (Mq, n, n))
    bias = torch.randn((Mq, S, H), generator=g).to(cuda) if with_bias else None
    w = torch.softmax(torch.randn((Mq, S, H), generator=g), dim=1).to(torch.float32 if with_bias else dtype).to(cuda)
    return q, k, v, bias, w, torch.randn((Mq, H * D), generator=g).to(dtype).to(cuda)


def within_composite(got, ref, comp, u, what):
    err, base = float((got.double() - ref).abs().max()), float((comp.double() - ref).abs().max())
    bound = 2 * base + u * float(ref.abs().max())
    print(f"{what}: err {err:.3e} bound {bound:.3e} ratio {err / bound if bound else 0:.3f}")
    assert err <= bound, what


def assert_forward(got, ref, comp, v, nb, H, name, what):
    u, key = DTYPES[name][1], keys_of(nb, LIVE)
    assert bool((bits(got[~key.any(1)]) == 0).all()), what                 # exactly +0 without a key
    if name == "f32":
        return within_composite(got, ref, comp, u, what)
    vabs = v.double().abs()[nb.rows.clamp(0, N - 1).long()].view(M, nb.rows.shape[1], H, -1).amax(3)
    vmax = vabs.masked_fill(~key[:, :, None], 0).amax(1)                     # [M, H]
    err = (got.double() - ref).abs().view(M, H, -1).amax(2)
    print(f"{what}: worst ratio {float((err / (4 * u * vmax).clamp_min(1e-300)).max()):.3f}")
    assert bool((err <= 4 * u * vmax).all()), what


@pytest.mark.parametrize("with_bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("S", [1, 5, 16, 33])
@pytest.mark.parametrize("H,D", HEADS)
@pytest.mark.parametrize("name", list(DTYPES))
def test_forward(cuda, name, H, D, S, with_bias):
    from spconv_amd.pytorch import functional as F
    nb = table(cuda, S, groups=False)
    q, k, v, bias, w, _ = inputs(cuda, name, H, D, S, with_bias)
    scale, dtype = D ** -0.5, DTYPES[name][0]
    got = F.neighbor_attention(q, k, v, nb, H, bias=bias)
    assert got.dtype == dtype and tuple(got.shape) == (M, H * D)
    assert_forward(got, attention(q, k, v, nb, LIVE, H, scale, bias, torch.float64),
                   attention(q, k, v, nb, LIVE, H, scale, bias, dtype), v, nb, H, name, "attention")
    got = F.neighbor_aggregate(w, v, nb)
    assert got.dtype == dtype and tuple(got.shape) == (M, H * D)
    assert_forward(got, aggregate(w, v, nb, LIVE, torch.float64), aggregate(w, v, nb, LIVE, dtype), v, nb, H, name,
                   "aggregate")


def grads(fn, tensors, dout):
    leaves = [t.detach().clone().requires_grad_(True) for t in tensors]
    out = fn(*leaves)
    return torch.autograd.grad(out, leaves, dout.to(out.dtype))


@pytest.mark.parametrize("S", [5, 33])
@pytest.mark.parametrize("H,D", HEADS)
@pytest.mark.parametrize("name", list(DTYPES))
def test_backward(cuda, name, H, D, S):
    from spconv_amd.pytorch import functional as F
    nb = table(cuda, S)
    q, k, v, bias, w, dout = inputs(cuda, name, H, D, S, True)
    scale, (dtype, u) = D ** -0.5, DTYPES[name]
    key, dead = keys_of(nb, LIVE), [UNNAMED] + list(range(LIVE, N))
    got = grads(lambda q, k, v, b: F.neighbor_attention(q, k, v, nb, H, bias=b), (q, k, v, bias), dout)
    ref = grads(lambda q, k, v, b: attention(q, k, v, nb, LIVE, H, scale, b, torch.float64),
                (q.double(), k.double(), v.double(), bias.double()), dout)
    comp = grads(lambda q, k, v, b: attention(q, k, v, nb, LIVE, H, scale, b, dtype), (q, k, v, bias), dout)
    for what, g, r, c in zip(("dq", "dk", "dv", "dbias"), got, ref, comp):
        assert g.dtype == (torch.float32 if what == "dbias" else dtype)
        within_composite(g, r, c, 2.0 ** -24 if what == "dbias" else u, what)
    assert bool((bits(got[1][dead]) == 0).all()) and bool((bits(got[2][dead]) == 0).all())
    assert bool((bits(got[3][~key]) == 0).all())
    got = grads(lambda w, v: F.neighbor_aggregate(w, v, nb), (w, v), dout)
    ref = grads(lambda w, v: aggregate(w, v, nb, LIVE, torch.float64), (w.double(), v.double()), dout)
    comp = grads(lambda w, v: aggregate(w, v, nb, LIVE, dtype), (w.to(dtype), v), dout)
    assert got[0].dtype == torch.float32 and got[1].dtype == dtype      # (w is float32 here: with_bias)
    within_composite(got[0], ref[0], comp[0], 2.0 ** -24, "dw")
    within_composite(got[1], ref[1], comp[1], u, "agg dv")
    assert bool((bits(got[0][~key]) == 0).all()) and bool((bits(got[1][dead]) == 0).all())


def test_missing_groups_are_refused(cuda):
    from spconv_amd.pytorch import functional as F
    nb = table(cuda, 5, groups=False)
    q, k, v, bias, w, _ = inputs(cuda, "f16", 3, 16, 5, True)
    with pytest.raises(ValueError, match="a gradient needs the neighbour groups"):
        F.neighbor_attention(q, k.requires_grad_(True), v, nb, 3)
    with pytest.raises(ValueError, match="a gradient needs the neighbour groups"):
        F.neighbor_aggregate(w, v.requires_grad_(True), nb)
    assert F.neighbor_attention(q.requires_grad_(True), k.detach(), v.detach(), nb, 3).requires_grad


def run_into(F, q, k, v, bias, w, dout, nb, H, scale):
    """forward and backward of both operators into NaN-filled buffers: (out, P, dq, dk, dv, dbias, agg, dw, agg dv)"""
    nan = lambda *shape, dtype=q.dtype: torch.full(shape, float("nan"), dtype=dtype, device=q.device)
    (Mq, S), n, C = nb.rows.shape, k.shape[0], q.shape[1]
    out, P, dq, dk, dv = nan(Mq, C), nan(Mq, S, H, dtype=torch.float32), nan(Mq, C), nan(n, C), nan(n, C)
    dbias, agg, dw, adv = nan(Mq, S, H, dtype=torch.float32), nan(Mq, C), nan(Mq, S, H, dtype=w.dtype), nan(n, C)
    F.neighbor_attention_into(q, k, v, nb, H, scale, bias, out, P)
    F.neighbor_attention_bwd_into(q, k, v, nb, H, scale, P, dout, dq, dk, dv, dbias)
    F.neighbor_aggregate_into(w, v, nb, agg)
    F.neighbor_aggregate_bwd_into(w, v, nb, dout, dw, adv)
    return out, P, dq, dk, dv, dbias, agg, dw, adv


def test_identical_bits(cuda):
    from spconv_amd.pytorch import functional as F
    H, D, S = 3, 16, 33
    nb = table(cuda, S)
    q, k, v, bias, w, dout = inputs(cuda, "f16", H, D, S, True)
    first = run_into(F, q, k, v, bias, w, dout, nb, H, 0.25)
    assert all(bool(torch.isfinite(t).all()) for t in first)            # (every element written)
    second = run_into(F, q, k, v, bias, w, dout, nb, H, 0.25)
    k[LIVE:], v[LIVE:] = float("nan"), float("nan")                     # dead rows are never read
    for other in (second, run_into(F, q, k, v, bias, w, dout, nb, H, 0.25)):
        for a, b in zip(first, other):
            np.testing.assert_array_equal(bits(a), bits(b))


def clouds(cuda, seed):
    g = torch.Generator().manual_seed(seed)
    pts = (torch.rand((200, 3), generator=g) * 4).to(cuda)
    bid = (torch.arange(200) % 2).to(torch.int32).to(cuda)
    return pts, bid


def test_public_tables(cuda):
    import spconv_amd.pytorch as spconv
    F = spconv.functional
    H, D = 2, 16
    pts, bid = clouds(cuda, 1)
    cells = torch.unique(torch.cat([bid[:, None], (pts / 0.5).floor().int().flip(1)], dim=1), dim=0).contiguous()
    x = spconv.SparseConvTensor(torch.zeros((cells.shape[0], 1), device=cuda), cells, [8, 8, 8], 2)
    tables = [F.knn_query(pts, bid, pts, bid, 2, 8, with_groups=True).neighbors(),
              F.voxel_query(pts, bid, x, [0.5] * 3, [0, 0, 0, 4, 4, 4], (1, 1, 1), 12, with_groups=True)]
    for nb in tables:
        Mq, S = nb.rows.shape
        assert int((nb.rows >= 0).sum()) > 4 * Mq
        q, k, v, bias, _, dout = inputs(cuda, "f32", H, D, S, True, Mq=Mq, n=nb.num_voxels)
        kv = torch.cat([k, v], dim=1)                                   # (k and v as the halves of one tensor)
        args = (q, kv[:, :H * D], kv[:, H * D:], bias)
        got = grads(lambda q, k, v, b: F.neighbor_attention(q, k, v, nb, H, bias=b), args, dout)
        ref = grads(lambda q, k, v, b: attention(q, k, v, nb, nb.num_voxels, H, D ** -0.5, b, torch.float64),
                    [t.double() for t in args], dout)
        comp = grads(lambda q, k, v, b: attention(q, k, v, nb, nb.num_voxels, H, D ** -0.5, b, torch.float32), args, dout)
        for what, g, r, c in zip(("dq", "dk", "dv", "dbias"), got, ref, comp):
            within_composite(g, r, c, 2.0 ** -24, what)
        np.testing.assert_array_equal(bits(F.neighbor_attention(*args[:3], nb, H)),     # (strided views, read in place)
                                      bits(F.neighbor_attention(q, k, v, nb, H)))
    layer = spconv.NeighborAttention(H * D, H).to(cuda)
    out = layer(q, k, tables[1])
    assert tuple(out.shape) == (200, H * D) and out.requires_grad


def test_capture_behind_knn_query(cuda):
    from spconv_amd.pytorch import functional as F
    from spconv_amd.pytorch._level import flat_groups
    H, D, K, n = 2, 16, 8, 200
    sets = [clouds(cuda, s) + inputs(cuda, "f16", H, D, K, True, seed=s, Mq=n, n=n) for s in (2, 3)]
    held = [torch.empty_like(t) for t in sets[0]]
    pts, bid, q, k, v, bias, w, dout = held
    rows = torch.empty((n, K), dtype=torch.int32, device=cuda)
    count = torch.empty((n,), dtype=torch.int32, device=cuda)
    bufs = [torch.empty_like(q), torch.empty_like(bias), torch.empty_like(q), torch.empty_like(k), torch.empty_like(v),
            torch.empty_like(bias)]

    def step():
        F.knn_query_into(pts, bid, None, pts, F.scene_groups(bid, n, 2), 3, K, 1e-8, False, rows, count)
        nb = F.VoxelNeighbors(rows, count, None, flat_groups(rows, n), n)
        out, P, dq, dk, dv, dbias = bufs
        F.neighbor_attention_into(q, k, v, nb, H, 0.25, bias, out, P)
        F.neighbor_attention_bwd_into(q, k, v, nb, H, 0.25, P, dout, dq, dk, dv, dbias)
        return [rows] + bufs

    def load(s):
        for dst, src in zip(held, sets[s]):
            dst.copy_(src)
    eager = []
    for s in (0, 1):
        load(s)
        eager.append([t.clone() for t in step()])
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
