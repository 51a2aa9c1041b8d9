"""Kernel point convolution on the kernels of csrc/kpconv.hip (spconv_amd/pytorch/_kpconv.py) against a float64
restatement of its formulas in torch, over hand-built tables of N = 53 rows whose float32 offsets are used as given
(|offset - kernel point| / sigma spans 0 .. 2.5: both branches of the max occur).

Criterion, forward and both gradients (the one of tests/test_gpu_nattn.py): max|got - ref| <= 2 max|composite - ref| + u
max|ref|, the composite being the same torch ops in the rows' dtype -- group_voxels, h in float32 cast to the dtype, two
einsums -- and u = 2^-11 (float16) or 2^-8 (bfloat16)."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N, LIVE, HOT, SIGMA = 53, 50, 3, 0.6
DTYPES = {"f16": (torch.float16, 2.0 ** -11), "bf16": (torch.bfloat16, 2.0 ** -8)}
CENTRE = dict(M=50, S=16, K=15, C=(64, 32))
SHAPES = [CENTRE] + [dict(CENTRE, **{axis: v}) for axis, values in (
    ("M", (1, 17)), ("S", (1, 5, 33)), ("K", (1, 16)),
    ("C", ((16, 16), (32, 64), (128, 128), (256, 16), (16, 256), (144, 48)))) for v in values]


def bits(t):
    return t.detach().contiguous().view(torch.int16).cpu().numpy()


@functools.lru_cache(maxsize=None)
def host_table(M, S, edges):
    g = np.random.default_rng(100 * M + S)
    rows = g.integers(0, LIVE, size=(M, S)).astype(np.int32)
    offsets = g.uniform(-0.6, 0.6, size=(M, S, 3)).astype(np.float32)
    if edges:
        rows[g.random((M, S)) < 0.4] = HOT                          # one row that more than 300 entries name
        rows[g.random((M, S)) < 0.2] = -1                           # holes anywhere in a row
        rows[5], rows[8] = -1, 51                                   # no slot at all; dead rows only
        rows[9, 0], rows[9, 1], rows[9, -1] = 50, 52, -1            # dead rows named next to live ones
        assert S < 33 or (rows == HOT).sum() > 300
    return rows, offsets


def table(cuda, M, S, edges=False, groups=False, nq=None):
    from spconv_amd.pytorch import functional as F
    from spconv_amd.pytorch._level import flat_groups
    rows, offsets = (torch.from_numpy(t).to(cuda) for t in host_table(M, S, edges))
    live = torch.tensor([LIVE], dtype=torch.int32, device=cuda)
    n_queries = None if nq is None else torch.tensor([nq], dtype=torch.int32, device=cuda)
    return F.VoxelNeighbors(rows, (rows >= 0).sum(1).to(torch.int32), offsets,
                            flat_groups(rows, N, live) if groups else None, N, n_queries, live)


def kernel_points(cuda, K):
    from spconv_amd.pytorch._kpconv import default_kernel_points
    return torch.cat([default_kernel_points(0.5), torch.tensor([[0.2, 0.1, -0.3]])])[:K].contiguous().to(cuda)


def inputs(cuda, name, M, K, Cin, Cout):
    g = torch.Generator().manual_seed(1000 * Cin + 10 * Cout + K)
    dtype = DTYPES[name][0]
    feats = torch.randn((N, Cin), generator=g).to(dtype).to(cuda)
    weight = (torch.randn((K, Cin, Cout), generator=g) * (K * Cin) ** -0.5).to(dtype).to(cuda)
    return feats, weight, torch.randn((M, Cout), generator=g).to(dtype).to(cuda)


def restated(feats, weight, nb, kp, normalize, dtype, nq=None):
    """the formulas in float64, or -- for a 16-bit dtype -- the composite a user would write without the kernels"""
    from spconv_amd.pytorch import functional as F
    (M, S), exact = nb.rows.shape, dtype == torch.float64
    valid = (nb.rows >= 0) & (nb.rows < LIVE) & (torch.arange(M, device=feats.device)[:, None] < (M if nq is None else nq))
    real = torch.float64 if exact else torch.float32
    d = (nb.offsets.to(real)[:, :, None, :] - kp.to(real)[None, None]).square().sum(3).sqrt()
    h = (1 - d / SIGMA).clamp_min(0).masked_fill(~valid[:, :, None], 0).to(dtype)
    grouped = feats[nb.rows.clamp(0, N - 1).long()] if exact else F.group_voxels(feats, nb)
    out = torch.einsum("mkc,kcd->md", torch.einsum("msk,msc->mkc", h, grouped), weight)
    return out / valid.sum(1).clamp_min(1)[:, None].to(dtype) if normalize else out


def within_composite(got, ref, comp, u, what):
    got, ref, comp = got.detach(), ref.detach(), comp.detach()
    err, base = float((got.double() - ref).abs().max()), float((comp.double() - ref).abs().max())
    bound = 2 * base + u * float(ref.abs().max())
    print(f"{what}: err {err:.3e} bound {bound:.3e} ratio {err / bound if bound else 0:.3f}")
    assert err <= bound, what


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "M{M}-S{S}-K{K}-C{C[0]}x{C[1]}".format(**s))
@pytest.mark.parametrize("name", list(DTYPES))
def test_forward_shapes(cuda, name, shape):
    from spconv_amd.pytorch import functional as F
    M, S, K, (Cin, Cout) = shape["M"], shape["S"], shape["K"], shape["C"]
    nb, kp, (dtype, u) = table(cuda, M, S), kernel_points(cuda, K), DTYPES[name]
    feats, weight, _ = inputs(cuda, name, M, K, Cin, Cout)
    got = F.kpconv(feats, nb, kp, weight, SIGMA)
    assert got.dtype == dtype and tuple(got.shape) == (M, Cout)
    within_composite(got, restated(feats.double(), weight.double(), nb, kp, False, torch.float64),
                     restated(feats, weight, nb, kp, False, dtype), u, "out")


@pytest.mark.parametrize("normalize", [False, True], ids=["sum", "normalize"])
@pytest.mark.parametrize("name", list(DTYPES))
def test_edges(cuda, name, normalize):
    from spconv_amd.pytorch import functional as F
    M, S, K, Cin, Cout, nq = 77, 33, 15, 64, 32, 70
    nb, kp, (dtype, u) = table(cuda, M, S, edges=True, nq=nq), kernel_points(cuda, K), DTYPES[name]
    feats, weight, _ = inputs(cuda, name, M, K, Cin, Cout)
    got = F.kpconv(feats, nb, kp, weight, SIGMA, normalize)
    within_composite(got, restated(feats.double(), weight.double(), nb, kp, normalize, torch.float64, nq),
                     restated(feats, weight, nb, kp, normalize, dtype, nq), u, "out")
    assert bool((bits(got[[5, 8]]) == 0).all())                     # exactly +0 without a valid slot
    assert bool((bits(got[nq:]) == 0).all())                        # the rows beyond the device n_queries
    feats[LIVE:] = float("nan")                                     # dead rows are never read
    np.testing.assert_array_equal(bits(F.kpconv(feats, nb, kp, weight, SIGMA, normalize)), bits(got))


def grads(fn, tensors, dout):
    leaves = [t.detach().clone().requires_grad_(True) for t in tensors]
    out = fn(*leaves)
    return (out,) + torch.autograd.grad(out, leaves, dout.to(out.dtype))


@pytest.mark.parametrize("normalize", [False, True], ids=["sum", "normalize"])
@pytest.mark.parametrize("S,Cin,Cout", [(16, 64, 32), (33, 128, 128)])
@pytest.mark.parametrize("name", list(DTYPES))
def test_gradients(cuda, name, S, Cin, Cout, normalize):
    from spconv_amd.pytorch import functional as F
    M, K, nq = 50, 15, 47
    nb, kp, (dtype, u) = table(cuda, M, S, edges=True, groups=True, nq=nq), kernel_points(cuda, K), DTYPES[name]
    feats, weight, dout = inputs(cuda, name, M, K, Cin, Cout)
    got = grads(lambda f, w: F.kpconv(f, nb, kp, w, SIGMA, normalize), (feats, weight), dout)
    ref = grads(lambda f, w: restated(f, w, nb, kp, normalize, torch.float64, nq), (feats.double(), weight.double()), dout)
    comp = grads(lambda f, w: restated(f, w, nb, kp, normalize, dtype, nq), (feats, weight), dout)
    for what, g, r, c in zip(("out", "dfeats", "dweight"), got, ref, comp):
        assert g.dtype == dtype
        within_composite(g, r, c, u, what)
    assert bool((bits(got[1][LIVE:]) == 0).all())
    again = grads(lambda f, w: F.kpconv(f, nb, kp, w, SIGMA, normalize), (feats, weight), dout)
    for a, b in zip(got, again):
        np.testing.assert_array_equal(bits(a), bits(b))


def test_capture(cuda):
    from spconv_amd.pytorch import functional as F
    from spconv_amd.pytorch._level import flat_groups
    M, S, K, Cin, Cout, name = 50, 16, 15, 64, 32, "f16"
    kp, live = kernel_points(cuda, K), torch.tensor([LIVE], dtype=torch.int32, device=cuda)
    sets = []
    for seed, nq in ((0, M), (1, 33)):
        rows, offsets = host_table(M + seed, S, True)
        feats, weight, dout = inputs(cuda, name, M, K, Cin + 16 * seed, Cout)
        sets.append([torch.from_numpy(rows[:M].copy()).to(cuda), torch.from_numpy(offsets[:M].copy()).to(cuda),
                     feats[:, :Cin].contiguous(), weight[:, :Cin].contiguous(), dout,
                     torch.tensor([nq], dtype=torch.int32, device=cuda)])
    held = [torch.empty_like(t) for t in sets[0]]
    rows, offsets, feats, weight, dout, nq = held
    nan = lambda *shape: torch.full(shape, float("nan"), dtype=feats.dtype, device=cuda)
    out, wf, dg, dfeats, dweight = nan(M, Cout), nan(M, K, Cin), nan(M, S, Cin), nan(N, Cin), nan(K, Cin, Cout)
    ws = torch.empty((F.kpconv_ws_bytes(M, K, Cin, Cout),), dtype=torch.uint8, device=cuda)
    bws = torch.empty((F.kpconv_ws_bytes(M, K, Cin, Cout, True),), dtype=torch.uint8, device=cuda)

    def step():
        nb = F.VoxelNeighbors(rows, None, offsets, flat_groups(rows, N, live), N, nq, live)
        F.kpconv_into(feats, nb, kp, weight, SIGMA, True, out, wf, ws)
        F.kpconv_bwd_into(wf, nb, kp, weight, SIGMA, True, dout, dg, dfeats, dweight, bws)
        return [out, dg, dfeats, dweight]

    def load(s):
        for dst, src in zip(held, sets[s]):
            dst.copy_(src)
    eager = []
    for s in (0, 1):
        load(s)
        eager.append([t.clone() for t in step()])
    assert all(bool(torch.isfinite(t).all()) for t in eager[1])         # (every element written)
    assert bool((bits(eager[1][0][33:]) == 0).all()) and not torch.equal(eager[0][0], eager[1][0])
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


def test_module_behind_knn_query(cuda):
    import spconv_amd.pytorch as spconv
    F = spconv.functional
    g = torch.Generator().manual_seed(7)
    pts = (torch.rand((200, 3), generator=g) * 2).to(cuda)
    bid = (torch.arange(200) % 2).to(torch.int32).to(cuda)
    nb = F.knn_query(pts, bid, pts, bid, 2, 16, with_offsets=True, with_groups=True).neighbors()
    layer = spconv.KPConv(32, 48, sigma=SIGMA, kp_radius=0.5, normalize=True).to(cuda)
    feats = torch.randn((200, 32), generator=g).half().to(cuda)
    dout = torch.randn((200, 48), generator=g).half().to(cuda)
    kp = layer.kernel_points

    def exact(f, w, dtype):
        valid = nb.rows >= 0
        real = torch.float64 if dtype == torch.float64 else torch.float32
        d = (nb.offsets.to(real)[:, :, None, :] - kp.to(real)[None, None]).square().sum(3).sqrt()
        h = (1 - d / SIGMA).clamp_min(0).masked_fill(~valid[:, :, None], 0).to(dtype)
        grouped = f[nb.rows.clamp(0, 199).long()] if dtype == torch.float64 else F.group_voxels(f, nb)
        out = torch.einsum("mkc,kcd->md", torch.einsum("msk,msc->mkc", h, grouped), w)
        return out / valid.sum(1).clamp_min(1)[:, None].to(dtype)
    weight = layer.weight.detach().half()                               # (the layer runs its weight in the rows' dtype)
    got = grads(lambda f, w: F.kpconv(f, nb, kp, w, SIGMA, True), (feats, weight), dout)
    ref = grads(lambda f, w: exact(f, w, torch.float64), (feats.double(), weight.double()), dout)
    comp = grads(lambda f, w: exact(f, w, torch.float16), (feats, weight), dout)
    for what, a, r, c in zip(("out", "dfeats", "dweight"), got, ref, comp):
        within_composite(a, r, c, 2.0 ** -11, what)
    out = layer(feats.requires_grad_(True), nb)
    np.testing.assert_array_equal(bits(out), bits(got[0]))
    out.backward(dout)
    np.testing.assert_array_equal(bits(layer.weight.grad.half()), bits(got[2]))
    np.testing.assert_array_equal(bits(feats.grad), bits(got[1]))
    other = spconv.KPConv(32, 48, sigma=SIGMA, kp_radius=0.5, normalize=True).to(cuda)
    other.load_state_dict(layer.state_dict())
    np.testing.assert_array_equal(bits(other(feats, nb)), bits(out))
