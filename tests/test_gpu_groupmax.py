"""Fused set abstraction on the kernels of csrc/groupmax.hip (spconv_amd/pytorch/_groupmax.py) against a float64
restatement of its formulas in torch, over hand-built tables of N = 53 rows (LIVE = 50) whose float32 offsets are used as
given.

Criterion, forward and every gradient (the one of tests/test_gpu_nattn.py / test_gpu_kpconv.py): max|got - ref| <= 2
max|composite - ref| + u max|ref|, the composite being the same steps in the rows' dtype -- group_voxels, the position
term in float32, add, ReLU, cast, matmul, masked amax -- and u = 2^-11 (float16) or 2^-8 (bfloat16).  The max routes its
gradient discontinuously, so the gradient references route through the arg of the native forward, which is checked on
its own: a valid slot whose float64 value is within the forward's bound of the float64 maximum.  The float64
pre-activation of every valid slot is held away from 0 (|x| > 1e-5, asserted on the reference alone): the fp32 and fp64
ReLU masks are then the same set."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N, LIVE, HOT, SEED = 53, 50, 3, 1                 # (the seed: the first that meets the input condition of test_gradients)
DTYPES = {"f16": (torch.float16, 2.0 ** -11), "bf16": (torch.bfloat16, 2.0 ** -8)}
CENTRE = dict(M=50, S=16, C=(64, 32))
SHAPES = [CENTRE] + [dict(CENTRE, **{axis: v}) for axis, values in (
    ("M", (1, 17)), ("S", (1, 5, 33, 128)),
    ("C", ((16, 16), (32, 64), (128, 128), (256, 16), (16, 256), (144, 48), (256, 256)))) for v in values]
EDGE = dict(M=77, S=33, nq=70)


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
    return rows, offsets


def table(cuda, M, S, edges=False, groups=False, nq=None):
    from spconv_amd.pytorch import functional as F
    from spconv_amd.pytorch._level import flat_groups
    rows, offsets = (torch.from_numpy(t).to(cuda) for t in host_table(M, S, edges))
    live = torch.tensor([LIVE], dtype=torch.int32, device=cuda)
    n_queries = None if nq is None else torch.tensor([nq], dtype=torch.int32, device=cuda)
    return F.VoxelNeighbors(rows, (rows >= 0).sum(1).to(torch.int32), offsets,
                            flat_groups(rows, N, live) if groups else None, N, n_queries, live)


def inputs(cuda, name, M, Cin, Cout, seed=SEED):
    """feats, weight, pos_weight, in_bias, d_out"""
    g = torch.Generator().manual_seed(100000 * seed + 1000 * Cin + 10 * Cout + (name == "bf16"))
    dtype = DTYPES[name][0]
    feats = torch.randn((N, Cin), generator=g).to(dtype)
    weight = (torch.randn((Cin, Cout), generator=g) * Cin ** -0.5).to(dtype)
    pw, bias = torch.randn((3, Cin), generator=g), torch.randn((Cin,), generator=g) * 0.5
    return [t.to(cuda) for t in (feats, weight, pw, bias, torch.randn((M, Cout), generator=g).to(dtype))]


def valid_slots(nb, nq=None):
    M = nb.rows.shape[0]
    return (nb.rows >= 0) & (nb.rows < LIVE) & (torch.arange(M, device=nb.rows.device)[:, None] < (M if nq is None else nq))


def restated(feats, weight, pw, bias, nb, relu, dtype, nq=None, arg=None, parts=False):
    """the formulas in float64, or -- for a 16-bit dtype -- the composite a user would write without the kernels; with arg
    the max is the gather of that slot"""
    from spconv_amd.pytorch import functional as F
    exact = dtype == torch.float64
    real, valid = torch.float64 if exact else torch.float32, valid_slots(nb, nq)
    x = (feats[nb.rows.clamp(0, N - 1).long()] if exact else F.group_voxels(feats, nb)).to(real)
    if pw is not None:
        x = x + nb.offsets.to(real) @ pw.to(real)
    if bias is not None:
        x = x + bias.to(real)
    y = torch.matmul((x.clamp_min(0) if relu else x).to(dtype), weight)
    if parts:
        return x, y
    if arg is not None:
        return y.gather(1, arg.clamp(max=y.shape[1] - 1).long()[:, None])[:, 0].masked_fill(arg == 255, 0)
    return y.masked_fill(~valid[:, :, None], float("-inf")).amax(1).masked_fill(~valid.any(1)[:, None], 0)


def within_composite(got, ref, comp, u, what):
    got, ref, comp = got.detach(), ref.detach(), comp.detach()
    err, base = float((got.double() - ref).abs().max()), float((comp.double() - ref).abs().max())
    bound = 2 * base + u * float(ref.abs().max())
    print(f"{what}: err {err:.3e} bound {bound:.3e} ratio {err / bound if bound else 0:.3f}")
    assert err <= bound, what
    return bound


def forward_holds(cuda, name, nb, M, Cin, Cout, terms, relu, nq=None):
    from spconv_amd.pytorch import functional as F
    (dtype, u), (feats, weight, pw, bias, _) = DTYPES[name], inputs(cuda, name, M, Cin, Cout)
    pw, bias = (pw, bias) if terms else (None, None)
    got = F.group_linear_max(feats, nb, weight, pw, bias, relu)
    assert got.dtype == dtype and tuple(got.shape) == (M, Cout)
    within_composite(got, restated(feats.double(), weight.double(), pw, bias, nb, relu, torch.float64, nq),
                     restated(feats, weight, pw, bias, nb, relu, dtype, nq), u, "out")
    return got, (feats, weight, pw, bias)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "M{M}-S{S}-C{C[0]}x{C[1]}".format(**s))
@pytest.mark.parametrize("name", list(DTYPES))
def test_forward_shapes(cuda, name, shape):
    M, S, (Cin, Cout) = shape["M"], shape["S"], shape["C"]
    forward_holds(cuda, name, table(cuda, M, S), M, Cin, Cout, True, True)


@pytest.mark.parametrize("relu", [False, True], ids=["linear", "relu"])
@pytest.mark.parametrize("terms", [False, True], ids=["rows", "xyz"])
@pytest.mark.parametrize("name", list(DTYPES))
def test_forward_variants(cuda, name, terms, relu):
    forward_holds(cuda, name, table(cuda, 50, 16), 50, 64, 32, terms, relu)


@pytest.mark.parametrize("name", list(DTYPES))
def test_edges(cuda, name):
    from spconv_amd.pytorch import functional as F
    M, S, nq, Cin, Cout = EDGE["M"], EDGE["S"], EDGE["nq"], 64, 32
    nb = table(cuda, M, S, edges=True, nq=nq)
    got, (feats, weight, pw, bias) = forward_holds(cuda, name, nb, M, Cin, Cout, True, True, nq)
    out, arg = torch.empty_like(got), torch.empty((M, Cout), dtype=torch.uint8, device=cuda)
    ws = torch.empty((F.group_linear_max_ws_bytes(M, S, Cin, Cout),), dtype=torch.uint8, device=cuda)
    F.group_linear_max_into(feats, nb, weight, pw, bias, True, out, arg, ws)
    np.testing.assert_array_equal(bits(out), bits(got))
    empty = ~valid_slots(nb, nq).any(1)
    assert bool(empty[[5, 8]].all()) and bool(empty[nq:].all())
    assert bool((bits(got[empty]) == 0).all()) and bool((arg[empty] == 255).all())     # exactly +0, no slot
    assert bool((arg[~empty] < S).all())
    feats[LIVE:] = float("nan")                                     # dead rows are never read
    np.testing.assert_array_equal(bits(F.group_linear_max(feats, nb, weight, pw, bias)), bits(got))
    # pad="first" style: every slot from 5 on repeats slot 0, offsets included; the lowest slot keeps the tie
    rows, offsets = nb.rows.clone(), nb.offsets.clone()
    rows[:, 5:], offsets[:, 5:] = rows[:, :1], offsets[:, :1]
    dup = F.VoxelNeighbors(rows, None, offsets, None, N, nb.n_queries, nb.n_live)
    F.group_linear_max_into(feats, dup, weight, pw, bias, True, out, arg, ws)
    assert bool(((arg < 5) | (arg == 255)).all()) and bool((arg < 5).any())


def grads(fn, tensors, dout):
    leaves = [t.detach().clone().requires_grad_(True) for t in tensors]
    out = fn(*leaves)
    return (out,) + torch.autograd.grad(out, leaves, dout.to(out.dtype))


@pytest.mark.parametrize("S,Cin,Cout", [(16, 64, 32), (33, 128, 128)])
@pytest.mark.parametrize("name", list(DTYPES))
def test_gradients(cuda, name, S, Cin, Cout):
    from spconv_amd.pytorch import functional as F
    M, nq = EDGE["M"], EDGE["nq"]
    nb, (dtype, u) = table(cuda, M, S, edges=True, groups=True, nq=nq), DTYPES[name]
    feats, weight, pw, bias, dout = inputs(cuda, name, M, Cin, Cout)
    wide, valid = (feats.double(), weight.double(), pw.double(), bias.double()), valid_slots(nb, nq)
    x64, y64 = restated(*wide, nb, True, torch.float64, nq, parts=True)
    assert float(x64[valid].abs().min()) > 1e-5                     # the input condition of the ReLU mask
    out, arg = torch.empty((M, Cout), dtype=dtype, device=cuda), torch.empty((M, Cout), dtype=torch.uint8, device=cuda)
    ws = torch.empty((F.group_linear_max_ws_bytes(M, S, Cin, Cout),), dtype=torch.uint8, device=cuda)
    F.group_linear_max_into(feats, nb, weight, pw, bias, True, out, arg, ws)
    bound = within_composite(out, restated(*wide, nb, True, torch.float64, nq),
                             restated(feats, weight, pw, bias, nb, True, dtype, nq), u, "out")
    has = valid.any(1)
    assert bool((arg[~has] == 255).all()) and bool(valid[has].gather(1, arg[has].long()).all())     # arg names a valid slot ...
    top = y64.masked_fill(~valid[:, :, None], float("-inf")).amax(1)[has]
    assert bool((y64[has].gather(1, arg[has].long()[:, None])[:, 0] >= top - bound).all())     # ... that holds the maximum
    got = grads(lambda f, w, p, b: F.group_linear_max(f, nb, w, p, b), (feats, weight, pw, bias), dout)
    np.testing.assert_array_equal(bits(got[0]), bits(out))
    ref = grads(lambda f, w, p, b: restated(f, w, p, b, nb, True, torch.float64, nq, arg), wide, dout)
    comp = grads(lambda f, w, p, b: restated(f, w, p, b, nb, True, dtype, nq, arg), (feats, weight, pw, bias), dout)
    for what, g, r, c in zip(("out", "dfeats", "dweight", "dpos_weight", "din_bias"), got, ref, comp):
        assert g.dtype == c.dtype
        within_composite(g, r, c, u, what)
    assert bool((bits(got[1][LIVE:]) == 0).all())
    again = grads(lambda f, w, p, b: F.group_linear_max(f, nb, w, p, b), (feats, weight, pw, bias), dout)
    for a, b in zip(got, again):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))


def test_capture(cuda):
    from spconv_amd.pytorch import functional as F
    from spconv_amd.pytorch._level import flat_groups
    M, S, Cin, Cout, name = 50, 16, 64, 32, "f16"
    live = torch.tensor([LIVE], dtype=torch.int32, device=cuda)
    sets = []
    for seed, nq in ((0, M), (1, 33)):
        rows, offsets = host_table(M + seed, S, True)
        sets.append([torch.from_numpy(rows[:M].copy()).to(cuda), torch.from_numpy(offsets[:M].copy()).to(cuda)] +
                    inputs(cuda, name, M, Cin, Cout, seed + 1) + [torch.tensor([nq], dtype=torch.int32, device=cuda)])
    held = [torch.empty_like(t) for t in sets[0]]
    rows, offsets, feats, weight, pw, bias, dout, nq = held
    nan = lambda *shape, dtype=feats.dtype: torch.full(shape, float("nan"), dtype=dtype, device=cuda)
    out, dg, dfeats, dweight = nan(M, Cout), nan(M, S, Cin), nan(N, Cin), nan(Cin, Cout)
    dpos, dbias = nan(3, Cin, dtype=torch.float32), nan(Cin, dtype=torch.float32)
    arg = torch.full((M, Cout), 77, dtype=torch.uint8, device=cuda)
    ws = torch.empty((F.group_linear_max_ws_bytes(M, S, Cin, Cout),), dtype=torch.uint8, device=cuda)
    bws = torch.empty((F.group_linear_max_ws_bytes(M, S, Cin, Cout, True),), dtype=torch.uint8, device=cuda)

    def step():
        nb = F.VoxelNeighbors(rows, None, offsets, flat_groups(rows, N, live), N, nq, live)
        F.group_linear_max_into(feats, nb, weight, pw, bias, True, out, arg, ws)
        F.group_linear_max_bwd_into(feats, nb, weight, pw, bias, True, arg, dout, dg, dfeats, dweight, dpos, dbias, bws)
        return [out, arg, dg, dfeats, dweight, dpos, dbias]

    def load(s):
        for dst, src in zip(held, sets[s]):
            dst.copy_(src)
    eager = []
    for s in (0, 1):
        load(s)
        eager.append([t.clone() for t in step()])
    assert all(bool(torch.isfinite(t.float()).all()) for t in eager[1])         # (every element written)
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
            assert torch.equal(got.view(torch.uint8), want.view(torch.uint8))


def test_module_equals_functional(cuda):
    import spconv_amd.pytorch as spconv
    F = spconv.functional
    nb = table(cuda, 50, 16, edges=True, groups=True)
    feats, _, _, _, dout = inputs(cuda, "f16", 50, 32, 48)
    layer = spconv.GroupLinearMax(32, 48).to(cuda)
    with torch.no_grad():
        layer.in_bias.copy_(torch.randn((32,), generator=torch.Generator().manual_seed(3)))
    params = (layer.weight.detach().half(), layer.pos_weight.detach(), layer.in_bias.detach())
    want = grads(lambda f, w, p, b: F.group_linear_max(f, nb, w, p, b), (feats,) + params, dout)
    out = layer(feats.requires_grad_(True), nb)
    out.backward(dout)
    got = (out, feats.grad, layer.weight.grad.half(), layer.pos_weight.grad, layer.in_bias.grad)
    for a, b in zip(got, want):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
    assert bool(out.abs().sum() > 0)
