"""Selective scan, causal convolution and SerializedMamba on the kernels of csrc/scan.hip (spconv_amd/pytorch/_scan.py)
against a plain float64 torch loop, one step per position, whose gradients come from autograd through the loop.  The
composite is the same loop in float32 on the inputs as given, its result rounded to their dtype.

Criterion, per tensor: max|got - ref| <= 2 max|composite - ref| + u max|ref|, u the unit roundoff of the tensor's dtype.

One scene set, T = _scan.CHUNK: sequences of 0, 1, T - 1, T, T + 1 and 2 T + 3 positions, then 5 rows of no sequence;
the order is the identity or a fixed permutation; delta is log-uniform in [1e-3, 1e-1] and A[d, k] = -(k + 1), so a state
entering a chunk is far above the tolerance at the chunk's first rows (test_dropped_carry_would_fail)."""
import functools

import numpy as np
import pytest
import torch

from spconv_amd.pytorch import _scan

pytestmark = pytest.mark.gpu

T = _scan.CHUNK
LENS = (0, 1, T - 1, T, T + 1, 2 * T + 3)
DEAD = 5
N_ROWS = sum(LENS) + DEAD
OFFSETS = np.concatenate([[0], np.cumsum(LENS)]).astype(np.int32)
PERM = np.random.default_rng(7).permutation(N_ROWS).astype(np.int32)
DTYPES = {"f16": (torch.float16, 2.0 ** -11), "bf16": (torch.bfloat16, 2.0 ** -8), "f32": (torch.float32, 2.0 ** -24)}
SHAPES = [(64, 1), (192, 1), (128, 2)]
SCAN_NAMES = ("u", "delta", "A", "B", "C", "D", "z", "delta_bias")


def bits(t):
    t = t.detach().contiguous()
    return t.view({2: torch.int16, 4: torch.int32}[t.element_size()]).cpu().numpy()


def within_composite(got, ref, comp, u, what):
    err, base = float((got.detach().double().cpu() - ref).abs().max()), float((comp.double() - ref).abs().max())
    bound = 2 * base + u * float(ref.abs().max())
    print(f"{what}: err {err:.3e} bound {bound:.3e} ratio {err / bound if bound else 0:.3f}")
    assert err <= bound, what


def walks(offsets, order, reverse):
    """per sequence the rows in walk order"""
    rows = np.arange(N_ROWS) if order is None else order
    out = [rows[offsets[s]:offsets[s + 1]] for s in range(len(offsets) - 1)]
    return [torch.from_numpy((w[::-1] if reverse else w).copy()).long() for w in out]


def scan_loop(u, delta, A, B, C, D, z, bias, softplus, seqs, work, reset_every=0):
    """the arithmetic of selective_scan, one step per position, in `work` precision; the result in u's dtype"""
    n, Dm = u.shape
    cpg = Dm // B.shape[1]
    dt = delta.to(work) + (0 if bias is None else bias.to(work))
    if softplus:
        dt = torch.where(dt <= 20, torch.log1p(torch.exp(dt)), dt)
    dA = torch.exp(dt[:, :, None] * A.to(work))
    dBu = (dt * u.to(work))[:, :, None] * B.to(work).repeat_interleave(cpg, dim=1)
    Cx = C.to(work).repeat_interleave(cpg, dim=1)
    rows, ys = [], []
    for walk in seqs:
        h = torch.zeros((Dm, A.shape[1]), dtype=work)
        for i, r in enumerate(walk.tolist()):
            if reset_every and i % reset_every == 0:
                h = torch.zeros_like(h)
            h = dA[r] * h + dBu[r]
            rows.append(r)
            ys.append((h * Cx[r]).sum(1))
    y = torch.zeros((n, Dm), dtype=work).index_copy(0, torch.tensor(rows), torch.stack(ys))
    if D is not None:
        live = torch.zeros((n, 1), dtype=work).index_fill(0, torch.tensor(rows), 1)          # (rows of no sequence stay zero)
        y = y + D.to(work) * u.to(work) * live
    if z is not None:
        y = y * z.to(work) * torch.sigmoid(z.to(work))
    return y.to(u.dtype)


@functools.lru_cache(maxsize=None)
def scan_inputs(name, Dm, G, full):
    g = torch.Generator().manual_seed(100 * Dm + 10 * G + full)
    dtype = DTYPES[name][0]
    rand = lambda *s: torch.randn(s, generator=g)
    dt = torch.exp(torch.rand((N_ROWS, Dm), generator=g) * np.log(100.0) + np.log(1e-3))
    bias = rand(Dm) * 0.5 if full else None
    delta = torch.log(torch.expm1(dt)) - bias if full else dt              # (softplus(delta + bias) gives dt back)
    A = -torch.arange(1, 17, dtype=torch.float32).repeat(Dm, 1)
    args = dict(u=rand(N_ROWS, Dm).to(dtype), delta=delta.to(dtype), A=A, B=rand(N_ROWS, G, 16).to(dtype),
                C=rand(N_ROWS, G, 16).to(dtype), D=rand(Dm) if full else None, z=rand(N_ROWS, Dm).to(dtype) if full else None,
                delta_bias=bias)
    return args, rand(N_ROWS, Dm).to(dtype)


@functools.lru_cache(maxsize=None)
def scan_expected(name, Dm, G, full, reverse, perm, work):
    """(y, {name: gradient}) of the loop in `work` precision on the inputs of `name`"""
    args, dout = scan_inputs(name, Dm, G, full)
    cast = (lambda t: t.double()) if work == torch.float64 else (lambda t: t)
    leaves = {k: cast(v).clone().requires_grad_(True) for k, v in args.items() if v is not None}
    y = scan_loop(*(leaves.get(k) for k in SCAN_NAMES), full, walks(OFFSETS, PERM if perm else None, reverse), work)
    grads = torch.autograd.grad(y, list(leaves.values()), cast(dout))
    return y.detach(), dict(zip(leaves, grads))


def native_scan(cuda, name, Dm, G, full, reverse, perm, grad):
    from spconv_amd.pytorch import functional as F
    args, dout = scan_inputs(name, Dm, G, full)
    seq = F.scan_sequences(offsets=torch.from_numpy(OFFSETS).to(cuda), order=torch.from_numpy(PERM).to(cuda) if perm else None,
                           n=N_ROWS)
    leaves = {k: v.to(cuda).requires_grad_(grad) for k, v in args.items() if v is not None}
    y = F.selective_scan(*(leaves.get(k) for k in SCAN_NAMES), full, seq=seq, reverse=reverse)
    return y, (dict(zip(leaves, torch.autograd.grad(y, list(leaves.values()), dout.to(cuda)))) if grad else None)


def dead_rows(perm):
    return (PERM if perm else np.arange(N_ROWS))[-DEAD:]


def test_dropped_carry_would_fail():
    args, _ = scan_inputs("f32", 64, 1, False)
    last = [walks(OFFSETS, None, False)[-1]]
    vals = [args[k] for k in SCAN_NAMES]
    ref = scan_loop(*(None if v is None else v.double() for v in vals), False, last, torch.float64)
    comp = scan_loop(*vals, False, last, torch.float32)
    broken = scan_loop(*vals, False, last, torch.float32, reset_every=T)
    with pytest.raises(AssertionError):
        within_composite(broken, ref, comp, 2.0 ** -11, "an entry state of zero")          # (even at f16's roundoff)


@pytest.mark.parametrize("perm", [False, True], ids=["identity", "perm"])
@pytest.mark.parametrize("reverse", [False, True], ids=["fwd", "rev"])
@pytest.mark.parametrize("full", [False, True], ids=["plain", "full"])
@pytest.mark.parametrize("Dm,G", SHAPES)
@pytest.mark.parametrize("name", list(DTYPES))
def test_scan_forward(cuda, name, Dm, G, full, reverse, perm):
    got, _ = native_scan(cuda, name, Dm, G, full, reverse, perm, False)
    ref, _ = scan_expected(name, Dm, G, full, reverse, perm, torch.float64)
    comp, _ = scan_expected(name, Dm, G, full, reverse, perm, torch.float32)
    assert got.dtype == DTYPES[name][0] and tuple(got.shape) == (N_ROWS, Dm)
    within_composite(got, ref, comp, DTYPES[name][1], "y")
    assert bool((bits(got)[dead_rows(perm)] == 0).all())                                     # exactly +0


@pytest.mark.parametrize("perm", [False, True], ids=["identity", "perm"])
@pytest.mark.parametrize("reverse", [False, True], ids=["fwd", "rev"])
@pytest.mark.parametrize("full", [False, True], ids=["plain", "full"])
@pytest.mark.parametrize("Dm,G", SHAPES)
@pytest.mark.parametrize("name", ["f16", "f32"])
def test_scan_backward(cuda, name, Dm, G, full, reverse, perm):
    _, got = native_scan(cuda, name, Dm, G, full, reverse, perm, True)
    _, ref = scan_expected(name, Dm, G, full, reverse, perm, torch.float64)
    _, comp = scan_expected(name, Dm, G, full, reverse, perm, torch.float32)
    assert sorted(got) == sorted(ref) and len(got) == (8 if full else 5)
    for k in got:
        rows = k in ("u", "delta", "B", "C", "z")
        assert got[k].dtype == (DTYPES[name][0] if rows else torch.float32)
        within_composite(got[k], ref[k], comp[k], DTYPES[name][1] if rows else 2.0 ** -24, "d" + k)
        assert not rows or bool((bits(got[k])[dead_rows(perm)] == 0).all())
    _, again = native_scan(cuda, name, Dm, G, full, reverse, perm, True)
    for k in got:
        np.testing.assert_array_equal(bits(got[k]), bits(again[k]))


def conv_loop(x, w, b, act, seqs, work):
    """out[r(p)] = act(b + sum_j w[:, j] x[r(p - (W - 1) + j)]) along every walk, taps before its start zero"""
    W = w.shape[1]
    out = torch.zeros(x.shape, dtype=work)
    for walk in seqs:
        rows = walk.tolist()
        for i, r in enumerate(rows):
            acc = b.to(work)
            for j in range(W):
                if i - (W - 1) + j >= 0:
                    acc = acc + w[:, j].to(work) * x[rows[i - (W - 1) + j]].to(work)
            out = out.index_copy(0, torch.tensor([r]), (acc * torch.sigmoid(acc) if act else acc)[None])
    return out.to(x.dtype)


@pytest.mark.parametrize("reverse", [False, True], ids=["fwd", "rev"])
@pytest.mark.parametrize("act", [None, "silu"])
@pytest.mark.parametrize("W", [2, 4])
@pytest.mark.parametrize("name", ["f16", "f32"])
def test_convolution(cuda, name, W, act, reverse):
    from spconv_amd.pytorch import functional as F
    (dtype, u), Dm = DTYPES[name], 128
    g = torch.Generator().manual_seed(W)
    x, dout = (torch.randn((N_ROWS, Dm), generator=g).to(dtype) for _ in range(2))
    w, b = torch.randn((Dm, W), generator=g) * 0.5, torch.randn((Dm,), generator=g)       # (float32 parameters)
    seqs = walks(OFFSETS, PERM, reverse)
    want = []
    for work in (torch.float64, torch.float32):
        cast = (lambda t: t.double()) if work == torch.float64 else (lambda t: t)
        leaves = [cast(t).clone().requires_grad_(True) for t in (x, w, b)]
        out = conv_loop(*leaves, act, seqs, work)
        want.append([out.detach()] + list(torch.autograd.grad(out, leaves, cast(dout))))
    seq = F.scan_sequences(offsets=torch.from_numpy(OFFSETS).to(cuda), order=torch.from_numpy(PERM).to(cuda))
    leaves = [t.to(cuda).requires_grad_(True) for t in (x, w, b)]
    out = F.causal_conv1d_rows(*leaves, seq=seq, reverse=reverse, activation=act)
    got = [out] + list(torch.autograd.grad(out, leaves, dout.to(cuda)))
    for what, t, r, c in zip(("out", "dx", "dweight", "dbias"), got, *want):
        within_composite(t, r, c, u if what in ("out", "dx") else 2.0 ** -24, what)
    assert bool((bits(got[0])[PERM[-DEAD:]] == 0).all()) and bool((bits(got[1])[PERM[-DEAD:]] == 0).all())


def test_capture_replays_other_offsets(cuda):
    from spconv_amd.pytorch import functional as F
    Dm, G, W, dtype = 128, 2, 4, torch.float16
    args, dout = scan_inputs("f16", Dm, G, True)
    a = {k: v.to(cuda) for k, v in args.items()}
    g = torch.Generator().manual_seed(3)
    w, b, dout = torch.randn((Dm, W), generator=g).to(cuda), torch.randn((Dm,), generator=g).to(cuda), dout.to(cuda)
    shorter = OFFSETS.copy()
    shorter[-1] -= T + 2                                                  # (one chunk and more rows of no sequence)
    offsets = torch.empty(len(OFFSETS), dtype=torch.int32, device=cuda)
    new = lambda t: torch.full_like(t, float("nan"))
    f32 = lambda *s: torch.full(s, float("nan"), device=cuda)
    bufs = [new(a["u"]) for _ in range(6)] + [new(a["B"]), new(a["C"]), f32(Dm, 16), f32(Dm), f32(Dm), f32(Dm, W), f32(Dm)]
    ws = torch.empty(_scan.scan_ws_bytes(N_ROWS, len(LENS), Dm, G), dtype=torch.uint8, device=cuda)
    cws = torch.empty(_scan.conv_ws_bytes(N_ROWS, Dm, W), dtype=torch.uint8, device=cuda)
    order = torch.from_numpy(PERM).to(cuda)

    def step():
        seq = F.scan_sequences(offsets=offsets, order=order)
        x, y, du, ddelta, dz, dx, dB, dC, dA, dD, dbias, dw, db = bufs
        F.causal_conv1d_rows_into(a["u"], w, b, seq, False, "silu", x)
        scan = (x, a["delta"], a["A"], a["B"], a["C"], a["D"], a["z"], a["delta_bias"], True, seq, False)
        F.selective_scan_into(*scan, y, ws)
        F.selective_scan_bwd_into(*scan, dout, du, ddelta, dA, dB, dC, dD, dz, dbias, ws)
        F.causal_conv1d_rows_bwd_into(a["u"], w, b, seq, False, "silu", du, dx, dw, db, cws)
        return bufs

    eager = []
    for off in (OFFSETS, shorter):
        offsets.copy_(torch.from_numpy(off))
        eager.append([t.clone() for t in step()])
    assert all(bool(torch.isfinite(t).all()) for t in eager[1])          # (every element written)
    assert not torch.equal(eager[0][1], eager[1][1])
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = step()
    for which in (1, 0, 1):
        offsets.copy_(torch.from_numpy((OFFSETS, shorter)[which]))
        graph.replay()
        torch.cuda.synchronize()
        for got, want in zip(outs, eager[which]):
            np.testing.assert_array_equal(bits(got), bits(want))


def mamba_loop(p, feats, seqs_fwd, seqs_rev, work):
    """SerializedMamba(bidirectional=True) restated from its state dict on the loops above"""
    lin = torch.nn.functional.linear
    Di, R = p["D"].shape[0], p["dt_proj.weight"].shape[1]
    x, z = lin(feats, p["in_proj.weight"][:Di]), lin(feats, p["in_proj.weight"][Di:])
    y = 0
    for sfx, seqs in (("", seqs_fwd), ("_b", seqs_rev)):
        xc = conv_loop(x, p[f"conv1d{sfx}.weight"][:, 0], p[f"conv1d{sfx}.bias"], "silu", seqs, work)
        dbl = lin(xc, p[f"x_proj{sfx}.weight"])
        delta = lin(dbl[:, :R], p[f"dt_proj{sfx}.weight"])
        y = y + scan_loop(xc, delta, -torch.exp(p["A_log" + sfx]), dbl[:, None, R:R + 16], dbl[:, None, R + 16:],
                          p["D" + sfx], z, p[f"dt_proj{sfx}.bias"], True, seqs, work)
    return lin(y, p["out_proj.weight"])


def test_module(cuda):
    import spconv_amd.pytorch as spconv
    F = spconv.functional
    g = torch.Generator().manual_seed(11)
    cells = torch.unique(torch.cat([torch.randint(0, 2, (3 * T, 1), generator=g),
                                    torch.randint(0, 16, (3 * T, 3), generator=g)], dim=1), dim=0).int()
    n = cells.shape[0]
    feats, dout = torch.randn((n, 64), generator=g), torch.randn((n, 64), generator=g)
    torch.manual_seed(5)
    layer = spconv.SerializedMamba(64, bidirectional=True)
    params = {k: v.detach().clone() for k, v in layer.state_dict().items()}
    layer = layer.to(cuda)
    x = spconv.SparseConvTensor(feats.to(cuda), cells.to(cuda).contiguous(), [16, 16, 16], 2)
    ser = F.serialize(x, orders=("hilbert",))
    out = layer(x, ser).features
    got = [out] + list(torch.autograd.grad(out, list(layer.parameters()), dout.to(cuda)))
    names = [k for k, _ in layer.named_parameters()]
    off, order = ser.offsets.cpu().numpy(), ser.order[0].cpu().numpy()
    assert off[-1] == n and sorted(order.tolist()) == list(range(n))
    rows = lambda rev: [torch.from_numpy(order[off[s]:off[s + 1]][::-1 if rev else 1].copy()).long()
                        for s in range(2)]
    want = []
    for work in (torch.float64, torch.float32):
        p = {k: v.to(work).requires_grad_(True) for k, v in params.items()}
        o = mamba_loop(p, feats.to(work), rows(False), rows(True), work)
        want.append([o.detach()] + list(torch.autograd.grad(o, [p[k] for k in names], dout.to(work))))
    for what, t, r, c in zip(["out"] + names, got, *want):
        within_composite(t, r, c, 2.0 ** -24, what)
