"""GPU: patch attention with Point Transformer V3's relative position bias inside the kernels (csrc/attn.hip, the
BIAS instances; functional.patch_attention(rel_bias=, coords=, pos_bnd=)) against a plain float64 restatement: the
reference of test_gpu_attn.py plus the bias built from the table.  Figures are printed ahead of every assertion."""
import functools

import numpy as np
import pytest
import torch

from test_gpu_attn import DTYPES, HEADS, F, bits, forward_bound, inputs

pytestmark = pytest.mark.gpu

GRID = [(K, pad) for K in (32, 96) for pad in ("mask", "borrow")]
BOUNDS = (2, 5)                                  # coordinates span 0 .. 15: both clamp on either side


@functools.lru_cache(maxsize=None)
def scene():
    """int32 index rows [n, 4] on a 16^3 grid: two scenes in shuffled row order (a scene's last patch is partial at K = 32
    and 96), three rows killed by batch -1 with garbage coordinates among them, four more behind n_live; (rows, n_live)."""
    rng = np.random.default_rng(16)
    rows = [np.stack([np.full(3, -1)] + [rng.integers(-2 ** 31, 2 ** 31, 3) for _ in range(3)], axis=1)]
    for b, c in enumerate((160, 140)):
        cells = rng.choice(16 ** 3, c, replace=False)
        rows.append(np.stack([np.full(c, b), cells // 256, cells // 16 % 16, cells % 16], axis=1))
    rows = rng.permutation(np.concatenate(rows))
    tail = np.stack([np.arange(4) % 2, np.full(4, 15), np.arange(4), np.arange(4)], axis=1)
    return np.concatenate([rows, tail]).astype(np.int32), len(rows)


def setup(cuda, K, pad):
    """(plan, coords int32 [n, 3]); the device-side patch count lies below the capacity"""
    idx, live = scene()
    idx = torch.from_numpy(idx).to(cuda)
    ser = F().serialize(idx, [16, 16, 16], 2, orders=("hilbert",), n_live=torch.tensor([live], dtype=torch.int32, device=cuda))
    plan = F().patch_plan(ser, K, pad=pad)
    assert int(plan.n_patches_dev.item()) < plan.patch_rows.shape[0] and int((plan.row_slot < 0).sum()) == 7
    return plan, idx[:, 1:].contiguous()


def table_of(cuda, pb, H, seed=0):
    """fp32 [3 (2 pb + 1), H], both signs, magnitude up to 2"""
    gen = torch.Generator(device=cuda).manual_seed(seed)
    return torch.rand((3 * (2 * pb + 1), H), device=cuda, generator=gen) * 4 - 2


def bin_index(coords, plan, pb):
    """[P, K(query), K(key), 3]: row of the table of every pair and axis"""
    c = coords.long()[plan.patch_rows.long().clamp(min=0)]
    return (c[:, :, None] - c[:, None, :]).clamp(-pb, pb) + pb + (2 * pb + 1) * torch.arange(3, device=c.device)


def attend(qkv, table, coords, plan, scale, pb, half=None):
    """test_gpu_attn.attend plus the bias.  half = None: float64 throughout.  half = a 16-bit dtype: the torch composite
    with the kernels' rounding points and a materialised fp32 bias."""
    n, _, H, D = qkv.shape
    wide = torch.float64 if half is None else torch.float32
    rows = plan.patch_rows.long()
    valid = rows >= 0
    q, k, v = (qkv[rows.clamp(min=0), s].transpose(1, 2) for s in range(3))                 # [P, H, K, D]
    bias = table.to(wide)[bin_index(coords, plan, pb)].sum(dim=3).permute(0, 3, 1, 2)        # [P, H, K, K]
    s = torch.matmul(q.to(wide), k.to(wide).transpose(2, 3)) * scale + bias
    s = s.masked_fill((~valid & valid.any(dim=1, keepdim=True))[:, None, None, :], float("-inf"))
    p = torch.softmax(s, dim=-1)
    o = torch.matmul(p, v) if half is None else torch.matmul(p.to(half), v)
    o = o.transpose(1, 2).reshape(-1, H * D)
    return torch.where((plan.row_slot >= 0)[:, None], o[plan.row_slot.long().clamp(min=0)], torch.zeros((), dtype=o.dtype, device=o.device))


@pytest.mark.parametrize("K,pad", GRID)
@pytest.mark.parametrize("H,D", HEADS)
@pytest.mark.parametrize("name", sorted(DTYPES))
def test_forward(cuda, name, H, D, K, pad):
    dtype, u = DTYPES[name]
    plan, coords = setup(cuda, K, pad)
    n = plan.row_slot.shape[0]
    for pb in BOUNDS:
        qkv, _ = inputs(cuda, n, H, D, dtype, K + pb)
        table = table_of(cuda, pb, H)
        pairs = bin_index(coords, plan, pb)[(plan.patch_rows_canon >= 0)[:, :, None] & (plan.patch_rows >= 0)[:, None, :]]
        assert bool((torch.bincount(pairs.flatten(), minlength=3 * (2 * pb + 1)) > 0).all())      # every bin of every axis
        out = F().patch_attention(qkv, plan, H, rel_bias=table, coords=coords, pos_bnd=pb)
        ref = attend(qkv.double(), table, coords, plan, D ** -0.5, pb)
        err = (out.double() - ref).abs().reshape(n, H, D)
        bound = forward_bound(qkv, plan, u)
        print(f"forward {name} H{H} D{D} K{K} {pad} pos_bnd {pb}: max err / (4 u max|V|) = {float((err / bound.clamp(min=1e-30)).max()):.3f}")
        assert bool((err <= bound).all())
        assert bool((out[plan.row_slot < 0] == 0).all()) and not bool(torch.signbit(out[plan.row_slot < 0]).any())


@pytest.mark.parametrize("K,pad", GRID)
@pytest.mark.parametrize("H,D", HEADS)
@pytest.mark.parametrize("name", sorted(DTYPES))
def test_backward(cuda, name, H, D, K, pad):
    """max|got - ref| <= 2 max|composite - ref| + u max|ref| for dq, dk, dv and dtable.  Worst ratios to the composite's
    error on an MI355X: dq 1.82, dk 2.28 (through the floor), dv 1.00, dtable 0.009."""
    dtype, u = DTYPES[name]
    plan, coords = setup(cuda, K, pad)
    n = plan.row_slot.shape[0]
    for pb in BOUNDS:
        qkv, d_out = inputs(cuda, n, H, D, dtype, 7 * K + pb)
        table = table_of(cuda, pb, H)
        grads = []
        for x, t, fn in ((qkv, table, lambda x, t: F().patch_attention(x, plan, H, rel_bias=t, coords=coords, pos_bnd=pb)),
                         (qkv.double(), table.double(), lambda x, t: attend(x, t, coords, plan, D ** -0.5, pb)),
                         (qkv, table, lambda x, t: attend(x, t, coords, plan, D ** -0.5, pb, half=dtype))):
            x, t = x.clone().requires_grad_(True), t.clone().requires_grad_(True)
            fn(x, t).backward(d_out.to(x.dtype))
            grads.append((x.grad[:, 0], x.grad[:, 1], x.grad[:, 2], t.grad))
        got, ref, comp = grads
        assert got[3].dtype == torch.float32 and got[3].shape == table.shape and got[0].dtype == dtype
        for s, what in enumerate(("dq", "dk", "dv", "dtable")):
            e_got = float((got[s].double() - ref[s]).abs().max())
            e_comp = float((comp[s].double() - ref[s]).abs().max())
            floor = u * float(ref[s].abs().max())
            print(f"backward {name} H{H} D{D} K{K} {pad} pos_bnd {pb} {what}: kernel {e_got:.3e} composite {e_comp:.3e} "
                  f"ratio {e_got / max(e_comp, 1e-30):.3f} floor {floor:.3e}")
            assert e_got <= 2 * e_comp + floor, what


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_sign_and_axis_of_the_difference(cuda, axis):
    """Bit for bit, no tolerance.  (1) A table of -1e4 where c_i - c_j < 0 on one axis and 0 elsewhere gives a key with
    the larger coordinate the probability exactly 0: negating V of the rows at coordinate 15 must leave every row below
    15 untouched and change rows at 15.  With the sign swapped the rows below 15 are the ones that see them.  (2) A ramp on
    that axis against the mirrored ramp on coordinates negated on that axis: every logit is the same number; a kernel
    that pairs the table's axis with another axis of the coordinates reads other entries in one of the two calls."""
    K, H, D, pb = 96, 3, 16, 16                  # nothing clamps
    plan, coords = setup(cuda, K, "borrow")
    qkv, _ = inputs(cuda, plan.row_slot.shape[0], H, D, torch.float16, axis)
    call = lambda x, t, c: F().patch_attention(x, plan, H, rel_bias=t.reshape(-1, H).contiguous(), coords=c, pos_bnd=pb)
    wall, top, flipped = torch.zeros((3, 2 * pb + 1, H), device=cuda), coords[:, axis] == 15, qkv.clone()
    wall[axis, :pb] = -1e4
    flipped[top, 2] *= -1
    a, b = call(qkv, wall, coords), call(flipped, wall, coords)
    assert torch.equal(bits(a[~top]), bits(b[~top])) and not torch.equal(bits(a[top]), bits(b[top]))
    ramp, negated = torch.zeros_like(wall), coords.clone()
    ramp[axis] = torch.linspace(-2, 1, 2 * pb + 1, device=cuda)[:, None] * torch.arange(1, H + 1, device=cuda)
    negated[:, axis] *= -1
    a = call(qkv, ramp, coords)
    assert torch.equal(bits(a), bits(call(qkv, ramp.flip(1), negated))) and not torch.equal(bits(a), bits(F().patch_attention(qkv, plan, H)))


def test_identical_run_to_run_and_blind_to_dirty_memory(cuda, monkeypatch):
    from spconv_amd.pytorch import _attn
    # both workspaces of the backward arrive filled with NaN (every fp32 word 0xffffffff)
    monkeypatch.setattr(_attn, "_ws", lambda nbytes, dev: torch.full((max(int(nbytes), 16),), 255, dtype=torch.uint8, device=dev))
    K, H, D, pb = 96, 3, 16, 20                  # |c_i - c_j| <= 15: the bins beyond are never reached
    plan, coords = setup(cuda, K, "borrow")
    n, dead = plan.row_slot.shape[0], plan.row_slot < 0
    qkv, d_out = inputs(cuda, n, H, D, torch.float16, 3)
    table = table_of(cuda, pb, H)
    used = int(plan.n_patches_dev.item())
    dirty_plan = plan._replace(patch_rows=plan.patch_rows.clone(), patch_rows_canon=plan.patch_rows_canon.clone())
    dirty_plan.patch_rows[used:] = -1
    dirty_plan.patch_rows_canon[used:] = -1
    dirty, dirty_coords = qkv.clone(), coords.clone()
    dirty[dead] = float("nan")
    dirty_coords[dead] = torch.tensor([2 ** 31 - 1, -2 ** 31, 77], dtype=torch.int32, device=cuda)
    results = []
    for x, c, p in ((qkv, coords, plan), (qkv, coords, plan), (dirty, dirty_coords, dirty_plan)):
        torch.full((n, H * D), float("nan"), device=cuda, dtype=torch.float16)      # (what the allocator hands out next)
        x, t = x.clone().requires_grad_(True), table.clone().requires_grad_(True)
        out = F().patch_attention(x, p, H, rel_bias=t, coords=c, pos_bnd=pb)
        torch.full((n, 3, H, D), float("nan"), device=cuda, dtype=torch.float16)
        out.backward(d_out)
        results.append((out.detach(), x.grad, t.grad))
    for res in results[1:]:
        assert all(torch.equal(bits(r), bits(r0)) for r, r0 in zip(res, results[0]))
    out, dqkv, dtable = results[2]
    assert all(bool(torch.isfinite(r).all()) for r in results[2])
    assert not bool(bits(out[dead]).any()) and not bool(bits(dqkv[dead]).any())      # exactly +0
    unreached = torch.ones(2 * pb + 1, dtype=torch.bool, device=cuda)
    unreached[pb - 15:pb + 16] = False
    assert not bool(bits(dtable.reshape(3, -1, H)[:, unreached]).any()) and bool((dtable.reshape(3, -1, H)[:, pb] != 0).all())


def test_capture_forward_and_backward_in_one_graph(cuda):
    """serialize -> patch_plan -> biased attention forward and backward in one graph, replayed on a second scene with a
    smaller device count in the same buffers; every replay equals its eager result bit for bit."""
    K, H, D, pb = 64, 2, 32, 5
    idx, live = scene()
    cap = idx.shape[0]
    scenes = [(torch.from_numpy(idx).to(cuda), inputs(cuda, cap, H, D, torch.float16, k), (live, 150)[k]) for k in (0, 1)]
    idx_buf = torch.empty((cap, 4), dtype=torch.int32, device=cuda)
    qkv_buf = torch.empty((cap, 3, H, D), dtype=torch.float16, device=cuda).requires_grad_(True)
    g_buf = torch.empty((cap, H * D), dtype=torch.float16, device=cuda)
    table = table_of(cuda, pb, H).requires_grad_(True)
    n_live = torch.zeros((1,), dtype=torch.int32, device=cuda)

    def load(k):
        with torch.no_grad():
            idx_buf.copy_(scenes[k][0])
            qkv_buf.copy_(scenes[k][1][0])
            g_buf.copy_(scenes[k][1][1])
            n_live.fill_(scenes[k][2])

    def block():
        ser = F().serialize(idx_buf, [16, 16, 16], 2, orders=("z",), n_live=n_live)
        out = F().patch_attention(qkv_buf, F().patch_plan(ser, K, pad="borrow"), H, rel_bias=table,
                                  coords=idx_buf[:, 1:].contiguous(), pos_bnd=pb)
        return (out,) + torch.autograd.grad(out, (qkv_buf, table), g_buf)

    eager = []
    for k in (0, 1):
        load(k)
        eager.append([t.detach().clone() for t in block()])
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        held = block()
    assert not torch.equal(eager[0][2], eager[1][2])
    for k in (1, 0, 1):
        load(k)
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(bits(h), bits(e)) for h, e in zip(held, eager[k]))


def test_refusals(cuda):
    K, H, D = 32, 2, 16
    plan, coords = setup(cuda, K, "mask")
    qkv, _ = inputs(cuda, plan.row_slot.shape[0], H, D, torch.float16, 0)
    good = dict(rel_bias=table_of(cuda, 5, H), coords=coords, pos_bnd=5)
    assert F().patch_attention(qkv, plan, H, **dict(good, pos_bnd=None, rel_bias=table_of(cuda, 10, H))) is not None      # K = 32: 10
    for change in (dict(rel_bias=good["rel_bias"].half()), dict(rel_bias=good["rel_bias"][:-1]), dict(rel_bias=table_of(cuda, 5, H + 1)),
                   dict(rel_bias=None), dict(coords=None), dict(coords=coords.long()), dict(coords=coords[:-1]),
                   dict(coords=coords.cpu()), dict(coords=coords[:, :2]), dict(pos_bnd=0), dict(pos_bnd=64), dict(pos_bnd=5.0)):
        with pytest.raises(ValueError, match="patch_attention"):
            F().patch_attention(qkv, plan, H, **dict(good, **change))


def test_module_owns_rpe_table(cuda):
    import spconv_amd.pytorch as spconv
    K, H, C = 32, 2, 32
    plan, coords = setup(cuda, K, "borrow")
    m = spconv.PatchAttention(C, H, proj=False, rpe=True, patch_size=K).to(cuda)
    assert m.state_dict()["rpe_table"].shape == (3 * 21, H) and not bool(m.rpe_table.any())      # PTv3: pos_bnd 10
    with torch.no_grad():
        m.rpe_table.copy_(table_of(cuda, 10, H))
    feats = torch.randn((plan.row_slot.shape[0], C), device=cuda)
    out = m(feats, plan, coords)
    want = F().patch_attention(m.qkv(feats).half(), plan, H, rel_bias=m.rpe_table, coords=coords).float()
    assert torch.equal(out, want)
    out.sum().backward()
    assert m.rpe_table.grad.shape == m.rpe_table.shape and bool(m.rpe_table.grad.any())
    for args in ((feats, plan), (feats, setup(cuda, 96, "borrow")[0], coords)):
        with pytest.raises(ValueError, match="PatchAttention"):
            m(*args)
