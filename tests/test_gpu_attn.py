"""GPU: serialised patch attention (csrc/attn.hip, functional.patch_attention) against a plain float64 restatement.

Measured on an MI355X: the figures are printed by every test ahead of its assertion."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DTYPES = {"f16": (torch.float16, 2.0 ** -11), "bf16": (torch.bfloat16, 2.0 ** -8)}
HEADS = [(1, 16), (3, 16), (2, 32), (1, 64)]
COUNTS = lambda K: ((0, 1, K + 1, 2 * K + 3), (K - 1, K, 5, 3 * K))


def F():
    import spconv_amd.pytorch.functional as fn
    return fn


@functools.lru_cache(maxsize=None)
def scene(K, run):
    """int32 index rows [n, 4] of four scenes with the live counts COUNTS(K)[run] in shuffled row order, three rows
    killed by batch -1 among them and four more behind n_live; (rows, n_live)."""
    rng = np.random.default_rng(100 * K + run)
    rows = [np.full((3, 4), -1)]
    for b, c in enumerate(COUNTS(K)[run]):
        cells = rng.choice(32 ** 3, c, replace=False)
        rows.append(np.stack([np.full(c, b), cells // 1024, cells // 32 % 32, cells % 32], axis=1))
    rows = rng.permutation(np.concatenate(rows))
    tail = np.stack([np.arange(4) % 4, np.full(4, 31), np.arange(4), np.arange(4)], axis=1)
    return np.concatenate([rows, tail]).astype(np.int32), len(rows)


def plan_of(cuda, K, run, pad):
    idx, live = scene(K, run)
    ser = F().serialize(torch.from_numpy(idx).to(cuda), [32, 32, 32], 4, orders=("hilbert",),
                        n_live=torch.tensor([live], dtype=torch.int32, device=cuda))
    plan = F().patch_plan(ser, K, pad=pad)
    assert int((plan.row_slot >= 0).sum()) == sum(COUNTS(K)[run]) and int((plan.row_slot < 0).sum()) == 7
    assert (int((plan.row_slot2 >= 0).sum()) > 0) == (pad == "borrow" and run == 0)      # (run 1 has no tail to fill)
    return plan


def inputs(cuda, n, H, D, dtype, seed):
    """qkv [n, 3, H, D] and d_out [n, H * D], randn rounded to the 16-bit type; Q and K scaled so that the logits have a
    standard deviation of 2.5"""
    gen = torch.Generator(device=cuda).manual_seed(seed)
    qkv = torch.randn((n, 3, H, D), device=cuda, generator=gen)
    qkv[:, :2] *= 2.5 ** 0.5
    return qkv.to(dtype), torch.randn((n, H * D), device=cuda, generator=gen).to(dtype)


def attend(qkv, plan, scale, half=None):
    """The reference: gather by patch_rows, scores times scale, -inf on invalid keys, softmax, times V; results taken at
    row_slot, dead rows zero.  half = None: float64 throughout.  half = a 16-bit dtype: the torch composite with the
    kernels' rounding points (16-bit Q, K, V; fp32 scores and softmax; P cast to 16 bits)."""
    n, _, H, D = qkv.shape
    wide = torch.float64 if half is None else torch.float32
    rows = plan.patch_rows.long()
    valid = rows >= 0
    q, k, v = (qkv[rows.clamp(min=0), s].transpose(1, 2) for s in range(3))                 # [P, H, K, D]
    s = torch.matmul(q.to(wide), k.to(wide).transpose(2, 3)) * scale
    s = s.masked_fill((~valid & valid.any(dim=1, keepdim=True))[:, None, None, :], float("-inf"))
    p = torch.softmax(s, dim=-1)
    o = torch.matmul(p, v) if half is None else torch.matmul(p.to(half), v)
    o = o.transpose(1, 2).reshape(-1, H * D)
    live = plan.row_slot >= 0
    return torch.where(live[:, None], o[plan.row_slot.long().clamp(min=0)], torch.zeros((), dtype=o.dtype, device=o.device))


def forward_bound(qkv, plan, u):
    """4 u max|V| of the row's (patch, head), [n, H, 1]"""
    rows = plan.patch_rows.long()
    v = qkv[rows.clamp(min=0), 2].double().abs().amax(dim=-1)                               # [P, K, H]
    vmax = v.masked_fill((rows < 0)[:, :, None], 0).amax(dim=1)                              # [P, H]
    patch = plan.row_slot.long().clamp(min=0) // plan.patch_size
    return 4 * u * vmax[patch][:, :, None]


@pytest.mark.parametrize("pad", ["mask", "borrow"])
@pytest.mark.parametrize("K", [32, 96, 256])
@pytest.mark.parametrize("H,D", HEADS)
@pytest.mark.parametrize("name", sorted(DTYPES))
def test_forward(cuda, name, H, D, K, pad):
    dtype, u = DTYPES[name]
    worst = 0.0
    for run in (0, 1):
        plan = plan_of(cuda, K, run, pad)
        n = plan.row_slot.shape[0]
        qkv, _ = inputs(cuda, n, H, D, dtype, K + run)
        out = F().patch_attention(qkv.reshape(n, -1) if run else qkv, plan, H)
        assert out.shape == (n, H * D) and out.dtype == dtype
        ref = attend(qkv.double(), plan, D ** -0.5)
        err = (out.double() - ref).abs().reshape(n, H, D)
        bound = forward_bound(qkv, plan, u)
        worst = max(worst, float((err / bound.clamp(min=1e-30)).max()))
        print(f"forward {name} H{H} D{D} K{K} {pad} run {run}: max err / (4 u max|V|) = {worst:.3f}")
        assert bool((err <= bound).all())
        assert bool((out[plan.row_slot < 0] == 0).all()) and not bool(torch.signbit(out[plan.row_slot < 0]).any())


BACKWARD = [(K, pad) for K in (32, 96) for pad in ("mask", "borrow")]


@pytest.mark.parametrize("K,pad,H,D", [(K, pad, H, D) for K, pad in BACKWARD for H, D in HEADS] + [(256, "borrow", 3, 16)])
@pytest.mark.parametrize("name", sorted(DTYPES))
def test_backward(cuda, name, K, pad, H, D):
    dtype, u = DTYPES[name]
    for run in (0, 1):
        plan = plan_of(cuda, K, run, pad)
        n = plan.row_slot.shape[0]
        qkv, d_out = inputs(cuda, n, H, D, dtype, 7 * K + run)
        got = qkv.clone().requires_grad_(True)
        F().patch_attention(got, plan, H).backward(d_out)
        ref = qkv.double().requires_grad_(True)
        attend(ref, plan, D ** -0.5).backward(d_out.double())
        comp = qkv.clone().requires_grad_(True)
        attend(comp, plan, D ** -0.5, half=dtype).backward(d_out)
        assert got.grad.shape == qkv.shape and got.grad.dtype == dtype
        dead = plan.row_slot < 0
        assert bool((got.grad[dead] == 0).all()) and bool((ref.grad[dead] == 0).all())
        for s, what in enumerate(("dq", "dk", "dv")):
            e_got = float((got.grad[:, s].double() - ref.grad[:, s]).abs().max())
            e_comp = float((comp.grad[:, s].double() - ref.grad[:, s]).abs().max())
            floor = u * float(ref.grad[:, s].abs().max())
            print(f"backward {name} H{H} D{D} K{K} {pad} run {run} {what}: kernel {e_got:.3e} composite {e_comp:.3e} "
                  f"ratio {e_got / max(e_comp, 1e-30):.3f} floor {floor:.3e}")
            assert e_got <= 2 * e_comp + floor, what


def bits(t):
    return t.contiguous().view(torch.int16)


def test_identical_run_to_run_and_blind_to_dirty_memory(cuda):
    K, H, D = 96, 3, 16
    plan = plan_of(cuda, K, 0, "borrow")
    n = plan.row_slot.shape[0]
    qkv, d_out = inputs(cuda, n, H, D, torch.float16, 3)
    used = int(plan.n_patches_dev.item())
    assert used < plan.patch_rows.shape[0]
    dirty_plan = plan._replace(patch_rows=plan.patch_rows.clone(), patch_rows_canon=plan.patch_rows_canon.clone())
    dirty_plan.patch_rows[used:] = -1
    dirty_plan.patch_rows_canon[used:] = -1
    dirty = qkv.clone()
    dirty[plan.row_slot < 0] = float("nan")
    results = []
    for x, p in ((qkv, plan), (qkv, plan), (dirty, dirty_plan)):
        torch.full((n, H * D), float("nan"), device=cuda, dtype=torch.float16)      # (what the allocator hands out next)
        x = x.clone().requires_grad_(True)
        out = F().patch_attention(x, p, H)
        torch.full((n, 3, H, D), float("nan"), device=cuda, dtype=torch.float16)
        out.backward(d_out)
        results.append((out.detach(), x.grad))
    for out, grad in results[1:]:
        assert torch.equal(bits(out), bits(results[0][0])) and torch.equal(bits(grad), bits(results[0][1]))
    assert bool(torch.isfinite(results[2][0]).all()) and bool(torch.isfinite(results[2][1]).all())


def test_capture_serialize_plan_attention_in_one_graph(cuda):
    """serialize -> patch_plan -> patch_attention in one graph, replayed on a scene of another live count in the same
    buffers; every replay equals its eager result bit for bit."""
    K, H, D, B = 64, 2, 32, 4
    idx, live = scene(K, 1)
    cap = idx.shape[0]
    scenes = [(torch.from_numpy(idx).to(cuda), inputs(cuda, cap, H, D, torch.float16, k)[0], (live, 150)[k]) for k in (0, 1)]
    idx_buf = torch.empty((cap, 4), dtype=torch.int32, device=cuda)
    qkv_buf = torch.empty((cap, 3, H, D), dtype=torch.float16, device=cuda)
    n_live = torch.zeros((1,), dtype=torch.int32, device=cuda)

    def load(k):
        idx_buf.copy_(scenes[k][0])
        qkv_buf.copy_(scenes[k][1])
        n_live.fill_(scenes[k][2])

    def block():
        ser = F().serialize(idx_buf, [32, 32, 32], B, orders=("z",), n_live=n_live)
        return F().patch_attention(qkv_buf, F().patch_plan(ser, K, pad="borrow"), H)

    eager = []
    with torch.no_grad():
        for k in (0, 1):
            load(k)
            eager.append(block().clone())
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = block()
    assert not torch.equal(eager[0], eager[1]) and int((eager[1] != 0).any(dim=1).sum()) > 100
    for k in (1, 0, 1):
        load(k)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(bits(out), bits(eager[k]))
