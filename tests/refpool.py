"""fp64 reference of sparse pooling as csrc/pool.hip defines it, over pairs derived from the coordinates alone.

Plain torch in float64, on the device of its inputs; nothing of this project's is used but refconv.pairs, which builds no
rulebook.  Every function takes the pair list [(k, in rows, out rows)] of refconv.pairs (per offset k an output row occurs
at most once) and float64 operands that hold values of the tensor dtype `dtype`.

  max forward    starts from the dtype's lowest FINITE value (zero with init_zero, the ConvAlgo.Native flavour), walks the
                 offsets in ascending k and replaces only on a strict cur < in: NaN is never selected, a window of -inf
                 keeps the lowest finite value, and a row without a single pair (a dead row of a static-shape tensor) is 0
  max backward   din[i] = sum of dout[o] over the pairs with feat[i] == out[o]: every tied input receives the gradient,
                 NaN (never equal) none
  avg forward    mean over the valid pairs and their int32 count; a row without pairs gives 0 and count 0
  avg backward   din[i] = sum of dout[o] / count[o] (reference_quirks: * count[o], the reference kernel's arithmetic)
Each summing operation also returns A, the same sum over the operands' magnitudes (util.assert_close_abs_sum)."""
from collections import namedtuple

import torch

RefSum = namedtuple("RefSum", "value abs_sum")
RefAvg = namedtuple("RefAvg", "value count abs_sum")

_LOWEST = {
    torch.float16: -65504.0,
    torch.bfloat16: -float.fromhex("0x1.fep127"),      # bits 0xff7f
    torch.float32: -float.fromhex("0x1.fffffep127"),   # -FLT_MAX
    torch.float64: -float.fromhex("0x1.fffffffffffffp1023"),
    torch.int8: -128.0,
}


def lowest(dtype):
    """the lowest finite value of `dtype`, as a Python float (exact in float64)"""
    return _LOWEST[dtype]


def max_fwd(cand, f, n_out, dtype, init_zero=False):
    """[n_out, C] float64: the max over each output row's pairs."""
    C = f.shape[1]
    cur = torch.full((n_out, C), 0.0 if init_zero else lowest(dtype), dtype=torch.float64, device=f.device)
    seen = torch.zeros((n_out,), dtype=torch.bool, device=f.device)
    for _, i, o in sorted(cand, key=lambda t: t[0]):
        if i.numel() == 0:
            continue
        c, v = cur[o], f[i]
        cur[o] = torch.where(c < v, v, c)
        seen[o] = True
    cur[~seen] = 0.0
    return cur


def max_bwd(cand, f, out, dout):
    """RefSum(din [n_in, C], the same sum over |dout|)."""
    din = torch.zeros_like(f, dtype=torch.float64)
    A = torch.zeros_like(din)
    for _, i, o in cand:
        if i.numel() == 0:
            continue
        hit = (f[i] == out[o]).to(torch.float64)
        g = dout[o].to(torch.float64)
        din.index_add_(0, i, g * hit)
        A.index_add_(0, i, g.abs() * hit)
    return RefSum(din, A)


def counts(cand, n_out, device="cpu"):
    """int32 [n_out]: valid pairs per output row."""
    cnt = torch.zeros((n_out,), dtype=torch.int64, device=device)
    for _, i, o in cand:
        if i.numel():
            cnt.index_add_(0, o, torch.ones_like(o))
    return cnt.to(torch.int32)


def avg_fwd(cand, f, n_out):
    """RefAvg(mean [n_out, C], count int32 [n_out], mean of |f|)."""
    C = f.shape[1]
    total = torch.zeros((n_out, C), dtype=torch.float64, device=f.device)
    A = torch.zeros_like(total)
    for _, i, o in cand:
        if i.numel() == 0:
            continue
        total.index_add_(0, o, f[i].to(torch.float64))
        A.index_add_(0, o, f[i].to(torch.float64).abs())
    cnt = counts(cand, n_out, f.device)
    div = cnt.to(torch.float64).clamp(min=1).unsqueeze(1)          # (a row without pairs: 0 / 1)
    return RefAvg(total / div, cnt, A / div)


def avg_bwd(cand, dout, count, n_in, reference_quirks=False):
    """RefSum(din [n_in, C], the same sum over |dout|)."""
    g = dout.to(torch.float64)
    cnt = count.to(torch.float64).unsqueeze(1)
    if reference_quirks:
        g = g * cnt
    else:
        g = torch.where(cnt > 0, g / cnt.clamp(min=1), torch.zeros_like(g))
    din = torch.zeros((n_in, dout.shape[1]), dtype=torch.float64, device=dout.device)
    A = torch.zeros_like(din)
    for _, i, o in cand:
        if i.numel() == 0:
            continue
        din.index_add_(0, i, g[o])
        A.index_add_(0, i, g[o].abs())
    return RefSum(din, A)


def global_pool(batch_index, f, batch_size, dtype, is_mean):
    """Per-scene reduction over all rows, scene by scene: RefSum([batch_size, C], mean of |f| or None).  Rows whose batch
    index lies outside [0, batch_size) belong to no scene; a scene without rows gives NaN for the mean and the dtype's
    lowest value for the max (SparseGlobalMaxOrAvgPool)."""
    b = batch_index.to(torch.int64)
    C = f.shape[1]
    out = torch.empty((batch_size, C), dtype=torch.float64, device=f.device)
    A = torch.zeros_like(out)
    for s in range(batch_size):
        rows = f[b == s].to(torch.float64)
        if is_mean:
            out[s] = rows.mean(0) if rows.shape[0] else float("nan")
            A[s] = rows.abs().mean(0) if rows.shape[0] else 0.0
        else:
            out[s] = rows.max(0)[0] if rows.shape[0] else lowest(dtype)
    return RefSum(out, A if is_mean else None)
