"""Reference of the int8 inference forward that uses nothing of this project: the accumulator from the coordinate-derived
pairs of refconv.py in float64 (exact: 127 * 127 * C * kv is far below 2^53), cast to int32, and the quantised epilogue in
numpy float32 with every operation rounded on its own, in the kernel's documented order

    v = ((acc.astype(f32) * scale) + bias) + (add.astype(f32) * f32(add_scale));  v = act(v)
    int8: clip(rint(v), -128, 127)    f32: v    f16: v.astype(f16)    bf16: torch bfloat16 of v (both round to nearest even)

`mutate` names one deliberate mistake; the host tests of test_gpu_int8_matrix.py use them to show that the data of the
content cases tells each of them from the formula."""
import numpy as np
import torch

from refconv import conv_from_pairs

F32 = np.float32
MUTATIONS = ("half_away", "floor_half", "clip127", "fma64")


def int_acc(out_idx, cand, f_i8, w_i8, device="cpu"):
    """(acc int32 [n_out, K], in the row order of out_idx) of int8 features [n_in, C] and weights [K, *ksize, C]."""
    f = torch.from_numpy(np.ascontiguousarray(f_i8)).to(device=device, dtype=torch.float64)
    w = torch.from_numpy(np.ascontiguousarray(w_i8)).to(device=device, dtype=torch.float64)
    cand = [(k, i.to(device), o.to(device)) for k, i, o in cand]
    acc = conv_from_pairs(out_idx.to(device), cand, f, w, None).out.cpu().numpy()
    assert np.array_equal(acc, np.rint(acc)), "the float64 accumulator is not integral"
    assert acc.size == 0 or np.abs(acc).max() < 2.0 ** 31, "the accumulator leaves int32"
    return acc.astype(np.int32)


def pre_activation(acc, scale, bias, add=None, add_scale=0.0, mutate=None):
    """float32 value in front of the activation.  scale / bias None: 1 / 0 (what the kernel substitutes)."""
    K = acc.shape[1]
    scale = np.ones((K,), F32) if scale is None else np.asarray(scale, F32)
    bias = np.zeros((K,), F32) if bias is None else np.asarray(bias, F32)
    if mutate == "fma64":           # a fused multiply-add: the product kept exact, one rounding after the sum
        v = (acc.astype(np.float64) * scale.astype(np.float64) + bias.astype(np.float64)).astype(F32)
    else:
        v = acc.astype(F32) * scale
        v = v + bias
    if add is not None:
        v = v + add.astype(F32) * F32(add_scale)
    assert v.dtype == F32
    return v


def activation(v, act=None, alpha=0.0):
    if act == "relu":
        return np.maximum(v, F32(0))
    if act == "leaky":
        return np.where(v > 0, v, v * F32(alpha)).astype(F32)
    assert act is None, act
    return v


def quantise(v, mutate=None):
    if mutate == "half_away":
        r = np.sign(v) * np.floor(np.abs(v) + F32(0.5))
    elif mutate == "floor_half":
        r = np.floor(v + F32(0.5))
    else:
        r = np.rint(v)
    lo = -127 if mutate == "clip127" else -128
    return np.clip(r, lo, 127).astype(np.int8)


def epilogue(acc, scale, bias, add=None, add_scale=0.0, act=None, alpha=0.0, out="i8", mutate=None):
    """The expected output tensor: numpy int8 / float32 / float16, or a torch.bfloat16 tensor for out = "bf16"."""
    assert mutate is None or mutate in MUTATIONS, mutate
    v = activation(pre_activation(acc, scale, bias, add, add_scale, mutate), act, alpha)
    if out == "i8":
        return quantise(v, mutate)
    if out == "f32":
        return v
    if out == "f16":
        with np.errstate(over="ignore"):
            return v.astype(np.float16)
    assert out == "bf16", out
    return torch.from_numpy(np.ascontiguousarray(v)).to(torch.bfloat16)


def sigmoid64(v):
    """float64 sigmoid of the exact float32 pre-activation (the kernel's is 1 / (1 + __expf(-v)): bounded, not exact)."""
    return 1.0 / (1.0 + np.exp(-v.astype(np.float64)))
