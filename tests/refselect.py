"""numpy reference of voxel pruning (csrc/select.hip, include/spconv_amd.h "voxel pruning"), written from the contract
alone:

  * score: |x| summed in the header's order -- lanes s = 0 .. G - 1 each add their pieces s, s + G, ... element by
    element, then acc[s] += acc[s + d] for d = G / 2 .. 1 -- with IEEE float32 (float64) additions, divided by C, one
    rounding to float32; absmax the plain maximum; -inf for rows at or beyond n_live
  * the key of a float32 score, k from a count or a ratio, the kept rows: key above the k-th largest, ties to the lowest
    row index
  * the three tables of a selection build, eager and with a cap
"""
from typing import NamedTuple, Optional

import numpy as np
import torch


# ---------------------------------------------------------------------------------------------- score
def score_groups(C: int, elem_bytes: int):
    """(V elements of a piece, P pieces, G lanes of a row)"""
    V = 16 // elem_bytes if (C * elem_bytes) % 16 == 0 else 1
    P = C // V
    G = 1
    while G < P and G < 64:
        G *= 2
    return V, P, G


def score(feat: torch.Tensor, op: str = "absmean", n_live: Optional[int] = None) -> np.ndarray:
    n, C = feat.shape
    at = np.float64 if feat.dtype == torch.float64 else np.float32
    a = np.abs(feat.to(torch.float64 if at == np.float64 else torch.float32).numpy())
    if op == "absmax":
        out = (a.max(axis=1) if n else np.zeros((0,), at)).astype(np.float32)
    else:
        V, P, G = score_groups(C, feat.element_size())
        acc = np.zeros((n, G), dtype=at)
        for p in range(P):                      # (ascending p visits every lane's pieces in that lane's order)
            for j in range(V):
                acc[:, p % G] = acc[:, p % G] + a[:, p * V + j]
        d = G // 2
        while d >= 1:
            acc[:, :d] = acc[:, :d] + acc[:, d:2 * d]
            d //= 2
        out = (acc[:, 0] / at(C)).astype(np.float32)
    if n_live is not None:
        out[int(n_live):] = -np.inf
    return out


def score_f64(feat: torch.Tensor, op: str = "absmean") -> np.ndarray:
    a = np.abs(feat.to(torch.float64).numpy())
    return a.max(axis=1) if op == "absmax" else a.sum(axis=1) / feat.shape[1]


def score_bound(dtype, C: int, want: np.ndarray) -> np.ndarray:
    """Absolute bound of an absmean score against its fp64 evaluation `want`.  f16 / bf16 / f32: (C + 2) 2^-24 relative
    -- a sum of C non-negative fp32 terms in any order errs by at most about C 2^-24 of the sum, the division and the
    rounding add one each.  f64: half an fp32 ulp of the result (one rounding), plus the fp64 sum's own C 2^-52."""
    if dtype == torch.float64:
        return 0.5 * np.spacing(np.abs(want).astype(np.float32)).astype(np.float64) + C * 2.0 ** -52 * np.abs(want)
    return (C + 2) * 2.0 ** -24 * np.abs(want)


# ---------------------------------------------------------------------------------------------- top-k
def keys(score_f32: np.ndarray) -> np.ndarray:
    """the unsigned order-preserving key of every float32 bit pattern"""
    b = np.ascontiguousarray(score_f32, dtype=np.float32).view(np.uint32)
    return b ^ np.where((b >> 31) != 0, np.uint32(0xffffffff), np.uint32(0x80000000))


def live_rows(n, indices=None, batch=None, n_live=None) -> np.ndarray:
    ok = np.ones((n,), dtype=bool)
    if n_live is not None:
        ok[int(n_live):] = False
    if indices is not None:
        b = np.asarray(indices)[:, 0]
        ok &= (b >= 0) & (b < batch)
    return ok


def count_k(live: int, k=None, ratio=None) -> int:
    if k is not None:
        return min(int(k), live)
    return int(np.float64(ratio) * np.float64(live))


class Topk(NamedTuple):
    keep: np.ndarray            # [n] uint8
    sel: list                   # {live, k, threshold key as int32, ties taken}


def topk(score_f32, k=None, ratio=None, indices=None, batch=None, n_live=None) -> Topk:
    n = score_f32.shape[0]
    ok = live_rows(n, indices, batch, n_live)
    live = int(ok.sum())
    kk = count_k(live, k, ratio)
    keep = np.zeros((n,), dtype=np.uint8)
    if kk == 0:
        return Topk(keep, [live, 0, -1, 0])
    key = keys(score_f32)
    T = np.sort(key[ok])[live - kk]             # the k-th largest
    above = ok & (key > T)
    ties = kk - int(above.sum())
    keep[above] = 1
    keep[np.nonzero(ok & (key == T))[0][:ties]] = 1
    return Topk(keep, [live, kk, int(np.uint32(T).astype(np.int32)), ties])


# ---------------------------------------------------------------------------------------------- selection
class Select(NamedTuple):
    out_indices: np.ndarray     # [live, ndim + 1] int32
    rows: np.ndarray            # [n] int64, -1: not selected or cut
    src: np.ndarray             # [live] int64
    found: int                  # selected rows (may exceed the cap)
    live: int                   # output rows = min(found, cap)
    live_rows: int              # live input rows


def select_live(idx, bs, shape, n_live=None) -> np.ndarray:
    idx = np.asarray(idx, dtype=np.int64).reshape(-1, len(shape) + 1)
    ok = (idx[:, 0] >= 0) & (idx[:, 0] < bs)
    for d, ext in enumerate(shape):
        ok &= (idx[:, 1 + d] >= 0) & (idx[:, 1 + d] < ext)
    if n_live is not None:
        ok[int(n_live):] = False
    return ok


def select(idx, bs, shape, keep, invert=False, n_live=None, cap=None) -> Select:
    idx = np.asarray(idx).reshape(-1, len(shape) + 1)
    ok = select_live(idx, bs, shape, n_live)
    sel = ok & ((np.asarray(keep) != 0) != bool(invert))
    src = np.nonzero(sel)[0]
    found = int(src.shape[0])
    live = found if cap is None else min(found, int(cap))
    src = src[:live]
    rows = np.full((idx.shape[0],), -1, dtype=np.int64)
    rows[src] = np.arange(live)
    return Select(idx[src].astype(np.int32), rows, src.astype(np.int64), found, live, int(ok.sum()))


# ---------------------------------------------------------------------------------------------- inputs
def scores(kind: str, n: int, seed: int) -> np.ndarray:
    """float32 [n]: the score sets of the flag tests"""
    rng = np.random.default_rng(seed)
    if kind == "normal":
        return rng.standard_normal(n).astype(np.float32)
    if kind == "equal":                         # ties span every block: the kept rows are the first k
        return np.full((n,), 0.375, dtype=np.float32)
    base = np.uint32(0x3f400000)                # 0.75
    if kind == "low_byte":                      # equal except the low byte: the threshold falls in the last digit
        return (base | rng.integers(0, 256, n).astype(np.uint32)).view(np.float32)
    if kind == "top_byte":                      # equal except the top byte: signs and exponents differ; bit 23 is never
        #                                         set, so the exponent is never all ones: no Inf and no NaN ("nan" has them)
        return ((rng.integers(0, 256, n).astype(np.uint32) << np.uint32(24)) | np.uint32(0x00400000)).view(np.float32)
    if kind == "mid_bytes":                     # equal except the two middle bytes
        return (base ^ (rng.integers(0, 65536, n).astype(np.uint32) << np.uint32(8))).view(np.float32)
    if kind == "special":                       # +-0, +-inf, subnormals, negatives
        pool = np.array([0.0, -0.0, np.inf, -np.inf, 1e-40, -1e-40, 2.0 ** -149, -1.5, -1.5, 3.0, 3.0, 0.25],
                        dtype=np.float32)
        return pool[rng.integers(0, pool.shape[0], n)]
    if kind == "nan":                           # NaNs of both signs and two payloads, +-inf, finite values: twelve bit
        #                                         patterns over n rows, so every pattern's ties span the blocks
        pool = np.array([0x7fc00000, 0x7fc12345, 0xffc00000, 0xffc12345, 0x7f800000, 0xff800000, 0x3f800000, 0x3f800000,
                         0xbf800000, 0x00000000, 0x40400000, 0x3e800000], dtype=np.uint32)
        return pool[rng.integers(0, pool.shape[0], n)].view(np.float32)
    raise KeyError(kind)


NAN_KEY_ORDER = (0xffc12345, 0xffc00000, 0xff800000, 0xbf800000, 0x00000000, 0x3e800000, 0x3f800000, 0x40400000,
                 0x7f800000, 0x7fc00000, 0x7fc12345)   # the "nan" kind's bit patterns in ascending key, written by hand

SCORE_KINDS = ("normal", "equal", "low_byte", "top_byte", "mid_bytes", "special", "nan")


def sorted_scene(bs, shape, n, seed):
    """n distinct live rows in ascending key order.  int32 [n, ndim + 1]."""
    rng = np.random.default_rng(seed)
    cells = bs * int(np.prod(shape))
    key = np.sort(rng.choice(cells, size=min(n, cells), replace=False))
    cols = []
    for ext in reversed(shape):
        cols.append(key % ext)
        key = key // ext
    return np.ascontiguousarray(np.stack([key] + cols[::-1], axis=1).astype(np.int32))
