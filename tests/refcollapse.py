"""numpy reference of the axis collapse (csrc/collapse.hip, include/spconv_amd.h "axis collapse"), written from the
contract alone:

  * a row is dead when it lies at or beyond n_live, when its batch index is outside [0, batch) or ANY coordinate -- a
    removed one included -- outside its extent
  * live rows are grouped by (batch, kept axes); output rows = the groups in ascending linear key of the projected grid;
    the rows of a group in ascending input row
  * sum: a sequential float32 (float64) loop that starts from the first row's value, one rounding to the dtype (torch's
    CPU cast), a group of one row copied bit for bit; mean: that sum / count in float32 (float64); max: the first of the
    largest stored values, or the group's first NaN in list order, moved with its bits; its backward gives a NaN output's
    gradient to every NaN of the group
  * the three backwards in float64, and the magnitude means the forward's bound is relative to
"""
from typing import NamedTuple, Optional

import numpy as np
import torch


class Ref(NamedTuple):
    out_indices: np.ndarray     # [live, kept + 1] int32
    rows: np.ndarray            # [n] int64, -1 dead or dropped
    offsets: np.ndarray         # [live + 1] int64
    list: np.ndarray            # [offsets[-1]] int64
    found: int                  # groups found (may exceed the cap)
    live: int                   # output rows = min(found, cap)
    kept_shape: list
    live_rows: int              # live input rows


def projected_keys(idx, bs, shape, axes, n_live=None):
    """int64 linear key per row on the projected grid (batch-major, last kept axis fastest), -1 for a dead row"""
    idx = np.asarray(idx, dtype=np.int64).reshape(-1, len(shape) + 1)
    ok = (idx[:, 0] >= 0) & (idx[:, 0] < bs)
    key = idx[:, 0].copy()
    for d, ext in enumerate(shape):
        ok &= (idx[:, 1 + d] >= 0) & (idx[:, 1 + d] < ext)
        if d not in axes:
            key = key * ext + idx[:, 1 + d]
    if n_live is not None:
        ok[int(n_live):] = False
    return np.where(ok, key, -1)


def decode(keys, shape):
    keys = np.asarray(keys, dtype=np.int64)
    cols = []
    for ext in reversed(shape):
        cols.append(keys % ext)
        keys = keys // ext
    return np.stack([keys] + cols[::-1], axis=1).astype(np.int32)


def build(idx, bs, shape, axes, n_live=None, cap=None) -> Ref:
    kept = [s for d, s in enumerate(shape) if d not in axes]
    keys = projected_keys(idx, bs, shape, axes, n_live)
    uniq = np.unique(keys[keys >= 0])
    found = int(uniq.shape[0])
    live = found if cap is None else min(found, int(cap))
    rows = np.full(keys.shape, -1, dtype=np.int64)
    alive = keys >= 0
    rows[alive] = np.searchsorted(uniq, keys[alive])
    rows[rows >= live] = -1
    held = np.nonzero(rows >= 0)[0]
    lst = held[np.argsort(rows[held], kind="stable")]          # groups in rank order, ascending input row inside
    offsets = np.concatenate([[0], np.cumsum(np.bincount(rows[held], minlength=live))]).astype(np.int64)
    return Ref(decode(uniq[:live], kept), rows, offsets, lst, found, live, kept, int(alive.sum()))


def _acc_type(dtype):
    return np.float64 if dtype == torch.float64 else np.float32


def _walk(feat: torch.Tensor, ref: Ref, step):
    """acc[g] over the rows of group g one by one in list order: acc starts from the first row's value, then
    acc = step(acc, value) for each further row.  Vectorised over the groups, sequential inside each."""
    at = _acc_type(feat.dtype)
    f = feat.to(torch.float64 if at == np.float64 else torch.float32).numpy()
    lens = np.diff(ref.offsets)
    acc = np.zeros((ref.live, f.shape[1]), dtype=at)
    has = lens > 0
    acc[has] = f[ref.list[ref.offsets[:-1][has]]]
    for k in range(1, int(lens.max(initial=0))):
        g = np.nonzero(lens > k)[0]
        acc[g] = step(acc[g], f[ref.list[ref.offsets[g] + k]])
    return acc, lens


def _max(feat: torch.Tensor, ref: Ref) -> torch.Tensor:
    """The stored element that wins the walk, moved with its bits: a later row takes the element when it is larger, or
    when it is the group's first NaN; a NaN is never displaced.  Zeros for an empty group."""
    f = feat.to(torch.float64 if feat.dtype == torch.float64 else torch.float32).numpy()
    lens = np.diff(ref.offsets)
    C = f.shape[1]
    src = np.full((ref.live, C), -1, dtype=np.int64)            # the input row whose element is held
    has = np.nonzero(lens > 0)[0]
    src[has] = ref.list[ref.offsets[:-1][has]][:, None]
    cols = np.arange(C)[None, :]
    for k in range(1, int(lens.max(initial=0))):
        g = np.nonzero(lens > k)[0]
        row = ref.list[ref.offsets[g] + k]
        v, a = f[row], f[src[g], cols]
        take = (v > a) | (np.isnan(v) & ~np.isnan(a))
        src[g] = np.where(take, row[:, None], src[g])
    out = torch.zeros((ref.live, C), dtype=feat.dtype)
    if has.size:
        idx = torch.from_numpy(src[has])
        out[torch.from_numpy(has)] = feat[idx, torch.arange(C)[None, :].expand_as(idx)]
    return out


def reduce(feat: torch.Tensor, ref: Ref, op: str) -> torch.Tensor:
    """[live, C] in feat's dtype: what spx_collapse_fwd must produce (sum and max: bit for bit)"""
    at = _acc_type(feat.dtype)
    if op == "max":
        return _max(feat, ref)
    acc, lens = _walk(feat, ref, lambda a, v: (a + v).astype(at))
    if op == "mean":
        acc = (acc / np.maximum(lens, 1).astype(at)[:, None]).astype(at)
    out = torch.from_numpy(acc).to(feat.dtype)                  # one rounding
    if op == "sum":
        one = np.nonzero(lens == 1)[0]
        out[torch.from_numpy(one)] = feat[torch.from_numpy(ref.list[ref.offsets[one]])]      # its bits as they are
    return out


def mean_f64(feat: torch.Tensor, ref: Ref):
    """(mean, mean of magnitudes A, group lengths) in float64: the forward bound's reference"""
    f = feat.double().numpy()
    lens = np.diff(ref.offsets)
    s = np.zeros((ref.live, f.shape[1]))
    a = np.zeros((ref.live, f.shape[1]))
    held = ref.list
    np.add.at(s, ref.rows[held], f[held])
    np.add.at(a, ref.rows[held], np.abs(f[held]))
    d = np.maximum(lens, 1)[:, None]
    return s / d, a / d, lens


def backward(feat: torch.Tensor, out: torch.Tensor, dout: torch.Tensor, ref: Ref, op: str) -> np.ndarray:
    """din [n, C] in float64: sum dout[r]; mean dout[r] / count[r]; max dout[r, c] where feat[i, c] == out[r, c] or both
    are NaN (a NaN output: every NaN of the group receives)"""
    n, C = ref.rows.shape[0], dout.shape[1]
    din = np.zeros((n, C))
    held = np.nonzero(ref.rows >= 0)[0]
    r = ref.rows[held]
    g = dout.double().numpy()[r]
    if op == "mean":
        g = g / np.diff(ref.offsets)[r][:, None]
    elif op == "max":
        f, o = feat.double().numpy()[held], out.double().numpy()[r]
        g = np.where((f == o) | (np.isnan(f) & np.isnan(o)), g, 0.0)
    din[held] = g
    return din


# ---------------------------------------------------------------------------------------- inputs shared by the tests
def scene(bs, shape, n, seed, dups=0, dead=True):
    """n rows drawn with replacement (a small grid repeats coordinates by itself), `dups` copies of earlier rows, and --
    dead=True -- rows no scene owns spread through the middle: batch -1, batch = bs, each axis once at its extent and
    once at -1.  int32 [rows, ndim + 1]."""
    rng = np.random.default_rng(seed)
    ndim = len(shape)
    idx = np.stack([rng.integers(0, bs, n)] + [rng.integers(0, s, n) for s in shape], axis=1)
    if dups and n:
        idx = np.concatenate([idx, idx[rng.integers(0, n, dups)]])
        idx = idx[rng.permutation(idx.shape[0])]
    if dead:
        extra = []
        base = [0] + [0] * ndim
        extra.append([-1] + [0] * ndim)
        extra.append([bs] + [0] * ndim)
        for d in range(ndim):
            hi, lo = list(base), list(base)
            hi[1 + d], lo[1 + d] = shape[d], -1
            extra += [hi, lo]
        extra = np.asarray(extra, dtype=np.int64)
        at = np.sort(rng.integers(0, idx.shape[0] + 1, extra.shape[0]))
        idx = np.insert(idx, at, extra, axis=0)
    return np.ascontiguousarray(idx.astype(np.int32))


def features(n, C, dtype, seed):
    """uniform in [-1, 1], rounded to the dtype"""
    g = torch.Generator().manual_seed(seed)
    return (torch.rand((n, C), generator=g, dtype=torch.float64) * 2 - 1).to(dtype)


FWD_SCENE = dict(bs=2, shape=[6, 10, 12], axes=(0,), n=700, seed=11, dups=40)      # the forward / backward tests' scene


def fwd_scene():
    s = FWD_SCENE
    return scene(s["bs"], s["shape"], s["n"], s["seed"], s["dups"])
