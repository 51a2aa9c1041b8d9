"""Where NaN, +Inf and -Inf land in a sparse convolution and its two gradients, by SET ARITHMETIC over the candidate pair
lists (refconv.pairs): which non-finite operand reaches which output element, and with which sign.  No floating sum is
formed, so this is independent of refconv.conv_from_pairs, which test_refconv.py holds to it.  Also the choice of the
rows the isolation tests poison or leave unnamed (tests/test_gpu_gemm_isolation.py), so that the CPU suite can assert the
conditions those inputs have to meet.

An element of a sum of products is
  NaN   if a term is NaN (a NaN factor, or Inf x 0), or if the terms hold +Inf and -Inf together;
  +Inf  if some term is +Inf and none is NaN or -Inf;   -Inf likewise;
  finite otherwise (the finite operands of the tests are far from overflow in float64)."""
from collections import namedtuple

import numpy as np
import torch

Classes = namedtuple("Classes", "nan pinf ninf mixed")      # bool tensors; mixed: NaN that +Inf and -Inf ALONE make


def _finish(any_nan, any_pos, any_neg):
    mixed = any_pos & any_neg & ~any_nan
    nan = any_nan | mixed
    return Classes(nan, any_pos & ~nan, any_neg & ~nan, mixed)


def _term_classes(a, b):
    """classes of the products a[p, m, 1] * b[p or 1, 1 or m, r] (broadcast): (nan, +inf, -inf) bool tensors"""
    nan = torch.isnan(a) | torch.isnan(b) | (torch.isinf(a) & (b == 0)) | (torch.isinf(b) & (a == 0))
    inf = (torch.isinf(a) | torch.isinf(b)) & ~nan
    neg = (a < 0) ^ (b < 0)                                  # (sign of the product; no NaN gets here)
    return nan, inf & ~neg, inf & neg


def _scatter_any(n, rows, flags):
    """[n, ...] bool: any of flags[j] over the j with rows[j] == r (integer counts: membership, not arithmetic)"""
    cnt = torch.zeros((n,) + tuple(flags.shape[1:]), dtype=torch.int32, device=flags.device)
    cnt.index_add_(0, rows, flags.to(torch.int32))
    return cnt > 0


def classify_rows(cand, x, weight, n_dst, transposed=False):
    """Classes of out [n_dst, K] = sum over pairs (k, src, dst) of x[src] @ W_k^T (transposed: of din = sum dout[src] @ W_k,
    with `cand` given as (k, src, dst) = (k, out rows, in rows)).  x [n_src, R] float64, weight [K, kv, C]."""
    K, kv, C = weight.shape
    ncol = C if transposed else K
    acc = [torch.zeros((n_dst, ncol), dtype=torch.bool, device=x.device) for _ in range(3)]
    bad_row = ~torch.isfinite(x).all(1)
    for k, src, dst in cand:
        keep = bad_row[src]                                   # only pairs that read a non-finite row can matter
        if not bool(keep.any()):
            continue
        s, d = src[keep], dst[keep]
        wk = weight[:, k, :].t() if transposed else weight[:, k, :]          # [ncol, R]
        t = _term_classes(x[s][:, None, :], wk[None, :, :])                  # [p, ncol, R]
        for a, f in zip(acc, t):
            a |= _scatter_any(n_dst, d, f.any(2))
    return _finish(*acc)


def classify_dw(cand, f, g, weight_shape):
    """Classes of dW [K, kv, C] = sum over pairs (k, i, o) of g[o]^T (x) f[i]."""
    K, kv, C = weight_shape
    acc = [torch.zeros((K, kv, C), dtype=torch.bool, device=f.device) for _ in range(3)]
    bad_f, bad_g = ~torch.isfinite(f).all(1), ~torch.isfinite(g).all(1)
    for k, i, o in cand:
        keep = bad_f[i] | bad_g[o]
        if not bool(keep.any()):
            continue
        t = _term_classes(g[o[keep]][:, :, None], f[i[keep]][:, None, :])    # [p, K, C]
        for a, fl in zip(acc, t):
            a[:, k, :] |= fl.any(0)
    return _finish(*acc)


def masks_of(t):
    return torch.isnan(t), t == float("inf"), t == float("-inf")


# ---------------------------------------------------------------- which rows the isolation tests touch
Poison = namedtuple("Poison", "nan pinf ninf channels")     # row index tensors (int64, CPU) and the channels they hold


def poison_rows(cand, n_src, width, seed, swap=False):
    """Rows of the SOURCE tensor of a product (feature rows for out / dW; with swap, dout rows for din / dW) to hold NaN,
    +Inf and -Inf, chosen from the pair lists alone:
      - about 4 % of the destination rows are reached (rows of each kind = 0.04 / 3 x destination rows / fan-out, at
        least one);
      - every -Inf row shares a destination row with a +Inf row, so some element receives both -- unless no destination
        row has two source rows (the input gradient of a 2x2x2 / stride-2 layer: one term per row; the two poisoned
        channels of ONE row then meet under weights of opposite sign);
      - two channels each (one when the tensor has a single channel)."""
    rng = np.random.default_rng(seed)
    src = torch.cat([(o if swap else i) for _, i, o in cand]).cpu().numpy()
    dst = torch.cat([(i if swap else o) for _, i, o in cand]).cpu().numpy()
    named = np.unique(src)
    fan = max(1.0, src.shape[0] / max(named.shape[0], 1))
    m = max(1, int(round(0.04 / 3 * np.unique(dst).shape[0] / fan)))
    pick = rng.permutation(named)
    # +Inf rows in the permutation's order, each with a partner: another source row of a destination row it reaches
    by_dst = np.argsort(dst, kind="stable")
    dst_s, src_s = dst[by_dst], src[by_dst]
    by_src = np.argsort(src, kind="stable")
    src_t, dst_t = src[by_src], dst[by_src]
    pinf, ninf, taken = [], [], set()
    for p in pick:
        if len(pinf) == m:
            break
        if int(p) in taken:
            continue
        for d in dst_t[np.searchsorted(src_t, p):np.searchsorted(src_t, p, side="right")]:
            lo, hi = np.searchsorted(dst_s, d), np.searchsorted(dst_s, d, side="right")
            other = [int(r) for r in src_s[lo:hi] if int(r) != int(p) and int(r) not in taken]
            if other:
                pinf.append(int(p))
                ninf.append(other[0])
                taken.update((int(p), other[0]))
                break
    if not ninf:                                            # no two source rows share a destination row
        pinf, ninf = [int(r) for r in pick[:m]], [int(r) for r in pick[m:2 * m]]
        taken.update(pinf + ninf)
    assert pinf and ninf, "too few named rows"
    pinf = np.sort(np.array(pinf))
    rest = np.array([r for r in pick if int(r) not in taken], dtype=np.int64)
    nan = np.sort(rest[:m])
    assert nan.size, "no row left for NaN"
    ch = rng.permutation(width)[:min(2, width)]
    as_t = lambda a: torch.from_numpy(np.asarray(a, dtype=np.int64))
    return Poison(as_t(nan), as_t(pinf), as_t(np.sort(np.array(ninf))), as_t(np.sort(ch)))


def poisoned(t, p):
    """a copy of t [n, width] with the poison in place"""
    t = t.clone()
    dev = t.device
    ch = p.channels.to(dev)
    for rows, v in ((p.nan, float("nan")), (p.pinf, float("inf")), (p.ninf, float("-inf"))):
        r = rows.to(dev)
        t[r[:, None], ch[None, :]] = v
    return t


def unnamed_rows(n, seed):
    """About 5 % of n rows: the first and the last row of the second 128-row tile, the last row of the first and of the
    tensor, and a random rest (sorted, distinct, int64, CPU)."""
    rng = np.random.default_rng(seed)
    fixed = np.array([r for r in (127, 128, 255, n - 1) if 0 <= r < n], dtype=np.int64)
    rest = rng.permutation(n)[:max(int(round(0.05 * n)) - fixed.shape[0], 0)].astype(np.int64)
    return torch.from_numpy(np.unique(np.concatenate([fixed, rest])))


# ---------------------------------------------------------------- the row operators (tests/test_gpu_rowop_isolation.py)
# A row operator's output element is a sum (or a maximum) over the ENTRIES of a group: the rows of a collapse group, the
# operands present at a union row, the corners of a point, the entries of a transposed list.  The classes below are
# derived from which entry holds what, by counting; no floating sum is formed.
def _any_by_group(n_groups, grp, flags):
    cnt = np.zeros((n_groups,) + flags.shape[1:], dtype=np.int64)
    np.add.at(cnt, grp, flags.astype(np.int64))
    return cnt > 0


def classify_entries(n_groups, grp, x, w=None):
    """Classes (numpy bool [n_groups, C]) of out[g] = sum over the entries e with grp[e] == g of x[e] (w given: of
    w[e] * x[e], so a zero weight on an Inf makes a NaN).  x float64 [E, C], w float64 [E]."""
    x = np.asarray(x, dtype=np.float64)
    if w is None:
        nan, pos, neg = np.isnan(x), x == np.inf, x == -np.inf
    else:
        w = np.asarray(w, dtype=np.float64)[:, None]
        nan = np.isnan(x) | np.isnan(w) | (np.isinf(x) & (w == 0)) | (np.isinf(w) & (x == 0))
        inf = (np.isinf(x) | np.isinf(w)) & ~nan
        sign = (x < 0) ^ (w < 0)
        pos, neg = inf & ~sign, inf & sign
    return _finish(*[_any_by_group(n_groups, grp, f) for f in (nan, pos, neg)])


def classify_max(n_groups, grp, x):
    """Classes of out[g] = max over the group's entries with NaN propagating: NaN if any entry is, else +Inf if any is,
    -Inf only when every entry is.  `mixed` is empty: +Inf and -Inf together give +Inf."""
    x = np.asarray(x, dtype=np.float64)
    nan = _any_by_group(n_groups, grp, np.isnan(x))
    pos = _any_by_group(n_groups, grp, x == np.inf) & ~nan
    some = _any_by_group(n_groups, grp, np.ones_like(x, dtype=bool))
    neg = some & ~_any_by_group(n_groups, grp, x != -np.inf)
    return Classes(nan, pos, neg, np.zeros_like(nan))


def masks_np(a):
    a = np.asarray(a, dtype=np.float64)
    return np.isnan(a), a == np.inf, a == -np.inf


def group_of_entries(offsets):
    """the group of every list position: [offsets[-1]] int64"""
    offsets = np.asarray(offsets, dtype=np.int64)
    return np.repeat(np.arange(offsets.shape[0] - 1), np.diff(offsets))


# two quiet NaNs per dtype that differ in their payload, as bit patterns (positive; | the sign bit for a negative one)
NAN_BITS = {torch.float16: (0x7e00, 0x7e55), torch.bfloat16: (0x7fc0, 0x7fd5), torch.float32: (0x7fc00000, 0x7fc12345),
            torch.float64: (0x7ff8000000000000, 0x7ff8000000012345)}
_INT_OF = {2: torch.int16, 4: torch.int32, 8: torch.int64}
BIG = 60000.0           # finite in every dtype; two of them exceed float16's range (65504) in a float32 sum

GroupPoison = namedtuple("GroupPoison", "cells roles channels")     # cells: [(input row, kind)], roles: {name: group}


def poison_groups(offsets, lst, C, seed):
    """Which rows of which groups hold what, chosen from the group table alone.  Eight groups of three rows or more take
    one role each: nan_first / nan_last / nan_mid (one NaN at that position of the list), nan_two (two NaNs with
    different payloads, the first of them at position 1), mixed (+Inf then -Inf: the sum is NaN, the maximum +Inf), pinf,
    ninf, big (EVERY row holds BIG: finite rows whose float16 sum overflows); a group of one row, when there is one,
    holds a NaN (nan_single: copied).  Two channels (one for C = 1)."""
    offsets, lst = np.asarray(offsets, dtype=np.int64), np.asarray(lst, dtype=np.int64)
    lens = np.diff(offsets)
    rng = np.random.default_rng(seed)
    long_ = rng.permutation(np.nonzero(lens >= 3)[0])
    names = ("nan_first", "nan_last", "nan_mid", "nan_two", "mixed", "pinf", "ninf", "big")
    assert long_.shape[0] >= len(names), "too few groups of three rows"
    roles = {k: int(g) for k, g in zip(names, long_)}
    at = lambda g, k: int(lst[offsets[g] + k])
    L = lambda g: int(lens[g])
    r = roles
    cells = [(at(r["nan_first"], 0), "nan_a"), (at(r["nan_last"], L(r["nan_last"]) - 1), "nan_a"),
             (at(r["nan_mid"], L(r["nan_mid"]) // 2), "nan_b"),
             (at(r["nan_two"], 1), "nan_b"), (at(r["nan_two"], L(r["nan_two"]) - 1), "nan_a"),
             (at(r["mixed"], 0), "pinf"), (at(r["mixed"], 1), "ninf"),
             (at(r["pinf"], L(r["pinf"]) - 1), "pinf"), (at(r["ninf"], 0), "ninf")]
    cells += [(at(r["big"], k), "big") for k in range(L(r["big"]))]
    ones = np.nonzero(lens == 1)[0]
    if ones.size:
        roles["nan_single"] = int(ones[rng.integers(0, ones.size)])
        cells.append((at(roles["nan_single"], 0), "nan_b"))
    return GroupPoison(cells, roles, np.sort(rng.permutation(C)[:min(2, C)]))


def poisoned_groups(feat, p):
    """a copy of feat [n, C] with the cells of `p` in place (NaNs as bit patterns: the payloads are the test's)"""
    t = feat.clone()
    raw = t.view(_INT_OF[t.element_size()])
    na, nb = NAN_BITS[t.dtype]
    if t.dtype == torch.float16:
        na, nb = na - 0x10000 if na >= 0x8000 else na, nb - 0x10000 if nb >= 0x8000 else nb
    for row, kind in p.cells:
        for c in p.channels.tolist():
            if kind == "nan_a":
                raw[row, c] = na
            elif kind == "nan_b":
                raw[row, c] = nb
            else:
                t[row, c] = {"pinf": float("inf"), "ninf": float("-inf"), "big": BIG}[kind]
    return t


def poison_rows_flat(grp, src, n_src, width, seed):
    """poison_rows for ONE list of entries: entry e adds source row src[e] into group grp[e]"""
    cand = [(0, torch.from_numpy(np.asarray(src, dtype=np.int64)), torch.from_numpy(np.asarray(grp, dtype=np.int64)))]
    return poison_rows(cand, n_src, width, seed)
