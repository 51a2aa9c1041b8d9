"""The inputs of the row operators' isolation tests (tests/test_gpu_rowop_isolation.py) and of the CPU tests that hold
the references to them (tests/test_refrowops.py): group tables, the rows that hold NaN / +Inf / -Inf, and the numpy
references' outputs -- each made once and never modified.  Scenes and references are the existing ones (refcollapse,
refselect, refinterp, the fixtures of test_gpu_interp / test_gpu_pointvoxel / test_gpu_union); tests/nonfinite.py chooses
the poisoned rows and derives where the non-finite values land."""
import functools

import numpy as np
import torch

import nonfinite as nf
import refcollapse as rc
import refinterp as ri
import refselect as rs

DTYPES = {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32, "f64": torch.float64}
# (dtype, C): the element path (C = 3), one 16-byte piece (8 x f16), five pieces in a group of eight lanes (C = 40), 65
# pieces = a second pass of a full wave (520 x f16); f64 where the unit has it
WIDTHS = [("f16", 3), ("f16", 8), ("f16", 40), ("f16", 520), ("bf16", 3), ("bf16", 40), ("f32", 3), ("f32", 40),
          ("f64", 3)]


# ---------------------------------------------------------------------------------------- collapse / point groups
@functools.lru_cache(maxsize=None)
def collapse_case(name):
    """(idx, bs, shape, axes, ref): `fwd` the scene of test_gpu_collapse's forward tests (740 rows + dead ones, groups
    of 1 .. 9 rows), `lengths` columns of 1 .. 9 rows twice over (every length on both sides of the four-entry walk),
    `rows3000`, `rows255` / `rows256` / `rows257` around one workgroup, `one` a single row"""
    if name == "fwd":
        s = rc.FWD_SCENE
        idx, bs, shape, axes = rc.fwd_scene(), s["bs"], s["shape"], s["axes"]
    elif name == "lengths":
        bs, shape, axes = 2, [10, 4, 4], (0,)
        rows = [(b, z, k // 4, k % 4) for b in range(2) for k in range(9) for z in range(k + 1)]
        idx = np.array(rows, np.int32)[np.random.default_rng(5).permutation(len(rows))]
    elif name == "rows3000":
        bs, shape, axes = 2, [6, 20, 24], (0,)
        idx = rc.scene(bs, shape, 3000, 77, 60)
    elif name in ("rows255", "rows256", "rows257"):             # one workgroup of 256 rows: short by one, full, one over
        bs, shape, axes = 2, [5, 14, 16], (0,)
        idx = rc.scene(bs, shape, int(name[4:]) - 8, 30 + int(name[4:]), 0)      # + the 8 rows no scene owns
        assert idx.shape[0] == int(name[4:])
    elif name == "one":
        bs, shape, axes = 1, [4, 3, 3], (0,)
        idx = np.array([[0, 2, 1, 1]], np.int32)
    else:
        raise KeyError(name)
    return idx, bs, shape, axes, rc.build(idx, bs, shape, axes)


@functools.lru_cache(maxsize=None)
def collapse_named(name, dt, C):
    """(feat with the poison in place, the plan): finite values in [-1, 1] elsewhere"""
    idx, _, _, _, ref = collapse_case(name)
    plan = nf.poison_groups(ref.offsets, ref.list, C, 7 + C)
    return nf.poisoned_groups(rc.features(idx.shape[0], C, DTYPES[dt], 500 + C), plan), plan


def collapse_classes(feat, ref, op):
    """where a reduction over the groups of `ref` is NaN / +Inf / -Inf, from the entries alone.  The `big` role (finite
    rows whose float16 sum leaves the type's range) is the caller's: nf.BIG is finite."""
    grp = nf.group_of_entries(ref.offsets)
    x = feat.double().numpy()[ref.list]
    return nf.classify_max(ref.live, grp, x) if op == "max" else nf.classify_entries(ref.live, grp, x)


def overflow_mask(plan, ref, C, dtype, op):
    """[live, C] bool: the elements of the `big` group that round to +Inf -- a float16 sum of two or more BIG"""
    m = np.zeros((ref.live, C), dtype=bool)
    if dtype == torch.float16 and op == "sum":
        m[plan.roles["big"], plan.channels] = True
    return m


def max_bwd_receivers(feat, out, ref):
    """[n, C] bool: the input elements that receive the gradient of a max -- equal to the output, or NaN under a NaN
    output -- from comparisons alone"""
    f, o = feat.double().numpy(), out.double().numpy()
    held = np.nonzero(ref.rows >= 0)[0]
    m = np.zeros(f.shape, dtype=bool)
    fo = o[ref.rows[held]]
    m[held] = (f[held] == fo) | (np.isnan(f[held]) & np.isnan(fo))
    return m


# ---------------------------------------------------------------------------------------- interpolation
@functools.lru_cache(maxsize=None)
def interp_case(C):
    """the main 3-d scene of test_gpu_interp (hash form: dead rows, ghosts behind the live count) with its reference
    corner table, and the voxel rows to poison in two of C channels: those of nonfinite.poison_rows over the live
    corners, plus the three rows (not the 600-point voxel) that the most live corners with weight EXACTLY 0 name, which
    hold +Inf"""
    import test_gpu_interp as TI
    sc = TI.scene(3)
    rows, w = sc.ref(True)
    n = len(sc.full)
    live = rows >= 0
    pt, c = np.nonzero(live)
    p = nf.poison_rows_flat(pt, rows[pt, c], n, C, 41)
    taken = set(torch.cat([p.nan, p.pinf, p.ninf]).tolist()) | {sc.long_row}
    zc = np.bincount(rows[live & (w == 0)], minlength=n)
    order = [int(r) for r in np.argsort(-zc, kind="stable") if int(r) not in taken][:3]
    return sc, rows, w, p, torch.tensor(sorted(order), dtype=torch.int64)


def interp_poisoned(vfeat, p, zero_rows):
    t = nf.poisoned(vfeat, p)
    t[zero_rows[:, None], p.channels[None, :]] = float("inf")
    return t


# ---------------------------------------------------------------------------------------- scores
@functools.lru_cache(maxsize=None)
def score_named(dt, C, n=600):
    """features with NaN, +Inf and -Inf rows (two channels each, by nonfinite.unnamed_rows' choice of rows: tile edges
    included) and the three row sets"""
    feat = rc.features(n, C, DTYPES[dt], 900 + C)
    rows = nf.unnamed_rows(n, 17).tolist()
    third = max(len(rows) // 3, 1)
    sets = {"nan": rows[:third], "pinf": rows[third:2 * third], "ninf": rows[2 * third:]}
    ch = np.sort(np.random.default_rng(C).permutation(C)[:min(2, C)])
    na, nb = nf.NAN_BITS[DTYPES[dt]]
    raw = feat.view(nf._INT_OF[feat.element_size()])
    for k, r in enumerate(sets["nan"]):
        bits = (na, nb)[k % 2] | ((1 << (8 * feat.element_size() - 1)) if k % 4 >= 2 else 0)      # both signs, two payloads
        if bits >= 1 << (8 * feat.element_size() - 1):
            bits -= 1 << (8 * feat.element_size())
        raw[r, int(ch[0])] = bits
    feat[torch.tensor(sets["pinf"])[:, None], torch.from_numpy(ch)[None, :]] = float("inf")
    feat[torch.tensor(sets["ninf"])[:, None], torch.from_numpy(ch)[None, :]] = float("-inf")
    return feat, sets


def keep_of_nan_scores(score):
    """refselect's selection must not depend on a computed NaN's payload: every NaN becomes the canonical positive one"""
    s = np.array(score, dtype=np.float32)
    s[np.isnan(s)] = np.array([0x7fc00000], dtype=np.uint32).view(np.float32)[0]
    return s


# ---------------------------------------------------------------------------------------- union merge
@functools.lru_cache(maxsize=None)
def union_case(dt, C):
    """Three operands of test_gpu_union's static-form scene with poisoned rows: nonfinite.poison_rows over the entries
    (operand row -> union row), and by hand a NaN at a row that ONE operand holds, at one that TWO and at one that all
    THREE hold (the second operand's row where there is a choice).  (idxs, feats, union keys, expected features, rows
    per operand, entries (group, flat source), operands present per union row)"""
    import test_gpu_union as TU
    bs, shape = TU.SMALL
    idxs = [TU.operand(bs, shape, 260 + 30 * t, 120 + t) for t in range(3)]
    feats = [TU.features(i.shape[0], C, DTYPES[dt], 123 + t) for t, i in enumerate(idxs)]
    uniq, _, rows_ref = TU.expect(idxs, feats, bs, shape)
    base = np.cumsum([0] + [i.shape[0] for i in idxs])
    grp = np.concatenate([r[r >= 0] for r in rows_ref])
    src = np.concatenate([base[t] + np.nonzero(r >= 0)[0] for t, r in enumerate(rows_ref)])
    present = np.bincount(grp, minlength=len(uniq))
    p = nf.poison_rows_flat(grp, src, int(base[-1]), C, 47)
    cat = nf.poisoned(torch.cat(feats), p)
    for k in (1, 2, 3):
        r = int(np.nonzero(present == k)[0][k])                 # (some row of that kind)
        e = np.nonzero(grp == r)[0]
        cat[int(src[e[min(1, k - 1)]]), p.channels] = float("nan")
    bad = [cat[base[t]:base[t + 1]].clone() for t in range(3)]
    with np.errstate(invalid="ignore"):
        _, want, _ = TU.expect(idxs, bad, bs, shape)
    return idxs, bad, uniq, want, rows_ref, (grp, src), present
