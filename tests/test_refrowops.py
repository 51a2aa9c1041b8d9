"""The references of the row operators on NaN / +Inf / -Inf (include/spconv_amd.h, "What the row operators may be handed"),
held on the CPU before tests/test_gpu_rowop_isolation.py holds the kernels to them:

  placement   where refcollapse.reduce / backward, refselect.score, refinterp.forward / backward and the union's
              expectation are NaN, +Inf or -Inf equals a derivation that forms no floating sum (tests/nonfinite.py: counting
              over the groups' entries)
  fixtures    the poisoned inputs of tests/rowopscenes.py meet the conditions the GPU tests rely on: +Inf and -Inf meet in
              some output element; a max group has its NaN first, one last, one in the middle, one two NaNs of different
              payloads; a float16 group of finite rows overflows; at least half of the output stays finite; the
              interpolation names poisoned rows through at least 20 live corners of weight exactly 0 and 20 of weight > 0
  score sets  refselect.scores("nan") holds NaNs of both signs and two payloads, and the key order is the documented one"""
import numpy as np
import pytest
import torch

import nonfinite as nf
import refcollapse as rc
import refinterp as ri
import refselect as rs
import rowopscenes as S

OPS = ("sum", "mean", "max")
# (the numpy references add Inf to -Inf and multiply 0 by Inf on purpose)
pytestmark = pytest.mark.filterwarnings("ignore:invalid value encountered:RuntimeWarning")


def assert_classes(out, cls, extra_pinf=None, what=""):
    nan, pinf, ninf = nf.masks_np(out.double().numpy() if isinstance(out, torch.Tensor) else out)
    want_pinf = cls.pinf if extra_pinf is None else (cls.pinf | extra_pinf)
    assert np.array_equal(nan, cls.nan), f"{what}: NaN placement"
    assert np.array_equal(pinf, want_pinf), f"{what}: +Inf placement"
    assert np.array_equal(ninf, cls.ninf), f"{what}: -Inf placement"
    return nan | pinf | ninf


# ---------------------------------------------------------------------------------------- collapse / point-voxel
@pytest.mark.parametrize("case", ["fwd", "lengths"])
@pytest.mark.parametrize("dt,C", S.WIDTHS)
def test_collapse_placement_and_fixture(case, dt, C):
    idx, _, _, _, ref = S.collapse_case(case)
    feat, plan = S.collapse_named(case, dt, C)
    dtype = S.DTYPES[dt]
    lens = np.diff(ref.offsets)
    for op in OPS:
        out = rc.reduce(feat, ref, op)
        cls = S.collapse_classes(feat, ref, op)
        over = S.overflow_mask(plan, ref, C, dtype, op)
        bad = assert_classes(out, cls, over, f"{case} {dt} C={C} {op}")
        assert bad.mean() <= 0.5                                            # at least half of the output stays finite
        if op != "max":
            assert cls.mixed[plan.roles["mixed"], plan.channels].all()      # +Inf and -Inf meet in one element
    if dt == "f16":                                                         # finite rows, an infinite float16 sum
        g = plan.roles["big"]
        rows = ref.list[ref.offsets[g]:ref.offsets[g + 1]]
        assert bool(torch.isfinite(feat[torch.from_numpy(rows)]).all()) and lens[g] >= 2
        assert bool(torch.isposinf(rc.reduce(feat, ref, "sum")[g, torch.from_numpy(plan.channels)]).all())
    # the max fixture: where each group's NaNs sit in its list
    isnan = torch.isnan(feat[:, int(plan.channels[0])]).numpy()
    where = {k: np.nonzero(isnan[ref.list[ref.offsets[g]:ref.offsets[g + 1]]])[0].tolist() for k, g in plan.roles.items()}
    L = {k: int(lens[g]) for k, g in plan.roles.items()}
    assert where["nan_first"] == [0] and where["nan_last"] == [L["nan_last"] - 1]
    assert len(where["nan_mid"]) == 1 and 0 < where["nan_mid"][0] < L["nan_mid"] - 1
    assert where["nan_two"] == [1, L["nan_two"] - 1]
    g = plan.roles["nan_two"]
    two = feat[torch.from_numpy(ref.list[ref.offsets[g]:ref.offsets[g + 1]][where["nan_two"]]), int(plan.channels[0])]
    raw = two.view(nf._INT_OF[two.element_size()])
    assert int(raw[0]) != int(raw[1])                                       # different payloads
    # max moves the FIRST NaN of the group, bits unchanged
    out = rc.reduce(feat, ref, "max").view(raw.dtype)
    assert int(out[g, int(plan.channels[0])]) == int(raw[0])


@pytest.mark.parametrize("dt,C", [("f16", 8), ("f32", 3), ("f64", 3)])
def test_collapse_max_without_nan_is_what_it_was(dt, C):
    """first of equals, -0.0 / +0.0 compared as equal: the walk that held before NaN was decided"""
    idx, _, _, _, ref = S.collapse_case("fwd")
    feat = (rc.features(idx.shape[0], C, S.DTYPES[dt], 3) * 2).round() / 2         # five values: ties everywhere
    feat[feat == 0] = -0.0
    feat[::7][feat[::7] == 0] = 0.0
    acc, _ = rc._walk(feat, ref, lambda a, v: np.where(v > a, v, a))
    want = torch.from_numpy(acc).to(feat.dtype)
    got = rc.reduce(feat, ref, "max")
    bits = lambda t: t.view(nf._INT_OF[t.element_size()])
    assert torch.equal(bits(got), bits(want))


@pytest.mark.parametrize("dt,C", [("f16", 8), ("bf16", 3), ("f32", 40), ("f64", 3)])
def test_collapse_backward_reference(dt, C):
    idx, _, _, _, ref = S.collapse_case("fwd")
    feat, plan = S.collapse_named("fwd", dt, C)
    dout = rc.features(ref.live, C, S.DTYPES[dt], 11)
    out = rc.reduce(feat, ref, "max")
    din = rc.backward(feat, out, dout, ref, "max")
    recv = S.max_bwd_receivers(feat, out, ref)
    held = ref.rows >= 0
    want = np.where(recv, dout.double().numpy()[np.maximum(ref.rows, 0)], 0.0) * held[:, None]
    assert np.array_equal(din, want)
    # a NaN output sends its gradient to every NaN of the group and to nobody else
    g, c = plan.roles["nan_two"], int(plan.channels[0])
    rows = ref.list[ref.offsets[g]:ref.offsets[g + 1]]
    nan_rows = rows[torch.isnan(feat[torch.from_numpy(rows), c]).numpy()]
    assert len(nan_rows) == 2 and (din[nan_rows, c] == float(dout[g, c])).all()
    assert (din[np.setdiff1d(rows, nan_rows), c] == 0).all()
    for k in ("nan_first", "nan_last", "nan_mid"):                          # the gradient does not vanish
        g = plan.roles[k]
        rows = ref.list[ref.offsets[g]:ref.offsets[g + 1]]
        assert (din[rows, c] != 0).sum() == 1
    # mean: dout / count for every held row, whatever feat holds
    din = rc.backward(feat, rc.reduce(feat, ref, "mean"), dout, ref, "mean")
    assert np.isfinite(din).all()


# ---------------------------------------------------------------------------------------- scores and top-k
@pytest.mark.parametrize("dt,C", S.WIDTHS)
@pytest.mark.parametrize("op", ["absmean", "absmax"])
def test_score_placement(dt, C, op):
    feat, sets = S.score_named(dt, C)
    f = feat.double().numpy()
    nan = np.isnan(f).any(axis=1)
    inf = np.isinf(f).any(axis=1) & ~nan
    assert nan.sum() == len(sets["nan"]) and inf.sum() == len(sets["pinf"]) + len(sets["ninf"])
    for s in (rs.score(feat, op), rs.score_f64(feat, op)):
        assert np.array_equal(np.isnan(s), nan) and np.array_equal(s == np.inf, inf) and not (s == -np.inf).any()
    assert (nan | inf).mean() <= 0.5
    # a NaN score sorts above +inf: the canonical positive NaN's key
    s = S.keep_of_nan_scores(rs.score(feat, op))
    k = rs.keys(s)
    assert k[nan].min() > k[~nan].max()


def test_nan_score_kind_and_key_order():
    pool = set(rs.NAN_KEY_ORDER)
    for n in (257, 3000, 20000):
        s = rs.scores("nan", n, 11 + n)
        b = s.view(np.uint32)
        assert set(b.tolist()) <= pool | {0x3f800000}
        if n >= 3000:
            assert set(b.tolist()) == pool
            for v in pool:                                                  # every pattern's ties span blocks of 256 rows
                at = np.nonzero(b == v)[0]
                assert at[0] // 256 != at[-1] // 256
        assert np.isnan(s).sum() > 0 and np.isinf(s).sum() > 0
    order = np.array(rs.NAN_KEY_ORDER, dtype=np.uint32)
    k = rs.keys(order.view(np.float32))
    assert (np.diff(k.astype(np.int64)) > 0).all()                          # -NaN < -inf < finite < +inf < +NaN, by payload
    # exactly the positive NaNs are the top rows, the larger payload first
    s = rs.scores("nan", 3000, 5)
    b = s.view(np.uint32)
    top = rs.topk(s, int((b == 0x7fc12345).sum())).keep
    assert np.array_equal(top != 0, b == 0x7fc12345)
    top = rs.topk(s, int(((b == 0x7fc12345) | (b == 0x7fc00000)).sum())).keep
    assert np.array_equal(top != 0, (b & 0xffc00000) == 0x7fc00000)
    bottom = rs.topk(s, 3000 - int((b == 0xffc12345).sum())).keep
    assert np.array_equal(bottom == 0, b == 0xffc12345)


@pytest.mark.parametrize("n", [257, 3000, 20000])
def test_top_byte_kind_holds_no_nan(n):
    s = rs.scores("top_byte", n, 11 + n)
    assert np.isfinite(s).all()


# ---------------------------------------------------------------------------------------- interpolation
@pytest.mark.parametrize("C", [3, 8])
def test_interp_placement_and_fixture(C):
    sc, rows, w, p, zero_rows = S.interp_case(C)
    n, N = len(sc.full), rows.shape[0]
    g = torch.Generator().manual_seed(C)
    vfeat = S.interp_poisoned(torch.randn((n, C), generator=g, dtype=torch.float32), p, zero_rows)
    bad_row = ~torch.isfinite(vfeat).all(1).numpy()
    live = rows >= 0
    assert (live & (w == 0) & bad_row[np.maximum(rows, 0)]).sum() >= 20     # zero-weight live corners at poisoned rows
    assert (live & (w != 0) & bad_row[np.maximum(rows, 0)]).sum() >= 20
    pt, c = np.nonzero(live)
    cls = nf.classify_entries(N, pt, vfeat.double().numpy()[rows[pt, c]], w[pt, c])
    out = ri.forward(vfeat.numpy(), rows, w)
    bad = assert_classes(out, cls, None, "interp forward")
    assert cls.mixed.any() and bad.mean() <= 0.5
    # 0 x Inf: some output is NaN although every poisoned row its point names with weight > 0 is finite
    zero_only = nf.classify_entries(N, pt, vfeat.double().numpy()[rows[pt, c]] * 1.0, np.where(w[pt, c] == 0, 1.0, 0.0))
    assert (cls.nan & ~nf.classify_entries(N, pt[w[pt, c] != 0], vfeat.double().numpy()[rows[pt, c]][w[pt, c] != 0],
                                           w[pt, c][w[pt, c] != 0]).nan).any() and zero_only.nan.any()


@pytest.mark.parametrize("C", [3, 8])
def test_interp_backward_placement(C):
    sc, rows, w, _, _ = S.interp_case(C)
    n, N = len(sc.full), rows.shape[0]
    K = rows.shape[1]
    offsets, lst = ri.transposed(rows, n)
    grp = nf.group_of_entries(offsets)
    keep = grp < sc.n_live                                                  # rows behind the live count get zeros
    p = nf.poison_rows_flat(grp[keep], lst[keep] // K, N, C, 43)
    g = torch.Generator().manual_seed(C + 1)
    dout = nf.poisoned(torch.randn((N, C), generator=g, dtype=torch.float32), p)
    cls = nf.classify_entries(n, grp[keep], dout.double().numpy()[lst[keep] // K], w.reshape(-1)[lst[keep]])
    dv = ri.backward(dout.numpy(), rows, w, n, sc.n_live)
    bad = assert_classes(dv, cls, None, "interp backward")
    assert cls.mixed.any() and bad.mean() <= 0.5 and not bad[sc.n_live:].any()


# ---------------------------------------------------------------------------------------- union merge
@pytest.mark.parametrize("dt,C", [("f16", 8), ("f32", 3)])
def test_union_placement(dt, C):
    idxs, feats, uniq, want, rows_ref, (grp, src), present = S.union_case(dt, C)
    cat = torch.cat(feats)
    cls = nf.classify_entries(len(uniq), grp, cat.double().numpy()[src])
    bad = assert_classes(want, cls, None, "union")
    assert cls.mixed.any() and bad.mean() <= 0.5
    assert set(present[bad.any(axis=1)].tolist()) == {1, 2, 3}               # rows held by one, two and three operands
