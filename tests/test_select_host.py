"""Voxel pruning (csrc/select.hip): what can be checked without a GPU -- the unit is linked, the size queries, the
launch-count keys, the argument checks that come before anything touches the device, the Python argument validation,
and the numpy reference (tests/refselect.py) against brute-force numpy."""
import ctypes
import os

import numpy as np
import pytest
import torch

import refselect as rs
from spconv_amd import _lib

NAMES = ("spx_row_score", "spx_topk_ws_bytes", "spx_topk_flags", "spx_select_ws_bytes", "spx_select_count",
         "spx_select_fill", "spx_select_static")
KEYS = ("select/score", "select/hist", "select/pick", "select/ties", "select/flags", "select/count", "select/scan",
        "select/scatter", "select/map")


def test_select_unit_is_linked():
    units = {os.path.splitext(os.path.basename(o))[0] for o in _lib.linked_objects()}
    assert "select" in units
    L = _lib.load()
    for name in NAMES:
        assert getattr(L, name) is not None


def test_ws_bytes_queries():
    L = _lib.load()
    sizes = [int(L.spx_select_ws_bytes(3, n)) for n in (0, 1, 256, 257, 3000, 20000, 400000, 2 ** 31 - 1)]
    assert all(s > 0 for s in sizes) and sizes == sorted(sizes) and sizes[-1] > sizes[0]
    assert [int(L.spx_select_ws_bytes(nd, 1000)) > 0 for nd in (1, 2, 3, 4)] == [True] * 4
    for ndim, n in ((3, -1), (0, 100), (5, 100), (-1, 100), (3, 2 ** 31)):
        assert L.spx_select_ws_bytes(ndim, n) == 0, (ndim, n)
    sizes = [int(L.spx_topk_ws_bytes(n)) for n in (0, 1, 256, 257, 3000, 20000, 400000, 2 ** 31 - 1)]
    assert all(s >= 4 * 256 * 4 for s in sizes) and sizes == sorted(sizes) and sizes[-1] > sizes[0]
    assert L.spx_topk_ws_bytes(-1) == 0 and L.spx_topk_ws_bytes(2 ** 31) == 0


def test_launch_count_keys():
    L = _lib.load()
    for key in KEYS:
        assert L.spx_launch_count(key.encode()) >= 0, key
    for key in ("select", "select/", "select/sort", "select/hist/", "select/score/f16"):
        assert L.spx_launch_count(key.encode()) == -1, key


def test_bad_arguments_are_refused_before_any_pointer_is_read():
    """Every call below passes NULL for every pointer: no device is needed to be told no."""
    L = _lib.load()
    err = lambda: L.spx_last_error().decode()
    F16 = _lib.DTYPE_F16
    score = lambda C, dt, op: L.spx_row_score(None, 4, C, dt, op, None, None, None)
    assert score(4, _lib.DTYPE_I8, _lib.SCORE_ABSMEAN) != 0 and "dtype" in err()
    assert score(4, 7, _lib.SCORE_ABSMEAN) != 0 and "dtype" in err()
    assert score(0, F16, _lib.SCORE_ABSMEAN) != 0 and "channel count" in err()
    assert score(4, F16, 2) != 0 and "op must be absmean" in err()
    assert score(4, F16, -1) != 0 and "op must be absmean" in err()
    assert L.spx_row_score(None, -1, 4, F16, 0, None, None, None) != 0 and "row count" in err()
    flags = lambda k, ratio: L.spx_topk_flags(None, None, 4, None, 0, 0, k, ratio, None, None, None, 0, None)
    for ratio in (-0.25, 1.5, float("nan")):
        assert flags(-1, ratio) != 0 and "ratio must be in [0, 1]" in err(), ratio
    with pytest.raises(RuntimeError, match="ratio must be in"):
        _lib.check(-1)
    assert flags(2, 7.0) != 0 and "NULL" in err()                 # (a count: the ratio is not looked at)
    sp = _lib.ints([4, 5, 6])
    result = (ctypes.c_int * 2)()
    builds = {
        "count": lambda nd, inv: L.spx_select_count(None, 4, None, nd, 1, sp, None, inv, None, 0, result, None),
        "fill": lambda nd, inv: L.spx_select_fill(None, 4, None, nd, 1, sp, None, inv, 2, None, None, None, None, 0, None,
                                                  None, 0, None),
        "static": lambda nd, inv: L.spx_select_static(None, 4, None, nd, 1, sp, None, inv, 4, None, None, None, None, None,
                                                      0, None, None, 0, None),
    }
    for name, call in builds.items():
        for inv in (2, -1):
            assert call(3, inv) != 0, name
            assert "invert must be 0 or 1" in err(), name
        assert call(5, 0) != 0 and "ndim must be in [1,4]" in err(), name
        assert call(3, 0) != 0 and "NULL" in err(), name          # (well-formed: refused for its pointers only)


def test_python_argument_validation():
    import spconv_amd.pytorch as spconv
    from spconv_amd.pytorch import _select
    F = spconv.functional
    for k, ratio in ((None, None), (3, 0.5)):
        with pytest.raises(ValueError, match="exactly one of k and ratio"):
            _select.check_count(k, ratio, "topk_mask")
        with pytest.raises(ValueError, match="exactly one of k and ratio"):
            F.topk_mask(torch.zeros(4), k=k, ratio=ratio)
        with pytest.raises(ValueError, match="exactly one of k and ratio"):
            spconv.SparsePrune(ratio=ratio, k=k)
    assert _select.check_count(3, None, "x") == (3, 0.0) and _select.check_count(None, 0.5, "x") == (-1, 0.5)
    for bad in (-0.1, 1.01, float("nan")):
        with pytest.raises(ValueError, match="ratio must be in"):
            _select.check_count(None, bad, "x")
    for bad in (-1, 2.5):
        with pytest.raises(ValueError, match="k must be an integer"):
            _select.check_count(bad, None, "x")
    with pytest.raises(ValueError, match="score must be"):
        spconv.SparsePrune(ratio=0.5, score="l2")


def test_cpu_tensors_raise():
    import spconv_amd.pytorch as spconv
    F = spconv.functional
    idx = torch.from_numpy(rs.sorted_scene(1, [4, 5, 6], 20, 0))
    x = spconv.SparseConvTensor(torch.zeros((idx.shape[0], 4)), idx, [4, 5, 6], 1)
    with pytest.raises(NotImplementedError, match="no CPU path"):
        F.row_score(x.features)
    with pytest.raises(NotImplementedError, match="no CPU path"):
        F.topk_mask(torch.zeros(20), k=3)
    with pytest.raises(NotImplementedError, match="no CPU path"):
        F.sparse_select(x, torch.ones(20, dtype=torch.bool))
    with pytest.raises(NotImplementedError, match="no CPU path"):
        F.sparse_prune(x, ratio=0.5)
    with pytest.raises(NotImplementedError, match="no CPU path"):
        spconv.SparsePrune(k=3)(x)


def test_install_as_spconv_exposes_the_module():
    import spconv_amd
    spconv_amd.install_as_spconv()
    import spconv.pytorch as sp
    from spconv.pytorch.spatial import SparsePrune
    assert sp.SparsePrune is SparsePrune is spconv_amd.pytorch.spatial.SparsePrune


# ---------------------------------------------------------------------------------------- the reference itself
def test_key_is_a_total_order_on_float32():
    vals = np.array([-np.inf, -3.0, -1e-40, -0.0, 0.0, 2.0 ** -149, 1e-40, 0.25, 3.0, np.inf], dtype=np.float32)
    k = rs.keys(vals).astype(np.int64)
    assert bool((np.diff(k) > 0).all())                             # -0.0 below +0.0 included
    nan = np.array([0x7fc00000, 0xffc00000], dtype=np.uint32).view(np.float32)
    kn = rs.keys(nan).astype(np.int64)
    assert kn[0] > k[-1] and kn[1] < k[0]                           # a positive NaN above +inf, a negative one below -inf
    rng = np.random.default_rng(0)
    x = rng.standard_normal(1000).astype(np.float32)
    np.testing.assert_array_equal(np.argsort(rs.keys(x), kind="stable"), np.argsort(x, kind="stable"))


@pytest.mark.parametrize("kind", rs.SCORE_KINDS)
@pytest.mark.parametrize("n", [0, 1, 257, 3000])
def test_topk_reference_against_a_stable_argsort(kind, n):
    s = rs.scores(kind, n, 5)
    rng = np.random.default_rng(6)
    idx = np.zeros((n, 4), dtype=np.int32)
    idx[:, 0] = rng.integers(-1, 3, n)                              # batch -1 and 2: dead under batch = 2
    n_live = n - n // 7
    ok = rs.live_rows(n, idx, 2, n_live)
    live = int(ok.sum())
    assert live == int(((idx[:n_live, 0] >= 0) & (idx[:n_live, 0] < 2)).sum())
    rows = np.nonzero(ok)[0]
    order = rows[np.argsort(-rs.keys(s)[rows].astype(np.int64), kind="stable")]      # by (-key, row)
    for k, ratio in ((0, None), (1, None), (live - 1, None), (live, None), (live + 5, None), (None, 0.0), (None, 0.3),
                     (None, 0.5), (None, 1.0)):
        if k is not None and k < 0:
            continue
        got = rs.topk(s, k, ratio, idx, 2, n_live)
        kk = min(k, live) if k is not None else int(live * ratio)
        want = np.zeros((n,), dtype=np.uint8)
        want[order[:kk]] = 1
        np.testing.assert_array_equal(got.keep, want)
        assert got.sel[:2] == [live, kk] and int(got.keep.sum()) == kk
        if kk:
            T = rs.keys(s)[order[kk - 1]]
            assert np.uint32(got.sel[2] & 0xffffffff) == T
            assert got.sel[3] == int((rs.keys(s)[order[:kk]] == T).sum())
        else:
            assert got.sel[2:] == [-1, 0]


def test_ratio_count_is_the_truncated_double_product():
    assert rs.count_k(10, ratio=0.3) == 3 == int(10 * 0.3) and rs.count_k(3000, ratio=0.5) == 1500
    assert rs.count_k(10, ratio=0.7) == 7 and rs.count_k(100, ratio=0.29) == int(100 * 0.29) == 28
    assert rs.count_k(7, ratio=1.0) == 7 and rs.count_k(7, ratio=0.0) == 0 and rs.count_k(0, ratio=1.0) == 0


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, torch.float32, torch.float64])
@pytest.mark.parametrize("C", [1, 3, 8, 64, 129, 260])
def test_score_reference_is_close_to_float64_and_clear_of_subnormals(dtype, C):
    """The reference in the documented order against an fp64 evaluation, inside the bound the GPU test uses; the inputs
    (uniform in [-1, 1] rounded to the dtype) give no fp32 subnormal score, so flush-to-zero modes cannot show."""
    g = torch.Generator().manual_seed(C)
    feat = (torch.rand((50, C), generator=g, dtype=torch.float64) * 2 - 1).to(dtype)
    got = rs.score(feat, "absmean").astype(np.float64)
    want = rs.score_f64(feat, "absmean")
    assert bool((np.abs(got - want) <= rs.score_bound(dtype, C, want)).all())
    assert bool((got >= 2.0 ** -126).all())
    np.testing.assert_array_equal(rs.score(feat, "absmax"), rs.score_f64(feat, "absmax").astype(np.float32))
    assert bool(np.isneginf(rs.score(feat, "absmean", 30)[30:]).all())


def test_score_order_is_lanes_then_butterfly():
    """C = 12 fp32: V = 4, P = 3, G = 4 -- lane sums of four elements each, then (l0 + l2) + (l1 + l3)."""
    assert rs.score_groups(12, 4) == (4, 3, 4) and rs.score_groups(260, 2) == (1, 260, 64)
    assert rs.score_groups(64, 2) == (8, 8, 8) and rs.score_groups(1, 8) == (1, 1, 1) and rs.score_groups(1024, 4) == (4, 256, 64)
    f = np.float32
    x = np.array([1.0, 2.0 ** -24, 2.0 ** -24, 2.0 ** -24, -3.0, 0.5, 0.25, 0.125, 2.0 ** -23, 1.0, 1.0, 1.0], dtype=f)
    lanes = []
    for s in range(3):
        a = f(0)
        for j in range(4):
            a = f(a + abs(x[4 * s + j]))
        lanes.append(a)
    want = f(f(f(lanes[0] + lanes[2]) + f(lanes[1] + f(0))) / f(12))
    assert rs.score(torch.from_numpy(x[None, :]))[0] == want
    assert lanes[0] == f(1.0)                                        # (1 + 2^-24 three times: every half rounds away)


@pytest.mark.parametrize("ndim", [1, 2, 3, 4])
def test_select_reference_against_a_plain_loop(ndim):
    import refcollapse as rc
    shape = [7, 6, 5, 9][:ndim]
    idx = rc.scene(2, shape, 150, 3 + ndim, 10)
    rng = np.random.default_rng(ndim)
    keep = (rng.random(idx.shape[0]) < 0.5).astype(np.uint8) * rng.integers(1, 255, idx.shape[0]).astype(np.uint8)
    for invert in (False, True):
        for n_live in (None, idx.shape[0] - 20):
            want_src = []
            for i, row in enumerate(idx.tolist()):
                if n_live is not None and i >= n_live:
                    continue
                if not 0 <= row[0] < 2 or any(not 0 <= row[1 + d] < shape[d] for d in range(ndim)):
                    continue
                if (keep[i] != 0) != invert:
                    want_src.append(i)
            ref = rs.select(idx, 2, shape, keep, invert, n_live)
            assert ref.src.tolist() == want_src and ref.found == ref.live == len(want_src)
            np.testing.assert_array_equal(ref.out_indices, idx[want_src])
            assert [int(ref.rows[i]) for i in want_src] == list(range(len(want_src))) and int((ref.rows >= 0).sum()) == ref.live
            cut = rs.select(idx, 2, shape, keep, invert, n_live, cap=ref.found - 3)
            assert (cut.found, cut.live) == (ref.found, ref.found - 3) and cut.src.tolist() == want_src[:-3]
            np.testing.assert_array_equal(cut.rows, np.where(ref.rows < cut.live, ref.rows, -1))
