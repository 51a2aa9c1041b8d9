"""Axis collapse (csrc/collapse.hip): what can be checked without a GPU -- the unit is linked, the size query's gates,
the launch-count keys, the argument checks that come before anything touches the device, and the numpy reference
(tests/refcollapse.py) against a brute-force grouping."""
import ctypes
import os

import numpy as np
import pytest
import torch

import refcollapse as rc
from spconv_amd import _lib

NAMES = ("spx_collapse_ws_bytes", "spx_collapse_count", "spx_collapse_fill", "spx_collapse_static", "spx_collapse_fwd",
         "spx_collapse_bwd")
KEYS = ("collapse/mark", "collapse/prefix", "collapse/rank", "collapse/list", "collapse/fwd", "collapse/bwd")


def mask_of(axes):
    return sum(1 << a for a in axes)


def test_collapse_unit_is_linked():
    units = {os.path.splitext(os.path.basename(o))[0] for o in _lib.linked_objects()}
    assert "collapse" in units
    L = _lib.load()
    for name in NAMES:
        assert getattr(L, name) is not None


@pytest.mark.parametrize("batch,shape,axes,fits", [
    (1, [41, 1600, 1408], (0,), True),                  # the flagship grid, height removed
    (2, [3, 160, 160], (1,), True), (1, [7], (), True), (1, [5, 6, 7, 9], (0, 3), True),
    (1, [0, 4, 4], (1,), False), (2, [4, 0], (0,), False), (1, [4, 4, 0], (2,), False),      # an empty grid, removed axis too
    (1, [4, 5, 6], (0, 1, 2), False), (1, [9], (0,), False),                                  # no axis kept
    (1, [4, 5, 6], (3,), False), (1, [4, 5], (2,), False),                                    # an axis >= ndim
    (1, [2, 65536, 32768], (0,), False),                # the projected space = 2^31 cells
    (1, [2, 65536, 32767], (0,), True),                 # just below
    (1, [2048, 1024, 1024], (), False),                 # nothing removed: the rank map's own gate
    (1, [2048, 1024, 1024], (0,), True),                # the same grid fits once the long axis is gone
])
def test_ws_bytes_gates(batch, shape, axes, fits):
    L = _lib.load()
    got = L.spx_collapse_ws_bytes(len(shape), batch, _lib.ints(shape), mask_of(axes), 1000)
    assert (got > 0) == fits
    kept = [s for d, s in enumerate(shape) if d not in axes]
    if fits:        # the same rule as the rank map's, on the projected grid
        assert L.spx_rankmap_bytes(len(kept), batch, _lib.ints(kept)) > 0


def test_ws_bytes_grows_with_rows_and_refuses_bad_counts():
    L = _lib.load()
    sp = _lib.ints([12, 14, 16])
    assert L.spx_collapse_ws_bytes(3, 2, sp, 1, 100000) > L.spx_collapse_ws_bytes(3, 2, sp, 1, 100)
    assert L.spx_collapse_ws_bytes(3, 2, sp, 1, -1) == 0
    assert L.spx_collapse_ws_bytes(3, 2, sp, -1, 100) == 0
    assert L.spx_collapse_ws_bytes(5, 2, _lib.ints([2] * 5), 1, 100) == 0
    assert L.spx_collapse_ws_bytes(3, 0, sp, 1, 100) == 0


def test_launch_count_keys():
    L = _lib.load()
    for key in KEYS:
        assert L.spx_launch_count(key.encode()) >= 0, key
    for key in ("collapse", "collapse/", "collapse/sort", "collapse/fwd/", "collapse/mark/f16"):
        assert L.spx_launch_count(key.encode()) == -1, key


def test_bad_arguments_are_refused_before_any_pointer_is_read():
    """Every call below passes NULL for every pointer: no device is needed to be told no."""
    L = _lib.load()
    sp = _lib.ints([4, 5, 6])
    result = (ctypes.c_int * 2)()
    builds = {
        "count": lambda m: L.spx_collapse_count(None, 4, None, 3, 1, sp, m, None, 0, None, 0, result, None),
        "fill": lambda m: L.spx_collapse_fill(None, 4, None, 3, 1, sp, m, 2, None, None, None, None, None, 0, None, 0, None),
        "static": lambda m: L.spx_collapse_static(None, 4, None, 3, 1, sp, m, 4, None, None, None, None, None, None, 0,
                                                  None, 0, None),
    }
    for name, call in builds.items():
        assert call(8) != 0, name
        assert "names an axis >= ndim" in L.spx_last_error().decode(), name
        assert call(7) != 0, name
        assert "at least one stays" in L.spx_last_error().decode(), name
        with pytest.raises(RuntimeError, match="at least one stays"):
            _lib.check(-1)
    F16 = _lib.DTYPE_F16
    fwd = lambda C, dt, op: L.spx_collapse_fwd(None, 4, None, None, 4, C, dt, op, None, None, None)
    bwd = lambda C, dt, op: L.spx_collapse_bwd(None, None, None, None, None, 4, 4, C, dt, op, None, None)
    for name, call in (("fwd", fwd), ("bwd", bwd)):
        assert call(4, _lib.DTYPE_I8, _lib.COLLAPSE_MEAN) != 0, name
        assert "dtype" in L.spx_last_error().decode(), name
        assert call(0, F16, _lib.COLLAPSE_MEAN) != 0, name
        assert "channel count" in L.spx_last_error().decode(), name
        assert call(4, F16, 3) != 0 and call(4, F16, -1) != 0, name
        assert "op must be sum" in L.spx_last_error().decode(), name
    assert bwd(4, F16, _lib.COLLAPSE_SUM) != 0
    assert "spx_union_add_bwd" in L.spx_last_error().decode()


def test_python_refusals():
    import spconv_amd.pytorch as spconv
    from spconv_amd.pytorch import _collapse
    with pytest.raises(ValueError, match="not distinct"):
        _collapse.check_axes((0, 0), 3)
    with pytest.raises(ValueError, match="outside"):
        _collapse.check_axes((3,), 3)
    with pytest.raises(ValueError, match="at least one stays"):
        _collapse.check_axes((0, 1, 2), 3)
    assert _collapse.check_axes((2, 0), 3) == (0, 2) and _collapse.check_axes((), 1) == ()
    with pytest.raises(ValueError, match="reduce"):
        spconv.SparseCollapse((0,), reduce="min")
    with pytest.raises(ValueError, match="distinct"):
        spconv.SparseCollapse((1, 1))


def test_module_on_a_cpu_tensor_raises():
    import spconv_amd.pytorch as spconv
    idx = torch.from_numpy(rc.scene(1, [4, 5, 6], 20, 0, dead=False))
    x = spconv.SparseConvTensor(torch.zeros((idx.shape[0], 4)), idx, [4, 5, 6], 1)
    with pytest.raises(NotImplementedError, match="no CPU path"):
        spconv.SparseCollapse((0,))(x)
    with pytest.raises(NotImplementedError, match="no CPU path"):
        spconv.functional.sparse_collapse(x, (0,), "max")


def test_install_as_spconv_exposes_the_module():
    import spconv_amd
    spconv_amd.install_as_spconv()
    import spconv.pytorch as sp
    from spconv.pytorch.spatial import SparseCollapse
    assert sp.SparseCollapse is SparseCollapse is spconv_amd.pytorch.spatial.SparseCollapse


# ---------------------------------------------------------------------------------------- the reference itself
def brute(idx, bs, shape, axes, n_live=None):
    """{(batch, kept coords): [rows]} over the live rows, by a plain loop"""
    groups = {}
    for i, row in enumerate(np.asarray(idx).tolist()):
        if n_live is not None and i >= n_live:
            continue
        if not 0 <= row[0] < bs or any(not 0 <= row[1 + d] < shape[d] for d in range(len(shape))):
            continue
        groups.setdefault((row[0],) + tuple(row[1 + d] for d in range(len(shape)) if d not in axes), []).append(i)
    return groups


@pytest.mark.parametrize("bs,shape,axes,n,dups", [
    (2, [5, 6, 7], (0,), 150, 10), (2, [5, 6, 7], (1,), 150, 10), (2, [5, 6, 7], (0, 2), 150, 0), (1, [5, 6, 7], (), 90, 30),
    (3, [40], (), 60, 10), (2, [9, 8], (1,), 80, 5), (1, [3, 4, 5, 6], (0, 3), 200, 20), (2, [4, 4], (0,), 0, 0),
])
def test_reference_against_a_dictionary_grouping(bs, shape, axes, n, dups):
    idx = rc.scene(bs, shape, n, 7, dups)
    for n_live in (None, idx.shape[0] // 2):
        groups = brute(idx, bs, shape, axes, n_live)
        ref = rc.build(idx, bs, shape, axes, n_live)
        order = sorted(groups)                          # tuples sort as the linear key does
        assert ref.found == ref.live == len(order) and ref.live_rows == sum(len(v) for v in groups.values())
        assert ref.out_indices.tolist() == [list(k) for k in order]
        want_rows = np.full(idx.shape[0], -1)
        for r, k in enumerate(order):
            want_rows[groups[k]] = r
            assert ref.list[ref.offsets[r]:ref.offsets[r + 1]].tolist() == groups[k]      # ascending input row
        np.testing.assert_array_equal(ref.rows, want_rows)
        # a cap keeps the first keys
        if len(order) > 2:
            cut = rc.build(idx, bs, shape, axes, n_live, cap=len(order) - 2)
            assert (cut.found, cut.live) == (len(order), len(order) - 2)
            np.testing.assert_array_equal(cut.rows, np.where(want_rows < cut.live, want_rows, -1))
            np.testing.assert_array_equal(cut.offsets, ref.offsets[:cut.live + 1])
            np.testing.assert_array_equal(cut.list, ref.list[:cut.offsets[-1]])


def test_reference_agrees_with_the_torch_composite():
    """unique of the projected keys + index_add_ in float64: the same coordinates in the same order, the same sums."""
    bs, shape, axes = 2, [5, 6, 7], (0,)
    idx = rc.scene(bs, shape, 200, 3, 20, dead=False)
    feat = rc.features(idx.shape[0], 5, torch.float32, 4)
    ref = rc.build(idx, bs, shape, axes)
    keys = torch.from_numpy(rc.projected_keys(idx, bs, shape, axes))
    uniq, inverse = torch.unique(keys, sorted=True, return_inverse=True)
    np.testing.assert_array_equal(ref.out_indices, rc.decode(uniq.numpy(), ref.kept_shape))
    np.testing.assert_array_equal(ref.rows, inverse.numpy())
    want = torch.zeros((uniq.shape[0], 5), dtype=torch.float64).index_add_(0, inverse, feat.double())
    lens = np.diff(ref.offsets)[:, None]
    got = rc.reduce(feat, ref, "sum").double()
    assert float((got - want).abs().max()) <= 2.0 ** -24 * float(lens.max() + 1) * float(want.abs().max() + lens.max())
    mean, A, _ = rc.mean_f64(feat, ref)
    np.testing.assert_allclose(mean, want.numpy() / lens, rtol=1e-14, atol=1e-300)
    assert bool((A >= np.abs(mean) - 1e-15).all())
    mx = torch.full((uniq.shape[0], 5), -2.0, dtype=torch.float32).scatter_reduce_(0, inverse[:, None].expand(-1, 5), feat,
                                                                                  "amax")
    assert torch.equal(rc.reduce(feat, ref, "max"), mx)


def test_reference_sum_is_the_sequential_loop_and_keeps_single_rows():
    bs, shape, axes = 1, [4, 2, 2], (0,)
    idx = np.array([[0, 0, 0, 0], [0, 1, 0, 0], [0, 2, 0, 0], [0, 3, 1, 1], [0, 0, 0, 1]], np.int32)
    feat = torch.tensor([[1.0], [2.0 ** -24], [2.0 ** -24], [-0.0], [0.5]], dtype=torch.float32)
    ref = rc.build(idx, bs, shape, axes)
    assert ref.offsets.tolist() == [0, 3, 4, 5] and ref.list.tolist() == [0, 1, 2, 4, 3]
    out = rc.reduce(feat, ref, "sum")
    assert float(out[0, 0]) == 1.0                      # (1 + 2^-24) + 2^-24 in row order: both halves round away
    assert float(out[1, 0]) == 0.5 and bool(torch.signbit(out[2, 0]))      # -0.0 as it came
    assert float(rc.reduce(feat, ref, "max")[0, 0]) == 1.0
    din = rc.backward(feat, rc.reduce(feat, ref, "mean"), torch.ones((3, 1)), ref, "mean")
    np.testing.assert_array_equal(din[:, 0], [1 / 3, 1 / 3, 1 / 3, 1.0, 1.0])


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, torch.float32, torch.float64])
def test_forward_inputs_stay_clear_of_fp32_subnormals_and_overflow(dtype):
    """The GPU forward test's inputs (uniform in [-1, 1], rounded to the dtype): no input, sum or mean is an fp32
    subnormal or overflows, so flush-to-zero modes cannot show; the scene holds a one-row group and groups of several."""
    s = rc.FWD_SCENE
    idx = rc.fwd_scene()
    ref = rc.build(idx, s["bs"], s["shape"], s["axes"])
    lens = np.diff(ref.offsets)
    assert int(lens.min()) == 1 and int(lens.max()) >= 5 and ref.live_rows < idx.shape[0]
    tiny, huge = 2.0 ** -126, float(np.finfo(np.float32).max)
    for C in (1, 8, 20, 64, 136, 264):
        feat = rc.features(idx.shape[0], C, dtype, 100 + C)
        for t in (feat, rc.reduce(feat, ref, "sum"), rc.reduce(feat, ref, "mean")):
            a = t.double().abs()
            assert bool(((a == 0) | (a >= tiny)).all()) and bool((a < huge).all())
