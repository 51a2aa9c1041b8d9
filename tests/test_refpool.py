"""The pooling reference (refpool.py) against torch's dense pooling, on the CPU.

A sparse max pool equals the dense max pool of a tensor filled with -inf at the empty sites, and a sparse average pool
the quotient of two dense window sums (values / occupancy), both at the ACTIVE output sites; their gradients are the
autograd gradients of those expressions.  Values are distinct, so no window ties.  The rules dense torch does not share
(ties, NaN, a window of -inf, the pair-less row, init_zero, the backward quirk) are pinned by hand-written cases."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import refpool
from refconv import out_spatial_shape, pairs

GEOMETRIES = [
    # shape, voxels per scene, batch, ksize, stride, padding, dilation, subm
    ([40], 17, 2, [3], [2], [1], [1], False),
    ([40], 19, 1, [3], [1], [0], [2], False),
    ([12, 14], 60, 2, [3, 3], [2, 2], [1, 1], [1, 1], False),
    ([12, 14], 60, 1, [2, 3], [1, 2], [0, 1], [2, 1], False),
    ([8, 9, 10], 150, 2, [3, 3, 3], [2, 2, 2], [1, 1, 1], [1, 1, 1], False),
    ([8, 9, 10], 150, 2, [2, 2, 2], [2, 2, 2], [0, 0, 0], [1, 1, 1], False),
    ([8, 9, 10], 150, 1, [3, 3, 3], [1, 1, 1], [0, 0, 0], [1, 1, 1], False),
    ([9, 9, 9], 200, 2, [3, 2, 3], [2, 1, 2], [1, 0, 1], [2, 1, 2], False),
    ([8, 9, 10], 150, 2, [3, 3, 3], [1, 1, 1], [1, 1, 1], [1, 1, 1], True),
    ([8, 9, 10], 150, 1, [3, 3, 3], [1, 1, 1], [2, 2, 2], [2, 2, 2], True),
]
IDS = [f"{len(g[0])}d-k{'x'.join(map(str, g[3]))}-s{g[4][0]}-p{g[5][0]}-d{g[6][0]}{'-subm' if g[7] else ''}-b{g[2]}"
       for g in GEOMETRIES]


def _scene(shape, n, bs, seed):
    rng = np.random.default_rng(seed)
    rows = []
    for b in range(bs):
        lin = rng.choice(int(np.prod(shape)), size=n, replace=False)
        rows.append(np.concatenate([np.full((n, 1), b), np.stack(np.unravel_index(lin, shape), -1)], 1))
    return np.concatenate(rows).astype(np.int32)


def _problem(geom, C=3, seed=0):
    shape, n, bs, ks, st, pd, dl, subm = geom
    idx = _scene(shape, n, bs, seed)
    g = torch.Generator().manual_seed(seed)
    n_in = idx.shape[0]
    f = (torch.randperm(n_in * C, generator=g).to(torch.float64).reshape(n_in, C) - n_in * C / 2) / 7.0   # distinct
    out_idx, cand = pairs(idx, bs, shape, ks, st, pd, dl, subm)
    dout = torch.rand((out_idx.shape[0], C), generator=g, dtype=torch.float64) * 2 - 1
    if subm:        # the dense pool of a SubM window: stride 1, the window centred on the output site
        pd = [(k // 2) * d for k, d in zip(ks, dl)]
    return idx, f, dout, out_idx, cand, (shape, bs, ks, st, pd, dl, subm)


def _scatter(idx, values, shape, bs, fill):
    """[B, C, *shape] float64 holding `values` at the rows' sites and `fill` elsewhere"""
    idx = torch.as_tensor(np.asarray(idx), dtype=torch.int64)
    dense = torch.full((bs, *shape, values.shape[1]), fill, dtype=torch.float64)
    dense[tuple(idx[:, j] for j in range(idx.shape[1]))] = values
    return dense.movedim(-1, 1).contiguous()


def _gather(dense, idx):
    idx = torch.as_tensor(np.asarray(idx), dtype=torch.int64)
    return dense.movedim(1, -1)[tuple(idx[:, j] for j in range(idx.shape[1]))]


def _pad(x, pd, value):
    flat = []
    for p in reversed(pd):
        flat += [p, p]
    return F.pad(x, flat, value=value)


def _window_sum(x, ks, st, dl):
    """sum over every window of a padded dense tensor: avg_pool with divisor 1; torch's avg_pool has no dilation, so a
    dilated window is the depthwise convolution with a kernel of ones"""
    nd = len(ks)
    if all(d == 1 for d in dl):
        if nd == 1:                                  # (avg_pool1d has no divisor_override)
            return F.avg_pool1d(x, ks, st) * ks[0]
        return getattr(F, f"avg_pool{nd}d")(x, ks, st, divisor_override=1)
    C = x.shape[1]
    return getattr(F, f"conv{nd}d")(x, torch.ones((C, 1, *ks), dtype=x.dtype), stride=st, dilation=dl, groups=C)


@pytest.mark.parametrize("geom", GEOMETRIES, ids=IDS)
def test_max_equals_dense_max_pool(geom):
    idx, f, dout, out_idx, cand, (shape, bs, ks, st, pd, dl, subm) = _problem(geom, seed=1)
    n_out = out_idx.shape[0]
    out = refpool.max_fwd(cand, f, n_out, torch.float64)
    x = _scatter(idx, f, shape, bs, float("-inf")).requires_grad_(True)
    y = getattr(F, f"max_pool{len(shape)}d")(_pad(x, pd, float("-inf")), ks, st, 0, dl)
    assert list(y.shape[2:]) == out_spatial_shape(shape, ks, st, geom[5], dl, subm)
    if not subm:    # the outputs are exactly the sites whose window holds an input
        assert int(torch.isfinite(y[:, 0]).sum()) == n_out
    assert torch.equal(_gather(y, out_idx), out)
    g = _scatter(out_idx, dout, list(y.shape[2:]), bs, 0.0)
    (torch.where(torch.isfinite(y), y, torch.zeros_like(y)) * g).sum().backward()
    ref = refpool.max_bwd(cand, f, out, dout)
    # (an input that is the maximum of several windows sums their gradients: the two sum in different orders)
    torch.testing.assert_close(_gather(x.grad, idx), ref.value, rtol=1e-13, atol=1e-13)
    assert bool((ref.abs_sum >= ref.value.abs()).all())


@pytest.mark.parametrize("geom", GEOMETRIES, ids=IDS)
def test_avg_equals_quotient_of_dense_window_sums(geom):
    idx, f, dout, out_idx, cand, (shape, bs, ks, st, pd, dl, subm) = _problem(geom, seed=2)
    n_out, n_in = out_idx.shape[0], idx.shape[0]
    ref = refpool.avg_fwd(cand, f, n_out)
    x = _scatter(idx, f, shape, bs, 0.0).requires_grad_(True)
    occ = _scatter(idx, torch.ones((n_in, f.shape[1]), dtype=torch.float64), shape, bs, 0.0)
    num = _window_sum(_pad(x, pd, 0.0), ks, st, dl)
    den = _window_sum(_pad(occ, pd, 0.0), ks, st, dl)
    cnt = _gather(den, out_idx)[:, 0]
    assert torch.equal(cnt, ref.count.to(torch.float64)) and ref.count.dtype == torch.int32
    if not subm:
        assert int((den[:, 0] > 0).sum()) == n_out
    y = num / den.clamp(min=1)
    torch.testing.assert_close(_gather(y, out_idx), ref.value, rtol=1e-13, atol=1e-13)
    torch.testing.assert_close(refpool.avg_fwd(cand, f.abs(), n_out).value, ref.abs_sum, rtol=1e-13, atol=0)
    (y * _scatter(out_idx, dout, list(y.shape[2:]), bs, 0.0)).sum().backward()
    back = refpool.avg_bwd(cand, dout, ref.count, n_in)
    torch.testing.assert_close(_gather(x.grad, idx), back.value, rtol=1e-13, atol=1e-13)
    torch.testing.assert_close(refpool.avg_bwd(cand, dout.abs(), ref.count, n_in).value, back.abs_sum, rtol=1e-13, atol=0)


# ---------------------------------------------------------------- the rules dense torch does not share, by hand
def _t(rows):
    return torch.tensor(rows, dtype=torch.float64)


def _l(*v):
    return torch.tensor(v, dtype=torch.int64)


# two outputs over three inputs: output 0 <- inputs 0, 1 (offsets 0, 1); output 1 <- inputs 1, 2 (offsets 0, 1)
CAND = [(0, _l(0, 1), _l(0, 1)), (1, _l(1, 2), _l(0, 1))]


def test_ties_send_the_gradient_to_every_tied_input():
    f = _t([[1.0, 5.0], [1.0, 2.0], [0.5, 2.0]])
    out = refpool.max_fwd(CAND, f, 2, torch.float32)
    assert out.tolist() == [[1.0, 5.0], [1.0, 2.0]]
    dout = _t([[10.0, 20.0], [3.0, -4.0]])
    r = refpool.max_bwd(CAND, f, out, dout)
    # column 0: inputs 0 and 1 tie in output 0, input 1 is output 1's maximum too; column 1: inputs 1 and 2 tie in output 1
    assert r.value.tolist() == [[10.0, 20.0], [13.0, -4.0], [0.0, -4.0]]
    assert r.abs_sum.tolist() == [[10.0, 20.0], [13.0, 4.0], [0.0, 4.0]]


def test_nan_is_never_selected_and_receives_nothing():
    nan = float("nan")
    f = _t([[nan, 1.0], [2.0, nan], [nan, nan]])
    out = refpool.max_fwd(CAND, f, 2, torch.float16)
    assert out.tolist() == [[2.0, 1.0], [2.0, -65504.0]]        # a window of NaN alone keeps the lowest value
    r = refpool.max_bwd(CAND, f, out, _t([[1.0, 1.0], [1.0, 1.0]]))
    assert r.value.tolist() == [[0.0, 1.0], [2.0, 0.0], [0.0, 0.0]]


@pytest.mark.parametrize("dtype,low", [(torch.float16, -65504.0), (torch.bfloat16, -3.3895313892515355e38),
                                       (torch.float32, -3.4028234663852886e38), (torch.float64, -1.7976931348623157e308),
                                       (torch.int8, -128.0)])
def test_a_window_of_minus_infinity_keeps_the_lowest_finite_value(dtype, low):
    assert refpool.lowest(dtype) == low
    if dtype != torch.int8:
        assert float(torch.tensor(low, dtype=torch.float64).to(dtype).to(torch.float64)) == low
        assert low == torch.finfo(dtype).min
    if dtype == torch.bfloat16:
        assert int(torch.tensor(low, dtype=torch.float64).to(dtype).view(torch.int16)) & 0xffff == 0xff7f
    inf = float("inf")
    f = _t([[-inf], [-inf], [low]])
    out = refpool.max_fwd(CAND, f, 2, dtype)
    assert out.tolist() == [[low], [low]]
    # -inf is not the output: no gradient; the input AT the lowest value equals it and receives its output's
    r = refpool.max_bwd(CAND, f, out, _t([[1.0], [2.0]]))
    assert r.value.tolist() == [[0.0], [0.0], [2.0]]


def test_a_row_without_pairs_is_zero():
    cand = [(0, _l(0), _l(0)), (1, _l(), _l())]                  # output 1 of 2 has no pair; offset 1 has none at all
    f = _t([[-3.0, 4.0]])
    assert refpool.max_fwd(cand, f, 2, torch.float16).tolist() == [[-3.0, 4.0], [0.0, 0.0]]
    a = refpool.avg_fwd(cand, f, 2)
    assert a.value.tolist() == [[-3.0, 4.0], [0.0, 0.0]] and a.count.tolist() == [1, 0]
    assert a.abs_sum.tolist() == [[3.0, 4.0], [0.0, 0.0]]
    # the dead row's gradient reaches no input, under either rule
    dout = _t([[1.0, 1.0], [100.0, 100.0]])
    out = refpool.max_fwd(cand, f, 2, torch.float16)
    assert refpool.max_bwd(cand, f, out, dout).value.tolist() == [[1.0, 1.0]]
    assert refpool.avg_bwd(cand, dout, a.count, 1).value.tolist() == [[1.0, 1.0]]
    assert refpool.avg_bwd(cand, dout, a.count, 1, reference_quirks=True).value.tolist() == [[1.0, 1.0]]


def test_init_zero_is_the_maximum_with_zero():
    f = _t([[-1.0, 3.0], [-2.0, -5.0], [-0.5, -6.0]])
    assert refpool.max_fwd(CAND, f, 2, torch.float32, init_zero=True).tolist() == [[0.0, 3.0], [0.0, 0.0]]
    assert refpool.max_fwd(CAND, f, 2, torch.float32).tolist() == [[-1.0, 3.0], [-0.5, -5.0]]
    out = refpool.max_fwd(CAND, f, 2, torch.float32, init_zero=True)
    r = refpool.max_bwd(CAND, f, out, _t([[1.0, 1.0], [1.0, 1.0]]))
    assert r.value.tolist() == [[0.0, 1.0], [0.0, 0.0], [0.0, 0.0]]      # a clamped output has no arg-max input


def test_avg_backward_divides_and_the_quirk_multiplies():
    cand = CAND + [(2, _l(0), _l(1))]                            # output 1 has three pairs
    cnt = refpool.counts(cand, 2)
    assert cnt.tolist() == [2, 3] and cnt.dtype == torch.int32
    dout = _t([[6.0], [12.0]])
    assert refpool.avg_bwd(cand, dout, cnt, 3).value.tolist() == [[7.0], [7.0], [4.0]]
    q = refpool.avg_bwd(cand, dout, cnt, 3, reference_quirks=True)
    assert q.value.tolist() == [[48.0], [48.0], [36.0]] and q.abs_sum.tolist() == [[48.0], [48.0], [36.0]]


def test_global_pools_scene_by_scene():
    b = torch.tensor([0, 2, 0, -1, 5, 2])
    f = _t([[1.0, -4.0], [2.0, 2.0], [3.0, -8.0], [100.0, 100.0], [200.0, 200.0], [-6.0, 4.0]])
    mx = refpool.global_pool(b, f, 3, torch.float16, False)
    assert mx.value.tolist() == [[3.0, -4.0], [-65504.0, -65504.0], [2.0, 4.0]] and mx.abs_sum is None
    mean = refpool.global_pool(b, f, 3, torch.float16, True)
    assert mean.value[0].tolist() == [2.0, -6.0] and mean.value[2].tolist() == [-2.0, 3.0]
    assert bool(torch.isnan(mean.value[1]).all())
    assert mean.abs_sum.tolist() == [[2.0, 6.0], [0.0, 0.0], [4.0, 3.0]]
