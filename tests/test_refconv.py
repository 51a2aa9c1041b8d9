"""The fp64 reference of tests/refconv.py, on the CPU: against dense torch convolutions in float64 on tiny dense grids,
and against the oracle's rulebook driver on the small scenes the suite uses.  Every comparison is to fp64 precision."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import oracle
from refconv import ref_conv
from util import dense_scene, match_rows, scene

F64_C = 1e-12      # |a - b| <= F64_C x (the same sum over magnitudes): a few hundred fp64 roundings at most


def _close(a, b, A, name):
    a, b, A = (np.asarray(t, dtype=np.float64) for t in (a, b, A))
    assert a.shape == b.shape == A.shape, (name, a.shape, b.shape, A.shape)
    bad = np.abs(a - b) > F64_C * A + 1e-300
    assert not bad.any(), f"{name}: {int(bad.sum())} of {a.size} elements differ; max {np.abs(a - b).max():.3g}"


def _grid_scene(shape, bs, frac, seed):
    """A random fraction of every cell of a tiny grid (dense neighbourhoods, holes and borders)."""
    rng = np.random.default_rng(seed)
    cells = np.stack(np.meshgrid(*[np.arange(s) for s in shape], indexing="ij"), -1).reshape(-1, len(shape))
    rows = []
    for b in range(bs):
        keep = cells[rng.random(cells.shape[0]) < frac]
        rows.append(np.concatenate([np.full((keep.shape[0], 1), b), keep], 1))
    idx = np.concatenate(rows).astype(np.int32)
    return idx[rng.permutation(idx.shape[0])]


def _dense(idx, feats, bs, shape):
    C = feats.shape[1]
    x = torch.zeros((bs, C, *shape), dtype=torch.float64)
    x[(torch.from_numpy(idx[:, 0]).long(), slice(None)) + tuple(torch.from_numpy(idx[:, 1 + j]).long()
                                                                 for j in range(len(shape)))] = feats
    return x


def _at(t, coords):
    """rows of a dense [bs, C, *shape] tensor at coordinates [n, 1 + ndim] -> [n, C]"""
    c = torch.as_tensor(np.asarray(coords)).long()
    return t[(c[:, 0], slice(None)) + tuple(c[:, 1 + j] for j in range(c.shape[1] - 1))]


DENSE_CASES = [
    # shape, ksize, stride, padding, dilation, subm, transposed
    ([6, 5, 7], [3, 3, 3], [1, 1, 1], [1, 1, 1], [1, 1, 1], True, False),       # SubM
    ([7, 7, 6], [3, 3, 3], [1, 1, 1], [2, 2, 2], [2, 2, 2], True, False),       # SubM, dilated
    ([5, 6, 7], [3, 1, 5], [1, 1, 1], [1, 0, 2], [1, 1, 1], True, False),       # SubM, asymmetric
    ([7, 6, 8], [3, 3, 3], [2, 2, 2], [1, 1, 1], [1, 1, 1], False, False),      # strided
    ([8, 7, 6], [2, 2, 2], [2, 2, 2], [0, 0, 0], [1, 1, 1], False, False),      # even kernel
    ([7, 8, 9], [2, 3, 4], [2, 1, 3], [1, 0, 2], [1, 2, 1], False, False),      # even + asymmetric + dilated
    ([9, 7, 8], [3, 3, 3], [1, 2, 1], [0, 1, 2], [2, 1, 1], False, False),      # padding > 0, dilation 2
    ([4, 5, 3], [3, 3, 3], [2, 2, 2], [1, 1, 1], [1, 1, 1], False, True),       # transposed
    ([3, 4, 5], [2, 3, 2], [2, 1, 2], [0, 1, 0], [1, 1, 1], False, True),       # transposed, even / asymmetric
    ([11, 9], [3, 3], [1, 1], [1, 1], [1, 1], True, False),                     # 2-d SubM
    ([12, 10], [3, 2], [2, 2], [1, 0], [1, 1], False, False),                   # 2-d strided
    ([5, 4], [3, 3], [2, 2], [1, 1], [1, 1], False, True),                      # 2-d transposed
    ([30], [5], [1], [2], [1], True, False),                                    # 1-d SubM
    ([31], [3], [2], [1], [1], False, False),                                   # 1-d strided
]


@pytest.mark.parametrize("shape,ksize,stride,pad,dil,subm,transposed", DENSE_CASES)
def test_ref_against_dense_conv_f64(shape, ksize, stride, pad, dil, subm, transposed):
    nd = len(shape)
    bs, C, K = 2, 3, 4
    idx = _grid_scene(shape, bs, 0.45, seed=sum(shape))
    rng = np.random.default_rng(1)
    f = torch.from_numpy(rng.standard_normal((idx.shape[0], C)))
    w = torch.from_numpy(rng.standard_normal((K, *ksize, C)))
    # torch weight [K, C, *ksize] (conv) / [C, K, *ksize] (conv_transpose) from KRSC
    wd = w.permute(0, nd + 1, *range(1, nd + 1)).contiguous()
    conv = {1: F.conv1d, 2: F.conv2d, 3: F.conv3d}[nd]
    convt = {1: F.conv_transpose1d, 2: F.conv_transpose2d, 3: F.conv_transpose3d}[nd]
    x = _dense(idx, f, bs, shape).requires_grad_(True)
    wdg = wd.clone().requires_grad_(True)
    if subm:
        y = conv(x, wdg, None, 1, [(k // 2) * d for k, d in zip(ksize, dil)], dil)
    elif transposed:
        y = convt(x, wdg.transpose(0, 1), None, stride, pad, 0, 1, dil)
    else:
        y = conv(x, wdg, None, stride, pad, dil)
    # the sparse outputs: SubM -- the inputs; otherwise every site the dense result can be non-zero at
    dout_full = torch.from_numpy(rng.standard_normal(tuple(y.shape)))
    if subm:
        ref = ref_conv(idx, bs, shape, f, w, None, ksize, stride, pad, dil, subm, transposed)
        sites = idx
    else:
        ref = ref_conv(idx, bs, shape, f, w, None, ksize, stride, pad, dil, subm, transposed)
        sites = ref.out_indices.numpy()
        # the reference's output set is exactly the support of the dense result on ones
        ones = _dense(idx, torch.ones((idx.shape[0], 1), dtype=torch.float64), bs, shape)
        w1 = torch.ones((1, 1, *ksize), dtype=torch.float64)
        sup = (convt(ones, w1, None, stride, pad, 0, 1, dil) if transposed else conv(ones, w1, None, stride, pad, dil))
        assert tuple(sup.shape[2:]) == tuple(y.shape[2:])
        nz = torch.nonzero(sup[:, 0] > 0.5).numpy()
        assert np.array_equal(nz, sites), "output coordinate set / key order"
    dout = _at(dout_full, sites)
    ref = ref_conv(idx, bs, shape, f, w, dout, ksize, stride, pad, dil, subm, transposed)
    assert np.array_equal(ref.out_indices.numpy(), np.asarray(sites, dtype=np.int64))
    mask = torch.zeros_like(y)
    c = torch.as_tensor(np.asarray(sites)).long()
    mask[(c[:, 0], slice(None)) + tuple(c[:, 1 + j] for j in range(nd))] = 1
    (y * mask * dout_full.masked_fill(mask == 0, 0)).sum().backward()
    _close(ref.out, _at(y.detach(), sites), ref.out_abs, "out")
    _close(ref.din, _at(x.grad, idx), ref.din_abs, "din")
    dw_dense = wdg.grad.permute(0, *range(2, nd + 2), 1)           # back to KRSC
    _close(ref.dW, dw_dense, ref.dW_abs, "dW")


ORACLE_CASES = [
    # shape, n, bs, ksize, stride, pad, dil, subm, transposed, dense
    ([24, 24, 24], 1500, 2, [3] * 3, [1] * 3, [1] * 3, [1] * 3, True, False, True),
    ([24, 24, 24], 1500, 2, [3] * 3, [2] * 3, [1] * 3, [1] * 3, False, False, True),
    ([24, 24, 24], 1200, 1, [3] * 3, [1] * 3, [2] * 3, [2] * 3, True, False, True),
    ([20, 20, 20], 1200, 1, [5, 3, 3], [1] * 3, [2, 1, 1], [1] * 3, True, False, False),
    ([20, 20, 20], 1000, 1, [2] * 3, [2] * 3, [0] * 3, [1] * 3, False, False, True),
    ([20, 20, 20], 900, 1, [3, 5, 3], [2, 1, 2], [1, 2, 1], [1] * 3, False, False, True),
    ([10, 10, 10], 300, 1, [3] * 3, [2] * 3, [1] * 3, [1] * 3, False, True, True),
    ([12, 10, 9, 8], 900, 2, [3] * 4, [1] * 4, [1] * 4, [1] * 4, True, False, True),      # 4-d SubM
    ([12, 10, 9, 8], 900, 1, [3, 3, 3, 2], [2, 2, 1, 2], [1, 1, 1, 0], [1] * 4, False, False, True),   # 4-d strided
    ([40, 40], 500, 2, [3, 3], [2, 2], [1, 1], [1, 1], False, False, False),              # 2-d
    ([30, 30, 30], 400, 1, [7, 7, 7], [1] * 3, [3] * 3, [1] * 3, True, False, True),      # kv 343
]


@pytest.mark.parametrize("shape,n,bs,ksize,stride,pad,dil,subm,transposed,dense", ORACLE_CASES)
def test_ref_against_oracle(shape, n, bs, ksize, stride, pad, dil, subm, transposed, dense):
    idx = dense_scene(shape, n, bs, 3) if dense else scene(shape, n, bs, 3)
    rng = np.random.default_rng(2)
    C, K = 5, 6
    out_inds, pair, num, _ = oracle.get_indice_pairs(idx, bs, shape, ksize, stride, pad, dil, None, subm, transposed)
    f = torch.from_numpy(rng.standard_normal((idx.shape[0], C)))
    w = torch.from_numpy(rng.standard_normal((K, *ksize, C)))
    g = torch.from_numpy(rng.standard_normal((out_inds.shape[0], K)))
    o_out = oracle.indice_conv(f, w, pair, num, out_inds.shape[0], subm=subm)
    o_din, o_dw = oracle.indice_conv_backward(f, w, g, pair, num, subm=subm)
    ref0 = ref_conv(idx, bs, shape, f, w, None, ksize, stride, pad, dil, subm, transposed)
    perm = match_rows(ref0.out_indices.numpy(), out_inds, shape if subm else ref0_shape(shape, ksize, stride, pad, dil,
                                                                                        transposed))
    ref = ref_conv(idx, bs, shape, f, w, g[perm], ksize, stride, pad, dil, subm, transposed)
    _close(ref.out, o_out[perm], ref.out_abs, "out")
    _close(ref.din, o_din, ref.din_abs, "din")
    _close(ref.dW, o_dw, ref.dW_abs, "dW")


def ref0_shape(shape, ksize, stride, pad, dil, transposed):
    from refconv import out_spatial_shape
    return out_spatial_shape(shape, ksize, stride, pad, dil, False, transposed)


def test_ref_empty_scene_and_dead_rows():
    shape, ks = [8, 8, 8], [3, 3, 3]
    f = torch.zeros((0, 4), dtype=torch.float64)
    w = torch.ones((2, *ks, 4), dtype=torch.float64)
    for subm in (True, False):
        r = ref_conv(np.zeros((0, 4), np.int32), 1, shape, f, w, torch.zeros((0, 2)), ks, [1] * 3, [1] * 3, [1] * 3,
                     subm)
        assert r.out.shape == (0, 2) and r.din.shape == (0, 4) and float(r.dW.abs().sum()) == 0.0
    # a row of a batch outside [0, batch) pairs with nothing; its output row (SubM) is zero
    idx = np.array([[0, 1, 1, 1], [0, 1, 1, 2], [5, 1, 1, 3]], np.int32)
    f = torch.ones((3, 4), dtype=torch.float64)
    r = ref_conv(idx, 1, shape, f, w, None, ks, [1] * 3, [1] * 3, [1] * 3, True)
    assert float(r.out[2].abs().sum()) == 0.0 and float(r.out[0, 0]) == 8.0


# ---------------------------------------------------------------- non-finite operands
# The isolation tests (test_gpu_gemm_isolation.py) compare the kernels' NaN / +Inf / -Inf placement with the reference's.
# Here the reference's placement is held to tests/nonfinite.py, which derives it from the pair lists by set arithmetic
# alone (which non-finite operand reaches which element, with which sign): no floating sum is formed there.
NONFINITE_CASES = [
    # shape, n, bs, ksize, stride, pad, dil, subm
    ([10, 10, 10], 400, 2, [3] * 3, [1] * 3, [1] * 3, [1] * 3, True),
    ([12, 12, 12], 500, 1, [3] * 3, [2] * 3, [1] * 3, [1] * 3, False),
    ([12, 12, 12], 500, 1, [2] * 3, [2] * 3, [0] * 3, [1] * 3, False),
    ([9, 9, 9], 250, 1, [5, 3, 3], [1] * 3, [2, 1, 1], [1] * 3, True),
]


def _same_classes(t, cls, name):
    from nonfinite import masks_of
    for kind, got, want in zip(("NaN", "+Inf", "-Inf"), masks_of(t), (cls.nan, cls.pinf, cls.ninf)):
        assert torch.equal(got, want), f"{name}: {kind} at {int(got.sum())} elements, set arithmetic gives {int(want.sum())}"
    assert bool(cls.nan.any()) and bool(cls.pinf.any()) and bool(cls.ninf.any()), f"{name}: a class does not occur"


@pytest.mark.parametrize("shape,n,bs,ksize,stride,pad,dil,subm", NONFINITE_CASES)
def test_ref_places_non_finite_values_as_set_arithmetic_does(shape, n, bs, ksize, stride, pad, dil, subm):
    from nonfinite import classify_dw, classify_rows, poison_rows, poisoned
    from refconv import conv_from_pairs, pairs
    idx = scene(shape, n, bs, 5)
    rng = np.random.default_rng(3)
    C, K = 5, 6
    out_idx, cand = pairs(idx, bs, shape, ksize, stride, pad, dil, subm)
    n_in, n_out = idx.shape[0], out_idx.shape[0]
    f = torch.from_numpy(rng.uniform(-1, 1, (n_in, C)))
    w = torch.from_numpy(rng.uniform(0.1, 1, (K, *ksize, C)) * rng.choice([-1.0, 1.0], (K, *ksize, C)))    # nonzero
    g = torch.from_numpy(rng.uniform(-1, 1, (n_out, K)))
    f[3, 1] = 0.0                                       # (an exact zero next to an Inf partner in dW: Inf x 0 = NaN)
    f = poisoned(f, poison_rows(cand, n_in, C, 1))
    g = poisoned(g, poison_rows(cand, n_out, K, 2, swap=True))
    ref = conv_from_pairs(out_idx, cand, f, w, g)
    w3 = w.reshape(K, -1, C)
    out_cls = classify_rows(cand, f, w3, n_out)
    _same_classes(ref.out, out_cls, "out")
    assert bool(out_cls.mixed.any()), "no output receives +Inf and -Inf together"
    _same_classes(ref.din, classify_rows([(k, o, i) for k, i, o in cand], g, w3, n_in, transposed=True), "din")
    _same_classes(ref.dW.reshape(K, -1, C), classify_dw(cand, f, g, (K, w3.shape[1], C)), "dW")
    # the magnitude sums are non-finite exactly where the values are (finite elements keep a finite bound)
    assert torch.equal(torch.isfinite(ref.out), torch.isfinite(ref.out_abs))
    assert torch.equal(torch.isfinite(ref.din), torch.isfinite(ref.din_abs))
    assert torch.equal(torch.isfinite(ref.dW), torch.isfinite(ref.dW_abs))


def _isolation_cases():
    import test_gpu_gemm_isolation as iso
    return iso.CASES + iso.ACT_CASES


def _iso_id(c):
    import test_gpu_gemm_isolation as iso
    return iso._id(c)


@pytest.mark.parametrize("c", _isolation_cases(), ids=[_iso_id(c) for c in _isolation_cases()])
def test_isolation_inputs_meet_their_conditions(c):
    """A condition on the INPUTS of test_gpu_gemm_isolation.py's named-rows group, not a measurement: with the rows that
    group poisons, between 1 % and 50 % of the rows of every row output are non-finite in the reference, and at least one
    element receives +Inf and -Inf together (NaN out of infinities alone)."""
    import test_gpu_gemm_isolation as iso
    import test_gpu_kernel_matrix as M
    from nonfinite import classify_rows
    from refconv import conv_from_pairs, pairs
    idx, shape, bs = M.scene_indices(c["scene"])
    ks, st, pd, dl, subm = M.GEOMS[c["geom"]]
    out_idx, cand = pairs(idx, bs, shape, ks, st, pd, dl, subm)      # (on the CPU, past the matrix's device-side cache)
    n_in, n_out = idx.shape[0], out_idx.shape[0]
    f, w, d, _ = M._operands(c, n_in, n_out, ks, "cpu")
    assert bool((w != 0).all()), "a zero weight"
    f, d = iso.named_inputs(c, cand, f, d)
    ref = conv_from_pairs(out_idx, cand, f, w, d)
    w3 = w.reshape(c["K"], -1, c["C"])
    checks = []
    if c["entry"] != "dgrad":
        checks.append(("out", ref.out, lambda: classify_rows(cand, f, w3, n_out)))
    if d is not None and c["entry"] != "wgrad":
        checks.append(("din", ref.din, lambda: classify_rows([(k, o, i) for k, i, o in cand], d, w3, n_in, transposed=True)))
    for name, t, classes in checks:
        frac = float((~torch.isfinite(t)).any(1).double().mean())
        assert 0.01 <= frac <= 0.5, f"{name}: {frac:.3%} of the rows are non-finite"
        assert bool(classes().mixed.any()), f"{name}: no element receives +Inf and -Inf together"
    if d is not None:
        bad = ~torch.isfinite(ref.dW)
        assert bool(bad.any()) and not bool(bad.all())
