"""float64 sparse convolution and pooling (csrc/igemm_f64.hip, the f64 cases of csrc/pool.hip).

Every entry is compared element by element with the float64 reference of refconv.py under
    |got - ref| <= 2^-53 |ref| + 1e-12 A        (A: the same sums over |operands|),
a bound an fp32 accumulator misses by five orders of magnitude (it errs at ~1e-7 A).  The instance counters show that
the float64 kernels ran and that none of the 16-bit / fp32 kernels did.  gradcheck, a LiDAR window against dense
torch conv3d, determinism and the pooling layers cover the module level."""
import zlib

import numpy as np
import pytest
import torch

from refconv import conv_from_pairs, out_spatial_shape, pairs
from util import gpu_rulebook, match_rows, scene

pytestmark = pytest.mark.gpu

F64 = torch.float64
U64 = 2.0 ** -53          # half an ulp of float64: the one rounding of the result
C_ABS = 1e-12             # float64 accumulation over <= 216 * 300 terms errs far below 1e-12 A
DEV = "cuda:0"
F64_KEYS = ("igemm_f64/fwd", "igemm_f64/dgrad", "wgrad_f64")
OTHER_KEYS = ("generic", "igemm_v4", "igemm_bwd", "igemm_ws", "igemm_bwd_rows")
ALPHA = float(np.float32(0.1))   # the leaky slope travels through the C ABI as a float (spx_igemm_fwd act_alpha)


def assert_f64_close(got, ref, A, name):
    assert got.dtype == F64, (name, got.dtype)
    assert tuple(got.shape) == tuple(ref.shape), (name, tuple(got.shape), tuple(ref.shape))
    a, r, A = got.detach().cpu().numpy(), ref.detach().cpu().numpy(), A.detach().cpu().numpy()
    if r.size == 0:
        return
    bound = U64 * np.abs(r) + C_ABS * A
    bad = np.abs(a - r) > bound
    if bad.any():
        i = np.unravel_index(np.argmax((np.abs(a - r) - bound) * bad), a.shape)
        raise AssertionError(f"{name}: {int(bad.sum())} of {a.size} elements outside 2^-53 |ref| + 1e-12 A; worst at "
                             f"{i}: got {a[i]!r}, want {r[i]!r}, A {A[i]:.6g}")


def _act(x, act):
    return {"none": x, "relu": torch.relu(x), "leaky": torch.where(x > 0, x, x * ALPHA),
            "sigmoid": torch.sigmoid(x)}[act]


GEOMS = {
    # ksize, stride, padding, dilation, subm, transposed
    "subm3": ([3, 3, 3], [1] * 3, [1] * 3, [1] * 3, True, False),
    "s2": ([3, 3, 3], [2] * 3, [1] * 3, [1] * 3, False, False),
    "k2s2": ([2, 2, 2], [2] * 3, [0] * 3, [1] * 3, False, False),
    "tr3s2": ([3, 3, 3], [2] * 3, [1] * 3, [1] * 3, False, True),
    "k45": ([5, 3, 3], [1] * 3, [2, 1, 1], [1] * 3, True, False),
    "k125": ([5, 5, 5], [1] * 3, [2] * 3, [1] * 3, True, False),
    "k216": ([6, 6, 6], [2] * 3, [2] * 3, [1] * 3, False, False),
}

CASES = [
    # name, geom, (shape, voxels, batch), C, K, table form, inverse, activation
    ("subm3", "subm3", ([16, 16, 16], 1200, 2), 16, 16, "row", False, None),
    ("s2", "s2", ([16, 16, 16], 1200, 2), 16, 32, "row", False, None),
    ("k2s2", "k2s2", ([16, 16, 16], 1200, 1), 8, 8, "row", False, None),
    ("transposed", "tr3s2", ([8, 8, 8], 300, 1), 8, 16, "row", False, None),
    ("inverse", "s2", ([16, 16, 16], 1200, 1), 16, 8, "row", True, None),
    ("kv45", "k45", ([12, 12, 12], 700, 1), 8, 8, "row", False, None),
    ("kv125", "k125", ([12, 12, 12], 700, 1), 8, 8, "row", False, None),
    ("kv216", "k216", ([12, 12, 12], 700, 1), 8, 8, "row", False, None),
    ("w3x16", "subm3", ([16, 16, 16], 1200, 1), 3, 16, "row", False, None),
    ("w5x7", "s2", ([16, 16, 16], 1200, 1), 5, 7, "row", False, None),
    ("w48x96", "subm3", ([16, 16, 16], 1000, 1), 48, 96, "row", False, None),
    ("w64x64", "subm3", ([16, 16, 16], 1000, 1), 64, 64, "row", False, None),
    ("w16x300", "s2", ([16, 16, 16], 800, 1), 16, 300, "row", False, None),
    ("sorted_subm", "subm3", ([16, 16, 16], 1200, 2), 16, 16, "sort", False, None),
    ("sorted_s2", "s2", ([16, 16, 16], 1200, 2), 8, 16, "sort", False, None),
    ("argsort", "subm3", ([16, 16, 16], 1200, 1), 8, 8, "argsort", False, None),
    ("layout", "subm3", ([40, 40, 40], 33000, 1), 8, 8, "layout", False, None),
    ("bias", "subm3", ([16, 16, 16], 1200, 1), 8, 24, "row", False, "none"),
    ("relu", "s2", ([16, 16, 16], 1200, 1), 8, 24, "row", False, "relu"),
    ("leaky", "subm3", ([16, 16, 16], 1200, 1), 8, 24, "row", False, "leaky"),
    ("sigmoid", "subm3", ([16, 16, 16], 1200, 1), 8, 24, "row", False, "sigmoid"),
]


def _tables(rb, which, width, table):
    from spconv_amd.pytorch import ops
    pair, mask = (rb.pair_fwd, rb.mask_fwd) if which == "fwd" else (rb.pair_bwd, rb.mask_bwd)
    if table == "row":
        return pair, mask, None, 0
    if table == "argsort":      # tile_order 0 with a row permutation over the row-order tables
        return pair, mask, ops.mask_argsort(mask[:, :1].contiguous()), 0
    return ops.tables_of(rb, which, width)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_entries_match_fp64_reference(case):
    """igemm_fwd / igemm_dgrad / igemm_wgrad / igemm_bwd on float64 against refconv, every element; the float64
    kernels ran (their counters moved), no other gather-GEMM did."""
    from spconv_amd import _lib
    from spconv_amd.pytorch import ops
    name, geom, (shape, n, bs), C, K, table, inverse, act = case
    ks, st, pd, dl, subm, tr = GEOMS[geom]
    kv = int(np.prod(ks))
    idx = scene(shape, n, bs, seed=len(name))
    sort = {"row": False, "argsort": False, "sort": True, "layout": "layout"}[table]
    rb, _ = gpu_rulebook(idx, bs, shape, ks, st, pd, dl, subm, transpose=tr, do_sort=sort)
    if table == "sort":
        assert rb.argsort_fwd is not None
    if table == "layout":
        assert rb.layout is not None
    out_idx, cand = pairs(idx, bs, shape, ks, st, pd, dl, subm, tr, device=DEV)
    assert rb.n_out == out_idx.shape[0]
    oshape = out_spatial_shape(shape, ks, st, pd, dl, subm, tr)
    perm = torch.from_numpy(match_rows(rb.out_indices.cpu().numpy(), out_idx.cpu().numpy(), oshape)).to(DEV)
    ident = torch.arange(idx.shape[0], device=DEV)
    if inverse:     # the strided layer's outputs back to its inputs: roles of the two row sets swap
        cand = [(k, o, i) for k, i, o in cand]
        ref_out_rows, p_in, p_out, n_in, n_out = torch.from_numpy(idx), perm, ident, rb.n_out, rb.n_in
    else:
        ref_out_rows, p_in, p_out, n_in, n_out = out_idx, ident, perm, rb.n_in, rb.n_out
    g = torch.Generator(device="cpu").manual_seed(zlib.crc32(name.encode()))
    f = (torch.rand((n_in, C), generator=g, dtype=F64) * 2 - 1).to(DEV)
    w = (torch.rand((K, *ks, C), generator=g, dtype=F64) * 2 - 1).to(DEV)
    d = (torch.rand((n_out, K), generator=g, dtype=F64) * 2 - 1).to(DEV)
    bias = (torch.rand((K,), generator=g, dtype=F64) * 2 - 1).to(DEV) if act else None
    f_ref, d_ref = torch.empty_like(f), torch.empty_like(d)
    f_ref[p_in] = f
    d_ref[p_out] = d
    ref = conv_from_pairs(ref_out_rows, cand, f_ref, w, d_ref)

    fwd_which = "bwd" if inverse else "fwd"
    bwd_which = "fwd" if (subm or inverse) else "bwd"
    native = rb.native_swapped() if inverse else rb.pair_native
    before = _lib.launch_counts(F64_KEYS + OTHER_KEYS)
    t = _tables(rb, fwd_which, K, table)
    out = ops.igemm_fwd(f, w, t[0], t[1], t[2], n_out, kv // 2 if subm else -1, bias=bias,
                        act_type={None: 0, "none": 0, "relu": ops.Activation.ReLU, "sigmoid": ops.Activation.Sigmoid,
                                  "leaky": ops.Activation.LeakyReLU}[act], act_alpha=ALPHA, tile_order=t[3])
    t = _tables(rb, bwd_which, C, table)
    din = ops.igemm_dgrad(d, w, t[0], t[1], t[2], n_in, subm, tile_order=t[3])
    dw = ops.igemm_wgrad(f, d, w.shape, native, rb.num_per_loc, subm, ops._plan_of(rb))
    din2, dw2 = ops.igemm_bwd(f, d, w, t[0], t[1], t[2], native, rb.num_per_loc, subm, ops._plan_of(rb),
                              tile_order=t[3])
    torch.cuda.synchronize()
    after = _lib.launch_counts(F64_KEYS + OTHER_KEYS)

    want, A = ref.out, ref.out_abs
    if bias is not None:
        want, A = _act(want + bias, act), A + bias.abs()
    assert_f64_close(out, want[p_out], A[p_out], "out")
    for nm, got in (("din", din), ("din (bwd)", din2)):
        assert_f64_close(got, ref.din[p_in], ref.din_abs[p_in], nm)
    for nm, got in (("dW", dw), ("dW (bwd)", dw2)):
        assert_f64_close(got, ref.dW, ref.dW_abs, nm)
    assert torch.equal(din, din2) and torch.equal(dw, dw2), "igemm_bwd differs from igemm_dgrad + igemm_wgrad"
    moved = {k: after[k] - before[k] for k in before}
    assert moved["igemm_f64/fwd"] == 1 and moved["igemm_f64/dgrad"] == 2, moved
    assert moved["wgrad_f64"] == 2 * (-(-kv // 128)), moved
    assert all(moved[k] == 0 for k in OTHER_KEYS), moved


@pytest.mark.parametrize("name", ["subm3", "s2", "sorted_subm", "kv216"])
def test_capi_bwd_float64(name):
    """spx_igemm_bwd(SPX_F64) called directly (ops.igemm_bwd takes the dgrad + wgrad calls in Python): din and dW equal
    the separate entries' bit for bit (kernel volumes up to 128: the same launches) and the fp64 reference within the
    bound; one float64 dgrad and one weight-gradient launch, no fused one; a workspace below
    spx_igemm_wgrad_ws_bytes_dtype is refused."""
    from spconv_amd import _lib
    from spconv_amd.pytorch import ops
    L = _lib.load()
    _, geom, (shape, n, bs), C, K, table, _, _ = next(c for c in CASES if c[0] == name)
    ks, st, pd, dl, subm, tr = GEOMS[geom]
    kv = int(np.prod(ks))
    idx = scene(shape, n, bs, seed=len(name))
    rb, _ = gpu_rulebook(idx, bs, shape, ks, st, pd, dl, subm, transpose=tr, do_sort=table == "sort")
    out_idx, cand = pairs(idx, bs, shape, ks, st, pd, dl, subm, tr, device=DEV)
    oshape = out_spatial_shape(shape, ks, st, pd, dl, subm, tr)
    perm = torch.from_numpy(match_rows(rb.out_indices.cpu().numpy(), out_idx.cpu().numpy(), oshape)).to(DEV)
    g = torch.Generator(device="cpu").manual_seed(zlib.crc32(("capi" + name).encode()))
    f = (torch.rand((rb.n_in, C), generator=g, dtype=F64) * 2 - 1).to(DEV)
    w = (torch.rand((K, *ks, C), generator=g, dtype=F64) * 2 - 1).to(DEV)
    d = (torch.rand((rb.n_out, K), generator=g, dtype=F64) * 2 - 1).to(DEV)
    d_ref = torch.empty_like(d)
    d_ref[perm] = d
    ref = conv_from_pairs(out_idx, cand, f, w, d_ref)
    t = _tables(rb, "fwd" if subm else "bwd", C, "row" if table == "row" else "sort")
    din, dw = torch.empty_like(f), torch.empty_like(w)
    ws_bytes = L.spx_igemm_wgrad_ws_bytes_dtype(rb.n_in, C, K, kv, _lib.DTYPE_F64)
    ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream

    def call(nbytes):
        return L.spx_igemm_bwd(f.data_ptr(), d.data_ptr(), w.data_ptr(), din.data_ptr(), dw.data_ptr(),
                               t[0].data_ptr(), t[1].data_ptr(), None if t[2] is None else t[2].data_ptr(), t[3],
                               rb.pair_native.data_ptr(), rb.num_per_loc.data_ptr(), None, rb.n_in, rb.n_out, C, K, kv,
                               _lib.DTYPE_F64, int(subm), ws.data_ptr(), nbytes, stream)

    before = _lib.launch_counts(F64_KEYS + OTHER_KEYS)
    assert call(ws_bytes - 256) != 0 and b"workspace too small" in L.spx_last_error()
    torch.cuda.synchronize()
    assert _lib.launch_counts(F64_KEYS + OTHER_KEYS) == before, "a refused call launched"
    _lib.check(call(ws_bytes))
    torch.cuda.synchronize()
    moved = {k: v - before[k] for k, v in _lib.launch_counts(F64_KEYS + OTHER_KEYS).items()}
    assert moved["igemm_f64/dgrad"] == 1 and moved["wgrad_f64"] == 1 and moved["igemm_f64/fwd"] == 0, moved
    assert all(moved[k] == 0 for k in OTHER_KEYS), moved
    assert_f64_close(din, ref.din, ref.din_abs, "din")
    assert_f64_close(dw, ref.dW, ref.dW_abs, "dW")
    if kv <= 128:
        din2 = ops.igemm_dgrad(d, w, t[0], t[1], t[2], rb.n_in, subm, tile_order=t[3])
        dw2 = ops.igemm_wgrad(f, d, w.shape, rb.pair_native, rb.num_per_loc, subm, None)
        assert torch.equal(din, din2) and torch.equal(dw, dw2)

def test_exact_integers_asymmetric_weights():
    """Small integers make every product and sum exact: the result must be EQUAL to the reference -- a fragment map
    that puts a value in the wrong row or column (the f32 16x16 accumulator map on the f64 MFMA) cannot pass."""
    from spconv_amd.pytorch import ops
    shape, bs, C, K = [10, 10, 10], 1, 20, 40
    ks = [3, 3, 3]
    idx = scene(shape, 400, bs, seed=3)
    rb, _ = gpu_rulebook(idx, bs, shape, ks, [1] * 3, [1] * 3, [1] * 3, True)
    out_idx, cand = pairs(idx, bs, shape, ks, [1] * 3, [1] * 3, [1] * 3, True, device=DEV)
    g = torch.Generator(device="cpu").manual_seed(5)
    f = torch.randint(-4, 5, (idx.shape[0], C), generator=g).to(DEV, F64)
    w = torch.randint(-3, 4, (K, 3, 3, 3, C), generator=g).to(DEV, F64)
    w += torch.arange(K, device=DEV, dtype=F64).reshape(K, 1, 1, 1, 1) * 8      # no two output channels alike
    d = torch.randint(-5, 6, (idx.shape[0], K), generator=g).to(DEV, F64)
    ref = conv_from_pairs(out_idx, cand, f, w, d)
    out = ops.igemm_fwd(f, w, rb.pair_fwd, rb.mask_fwd, None, rb.n_out, 13)
    din, dw = ops.igemm_bwd(f, d, w, rb.pair_fwd, rb.mask_fwd, None, rb.pair_native, rb.num_per_loc, True, None)
    assert torch.equal(out, ref.out) and torch.equal(din, ref.din) and torch.equal(dw, ref.dW)


def test_empty_scene():
    import spconv_amd.pytorch as spconv
    net = spconv.SubMConv3d(4, 6, 3, bias=True, indice_key="e").to(DEV, F64)
    feats = torch.zeros((0, 4), dtype=F64, device=DEV, requires_grad=True)
    x = spconv.SparseConvTensor(feats, torch.zeros((0, 4), dtype=torch.int32, device=DEV), [8, 8, 8], 1)
    y = net(x)
    assert y.features.shape == (0, 6) and y.features.dtype == F64
    y.features.sum().backward()
    assert feats.grad.shape == (0, 4)
    assert torch.equal(net.weight.grad, torch.zeros_like(net.weight))


def test_bias_act_inplace():
    from spconv_amd.pytorch import ops
    g = torch.Generator(device="cpu").manual_seed(1)
    x = (torch.rand((301, 7), generator=g, dtype=F64) * 4 - 2).to(DEV)
    b = (torch.rand((7,), generator=g, dtype=F64) - 0.5).to(DEV)
    for act, name in ((ops.Activation.None_, "none"), (ops.Activation.ReLU, "relu"),
                      (ops.Activation.LeakyReLU, "leaky"), (ops.Activation.Sigmoid, "sigmoid")):
        got = ops.bias_act_inplace(x.clone(), b, act, ALPHA)
        assert_f64_close(got, _act(x + b, name), (x.abs() + b.abs()) * 4, name)


# ---------------------------------------------------------------- module level
def _scene_tensor(n, shape, C, seed, grad=True, distinct=False):
    idx = scene(shape, n, 1, seed)
    g = torch.Generator(device="cpu").manual_seed(seed)
    if distinct:        # no ties anywhere: max pooling is differentiable at every input
        f = (torch.randperm(idx.shape[0] * C, generator=g).to(F64) + 1.0).reshape(-1, C) * 0.01
    else:
        f = torch.rand((idx.shape[0], C), generator=g, dtype=F64) * 2 - 1
    return torch.from_numpy(idx).to(DEV), f.to(DEV).requires_grad_(grad), shape


def _gradcheck_layer(net, idx, feats, shape, prep=None):
    import spconv_amd.pytorch as spconv
    params = dict(net.named_parameters())
    names = sorted(params)

    def fn(x, *ps):
        t = spconv.SparseConvTensor(x, idx, shape, 1) if prep is None else prep(x)
        y = torch.func.functional_call(net, dict(zip(names, ps)), (t,))
        return y.features

    inputs = (feats,) + tuple(params[k].detach().clone().requires_grad_(True) for k in names)
    assert torch.autograd.gradcheck(fn, inputs, nondet_tol=0.0, eps=1e-6, atol=1e-8, rtol=1e-6)


@pytest.mark.parametrize("layer", ["subm", "conv_s2", "transposed"])
def test_gradcheck_conv(layer):
    import spconv_amd.pytorch as spconv
    torch.manual_seed(0)
    idx, feats, shape = _scene_tensor(160, [8, 8, 8], 4, seed=11)
    net = {"subm": lambda: spconv.SubMConv3d(4, 5, 3, bias=True),
           "conv_s2": lambda: spconv.SparseConv3d(4, 5, 3, 2, 1, bias=True),
           "transposed": lambda: spconv.SparseConvTranspose3d(4, 5, 3, 2, 1, bias=True)}[layer]().to(DEV, F64)
    _gradcheck_layer(net, idx, feats, shape)


def test_gradcheck_inverse():
    import spconv_amd.pytorch as spconv
    torch.manual_seed(0)
    idx, feats, shape = _scene_tensor(200, [8, 8, 8], 4, seed=12, grad=False)
    down = spconv.SparseConv3d(4, 6, 3, 2, 1, bias=False, indice_key="d").to(DEV, F64)
    with torch.no_grad():
        y = down(spconv.SparseConvTensor(feats, idx, shape, 1))
    net = spconv.SparseInverseConv3d(6, 4, 3, indice_key="d", bias=True).to(DEV, F64)
    x = y.features.detach().clone().requires_grad_(True)
    _gradcheck_layer(net, idx, x, shape, prep=lambda f: y.replace_feature(f))


@pytest.mark.parametrize("kind", ["max", "avg"])
def test_gradcheck_pool(kind):
    import spconv_amd.pytorch as spconv
    from spconv_amd import _lib
    L = _lib.load()
    idx, feats, shape = _scene_tensor(250, [10, 10, 10], 6, seed=13, distinct=kind == "max")
    net = (spconv.SparseMaxPool3d if kind == "max" else spconv.SparseAvgPool3d)(3, 2, 1).to(DEV)
    before = L.spx_launch_count(b"pool/f64")

    def fn(x):
        return net(spconv.SparseConvTensor(x, idx, shape, 1)).features

    assert torch.autograd.gradcheck(fn, (feats,), nondet_tol=0.0, eps=1e-6, atol=1e-8, rtol=1e-6)
    assert L.spx_launch_count(b"pool/f64") > before


def test_pool_forward_values():
    """max / avg pooling in float64 against a torch loop over the reference pairs (sums in float64)."""
    import spconv_amd.pytorch as spconv
    idx, feats, shape = _scene_tensor(600, [12, 12, 12], 10, seed=14, grad=False)
    ks = [3, 3, 3]
    out_idx, cand = pairs(idx, 1, shape, ks, [2] * 3, [1] * 3, [1] * 3, False, device=DEV)
    for kind in ("max", "avg"):
        net = (spconv.SparseMaxPool3d if kind == "max" else spconv.SparseAvgPool3d)(3, 2, 1)
        y = net(spconv.SparseConvTensor(feats, idx, shape, 1))
        n_out = out_idx.shape[0]
        if kind == "max":
            ref = torch.full((n_out, 10), -np.inf, dtype=F64, device=DEV)
            for _, i, o in cand:
                ref.index_reduce_(0, o, feats[i], "amax")
        else:
            s = torch.zeros((n_out, 10), dtype=F64, device=DEV)
            cnt = torch.zeros((n_out, 1), dtype=F64, device=DEV)
            for _, i, o in cand:
                s.index_add_(0, o, feats[i])
                cnt.index_add_(0, o, torch.ones((o.numel(), 1), dtype=F64, device=DEV))
            ref = s / cnt
        perm = torch.from_numpy(match_rows(y.indices.cpu().numpy(), out_idx.cpu().numpy(),
                                           out_spatial_shape(shape, ks, [2] * 3, [1] * 3, [1] * 3, False))).to(DEV)
        assert y.features.dtype == F64
        assert_f64_close(y.features, ref[perm], torch.ones_like(ref), kind)     # (|values| <= 1)


def _dense_from(feat, idx, shape):
    dense = torch.zeros((1, feat.shape[1], *shape), dtype=feat.dtype, device=feat.device)
    i = idx.long()
    dense[0, :, i[:, 1], i[:, 2], i[:, 3]] = feat.t()
    return dense


def test_lidar_window_sequential_matches_dense_conv3d():
    """SubM -> BatchNorm1d -> ReLU -> strided conv -> SubM in float64 on a real-LiDAR window, forward and backward,
    against torch's dense float64 conv3d on the scattered input (BatchNorm / ReLU applied at the active sites)."""
    import spconv_amd.pytorch as spconv
    from golden import lidar_scene
    full, _ = lidar_scene()
    z0, y0, x0, shape = 10, 768, 768, [40, 256, 256]
    m = ((full[:, 1] >= z0) & (full[:, 1] < z0 + 40) & (full[:, 2] >= y0) & (full[:, 2] < y0 + 256)
         & (full[:, 3] >= x0) & (full[:, 3] < x0 + 256))
    idx = full[m] - np.array([0, z0, y0, x0], dtype=np.int32)
    assert idx.shape[0] > 10000
    C, H, K = 4, 8, 8
    torch.manual_seed(7)
    net = spconv.SparseSequential(
        spconv.SubMConv3d(C, H, 3, bias=False, indice_key="s1"),
        torch.nn.BatchNorm1d(H),
        torch.nn.ReLU(),
        spconv.SparseConv3d(H, K, 3, 2, 1, bias=False),
        spconv.SubMConv3d(K, K, 3, bias=True, indice_key="s2"),
    ).to(DEV).double()
    net.train()
    it = torch.from_numpy(np.ascontiguousarray(idx)).to(DEV)
    g = torch.Generator(device="cpu").manual_seed(8)
    f = (torch.rand((idx.shape[0], C), generator=g, dtype=F64) * 2 - 1).to(DEV).requires_grad_(True)
    y = net(spconv.SparseConvTensor(f, it, shape, 1))

    # dense float64 reference with the same parameters
    conv1, bn, _, conv2, conv3 = net
    w = lambda m_: m_.weight.detach().permute(0, 4, 1, 2, 3).clone().requires_grad_(True)
    w1, w2, w3 = w(conv1), w(conv2), w(conv3)
    b3 = conv3.bias.detach().clone().requires_grad_(True)
    bn_ref = torch.nn.BatchNorm1d(H).to(DEV).double().train()
    fd = f.detach().clone().requires_grad_(True)
    ii = it.long()
    dense = _dense_from(fd, it, shape)
    h = torch.nn.functional.conv3d(dense, w1, padding=1)[0, :, ii[:, 1], ii[:, 2], ii[:, 3]].t()
    h = torch.relu(bn_ref(h))
    h2 = torch.nn.functional.conv3d(_dense_from(h, it, shape), w2, stride=2, padding=1)
    oi = y.indices.long()
    occupied = torch.zeros(h2.shape[2:], dtype=torch.bool, device=DEV)
    occupied[oi[:, 1], oi[:, 2], oi[:, 3]] = True
    h2 = h2 * occupied
    ref = torch.nn.functional.conv3d(h2, w3, b3, padding=1)[0, :, oi[:, 1], oi[:, 2], oi[:, 3]].t()

    def close(a, b, A, name):
        a, b, A = a.detach(), b.detach(), A.detach()
        err = float((a - b).abs().max() / A.abs().max())
        assert err <= 1e-12, f"{name}: {err:.3g} of the largest magnitude"

    close(y.features, ref, ref, "out")
    gout = (torch.rand(tuple(ref.shape), generator=g, dtype=F64) - 0.5).to(DEV)
    y.features.backward(gout)
    ref.backward(gout)
    close(f.grad, fd.grad, fd.grad, "din")
    close(conv1.weight.grad.permute(0, 4, 1, 2, 3), w1.grad, w1.grad, "dW1")
    close(conv2.weight.grad.permute(0, 4, 1, 2, 3), w2.grad, w2.grad, "dW2")
    close(conv3.weight.grad.permute(0, 4, 1, 2, 3), w3.grad, w3.grad, "dW3")
    close(conv3.bias.grad, b3.grad, b3.grad, "db3")


def test_backward_is_deterministic():
    """Two backward passes of one float64 layer: bit-identical din and dW (no floating-point atomics)."""
    import spconv_amd.pytorch as spconv
    idx, feats, shape = _scene_tensor(3000, [24, 24, 24], 32, seed=15)
    net = spconv.SubMConv3d(32, 48, 3, bias=False, indice_key="det").to(DEV, F64)
    x = spconv.SparseConvTensor(feats, idx, shape, 1)
    gout = torch.rand((idx.shape[0], 48), dtype=F64, device=DEV)
    res = []
    for _ in range(2):
        feats.grad, net.weight.grad = None, None
        net(x).features.backward(gout)
        res.append((feats.grad.clone(), net.weight.grad.clone()))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
