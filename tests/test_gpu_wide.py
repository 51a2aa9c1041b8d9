"""Layers wider than 256 channels on the column-blocked MFMA gather-GEMM (csrc/igemm_wide.hip).

1. every wide instance against the fp64 pair reference of refconv.py, with the runner, checker and constants of
   test_gpu_kernel_matrix.py (c = 1e-6 for 16-bit tensors, 1e-5 for fp32.  Those constants were argued for reductions
   of at most 27 x 64 terms; the 256-wide kernel of before already ran 27 x 512-term reductions, and measured there --
   (C, K) = (512, 256), SubM 3x3x3, the measurement of tools/tol_probe.py -- the excess over u |ref| is at most
   MEASURED_EXCESS_512 of the magnitude sum, below the constants, which therefore stay);
2. bit identity with the 256-wide kernels on slices of the weights (no tolerance);
3. int8 bit-exact against oracle.int8_conv_ref;
4. modules against a dense convolution in fp64; deferred weight gradient;
5. a captured backbone with a 512-wide stage;
6. conv + BatchNorm at 512 channels: the statistics sink stays empty.
Every case checks through spx_launch_count that the wide instance ran and that the generic kernel did not."""
import copy
import zlib

import numpy as np
import pytest
import torch
from torch import nn

import oracle
import test_gpu_kernel_matrix as km
from golden import lidar_scene
from util import dense_scene, gpu_rulebook, oracle_rulebook, rel_err, scene, to_np

F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32
DTN = km.DTN
# largest (|got - ref| - u |ref|) / A of the 256-wide kernels over 27 x 512-term reductions -- out at (C, K) = (512, 256),
# din at (256, 512), SubM 3x3x3, 3000 voxels, measured on MI355X: f16 2.4e-8, bf16 1.4e-8, fp32 2.7e-7 (the wide launches
# at (512, 512): 2.1e-8, 2.5e-8, 3.0e-7).  Below c = 1e-6 / 1e-5 by a factor of more than 30: the constants stay.
MEASURED_EXCESS_512 = {"16-bit": 2.4e-8, "f32": 2.7e-7}

WIDTHS = [(64, 512), (512, 64), (512, 512), (256, 320), (384, 384), (40, 260)]


def _generic(L, dtype):
    return L.spx_launch_count(f"generic/{DTN[dtype]}".encode())


def wide_key(dtype, red, bt):
    """instance of a column-blocked launch whose reduction rows hold `red` (lane-padded) channels"""
    if dtype == F32:
        nks, pk = (1 if red * 4 <= 64 else 2), 1
    else:
        nks, pk = km.pack_form(dtype, red, 1, False)
    return f"igemm_v4w/128/{DTN[dtype]}/{'bt' if bt else 'fwd'}/{nks}/{pk}"


def expected_key(entry, dtype, C, K, kv, n_dst):
    """The instance a driver call must reach (ops.igemm_fwd / igemm_dgrad / igemm_bwd): the wide one where the output
    side of the launch is beyond 256 columns, the one of before elsewhere."""
    if entry == "bwd" and C in km.MFMA_COUT and C <= 128 and kv <= 32:
        return km.bwd_key(dtype, C, K)                      # the fused launch: dgrad tiles are C wide
    red, out, bt = (C, K, False) if entry == "fwd" else (K, C, True)
    red = km.padw(red, dtype)
    if out > 256:
        return wide_key(dtype, red, bt)
    return km.v4_key(dtype, red, km.round_cout(out), n_dst, bt)


def _matrix_cases():
    sites = [("small", "subm3"), ("small", "s2"), ("mid", "k2s2"), ("mid", "k125")]
    acts = [None, "relu", "leaky", "sigmoid"]
    out, i = [], 0
    for C0, K0 in WIDTHS:
        for dtype in (F16, BF16, F32):
            for scene_name, geom in sites:
                kv = int(np.prod(km.GEOMS[geom][0]))
                subm = km.GEOMS[geom][4]
                for entry in ("fwd", "dgrad", "bwd"):
                    i += 1
                    C, K = C0, K0
                    if geom == "k125":              # (bounds the fp64 reference: the reduction side shrinks)
                        C, K = (min(C0, 64), K0) if entry == "fwd" else (C0, min(K0, 64))
                    table = "row" if kv > 32 else ["row", "sort"][i % 2]
                    n_src = km.SCENES[scene_name][2] * km.SCENES[scene_name][3]
                    key = expected_key(entry, dtype, C, K, kv, n_src if (subm or entry != "fwd") else 0)
                    act = acts[i % 4] if entry == "fwd" else None
                    out.append(km.case(entry, key, scene_name, geom, dtype, C, K, table, act=act,
                                       name=f"act-{act}" if act else None))
    # rows layout (SubM rulebooks from 32768 rows on) and a launch of more than 512 column-block tiles in tile order (lpt)
    for C, K in WIDTHS:
        for dtype in (F16, BF16, F32):
            i += 1
            entries = ("fwd", "dgrad", "bwd") if (C, K) == (512, 512) else (("fwd", "dgrad", "bwd")[i % 3],)
            for entry in entries:
                out.append(km.case(entry, expected_key(entry, dtype, C, K, 3, 32769), "n32769", "line", dtype, C, K,
                                   "layout", name="layout"))
    for dtype, entry in ((F16, "fwd"), (BF16, "dgrad"), (F32, "fwd")):
        out.append(km.case(entry, expected_key(entry, dtype, 384, 384, 3, 40000), "n40000", "line", dtype, 384, 384,
                           "sort", name="lpt"))
    out.append(km.case("fwd", expected_key("fwd", F16, 64, 512, 27, 32769), "n32769", "subm3", F16, 64, 512, "layout",
                       name="layout-subm3"))
    out.append(km.case("dgrad", expected_key("dgrad", BF16, 512, 64, 27, 32769), "n32769", "subm3", BF16, 512, 64,
                       "layout", name="layout-subm3"))
    # offset packing: reduction rows of 8 / 16 channels into a wide output
    narrow = [(dtype, entry, red) for dtype in (F16, BF16) for entry in ("fwd", "dgrad") for red in (5, 16, 24)]
    narrow += [(F32, "fwd", 12), (F32, "dgrad", 16)]
    for j, (dtype, entry, red) in enumerate(narrow):
        width = (512, 384, 300)[j % 3]
        C, K = (red, width) if entry == "fwd" else (width, red)
        out.append(km.case(entry, expected_key(entry, dtype, C, K, 27, 3000), "small", "subm3", dtype, C, K,
                           ["row", "sort"][j % 2], name="narrow-rows"))
    return out


CASES = _matrix_cases()


@pytest.mark.gpu
@pytest.mark.parametrize("c", CASES, ids=[km._case_id(c) for c in CASES])
def test_wide_instance_against_fp64(cuda, c):
    from spconv_amd import _lib
    L = _lib.load()
    before = _generic(L, c["dtype"])
    km._run(c, cuda)                    # (asserts that c["key"] was launched, and every element against fp64)
    assert _generic(L, c["dtype"]) == before, "the generic kernel ran"


def test_matrix_claims_every_wide_float_instance():
    from test_wide import wide_keys
    claimed = {c["key"] for c in CASES}
    floats = {k for k in wide_keys() if "/i8/" not in k}
    assert floats <= claimed, sorted(floats - claimed)


# ------------------------------------------------------------------ 2. bit identity with the 256-wide kernels
def _scene_of(which):
    if which == "uniform100k":
        shape = [40, 400, 400]
        return scene(shape, 100_000, 1, 21), shape
    return lidar_scene()


_RB = {}


def _rb(which, table):
    if (which, table) not in _RB:
        if len(_RB) > 3:
            _RB.clear()
        idx, shape = _scene_of(which)
        sort = {"row": False, "sort": True, "layout": "layout"}[table]
        _RB[(which, table)] = gpu_rulebook(idx, 1, shape, [3] * 3, [1] * 3, [1] * 3, [1] * 3, True, do_sort=sort)[0]
    return _RB[(which, table)]


def _tabs(rb, table, width):
    from spconv_amd.pytorch import ops
    if table == "row":
        return rb.pair_fwd, rb.mask_fwd, None, 0
    tabs = ops.tables_of(rb, "fwd", width)
    assert tabs[3] == {"sort": 1, "layout": 2}[table], "tables_of dropped the table form of a wide layer"
    return tabs


@pytest.mark.gpu
@pytest.mark.parametrize("table", ["row", "sort", "layout"])
@pytest.mark.parametrize("which", ["uniform100k", "lidar"])
@pytest.mark.parametrize("dtype", [F16, BF16, F32], ids=["f16", "bf16", "f32"])
def test_wide_equals_256_wide_launches_on_weight_slices(cuda, dtype, which, table):
    from spconv_amd import _lib
    from spconv_amd.pytorch import ops
    L = _lib.load()
    rb = _rb(which, table)
    n, C, K = rb.n_out, 64, 512
    g = torch.Generator(device="cpu").manual_seed(zlib.crc32(f"{which}{table}{dtype}".encode()))
    f = (torch.rand((n, C), generator=g) * 2 - 1).to(cuda, dtype)
    w = (torch.rand((K, 3, 3, 3, C), generator=g) * 2 - 1).to(cuda, dtype)
    d = ((torch.rand((n, C), generator=g) * 2 - 1) * 0.2).to(cuda, dtype)
    bias = (torch.rand((K,), generator=g) * 2 - 1).to(cuda, dtype)
    tabs = _tabs(rb, table, K)
    gen0 = _generic(L, dtype)
    k_fwd, k_bt = wide_key(dtype, C, False).encode(), wide_key(dtype, C, True).encode()
    n_fwd, n_bt = L.spx_launch_count(k_fwd), L.spx_launch_count(k_bt)
    act = ops.Activation.ReLU
    got = ops.igemm_fwd(f, w, tabs[0], tabs[1], tabs[2], n, 13, bias=bias, act_type=act, tile_order=tabs[3])
    parts = [ops.igemm_fwd(f, w[j:j + 256].contiguous(), tabs[0], tabs[1], tabs[2], n, 13, bias=bias[j:j + 256].contiguous(),
                           act_type=act, tile_order=tabs[3]) for j in range(0, K, 256)]
    assert L.spx_launch_count(k_fwd) == n_fwd + 1, "one launch per layer"
    assert torch.equal(got, torch.cat(parts, 1))
    # dgrad of the transposed shape: W [64, 27, 512] is a layer 512 -> 64; din is 512 wide, the slices are over C
    wt = w.reshape(K, 27, C).permute(2, 1, 0).contiguous().reshape(C, 3, 3, 3, K)
    din = ops.igemm_dgrad(d, wt, tabs[0], tabs[1], tabs[2], n, True, tile_order=tabs[3])
    dparts = [ops.igemm_dgrad(d, wt[..., j:j + 256].contiguous(), tabs[0], tabs[1], tabs[2], n, True, tile_order=tabs[3])
              for j in range(0, K, 256)]
    assert L.spx_launch_count(k_bt) == n_bt + 1
    assert torch.equal(din, torch.cat(dparts, 1))
    assert float(got.float().abs().max()) > 0 and float(din.float().abs().max()) > 0
    assert _generic(L, dtype) == gen0


@pytest.mark.gpu
@pytest.mark.parametrize("table", ["row", "sort", "layout"])
@pytest.mark.parametrize("which", ["uniform100k", "lidar"])
def test_wide_int8_equals_256_wide_launches_on_weight_slices(cuda, which, table):
    from spconv_amd import _lib
    from spconv_amd.pytorch import ops
    L = _lib.load()
    rb = _rb(which, table)
    n, C, K = rb.n_out, 64, 512
    rng = np.random.default_rng(5)
    f = torch.from_numpy(rng.integers(-127, 128, (n, C), dtype=np.int8)).to(cuda)
    w = torch.from_numpy(rng.integers(-127, 128, (K, 3, 3, 3, C), dtype=np.int8)).to(cuda)
    scale = torch.from_numpy((rng.uniform(0.5, 1.5, K) * 2e-3).astype(np.float32))
    bias = torch.from_numpy(rng.uniform(-5, 5, K).astype(np.float32))
    add = torch.from_numpy(rng.integers(-127, 128, (n, K), dtype=np.int8)).to(cuda)
    tabs = _tabs(rb, table, K)
    key = b"igemm_v4w/128/i8/fwd/1/1"
    before = L.spx_launch_count(key)
    for out_dtype in (torch.int8, F16, BF16, F32):
        run = lambda ww, sc, bi, ad: ops.igemm_fwd_int8(f, ww, tabs[0], tabs[1], tabs[2], n, 13, sc, bi, ad, 0.25, out_dtype,
                                                        ops.Activation.ReLU, tile_order=tabs[3])
        got = run(w, scale, bias, add)
        parts = [run(w[j:j + 256].contiguous(), scale[j:j + 256], bias[j:j + 256], add[:, j:j + 256].contiguous())
                 for j in range(0, K, 256)]
        assert torch.equal(got, torch.cat(parts, 1)), out_dtype
    assert L.spx_launch_count(key) == before + 4
    assert 0 < float((got != 0).float().mean()) < 1


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
def test_wide_layer_beyond_32_bit_offsets_keeps_the_generic_kernel(cuda, dtype):
    """2.1 M rows x 512 16-bit channels are 2 GiB: past the 32-bit buffer offsets of the column-blocked launch, and the
    first-generation kernel has no instance beyond 256 columns -- such a layer keeps the generic kernel, forward and
    dgrad (a 1x1x1 SubM layer: every row reads itself, so the expected values are a plain matrix product)."""
    from spconv_amd import _lib
    from spconv_amd.pytorch import ops
    L = _lib.load()
    n, red, width = 2_100_000, 8, 512
    assert n * width * 2 >= 0x7fff0000
    g = torch.Generator().manual_seed(3)
    f = torch.empty((n, red), dtype=dtype, device=cuda).uniform_(-1, 1)
    rows = torch.randint(0, n, (2048,), generator=g).to(cuda)
    rows[:4] = torch.tensor([0, 1, n - 2, n - 1])
    gen0, wide0 = _generic(L, dtype), L.spx_launch_count(b"igemm_v4w")
    w = (torch.rand((width, 1, 1, 1, red), generator=g) * 2 - 1).to(cuda, dtype)
    out = ops.igemm_fwd(f, w, None, None, None, n, 0)
    assert tuple(out.shape) == (n, width)
    want = f[rows].float() @ w.reshape(width, red).float().t()
    assert float((out[rows].float() - want).abs().max()) <= 2.0 ** -7 * float(want.abs().max())    # (one output rounding)
    del out
    wd = (torch.rand((red, 1, 1, 1, width), generator=g) * 2 - 1).to(cuda, dtype)                  # a layer 512 -> 8
    din = ops.igemm_dgrad(f, wd, None, None, None, n, True)
    assert tuple(din.shape) == (n, width)
    want = f[rows].float() @ wd.reshape(red, width).float()
    assert float((din[rows].float() - want).abs().max()) <= 2.0 ** -7 * float(want.abs().max())
    assert _generic(L, dtype) == gen0 + 2 and L.spx_launch_count(b"igemm_v4w") == wide0


# ------------------------------------------------------------------ 3. int8 against the reference formula
@pytest.mark.gpu
@pytest.mark.parametrize("K", [320, 512])
@pytest.mark.parametrize("C", [64, 144])
def test_wide_int8_bit_exact_against_the_formula(cuda, C, K):
    from spconv_amd import _lib
    from spconv_amd.pytorch import ops
    from test_gpu_int8 import _int8_case
    L = _lib.load()
    shape, ks, one = [24, 24, 24], [3] * 3, [1] * 3
    idx, ref, f, w, scale, bias, add = _int8_case(shape, 2500, 1, C, K, ks, one, one, one, True, seed=3)
    rb, _ = gpu_rulebook(idx, 1, shape, ks, one, one, one, True)
    key = f"igemm_v4w/128/i8/fwd/{1 if C <= 64 else 2}/1".encode()
    before = L.spx_launch_count(key)
    args = (torch.from_numpy(f).to(cuda), torch.from_numpy(w).to(cuda), rb.pair_fwd, rb.mask_fwd, None, rb.n_out, 13,
            torch.from_numpy(scale), torch.from_numpy(bias), torch.from_numpy(add).to(cuda), 0.37)
    want = oracle.int8_conv_ref(f, w, ref["pair"], ref["num"], ref["n_out"], True, scale, bias, add, 0.37, True)
    got = to_np(ops.igemm_fwd_int8(*args, torch.int8, ops.Activation.ReLU))
    assert got.shape == (ref["n_out"], K) and got.dtype == np.int8
    assert np.abs(want.astype(np.int32)).max() == 127
    np.testing.assert_array_equal(got, want)
    # f16 output: the fp32 value of the formula, rounded once
    want32 = oracle.int8_conv_ref(f, w, ref["pair"], ref["num"], ref["n_out"], True, scale, bias, add, 0.37, True,
                                  out_dtype=np.float32)
    got16 = to_np(ops.igemm_fwd_int8(*args, torch.float16, ops.Activation.ReLU))
    np.testing.assert_array_equal(got16, want32.astype(np.float16))
    assert L.spx_launch_count(key) == before + 2


@pytest.mark.gpu
def test_quantized_module_with_512_output_channels(cuda):
    import spconv_amd.pytorch as spconv
    from spconv_amd import _lib
    from spconv_amd.pytorch.quantization import quantized as spq
    L = _lib.load()
    shape, n, bs, C, K = [20, 20, 20], 1500, 2, 64, 512
    rng = np.random.default_rng(11)
    idx = dense_scene(shape, n, bs, 11)
    ref = oracle_rulebook(idx, bs, shape, [3] * 3, [1] * 3, [1] * 3, [1] * 3, True)
    torch.manual_seed(3)
    conv = spconv.SubMConv3d(C, K, 3, bias=True, indice_key="q").to(cuda)
    conv.act_type = spconv.ops.Activation.ReLU
    in_scale, out_scale, add_q_scale = 0.02, 0.05, 0.04
    q = spq.SparseConv.from_float_conv(conv, out_scale).to(cuda)
    f_i8 = rng.integers(-127, 128, (idx.shape[0], C), dtype=np.int8)
    add_i8 = rng.integers(-127, 128, (idx.shape[0], K), dtype=np.int8)
    qf = torch._make_per_tensor_quantized_tensor(torch.from_numpy(f_i8).to(cuda), in_scale, 0)
    qa = torch._make_per_tensor_quantized_tensor(torch.from_numpy(add_i8).to(cuda), add_q_scale, 0)
    ind = torch.from_numpy(idx).to(cuda)
    before = L.spx_launch_count(b"igemm_v4w/128/i8/fwd/1/1")
    y = q(spconv.SparseConvTensor(qf, ind, shape, bs), spconv.SparseConvTensor(qa, ind, shape, bs))
    assert L.spx_launch_count(b"igemm_v4w/128/i8/fwd/1/1") == before + 1
    assert y.features.dtype == torch.qint8 and tuple(y.features.shape) == (idx.shape[0], K)
    w_i8 = to_np(q.weight().int_repr())
    ch_scale = (in_scale * to_np(q.weight().q_per_channel_scales().float())) / out_scale
    b = to_np(q.bias().float()) / out_scale
    want = oracle.int8_conv_ref(f_i8, w_i8, ref["pair"], ref["num"], ref["n_out"], True, ch_scale.astype(np.float32),
                                b.astype(np.float32), add_i8, add_q_scale / out_scale, True)
    np.testing.assert_array_equal(to_np(y.features.int_repr()), want)


# ------------------------------------------------------------------ 4. modules against a dense convolution in fp64
def _dense_ref(idx, bs, shape, feat, weight, stride, padding):
    """fp64 dense convolution on the CPU over the scattered input: (dense input, KCRS weight, dense output)."""
    i = torch.from_numpy(idx.astype(np.int64))
    dense = torch.zeros((bs, feat.shape[1], *shape), dtype=torch.float64)
    dense[i[:, 0], :, i[:, 1], i[:, 2], i[:, 3]] = feat.double()
    dense.requires_grad_(True)
    w = weight.double().permute(0, 4, 1, 2, 3).contiguous().requires_grad_(True)      # KRSC -> KCRS
    out = torch.nn.functional.conv3d(dense, w, None, stride, padding)
    return dense, w, out


MODULE_CASES = [
    # name, C, K, ksize, stride, padding, subm
    ("subm512", 512, 512, (3, 3, 3), 1, (1, 1, 1), True),
    ("down256to512", 256, 512, (3, 3, 3), 2, (1, 1, 1), False),
    ("asym256to512", 256, 512, (3, 1, 3), 1, (1, 0, 1), True),
]
# Norm-wise bounds (util.rel_err = max |a - ref| / max |ref|).  fp32: the 1e-4 of test_gpu_modules.py.  AMP: operands
# are given in f16-representable values, so what is left is one f16 rounding of every result element, 2^-11 of ITS
# magnitude <= 2^-11 of the largest, and the fp32 accumulation far below it: 2^-10 leaves a factor two.
MODULE_TOL = {"f32": 1e-4, "amp": 2.0 ** -10}


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["f32", "amp"])
@pytest.mark.parametrize("name,C,K,ksize,stride,padding,subm", MODULE_CASES, ids=[m[0] for m in MODULE_CASES])
def test_wide_modules_match_dense_fp64(cuda, name, C, K, ksize, stride, padding, subm, mode):
    import spconv_amd.pytorch as spconv
    from spconv_amd import _lib
    L = _lib.load()
    shape, bs = [8, 7, 6], 1
    idx = scene(shape, 150, bs, 484)
    rng = np.random.default_rng(484)
    rnd = (lambda t: t.half().float()) if mode == "amp" else (lambda t: t)
    feat = rnd(torch.from_numpy(rng.uniform(-1, 1, (idx.shape[0], C)).astype(np.float32)))
    torch.manual_seed(48848)
    if subm:
        net = spconv.SubMConv3d(C, K, ksize, bias=False, indice_key="m").to(cuda)
    else:
        net = spconv.SparseConv3d(C, K, ksize, stride, padding, bias=False, indice_key="m").to(cuda)
    with torch.no_grad():
        net.weight.copy_(rnd(net.weight))
    f = feat.to(cuda).requires_grad_(True)
    x = spconv.SparseConvTensor(f, torch.from_numpy(idx).to(cuda), shape, bs)
    dt = F16 if mode == "amp" else F32
    gen0 = _generic(L, dt)
    w0 = L.spx_launch_count(b"igemm_v4w")
    with torch.autocast("cuda", dtype=torch.float16, enabled=mode == "amp"):
        out = net(x)
    assert out.features.dtype == dt
    dense, w, out_ref = _dense_ref(idx, bs, shape, feat, net.weight.detach().cpu(), stride, padding)
    oi = out.indices.long().cpu()
    want = out_ref[oi[:, 0], :, oi[:, 1], oi[:, 2], oi[:, 3]]
    tol = MODULE_TOL[mode]
    assert rel_err(out.features.detach().float().cpu().numpy(), want.detach().numpy()) < tol
    dout = rnd(torch.from_numpy(np.random.default_rng(1).uniform(-0.2, 0.2, tuple(want.shape)).astype(np.float32)))
    want.backward(dout.double())
    out.features.backward(dout.to(cuda, dt))
    ii = torch.from_numpy(idx.astype(np.int64))
    din_ref = dense.grad[ii[:, 0], :, ii[:, 1], ii[:, 2], ii[:, 3]]
    assert rel_err(f.grad.float().cpu().numpy(), din_ref.numpy()) < tol
    assert rel_err(net.weight.grad.float().cpu().numpy(), w.grad.permute(0, 2, 3, 4, 1).numpy()) < tol
    assert L.spx_launch_count(b"igemm_v4w") > w0 and _generic(L, dt) == gen0
    if name == "down256to512":
        # the inverse convolution back to the input coordinates: 512 -> 256 over the same rulebook
        inv = spconv.SparseInverseConv3d(K, C, ksize, indice_key="m", bias=False).to(cuda)
        with torch.no_grad():
            inv.weight.copy_(rnd(inv.weight))
        f2 = rnd(torch.from_numpy(rng.uniform(-1, 1, tuple(out.features.shape)).astype(np.float32)))
        g2 = f2.to(cuda).requires_grad_(True)
        with torch.autocast("cuda", dtype=torch.float16, enabled=mode == "amp"):
            back = inv(out.replace_feature(g2))
        assert torch.equal(back.indices, x.indices)
        # transposed dense convolution in fp64: weight [K_in = 512, kv, C_out = 256] KRSC of the INVERSE layer is
        # [C_out, *ksize, K_in]; conv_transpose3d takes [in, out, *ksize]
        dz = torch.zeros((bs, K, *out.spatial_shape), dtype=torch.float64)
        dz[oi[:, 0], :, oi[:, 1], oi[:, 2], oi[:, 3]] = f2.double()
        dz.requires_grad_(True)
        wt = inv.weight.detach().cpu().double().permute(4, 0, 1, 2, 3).contiguous().requires_grad_(True)
        # (output_padding: the rows at the far edge that the symmetric crop of the transposed convolution drops)
        opad = [shape[j] - ((out.spatial_shape[j] - 1) * stride - 2 * padding[j] + ksize[j]) for j in range(3)]
        full = torch.nn.functional.conv_transpose3d(dz, wt, None, stride, padding, opad)
        assert list(full.shape[2:]) == shape
        want2 = full[ii[:, 0], :, ii[:, 1], ii[:, 2], ii[:, 3]]
        assert rel_err(back.features.detach().float().cpu().numpy(), want2.detach().numpy()) < tol
        d2 = rnd(torch.from_numpy(np.random.default_rng(2).uniform(-0.2, 0.2, tuple(want2.shape)).astype(np.float32)))
        want2.backward(d2.double())
        back.features.backward(d2.to(cuda, dt))
        din2 = dz.grad[oi[:, 0], :, oi[:, 1], oi[:, 2], oi[:, 3]]
        assert rel_err(g2.grad.float().cpu().numpy(), din2.numpy()) < tol
        assert rel_err(inv.weight.grad.float().cpu().numpy(), wt.grad.permute(1, 2, 3, 4, 0).numpy()) < tol
        assert _generic(L, dt) == gen0


@pytest.mark.gpu
@pytest.mark.parametrize("C,K", [(512, 512), (256, 512)])
def test_deferred_weight_gradient_of_a_wide_layer(cuda, C, K):
    """The weight gradient of a wide layer inside and outside deferred_wgrad(), sized by the real widths.
    (256, 512), 3.5 M weights: the second stage really is deferred to the end of the pass (spx_wgrad_stage2_batch, the
    counter is asserted) and writes the dW of the immediate one.  (512, 512), 7 M weights: NOTHING is deferred -- C > 256
    leaves ops.igemm_bwd for igemm_dgrad + igemm_wgrad before deferral is looked at, so the two passes run the same
    calls; that case shows that the context changes nothing and, with the fp64 check below, that dW of 512 x 27 x 512
    is right, not anything about the batched second stage."""
    import spconv_amd.pytorch as spconv
    from spconv_amd import _lib
    from spconv_amd.pytorch import ops
    L = _lib.load()
    shape, bs = [16, 16, 16], 2
    idx = scene(shape, 1500, bs, 9)
    torch.manual_seed(5)
    net = spconv.SubMConv3d(C, K, 3, bias=False, indice_key="m").to(cuda, F16)
    assert net.weight.numel() == C * 27 * K
    f = (torch.rand((idx.shape[0], C), device=cuda) * 2 - 1).half()
    d = ((torch.rand((idx.shape[0], K), device=cuda) * 2 - 1) * 0.2).half()
    grads = []
    for deferred in (False, True):
        net.zero_grad(set_to_none=True)
        x = spconv.SparseConvTensor(f.clone().requires_grad_(True), torch.from_numpy(idx).to(cuda), shape, bs)
        batch0 = L.spx_launch_count(b"wgrad_stage2_batch")
        if deferred:
            with ops.deferred_wgrad():
                net(x).features.backward(d)
        else:
            net(x).features.backward(d)
        torch.cuda.synchronize()
        if deferred and C in km.MFMA_COUT:      # (C = 512 takes dgrad + wgrad from Python: nothing to defer)
            assert L.spx_launch_count(b"wgrad_stage2_batch") == batch0 + 1
        grads.append((net.weight.grad.clone(), x.features.grad.clone()))
    assert tuple(grads[0][0].shape) == (K, 3, 3, 3, C)
    assert torch.equal(grads[0][0], grads[1][0]) and torch.equal(grads[0][1], grads[1][1])
    # ... and it is the gradient: against the fp64 pair reference
    out_idx, cand = km.pairs(idx, bs, shape, [3] * 3, [1] * 3, [1] * 3, [1] * 3, True, device=cuda)
    ref = km.conv_from_pairs(out_idx, cand, f.double(), net.weight.detach().double(), d.double())
    km._check(grads[1][0], ref.dW, ref.dW_abs, F16, "dW", (K, 3, 3, 3, C))
    km._check(grads[1][1], ref.din, ref.din_abs, F16, "din", (idx.shape[0], C))


# ------------------------------------------------------------------ 5. captured
def _wide_backbone(spconv, C, dev, dtype, norm512=True):
    """three levels, the last 512 wide.  norm512 = False: bias + ReLU behind the 512-wide layers instead of BatchNorm
    (training-mode statistics over a static-shape tensor exist up to 256 channels: csrc/norm.hip)"""
    torch.manual_seed(7)
    tail = (lambda: [nn.BatchNorm1d(512), nn.ReLU()]) if norm512 else (lambda: [nn.ReLU()])
    net = spconv.SparseSequential(
        spconv.SubMConv3d(C, 64, 3, bias=False, indice_key="s0"), nn.BatchNorm1d(64), nn.ReLU(),
        spconv.SparseConv3d(64, 256, 3, 2, 1, bias=False, indice_key="d1"), nn.BatchNorm1d(256), nn.ReLU(),
        spconv.SubMConv3d(256, 256, (3, 1, 3), bias=True, indice_key="s1"), nn.ReLU(),
        spconv.SparseConv3d(256, 512, 3, 2, 1, bias=not norm512, indice_key="d2"), *tail(),
        spconv.SubMConv3d(512, 512, 3, bias=not norm512, indice_key="s2"), *tail(),
    ).to(dev)
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, nn.BatchNorm1d):
                m.running_mean.uniform_(-0.2, 0.2)
                m.running_var.uniform_(0.5, 1.5)
                m.weight.uniform_(0.5, 1.5)
                m.bias.uniform_(-0.2, 0.2)
    return net.to(dtype)


@pytest.mark.gpu
def test_captured_inference_with_a_512_wide_stage(cuda):
    import spconv_amd.pytorch as spconv
    from spconv_amd import _lib
    from spconv_amd.pytorch.static import StaticInference, strided_layers
    from test_gpu_static import _scene_tensors
    L = _lib.load()
    shape, bs, C, dtype = [32, 40, 40], 2, 8, F16
    net = _wide_backbone(spconv, C, cuda, dtype).eval()
    names = list(strided_layers(net))
    eager = copy.deepcopy(net)
    gen0, w0 = _generic(L, dtype), L.spx_launch_count(b"igemm_v4w")
    runner = StaticInference(net, max_voxels=12_000, in_channels=C, spatial_shape=shape, batch_size=bs, dtype=dtype,
                             bounds={names[0]: 13_000, names[1]: 1_700})
    assert L.spx_launch_count(b"igemm_v4w") > w0
    for n, seed in ((4500, 1), (2001, 2), (5999, 3)):
        f, idx = _scene_tensors(shape, n, bs, C, seed, cuda, dtype)
        with torch.no_grad():
            want = eager(spconv.SparseConvTensor(f, idx, shape, bs))
        got = runner(f, idx)
        assert runner.overflowed() == {}, runner.counts()
        n_live = int((got.indices[:, 0] >= 0).sum())
        assert n_live == want.indices.shape[0] and want.features.shape[1] == 512
        assert torch.equal(got.indices[:n_live], want.indices)
        assert torch.equal(got.features[:n_live], want.features)
    assert _generic(L, dtype) == gen0


@pytest.mark.gpu
def test_captured_training_step_with_a_512_wide_stage(cuda):
    import spconv_amd.pytorch as spconv
    from spconv_amd import _lib
    from spconv_amd.pytorch.static import StaticTrainingStep, strided_layers
    from test_gpu_static import _scene_tensors
    L = _lib.load()
    shape, bs, C, dtype = [32, 40, 40], 2, 8, F16
    net = _wide_backbone(spconv, C, cuda, dtype, norm512=False).train()
    eager = copy.deepcopy(net)
    names = list(strided_layers(net))
    g0 = ((torch.rand((1_700, 512), device=cuda) - 0.5) * 0.2).half()
    g = g0.clone()
    scenes = [_scene_tensors(shape, n, bs, C, seed, cuda, dtype) for n, seed in ((4000, 1), (1500, 2), (5500, 3))]
    gen0 = _generic(L, dtype)
    step = StaticTrainingStep(net, 12_000, C, shape, bs, dtype, bounds={names[0]: 13_000, names[1]: 1_700},
                              out_grad=g, input_grad=True, example=scenes[0])
    for f, idx in scenes:
        eager.zero_grad(set_to_none=True)
        fe = f.clone().requires_grad_(True)
        ye = eager(spconv.SparseConvTensor(fe, idx, shape, bs))
        n_out = ye.features.shape[0]
        ye.features.backward(g0[:n_out])
        # the padding rows of the output carry no gradient, as a loss over the live rows leaves them (this network
        # does not end in a BatchNorm, which would zero them itself)
        g.copy_(g0)
        g[n_out:] = 0
        out = step(f, idx)
        assert step.overflowed() == {}
        assert int(out.n_live_dev) == n_out and torch.equal(out.indices[:n_out], ye.indices)
        # live rows against the eager pass, up to the summation order of the BatchNorm statistics of the first two
        # levels (the bound of test_static_training_step_with_subm_and_batchnorm)
        assert out.features.shape[1] == 512
        err = float((out.features[:n_out].float() - ye.features.detach().float()).abs().max())
        assert err <= 2e-2 * float(ye.features.detach().float().abs().max()), err
        for (name, pa), pb in zip(net.named_parameters(), eager.parameters()):      # (the criterion of test_gpu_static.py)
            rel = float((pa.grad.float() - pb.grad.float()).norm() / pb.grad.float().norm().clamp_min(1e-12))
            assert rel < 3e-2, (name, rel)
        rel = float((step.features.grad[:f.shape[0]].float() - fe.grad.float()).norm() / fe.grad.float().norm())
        assert rel < 3e-2, rel
    assert _generic(L, dtype) == gen0


# ------------------------------------------------------------------ 6. conv + BatchNorm at 512 channels
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [F16, F32], ids=["f16", "f32"])
def test_conv_batchnorm_512_takes_the_empty_sink_fallback(cuda, dtype):
    import spconv_amd.pytorch as spconv
    from spconv_amd.pytorch import norm, ops
    shape, bs, C, K = [16, 16, 16], 2, 64, 512
    idx = scene(shape, 1500, bs, 4)
    torch.manual_seed(11)
    conv = spconv.SubMConv3d(C, K, 3, bias=False, indice_key="m")
    bn = nn.BatchNorm1d(K)
    seq = spconv.SparseSequential(conv, bn).to(cuda, dtype).train()
    one = copy.deepcopy(seq)
    f = (torch.rand((idx.shape[0], C), device=cuda) * 2 - 1).to(dtype)
    ind = torch.from_numpy(idx).to(cuda)
    got = seq(spconv.SparseConvTensor(f, ind, shape, bs))
    # the same layers called one by one: the convolution inside the statistics context leaves the sink empty ...
    with ops.collect_bn_stats() as sink:
        y = one[0](spconv.SparseConvTensor(f, ind, shape, bs))
    assert sink.records is None and sink.count == 0
    # ... and the normalisation layer runs its own pass
    if norm.supported(y.features, one[1]):
        z = norm.batch_norm(y.features, one[1], relu=False, n_live=None, stats=None)
    else:
        z = one[1](y.features)
    assert torch.equal(got.features, z)
    assert torch.equal(seq[1].running_mean, one[1].running_mean) and torch.equal(seq[1].running_var, one[1].running_var)
    assert float(got.features.detach().float().abs().max()) > 0
