"""CPU: the shape rule of BatchNorm beyond 256 channels (csrc/norm.hip runs wide matrices over column blocks of 256
channels).  Through the C ABI as test_capi.py loads it, with n = 0 -- the shape check precedes the early return and no
kernel is launched in this file -- and through norm.shape_supported, which states the same rule on the Python side."""
import ctypes

import pytest
import torch

from spconv_amd import _lib

DT = {"f16": (_lib.DTYPE_F16, torch.float16), "bf16": (_lib.DTYPE_BF16, torch.bfloat16),
      "f32": (_lib.DTYPE_F32, torch.float32)}
WIDE_SHAPES = [(25_000, 512), (6_000, 512), (25_000, 384), (12_000, 1024), (64, 2048), (300, 320), (2_000_000, 2048)]


@pytest.fixture(scope="module")
def lib():
    import os
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


def _fwd(lib, C, dt, training=1):
    return lib.spx_batchnorm_fwd(None, None, 0, C, dt, None, None, None, None, None, _lib.DTYPE_F32, training, 0.1, 1e-5,
                                 1, None, None, None, 0, None, None)


def _bwd(lib, C, dt):
    stat = (ctypes.c_float * 4)()              # mean / invstd must be given; nothing reads them at n = 0
    p = ctypes.cast(stat, ctypes.c_void_p)
    return lib.spx_batchnorm_bwd(None, None, None, 0, C, dt, None, None, _lib.DTYPE_F32, p, p, 1, 1, None, None, None,
                                 0, None, None)


@pytest.mark.parametrize("name", ["f16", "bf16", "f32"])
def test_an_empty_512_wide_matrix_is_accepted(lib, name):
    dt = DT[name][0]
    assert _fwd(lib, 512, dt) == 0, lib.spx_last_error()
    assert _fwd(lib, 512, dt, training=0) == 0, lib.spx_last_error()
    assert _bwd(lib, 512, dt) == 0, lib.spx_last_error()


def test_refusals_that_stay(lib):
    for name in ("f16", "bf16"):
        assert _fwd(lib, 516, DT[name][0]) != 0 and b"multiple of 8" in lib.spx_last_error()
        assert _bwd(lib, 516, DT[name][0]) != 0
    assert _fwd(lib, 516, _lib.DTYPE_F32) == 0 and _bwd(lib, 516, _lib.DTYPE_F32) == 0
    for name in DT:
        assert _fwd(lib, 0, DT[name][0]) != 0 and _bwd(lib, 0, DT[name][0]) != 0
        assert _fwd(lib, -8, DT[name][0]) != 0
    assert _fwd(lib, 512, _lib.DTYPE_I8) != 0 and _fwd(lib, 512, _lib.DTYPE_F64) != 0


def test_the_cap_is_named_where_it_is_kept(lib):
    """the widest matrix the kernels take: the same number in norm.py, in the error message and in the header"""
    import os
    from spconv_amd.pytorch import norm
    cap = norm.MAX_CHANNELS
    assert cap >= 2048
    for name in DT:
        assert _fwd(lib, cap, DT[name][0]) == 0 and _bwd(lib, cap, DT[name][0]) == 0
        assert _fwd(lib, cap + 8, DT[name][0]) != 0 and str(cap).encode() in lib.spx_last_error()
        assert _bwd(lib, cap + 8, DT[name][0]) != 0 and str(cap).encode() in lib.spx_last_error()
        assert norm.shape_supported(cap, DT[name][1]) and not norm.shape_supported(cap + 8, DT[name][1])
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert f"C <= {cap}" in open(os.path.join(root, "include", "spconv_amd.h")).read()


@pytest.mark.parametrize("C", [8, 256, 264, 320, 384, 512, 516, 1024, 2048])
@pytest.mark.parametrize("name", ["f16", "bf16", "f32"])
def test_shape_rule_agrees_with_the_abi(lib, C, name):
    from spconv_amd.pytorch import norm
    dt, tdt = DT[name]
    ok = norm.shape_supported(C, tdt)
    assert ok == (C % (4 if name == "f32" else 8) == 0)
    assert (_fwd(lib, C, dt) == 0) == ok
    assert (_bwd(lib, C, dt) == 0) == ok
    assert not norm.shape_supported(C, torch.float64) and not norm.shape_supported(0, tdt)


@pytest.mark.parametrize("n,C", WIDE_SHAPES)
def test_workspace_holds_the_records_of_every_column_block(lib, n, C):
    """3 floats per channel and row block (forward records; the backward pass keeps 2) + the [2][C] sums, computed in
    size_t; also at the largest row count and width the entry points take"""
    blocks = min(max((n + 63) // 64, 1), 1024)            # bn_blocks(n): depends on n only
    need = ((3 * blocks + 2) * C) * 4
    got = lib.spx_batchnorm_ws_bytes(n, C)
    assert need <= got <= need + 512
    from spconv_amd.pytorch import norm
    top = lib.spx_batchnorm_ws_bytes(2**31 - 1, norm.MAX_CHANNELS)
    assert top >= ((3 * 1024 + 2) * norm.MAX_CHANNELS) * 4 and top == lib.spx_batchnorm_ws_bytes(65_536, norm.MAX_CHANNELS)
