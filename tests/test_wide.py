"""Layers wider than 256 channels, host side: the padding rule and the instance keys of the column-blocked launches
(csrc/igemm_wide.hip).  Nothing here launches a kernel."""
import pytest
import torch

from spconv_amd.pytorch._gemm import _padded_ck

F16, BF16, F32, F64, I8 = torch.float16, torch.bfloat16, torch.float32, torch.float64, torch.int8

# (width asked for, width run): beyond 256 the next multiple of the 128-column block
WIDE = [(257, 384), (320, 384), (384, 384), (500, 512), (512, 512), (640, 640)]
# reduction length 40 in whole 16-byte lane pieces
RED40 = {F16: 40, F32: 40, I8: 48}


@pytest.mark.parametrize("dtype", [F16, F32, I8])
@pytest.mark.parametrize("asked,run", WIDE)
def test_wide_widths_round_to_column_blocks(dtype, asked, run):
    _padded_ck.cache_clear()
    assert _padded_ck(dtype, "fwd", 40, asked, 27) == (RED40[dtype], run)
    assert _padded_ck(dtype, "fwd", 64, asked, 125 if dtype != I8 else 27) == (64, run)
    if dtype != I8:                                     # (int8 is forward only)
        assert _padded_ck(dtype, "dgrad", asked, 40, 27) == (run, RED40[dtype])
        assert _padded_ck(dtype, "dgrad", asked, 64, 8) == (run, 64)


# (dtype, role, C0, K0, kv) -> (C, K): the values of the rule before wide layers existed, written out
NARROW = [
    ((F16, "fwd", 3, 16, 27), (8, 16)),
    ((F16, "fwd", 64, 64, 27), (64, 64)),
    ((F16, "fwd", 40, 200, 27), (40, 256)),
    ((F16, "fwd", 17, 129, 8), (24, 256)),
    ((BF16, "fwd", 5, 48, 27), (8, 64)),
    ((BF16, "fwd", 256, 256, 1), (256, 256)),
    ((F16, "dgrad", 48, 20, 27), (64, 24)),
    ((F16, "dgrad", 256, 256, 27), (256, 256)),
    ((BF16, "dgrad", 130, 12, 125), (256, 16)),
    ((F32, "fwd", 3, 24, 27), (4, 32)),
    ((F32, "fwd", 16, 129, 27), (16, 256)),
    ((F32, "dgrad", 100, 6, 125), (128, 8)),
    ((I8, "fwd", 16, 48, 27), (16, 64)),
    ((I8, "fwd", 20, 256, 27), (32, 256)),
    ((I8, "fwd", 64, 5, 8), (64, 16)),
    # kernel volumes beyond 128: the generic kernel, every width as it is
    ((F16, "fwd", 5, 12, 343), (8, 12)),
    ((F16, "fwd", 16, 300, 343), (16, 300)),
    ((F32, "dgrad", 300, 6, 216), (300, 8)),
    # the weight gradient: lane multiples on both sides, at every width
    ((F16, "wgrad", 5, 7, 27), (8, 8)),
    ((F16, "wgrad", 512, 300, 27), (512, 304)),
    ((F32, "wgrad", 130, 6, 27), (132, 8)),
    # float64 runs every shape as it is
    ((F64, "fwd", 5, 300, 27), (5, 300)),
    ((F64, "dgrad", 300, 7, 27), (300, 7)),
]


@pytest.mark.parametrize("args,want", NARROW, ids=[f"{a[1]}-{str(a[0])[6:]}-{a[2]}-{a[3]}-{a[4]}" for a, _ in NARROW])
def test_shapes_up_to_256_keep_their_padding(args, want):
    _padded_ck.cache_clear()
    assert _padded_ck(*args) == want


def wide_keys():
    """Every instance of the column-blocked launch (igemm_wide.hip launch_v4w): 128-column tiles; 16-bit types with the
    (NKS, PK) forms (2, 1), (1, 1), (1, 2), (1, 4), fp32 with (2, 1), (1, 1), forward and dgrad; int8 forward only."""
    keys = []
    for dt in ("f16", "bf16"):
        for d in ("fwd", "bt"):
            for nks, pk in ((2, 1), (1, 1), (1, 2), (1, 4)):
                keys.append(f"igemm_v4w/128/{dt}/{d}/{nks}/{pk}")
    for d in ("fwd", "bt"):
        for nks in (1, 2):
            keys.append(f"igemm_v4w/128/f32/{d}/{nks}/1")
    for nks in (1, 2):
        keys.append(f"igemm_v4w/128/i8/fwd/{nks}/1")
    return keys


def test_wide_instance_keys_parse():
    from spconv_amd import _lib
    L = _lib.load()
    keys = wide_keys()
    assert len(keys) == 22 and len(set(keys)) == 22
    for k in keys:
        assert L.spx_launch_count(k.encode()) >= 0, k
    assert L.spx_launch_count(b"igemm_v4w") >= 0
    for bad in ("igemm_v4w/256/f16/fwd/2/1",          # the tile is 128 columns wide
                "igemm_v4w/64/f16/fwd/2/1",
                "igemm_v4w/128/1/f16/fwd/2/1",        # no tile-height field in this family
                "igemm_v4w/128/f16/fwd/2",
                "igemm_v4w/128/f16/up/2/1",
                "igemm_v4w/128/f64/fwd/2/1",
                "igemm_v4w/128/f16/fwd/3/1",
                "igemm_v4w/128/f16/fwd/2/2",          # offset packing belongs to one-piece rows
                "igemm_v4w/128/f16/fwd/2/8",
                "igemm_v4w/128/f16/fwd/1/8",
                "igemm_v4w/128/f32/fwd/1/2",          # ... of a 16-bit type
                "igemm_v4w/128/i8/fwd/1/4",
                "igemm_v4w/128/i8/bt/2/1",            # int8 is forward only
                "igemm_v4w/", "igemm_v4w//f16/fwd/2/1"):
        assert L.spx_launch_count(bad.encode()) == -1, bad


def test_int8_entry_refuses_widths_that_are_no_column_block_multiple():
    """spx_igemm_fwd_int8 itself takes 16 / 32 / 64 / 128 / 256 or a multiple of 128 beyond (the drivers pad); the check
    comes before anything is read or launched, so the pointers here are never followed."""
    import ctypes
    from spconv_amd import _lib
    L = _lib.load()
    p = ctypes.c_void_p(64)

    def call(K):
        return L.spx_igemm_fwd_int8(p, p, p, p, None, None, 10, 10, 64, K, 27, 13, None, None, None, 0.0, _lib.DTYPE_I8, 0,
                                    0.0, None)
    for K in (320, 257, 600):
        assert call(K) != 0
        msg = L.spx_last_error().decode()
        assert "multiple of 128" in msg and str(K) in msg, msg
    assert call(48) != 0 and "out_channels" in L.spx_last_error().decode()


def test_narrow_key_grammar_is_unchanged():
    """The keys of the <= 256-wide instances neither gain nor lose a field, and no wide width slips into them."""
    from spconv_amd import _lib
    L = _lib.load()
    for k in ("igemm_v4/256/1/f16/fwd/2/1", "igemm_v4/128/1/bf16/bt/1/2", "igemm_v4/64/2/i8/fwd/2/1", "gen1/256/f16",
              "generic/f32"):
        assert L.spx_launch_count(k.encode()) >= 0, k
    for bad in ("igemm_v4/512/1/f16/fwd/2/1", "igemm_v4/384/1/f16/fwd/2/1", "gen1/512/f16", "igemm_bwd/512/2/f16/2/1"):
        assert L.spx_launch_count(bad.encode()) == -1, bad
