"""CPU: the host side of serialised patch attention (csrc/attn.hip, pytorch/_attn.py) -- the three entry points, the
workspace query and every refusal, all of which come before any launch (nothing here touches a GPU)."""
import pytest
import torch

from spconv_amd import _lib
from spconv_amd.pytorch import functional as F


@pytest.fixture(scope="module")
def lib():
    if not __import__("os").path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


NAMES = ("spx_patch_attn_ws_bytes", "spx_patch_attn_fwd", "spx_patch_attn_bwd")


def test_entry_points_are_declared_and_exported(lib):
    for name in NAMES:
        assert name in _lib.signatures() and getattr(lib, name).argtypes == _lib.signatures()[name][1]
    assert len(_lib.signatures()["spx_patch_attn_fwd"][1]) == 15 and len(_lib.signatures()["spx_patch_attn_bwd"][1]) == 20


def test_workspace_query_and_c_refusals(lib):
    sizes = [int(lib.spx_patch_attn_ws_bytes(n, n // 128 + 4, 128, 4, 16)) for n in (0, 1, 1000, 400_000)]
    assert sizes[0] > 0 and sizes == sorted(sizes) and sizes[3] >= (400_000 // 128 + 4) * 128 * 2 * 64 * 4
    for args in ((-1, 4, 128, 4, 16), (100, 4, 48, 4, 16), (100, 4, 0, 4, 16), (100, 4, 128, 0, 16), (100, 4, 128, 4, 48),
                 (100, 2 ** 24, 128, 4, 16)):
        assert lib.spx_patch_attn_ws_bytes(*args) == 0, args
    fwd = lambda n=8, P=2, K=32, H=1, D=16, dt=_lib.DTYPE_F16: lib.spx_patch_attn_fwd(
        None, None, None, None, None, n, P, K, H, D, dt, 1.0, None, None, None)
    for kw, word in ((dict(D=48), "head size"), (dict(K=48), "multiple of 32"), (dict(dt=_lib.DTYPE_F32), "f16 or bf16"),
                     (dict(n=-1), "bad sizes"), (dict(P=2 ** 27), "2^31"), (dict(), "null")):
        assert fwd(**kw) != 0 and word.encode() in lib.spx_last_error(), kw
    assert fwd(n=0) == 0                                         # nothing to do: no pointer is needed
    assert lib.spx_patch_attn_bwd(*([None] * 9), 8, 2, 32, 1, 16, _lib.DTYPE_I8, 1.0, None, None, 0, None) != 0


def _plan(n=40, K=32, P_cap=3):
    i32 = dict(dtype=torch.int32)
    return F.PatchPlan(torch.zeros((P_cap, K), **i32), torch.zeros((P_cap, K), **i32), torch.zeros((n,), **i32),
                       torch.zeros((n,), **i32), torch.zeros((P_cap,), **i32), torch.zeros((1,), **i32), K, "borrow")


def test_every_refusal_is_raised_before_any_launch():
    plan, half = _plan(), torch.zeros((40, 3 * 2 * 16), dtype=torch.float16)
    with pytest.raises(NotImplementedError, match="MI355X"):
        F.patch_attention(half, plan, 2)                                           # everything else is in order: CPU rows
    with pytest.raises(NotImplementedError, match=r"\[16, 32, 64\]"):
        F.patch_attention(torch.zeros((40, 3 * 2 * 24), dtype=torch.float16), plan, 2)
    with pytest.raises(NotImplementedError, match=r"\[16, 32, 64\]"):
        F.patch_attention(torch.zeros((40, 3, 2, 128), dtype=torch.float16), plan, 2)
    with pytest.raises(ValueError, match="multiple of 32"):
        F.patch_attention(half, _plan(K=48), 2)
    for dtype in (torch.float32, torch.float64):
        with pytest.raises(NotImplementedError, match="float16 or bfloat16"):
            F.patch_attention(half.to(dtype), plan, 2)
    with pytest.raises(ValueError, match="one row per voxel"):
        F.patch_attention(half[:39], plan, 2)
    with pytest.raises(ValueError, match="contiguous int32"):
        F.patch_attention(half, plan._replace(patch_rows=torch.zeros((32, 3), dtype=torch.int32).t()), 2)
    with pytest.raises(ValueError, match="contiguous"):
        F.patch_attention(torch.zeros((40, 2 * 96), dtype=torch.float16)[:, ::2], plan, 2)
    for shape in ((40, 3 * 2 * 16 + 1), (40, 2, 2, 16), (40, 3, 3, 16)):
        with pytest.raises(ValueError, match="qkv is"):
            F.patch_attention(torch.zeros(shape, dtype=torch.float16), plan, 2)
    with pytest.raises(ValueError, match="num_heads"):
        F.patch_attention(half, plan, 0)


def test_module_is_exported_and_checks_its_head_size():
    import spconv_amd.pytorch as spconv
    m = spconv.PatchAttention(64, 4, qkv_bias=False, proj=False)
    assert m.qkv.weight.shape == (192, 64) and m.qkv.bias is None and m.proj is None
    assert spconv.PatchAttention(64, 4).proj.weight.shape == (64, 64)
    with pytest.raises(NotImplementedError, match=r"\[16, 32, 64\]"):
        spconv.PatchAttention(96, 4)
    with pytest.raises(ValueError, match="multiple of num_heads"):
        spconv.PatchAttention(64, 3)
