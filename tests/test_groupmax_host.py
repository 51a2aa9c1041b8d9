"""Fused set abstraction without a GPU (spconv_amd/pytorch/_groupmax.py): every refusal names its argument and comes
before the refusal of CPU tensors; the entry points are declared and exported; the module carries its parameters."""
import pytest
import torch

from spconv_amd import _lib


def call(dtype=torch.float16, Cin=32, Cout=16, S=8, offsets=True, weight=None, pos_weight=None, in_bias=None, grad=False,
         feats=None):
    from spconv_amd.pytorch import functional as F
    M, n = 4, 6
    nb = F.VoxelNeighbors(torch.zeros((M, S), dtype=torch.int32), torch.zeros((M,), dtype=torch.int32),
                          torch.zeros((M, S, 3)) if offsets else None, None, n)
    feats = torch.zeros((n, Cin), dtype=dtype, requires_grad=grad) if feats is None else feats
    weight = torch.zeros((Cin, Cout), dtype=dtype) if weight is None else weight
    return F.group_linear_max(feats, nb, weight, pos_weight, in_bias)


@pytest.mark.parametrize("kwargs,error,match", [
    (dict(dtype=torch.float32), NotImplementedError, "feats must be float16 or bfloat16"),
    (dict(feats=torch.zeros((5, 32), dtype=torch.float16)), ValueError, "feats holds one row per voxel"),
    (dict(Cin=24), NotImplementedError, r"Cin \(feats\) must be a multiple of 16"),
    (dict(Cout=272), NotImplementedError, r"Cout \(weight\) must be a multiple of 16 in 16 .. 256"),
    (dict(S=129), ValueError, r"nsample \(nb.rows\) must be in 1 .. 128"),
    (dict(weight=torch.zeros((32, 16), dtype=torch.bfloat16)), ValueError, "weight is"),
    (dict(weight=torch.zeros((16, 16), dtype=torch.float16)), ValueError, "weight is"),
    (dict(pos_weight=torch.zeros((3, 32)), offsets=False), ValueError, "pos_weight needs nb.offsets"),
    (dict(pos_weight=torch.zeros((3, 16))), ValueError, "pos_weight is float32"),
    (dict(pos_weight=torch.zeros((3, 32), dtype=torch.float16)), ValueError, "pos_weight is float32"),
    (dict(in_bias=torch.zeros((16,))), ValueError, "in_bias is float32"),
    (dict(grad=True), ValueError, "a gradient needs the neighbour groups"),
], ids=["f32", "feats-rows", "cin24", "cout272", "s129", "weight-dtype", "weight-shape", "no-offsets", "pos-shape", "pos-dtype",
        "bias-shape", "no-groups"])
def test_refusals_name_the_argument(kwargs, error, match):
    with pytest.raises(error, match=match):
        call(**kwargs)


def test_cpu_tensors_are_refused_last():
    with pytest.raises(NotImplementedError, match="feats is on cpu"):
        call(pos_weight=torch.zeros((3, 32)), in_bias=torch.zeros((32,)))


def test_declared_and_exported():
    import spconv_amd.pytorch as spconv
    decl = _lib.parse_header(open(_lib.HEADER_PATH).read())
    assert {"spx_group_linear_max_fwd", "spx_group_linear_max_bwd", "spx_group_linear_max_ws_bytes"} <= set(decl)
    for name in ("group_linear_max", "group_linear_max_into", "group_linear_max_bwd_into", "group_linear_max_ws_bytes",
                 "GroupLinearMaxFunction"):
        assert hasattr(spconv.functional, name), name
    assert spconv.group_linear_max is spconv.functional.group_linear_max
    layer = spconv.GroupLinearMax(32, 64)
    shapes = {k: (tuple(v.shape), v.dtype) for k, v in layer.state_dict().items()}
    assert shapes == {"weight": ((32, 64), torch.float32), "pos_weight": ((3, 32), torch.float32),
                      "in_bias": ((32,), torch.float32)}
    assert list(spconv.GroupLinearMax(16, 16, use_xyz=False).state_dict()) == ["weight"]
    with pytest.raises(NotImplementedError, match="in_channels must be a multiple of 16"):
        spconv.GroupLinearMax(20, 16)
