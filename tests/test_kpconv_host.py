"""Kernel point convolution without a GPU (spconv_amd/pytorch/_kpconv.py): every refusal names its argument and comes
before the refusal of CPU tensors; the entry points are declared and exported; the module carries KPConv's weight."""
import pytest
import torch

from spconv_amd import _lib


def call(dtype=torch.float16, Cin=32, Cout=16, K=15, S=8, offsets=True, weight=None, kernel_points=None, grad=False,
         groups=None):
    from spconv_amd.pytorch import functional as F
    M, n = 4, 6
    nb = F.VoxelNeighbors(torch.zeros((M, S), dtype=torch.int32), torch.zeros((M,), dtype=torch.int32),
                          torch.zeros((M, S, 3)) if offsets else None, groups, n)
    feats = torch.zeros((n, Cin), dtype=dtype, requires_grad=grad)
    weight = torch.zeros((K, Cin, Cout), dtype=dtype) if weight is None else weight
    kernel_points = torch.zeros((K, 3)) if kernel_points is None else kernel_points
    return F.kpconv(feats, nb, kernel_points, weight, 0.5)


@pytest.mark.parametrize("kwargs,error,match", [
    (dict(dtype=torch.float32), NotImplementedError, "feats must be float16 or bfloat16"),
    (dict(Cin=24), NotImplementedError, r"Cin \(feats\) must be a multiple of 16"),
    (dict(K=17), NotImplementedError, r"K \(weight, kernel_points\) must be in 1 .. 16"),
    (dict(S=129), ValueError, r"nsample \(nb.rows\) must be in 1 .. 128"),
    (dict(offsets=False), ValueError, "nb.offsets is missing"),
    (dict(weight=torch.zeros((15, 32, 16), dtype=torch.bfloat16)), ValueError, "weight is"),
    (dict(weight=torch.zeros((15, 16, 16), dtype=torch.float16)), ValueError, "weight is"),
    (dict(kernel_points=torch.zeros((15, 3), dtype=torch.float64)), ValueError, "kernel_points is float32"),
    (dict(kernel_points=torch.zeros((14, 3))), ValueError, "kernel_points is float32"),
    (dict(grad=True), ValueError, "a gradient needs the neighbour groups"),
], ids=["f32", "cin24", "k17", "s129", "no-offsets", "weight-dtype", "weight-shape", "kp-dtype", "kp-shape", "no-groups"])
def test_refusals_name_the_argument(kwargs, error, match):
    with pytest.raises(error, match=match):
        call(**kwargs)


def test_cpu_tensors_are_refused_last():
    with pytest.raises(NotImplementedError, match="feats is on cpu"):
        call()


def test_declared_and_exported():
    import spconv_amd.pytorch as spconv
    decl = _lib.parse_header(open(_lib.HEADER_PATH).read())
    assert {"spx_kpconv_fwd", "spx_kpconv_bwd", "spx_kpconv_ws_bytes"} <= set(decl)
    for name in ("kpconv", "kpconv_into", "kpconv_bwd_into", "kpconv_ws_bytes", "KPConvFunction"):
        assert hasattr(spconv.functional, name), name
    layer = spconv.KPConv(32, 64, sigma=0.3, kp_radius=0.5, normalize=True)
    assert tuple(layer.weight.shape) == (15, 32, 64) and "kernel_points" in dict(layer.named_buffers())
    assert "weight" in layer.state_dict() and "kernel_points" in layer.state_dict()
    kp = layer.kernel_points
    assert kp.dtype == torch.float32 and torch.equal(kp[0], torch.zeros(3))
    torch.testing.assert_close(kp[1:].norm(dim=1), torch.full((14,), 0.5))
    assert torch.equal(kp, spconv.KPConv(16, 16, 0.3, kp_radius=0.5).kernel_points)         # deterministic
    assert tuple(spconv.KPConv(16, 16, 0.3, kernel_points=torch.rand(7, 3)).weight.shape) == (7, 16, 16)
