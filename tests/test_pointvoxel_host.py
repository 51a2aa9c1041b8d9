"""CPU: the argument checks of the point <-> voxel entry points (csrc/pointvoxel.hip) come before any pointer is looked
at (no kernel is launched in this file); the Python layer has the new names.  (Declared, exported and bound as
declared: test_capi.py, for the whole header.)"""
import ctypes
import inspect

import pytest

from capi import fails as _fails
from spconv_amd import _lib


def test_ws_bytes_is_monotone_and_rejects_bad_sizes():
    L = _lib.load()
    assert L.spx_point_groups_ws_bytes(-1, 10) == 0 and L.spx_point_groups_ws_bytes(10, 0) == 0
    assert L.spx_point_groups_ws_bytes(10, -3) == 0
    assert L.spx_point_groups_ws_bytes(0, 1) > 0
    ns, vs = (0, 1, 511, 512, 513, 5000, 300_000, 2_000_000), (1, 2, 255, 256, 257, 700, 150_000, 1 << 30)
    for v in vs:
        sizes = [L.spx_point_groups_ws_bytes(n, v) for n in ns]
        assert sizes == sorted(sizes) and sizes[-1] > 5 * 4 * ns[-1], (v, sizes)      # keys + the sort's four buffers
    for n in ns:
        sizes = [L.spx_point_groups_ws_bytes(n, v) for v in vs]
        assert sizes == sorted(sizes) and sizes[0] > 0, (n, sizes)


def test_argument_checks_need_no_pointer():
    L = _lib.load()
    groups = lambda id_bytes, n, nv: L.spx_point_groups(None, id_bytes, n, None, nv, None, None, None, None, 0, None)
    _fails(groups(2, 10, 5), "id_bytes")
    _fails(groups(16, 10, 5), "id_bytes")
    _fails(groups(8, -1, 5), "point count")
    _fails(groups(8, 10, 0), "num_voxels")
    _fails(groups(4, 10, -2), "num_voxels")
    _fails(groups(8, 10, 5), "NULL")
    gather = lambda nv, n, C, eb: L.spx_voxel_to_point(None, nv, None, n, C, eb, 0, None, None)
    _fails(gather(5, 10, 4, 3), "elem_bytes")
    _fails(gather(5, 10, 4, 16), "elem_bytes")
    _fails(gather(5, 10, 0, 2), "channel count")
    _fails(gather(5, -1, 4, 2), "row counts")
    _fails(gather(-1, 10, 4, 2), "row counts")
    assert gather(5, 0, 4, 2) == 0                  # no points: nothing to do
    _fails(gather(5, 10, 4, 2), "NULL")
    f3, f6 = (ctypes.c_float * 3)(1, 1, 1), (ctypes.c_float * 6)(0, 0, 0, 1, 1, 1)
    deco = lambda nfeat, n, ndim, flags, dt, C: L.spx_point_decorate(None, nfeat, n, None, None, ndim, f3, f6, None, flags,
                                                                     None, dt, C, None)
    _fails(deco(4, 10, 5, 3, _lib.DTYPE_F32, 10), "ndim")
    _fails(deco(2, 10, 3, 3, _lib.DTYPE_F32, 10), "columns")
    _fails(deco(4, 10, 3, 4, _lib.DTYPE_F32, 10), "flags")
    _fails(deco(4, 10, 3, 3, _lib.DTYPE_F64, 10), "out_dtype")
    _fails(deco(4, 10, 3, 3, _lib.DTYPE_I8, 10), "out_dtype")
    _fails(deco(4, 10, 3, 3, _lib.DTYPE_F16, 9), "narrower")
    _fails(deco(4, 10, 3, 1, _lib.DTYPE_F16, 6), "narrower")
    _fails(deco(4, -1, 3, 3, _lib.DTYPE_F16, 10), "point count")
    assert deco(4, 0, 3, 3, _lib.DTYPE_F16, 10) == 0
    _fails(deco(4, 10, 3, 3, _lib.DTYPE_F16, 10), "NULL")


def test_launch_counter_keys():
    L = _lib.load()
    for key in ("pointvoxel/groups", "pointvoxel/gather", "pointvoxel/decorate"):
        assert L.spx_launch_count(key.encode()) >= 0, key
    for bad in ("pointvoxel", "pointvoxel/", "pointvoxel/reduce"):
        assert L.spx_launch_count(bad.encode()) == -1, bad


def test_python_argument_checks():
    import torch
    from spconv_amd.pytorch import functional as F
    from spconv_amd.pytorch.vfe import DynamicVFE
    rows = torch.zeros((6,), dtype=torch.int32)
    g = F.PointGroups(rows, torch.zeros((4,), dtype=torch.int32), rows.clone(), 3)
    assert g.n_points is None and g.n_live is None and g.n_out == 3
    with pytest.raises(ValueError, match="reduce"):
        F.points_to_voxels(torch.zeros((6, 4)), g, "min")
    with pytest.raises(NotImplementedError, match="MI355X"):
        F.points_to_voxels(torch.zeros((6, 4)), g, "max")
    with pytest.raises(NotImplementedError, match="MI355X"):
        F.point_groups(torch.zeros((6,), dtype=torch.int64), 3)
    with pytest.raises(ValueError, match="reduce"):
        DynamicVFE(4, (8,), reduce="median")
    with pytest.raises(ValueError, match="channels"):
        DynamicVFE(4, ())
    vfe = DynamicVFE(5, (8, 16), ndim=3, with_center=False)
    assert vfe.in_channels == 8 and vfe.out_channels == 16
    assert [(l.in_features, l.out_features, l.bias is None) for l in vfe.linears] == [(8, 8, True), (16, 16, True)]
    assert DynamicVFE(4, (8,), norm=False).linears[0].bias is not None


def test_new_names_and_signatures():
    import spconv_amd
    import spconv_amd.pytorch as sp
    from spconv_amd.pytorch.static import StaticInference
    from spconv_amd.pytorch.utils import StaticPointToVoxel
    for name in ("DynamicVFE", "point_groups", "points_to_voxels", "voxels_to_points"):
        assert callable(getattr(sp, name)), name
    for name in ("PointGroups", "point_groups", "points_to_voxels", "voxels_to_points", "decorate_points"):
        assert hasattr(sp.functional, name), name
    assert inspect.signature(sp.functional.points_to_voxels).parameters["reduce"].default == "max"
    assert inspect.signature(sp.functional.voxels_to_points).parameters["invalid_value"].default == 0
    deco = inspect.signature(sp.functional.decorate_points).parameters
    assert deco["cluster"].default is True and deco["center"].default is True and deco["pad_to"].default is None
    assert callable(StaticPointToVoxel.point_groups)
    assert inspect.signature(StaticInference.__init__).parameters["point_encoder"].default is None
    assert "not part of the reference" in " ".join(sp.DynamicVFE.__doc__.lower().split())
    spconv_amd.install_as_spconv()
    import spconv.pytorch as spconv
    for name in ("DynamicVFE", "point_groups", "points_to_voxels", "voxels_to_points"):
        assert getattr(spconv, name) is getattr(sp, name), name
    import spconv.pytorch.vfe as vfe
    assert vfe.DynamicVFE is sp.DynamicVFE
