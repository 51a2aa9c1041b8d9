"""CPU: the argument checks of the trilinear-devoxelisation entry points (csrc/interp.hip) come before any pointer is
looked at (no kernel is launched in this file); the Python layer has the new names.  (Declared, exported and bound as
declared: test_capi.py, for the whole header.)"""
import ctypes
import inspect

import pytest

from capi import fails as _fails
from spconv_amd import _lib


def test_ws_bytes_is_monotone_and_rejects_bad_sizes():
    ws = _lib.load().spx_point_corners_ws_bytes
    assert ws(-1, 3, 10) == 0 and ws(10, 3, -1) == 0
    assert ws(10, 1, 10) == 0 and ws(10, 4, 10) == 0
    assert ws(1 << 28, 3, 10) == 0 and ws((1 << 28) - 1, 3, 10) > 0         # n_cap * 8 >= 2^31
    assert ws(1 << 29, 2, 10) == 0 and ws((1 << 29) - 1, 2, 10) > 0         # n_cap * 4 >= 2^31
    assert ws(0, 3, 0) > 0
    assert ws(10, 3, (1 << 30) + 1) == 0 and ws(10, 3, 1 << 30) >= 8 * (1 << 31)      # two slots per row fit 32 bits
    caps, ns = (0, 1, 5000, 300_000, (1 << 28) - 1), (0, 1, 127, 128, 129, 255, 256, 257, 700, 150_000, 2_000_000, 1 << 30)
    for ndim in (2, 3):
        for cap in caps:
            sizes = [ws(cap, ndim, n) for n in ns]
            assert sizes == sorted(sizes) and sizes[0] > 0, (cap, sizes)
            assert sizes[-1] >= 2 * 8 * ns[-1]                                 # a table of at least two slots per row
        for n in ns:
            sizes = [ws(cap, ndim, n) for cap in caps]
            assert sizes == sorted(sizes), (n, sizes)
    for cap in caps:
        for n in ns:
            assert ws(cap, 2, n) <= ws(cap, 3, n)


def test_argument_checks_need_no_pointer():
    L = _lib.load()
    f3, f6, i3 = (ctypes.c_float * 3)(1, 1, 1), (ctypes.c_float * 6)(0, 0, 0, 1, 1, 1), _lib.ints([4, 4, 4])

    def corners(nfeat, n_cap, ndim, n, batch, flags, vsize=f3, rng=f6, shape=i3):
        return L.spx_point_corners(None, nfeat, None, n_cap, None, ndim, vsize, rng, None, n, None, batch, shape, None, 0,
                                   flags, None, None, None, 0, None)
    _fails(corners(4, 10, 1, 5, 1, 1), "ndim")
    _fails(corners(4, 10, 4, 5, 1, 1), "ndim")
    _fails(corners(4, -1, 3, 5, 1, 1), "counts")
    _fails(corners(4, 10, 3, -5, 1, 1), "counts")
    _fails(corners(4, 1 << 28, 3, 5, 1, 1), "2^31")
    _fails(corners(4, 1 << 29, 2, 5, 1, 1), "2^31")
    _fails(corners(2, 10, 3, 5, 1, 1), "columns")
    _fails(corners(4, 10, 3, 5, 0, 1), "batch")
    _fails(corners(4, 10, 3, 5, 1, 2), "flags")
    _fails(corners(4, 10, 3, 5, 1, 1, vsize=None), "NULL")
    _fails(corners(4, 10, 3, 5, 1, 1, shape=_lib.ints([4, 0, 4])), "empty grid")
    _fails(corners(4, 10, 3, 5, 1, 1, vsize=(ctypes.c_float * 3)(1, 0, 1)), "positive")
    _fails(corners(4, 10, 3, (1 << 30) + 1, 1, 1), "2^30")
    big = _lib.ints([1 << 30] * 3)
    _fails(corners(4, 10, 3, 5, 1 << 20, 1, shape=big), "63 bits")             # batch x grid beyond a 63-bit key
    small_map = lambda nbytes: L.spx_point_corners(None, 4, None, 10, None, 3, f3, f6, None, 5, None, 1, i3,
                                                   ctypes.c_void_p(256), nbytes, 1, None, None, None, 0, None)
    _fails(small_map(8), "rank map")                # the map's SIZE is checked before any device pointer is looked at
    assert corners(4, 0, 3, 5, 1, 1) == 0              # no points: nothing to do
    _fails(corners(4, 10, 3, 5, 1, 1), "NULL")

    fwd = lambda n, n_cap, ndim, C, dt: L.spx_interp_fwd(None, n, None, None, n_cap, ndim, C, dt, None, None)
    bwd = lambda n, n_cap, ndim, C, dt: L.spx_interp_bwd(None, n_cap, ndim, None, None, None, n, None, C, dt, None, None)
    for call in (fwd, bwd):
        _fails(call(5, 10, 1, 4, _lib.DTYPE_F32), "ndim")
        _fails(call(5, 10, 5, 4, _lib.DTYPE_F32), "ndim")
        _fails(call(5, 10, 3, 4, _lib.DTYPE_I8), "dtype")
        _fails(call(5, 10, 3, 4, 9), "dtype")
        _fails(call(5, 10, 3, 0, _lib.DTYPE_F16), "channel count")
        _fails(call(5, -1, 3, 4, _lib.DTYPE_F16), "counts")
        _fails(call(-5, 10, 3, 4, _lib.DTYPE_F16), "counts")
        _fails(call(5, 1 << 28, 3, 4, _lib.DTYPE_F16), "2^31")
        _fails(call(5, 10, 3, 4, _lib.DTYPE_F64), "NULL")
    assert fwd(5, 0, 3, 4, _lib.DTYPE_BF16) == 0       # no points
    assert bwd(0, 10, 3, 4, _lib.DTYPE_BF16) == 0      # no voxel rows


def test_launch_counter_keys():
    L = _lib.load()
    for key in ("interp/corners_ranked", "interp/corners_hash", "interp/fwd", "interp/bwd"):
        assert L.spx_launch_count(key.encode()) >= 0, key
    for bad in ("interp", "interp/", "interp/corners", "interp/fwd/"):
        assert L.spx_launch_count(bad.encode()) == -1, bad


def test_python_argument_checks():
    import torch
    import spconv_amd.pytorch as sp
    from spconv_amd.pytorch import functional as F
    rows = torch.zeros((6, 8), dtype=torch.int32)
    c = F.PointCorners(rows, torch.zeros((6, 8)), None, 3)
    assert c.groups is None and c.n_points is None and c.n_live is None and c.num_voxels == 3
    assert F.PointCorners._fields == ("rows", "weights", "groups", "num_voxels", "n_points", "n_live")
    with pytest.raises(NotImplementedError, match="MI355X"):
        F.voxels_to_points_trilinear(torch.zeros((3, 4)), c)
    x = sp.SparseConvTensor(torch.zeros((3, 4)), torch.zeros((3, 4), dtype=torch.int32), [4, 4, 4], 1)
    with pytest.raises(NotImplementedError, match="MI355X"):
        F.point_corners(torch.zeros((6, 3)), None, x, [1.0] * 3, [0.0] * 3 + [4.0] * 3)
    with pytest.raises(ValueError, match="ndim"):
        sp.TrilinearDevoxelize([1.0], [0.0, 4.0])
    with pytest.raises(ValueError, match="ndim"):
        sp.TrilinearDevoxelize([1.0] * 4, [0.0] * 4 + [4.0] * 4)
    with pytest.raises(ValueError, match="coors_range_xyz"):
        sp.TrilinearDevoxelize([1.0] * 3, [0.0] * 3 + [4.0] * 2)
    with pytest.raises(ValueError, match="positive"):
        sp.TrilinearDevoxelize([1.0, 0.0, 1.0], [0.0] * 3 + [4.0] * 3)
    m = sp.TrilinearDevoxelize([0.3, 0.3, 0.3], [0.0] * 3 + [4.0] * 3, normalize=False)
    assert m.normalize is False and "vsize_xyz" in repr(m)


def test_unsupported_dtypes_are_refused_in_the_wording_of_the_reductions():
    import torch
    from spconv_amd.pytorch import _interp, _pointvoxel
    t = torch.zeros((3, 4), dtype=torch.int32)
    with pytest.raises(NotImplementedError) as mine:
        _interp._float_code(t, "op")
    with pytest.raises(NotImplementedError) as theirs:
        _pointvoxel._float_code(t, "op")
    assert str(mine.value) == str(theirs.value)
    assert str(mine.value) == "op: features must be float16, bfloat16, float32 or float64, got torch.int32"
    for dt in (torch.float16, torch.bfloat16, torch.float32, torch.float64):
        _interp._float_code(torch.zeros((1, 1), dtype=dt), "op")


def test_new_names_and_signatures():
    import spconv_amd
    import spconv_amd.pytorch as sp
    from spconv_amd.pytorch.utils import StaticPointToVoxel
    for name in ("TrilinearDevoxelize", "point_corners", "voxels_to_points_trilinear"):
        assert callable(getattr(sp, name)), name
    for name in ("PointCorners", "point_corners", "point_corners_into", "voxels_to_points_trilinear"):
        assert hasattr(sp.functional, name), name
    pc = inspect.signature(sp.functional.point_corners).parameters
    assert list(pc) == ["points", "batch_ids", "x", "vsize_xyz", "coors_range_xyz", "normalize", "n_points", "with_groups"]
    assert pc["normalize"].default is True and pc["n_points"].default is None and pc["with_groups"].default is None
    assert list(inspect.signature(sp.functional.voxels_to_points_trilinear).parameters) == ["vfeat", "corners"]
    init = inspect.signature(sp.TrilinearDevoxelize.__init__).parameters
    assert list(init)[1:] == ["vsize_xyz", "coors_range_xyz", "normalize"] and init["normalize"].default is True
    fwd = inspect.signature(sp.TrilinearDevoxelize.forward).parameters
    assert list(fwd)[1:] == ["x", "points", "batch_ids", "n_points"] and fwd["n_points"].default is None
    assert inspect.signature(StaticPointToVoxel.point_corners).parameters["x"].default is None
    for obj in (sp.functional.point_corners, sp.functional.voxels_to_points_trilinear, sp.TrilinearDevoxelize):
        assert "no gradient with respect to the points" in " ".join(obj.__doc__.lower().split()), obj
    spconv_amd.install_as_spconv()
    import spconv.pytorch as spconv
    for name in ("TrilinearDevoxelize", "point_corners", "voxels_to_points_trilinear"):
        assert getattr(spconv, name) is getattr(sp, name), name
    import spconv.pytorch.spatial as spatial
    assert spatial.TrilinearDevoxelize is sp.TrilinearDevoxelize
    assert spconv.functional.point_corners is sp.functional.point_corners
