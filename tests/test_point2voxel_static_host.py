"""Static-shape voxeliser (csrc/voxelize.hip spx_point2voxel_static): what can be checked without a GPU -- the header
declares the entry points, the library exports them, the binding knows them, the Python layer has the class and the
runner hook, and the size query and the argument checks that come before anything touches the device."""
import inspect
import os

import pytest

from spconv_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("spx_point2voxel_static_ws_bytes", "spx_point2voxel_static")


def test_entry_points_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "spconv_amd.h")).read()
    L = _lib.load()
    for name in NAMES:
        assert name + "(" in header, name
        assert getattr(L, name) is not None, name


def test_python_layer_has_the_class_and_the_runner_hook():
    from spconv_amd.pytorch.static import StaticInference
    from spconv_amd.pytorch.utils import StaticPointToVoxel
    ctor = inspect.signature(StaticPointToVoxel.__init__).parameters
    for arg in ("vsize_xyz", "coors_range_xyz", "num_point_features", "max_num_voxels", "max_num_points_per_voxel",
                "max_num_points", "batch_size", "key_order", "mean_dtype", "keep_voxels", "device"):
        assert arg in ctor, arg
    assert ctor["batch_size"].default == 1 and ctor["key_order"].default is True
    assert ctor["mean_dtype"].default is None and ctor["keep_voxels"].default is True
    for method in ("load", "run", "__call__", "overflowed"):
        assert callable(getattr(StaticPointToVoxel, method))
    assert inspect.signature(StaticInference.__init__).parameters["voxelizer"].default is None
    assert callable(StaticInference.run_points)


@pytest.mark.parametrize("batch,grid,key_fits", [
    (1, [20, 80, 80], True), (4, [41, 1600, 1408], True),
    (1, [1000, 2000, 2667], False),          # beyond 2^32 cells: first-seen only (64-bit keys)
    (2, [1024, 1024, 1024], False),          # 2^31 cells: no rank map
])
def test_ws_bytes(batch, grid, key_fits):
    L = _lib.load()
    g = _lib.ints(grid)
    first_seen = L.spx_point2voxel_static_ws_bytes(20000, 30000, 3, batch, g, 0)
    keyed = L.spx_point2voxel_static_ws_bytes(20000, 30000, 3, batch, g, 1)
    assert first_seen >= L.spx_point2voxel_ws_bytes(20000, 30000)
    assert (keyed > 0) == key_fits
    if key_fits:        # + a rank map of the call's own, for a caller that keeps none
        assert keyed >= first_seen + L.spx_rankmap_bytes(3, batch, g)


def test_bad_arguments_are_refused_before_the_device_is_touched():
    import ctypes
    L = _lib.load()
    f = lambda v: (ctypes.c_float * len(v))(*v)
    vs, cr, grid = f([0.2, 0.1, 0.1]), f([-2, -4, 0, 2, 4, 8]), _lib.ints([20, 80, 80])
    p = 256          # (never dereferenced: every call below fails its argument checks)

    def call(n_cap=100, nfeat=4, batch=1, max_voxels=10, max_points=2, empty_mean=0, key_order=0, voxels=p,
             mean=None, mean_dtype=0, rankmap=None, grid=grid):
        return L.spx_point2voxel_static(p, None, n_cap, p, nfeat, 3, vs, cr, grid, batch, max_voxels, max_points,
                                        empty_mean, key_order, voxels, p, p, p, p, mean, mean_dtype, rankmap, 0,
                                        p, 0, None)
    assert call(empty_mean=2) != 0 and "empty_mean" in L.spx_last_error().decode()
    assert call(empty_mean=1, voxels=None) != 0 and "empty_mean" in L.spx_last_error().decode()
    assert call(n_cap=0) != 0 and call(batch=0) != 0 and call(nfeat=2) != 0
    assert call(mean=p, mean_dtype=_lib.DTYPE_I8) != 0 and "mean_dtype" in L.spx_last_error().decode()
    assert call(rankmap=p) != 0 and "key_order" in L.spx_last_error().decode()
    assert call(key_order=1, grid=_lib.ints([1000, 2000, 2667])) != 0 and "rank map" in L.spx_last_error().decode()
    assert call() != 0 and "workspace" in L.spx_last_error().decode()
