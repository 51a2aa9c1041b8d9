"""CPU: the argument checks of the voxel-query entry points (csrc/query.hip) come before any pointer is looked at (no
kernel is launched in this file); the Python layer has the new names and refuses bad arguments.  (Declared, exported
and bound as declared: test_capi.py, for the whole header.)"""
import ctypes
import inspect

import pytest

from capi import fails as _fails
from spconv_amd import _lib


def test_ws_bytes_is_zero_for_the_ranked_form_and_grows_with_n():
    ws = _lib.load().spx_voxel_query_ws_bytes
    ns = (0, 1, 127, 128, 129, 700, 150_000, 2_000_000, 1 << 30)
    for ndim in (2, 3):
        assert all(ws(5000, 16, ndim, n, 1) == 0 for n in ns)
        sizes = [ws(5000, 16, ndim, n, 0) for n in ns]
        assert sizes == sorted(sizes) and sizes[0] > 0 and sizes[-1] > sizes[4] > sizes[0], sizes
        assert sizes[-1] >= 2 * 8 * ns[-1]                                     # a table of at least two slots per row
    assert ws(10, 16, 1, 10, 0) == 0 and ws(10, 16, 4, 10, 0) == 0
    assert ws(-1, 16, 3, 10, 0) == 0 and ws(10, 16, 3, -1, 0) == 0 and ws(10, 16, 3, (1 << 30) + 1, 0) == 0
    assert ws(10, 0, 3, 10, 0) == 0 and ws(10, 129, 3, 10, 0) == 0
    assert ws(1 << 24, 128, 3, 10, 0) == 0 and ws((1 << 24) - 1, 128, 3, 10, 0) > 0      # n_cap * nsample >= 2^31


def test_argument_checks_need_no_pointer():
    L = _lib.load()
    f3, f6, i3 = (ctypes.c_float * 3)(1, 1, 1), (ctypes.c_float * 6)(0, 0, 0, 1, 1, 1), _lib.ints([4, 4, 4])
    r3 = _lib.ints([1, 1, 1])

    def query(nfeat=4, n_cap=10, ndim=3, n=5, batch=1, nsample=8, flags=0, r2=0.0, vsize=f3, rng=f6, shape=i3, qrange=r3,
              rankmap=None, rankmap_bytes=0):
        return L.spx_voxel_query(None, nfeat, None, n_cap, None, ndim, vsize, rng, None, n, None, batch, shape, rankmap,
                                 rankmap_bytes, qrange, nsample, r2, flags, None, None, None, None, 0, None)
    _fails(query(ndim=1), "ndim")
    _fails(query(ndim=4), "ndim")
    _fails(query(n_cap=-1), "counts")
    _fails(query(n=-5), "counts")
    _fails(query(nsample=0), "nsample")
    _fails(query(nsample=129), "nsample")
    _fails(query(n_cap=1 << 28, nsample=8), "2^31")
    _fails(query(n_cap=1 << 24, nsample=128), "2^31")
    _fails(query(n=(1 << 30) + 1), "2^30")
    _fails(query(nfeat=2), "columns")
    _fails(query(batch=0), "batch")
    _fails(query(flags=4), "flags")
    _fails(query(flags=8 << 8), "flags")
    _fails(query(flags=1, r2=-1.0), "radius")
    _fails(query(flags=1, r2=float("nan")), "radius")
    _fails(query(vsize=None), "NULL")
    _fails(query(qrange=None), "NULL")
    _fails(query(shape=_lib.ints([4, 0, 4])), "empty grid")
    _fails(query(vsize=(ctypes.c_float * 3)(1, 0, 1)), "positive")
    _fails(query(qrange=_lib.ints([1, 16, 1])), "query_range")
    _fails(query(qrange=_lib.ints([1, 1, -1])), "query_range")
    _fails(query(batch=1 << 20, shape=_lib.ints([1 << 30] * 3)), "63 bits")
    _fails(query(rankmap=ctypes.c_void_p(256), rankmap_bytes=8), "rank map")  # its SIZE, before any device pointer
    assert query(n_cap=0) == 0                          # no queries: nothing to do
    assert query(n_cap=0, qrange=_lib.ints([15, 15, 15]), nsample=128, flags=3 | (7 << 8)) == 0
    _fails(query(), "NULL")                             # data is required, the pointers are null: refused, no launch

    fwd = lambda n=5, n_cap=10, ns=8, C=4, dt=_lib.DTYPE_F32: L.spx_group_fwd(None, n, None, n_cap, ns, C, dt, None, None)
    bwd = lambda n=5, n_cap=10, ns=8, C=4, dt=_lib.DTYPE_F32: L.spx_group_bwd(None, n_cap, ns, None, None, n, None, C, dt,
                                                                            None, None)
    for call in (fwd, bwd):
        _fails(call(dt=_lib.DTYPE_I8), "dtype")
        _fails(call(dt=9), "dtype")
        _fails(call(C=0), "channel count")
        _fails(call(n_cap=-1), "counts")
        _fails(call(n=-5), "counts")
        _fails(call(ns=0), "nsample")
        _fails(call(ns=129), "nsample")
        _fails(call(n_cap=1 << 24, ns=128), "2^31")
        _fails(call(dt=_lib.DTYPE_F64), "NULL")
    assert fwd(n_cap=0) == 0                            # no queries
    assert bwd(n=0) == 0                                # no voxel rows


def test_launch_counter_keys():
    L = _lib.load()
    for key in ("query/ranked", "query/hash", "query/group_fwd", "query/group_bwd"):
        assert L.spx_launch_count(key.encode()) >= 0, key
    for bad in ("query", "query/", "query/group", "query/hash/"):
        assert L.spx_launch_count(bad.encode()) == -1, bad


def _level(ndim=3):
    import torch
    import spconv_amd.pytorch as sp
    return sp.SparseConvTensor(torch.zeros((3, 4)), torch.zeros((3, ndim + 1), dtype=torch.int32), [4] * ndim, 1)


def test_python_argument_checks():
    import torch
    from spconv_amd.pytorch import functional as F
    x, q = _level(), torch.zeros((6, 3))
    vs, rng = [1.0] * 3, [0.0] * 3 + [4.0] * 3
    call = lambda queries=q, batch_ids=None, level=x, vsize=vs, crange=rng, qrange=(1, 1, 1), nsample=8, **kw: \
        F.voxel_query(queries, batch_ids, level, vsize, crange, qrange, nsample, **kw)
    with pytest.raises(ValueError, match="float32"):
        call(queries=q.double())
    with pytest.raises(ValueError, match="float32"):
        call(queries=torch.zeros((6,)))
    with pytest.raises(ValueError, match="float32"):
        call(queries=torch.zeros((6, 2)))
    with pytest.raises(ValueError, match="batch_ids"):
        call(batch_ids=torch.zeros((6,), dtype=torch.int64))
    with pytest.raises(ValueError, match="batch_ids"):
        call(batch_ids=torch.zeros((5,), dtype=torch.int32))
    with pytest.raises(ValueError, match="query_range"):
        call(qrange=(1, 16, 1))
    with pytest.raises(ValueError, match="query_range"):
        call(qrange=(1, -1, 1))
    with pytest.raises(ValueError, match="query_range"):
        call(qrange=(1, 1))
    for bad in (0, 129):
        with pytest.raises(ValueError, match="nsample"):
            call(nsample=bad)
    with pytest.raises(ValueError, match="ndim"):
        call(level=_level(2))
    with pytest.raises(ValueError, match="ndim"):
        call(vsize=[1.0], crange=[0.0, 4.0])
    with pytest.raises(ValueError, match="pad"):
        call(pad="zero")
    with pytest.raises(ValueError, match="radius"):
        call(radius=-1.0)
    with pytest.raises(NotImplementedError, match="MI355X"):          # every check passed: there is no CPU path
        call()
    import spconv_amd.pytorch as sp
    with pytest.raises(ValueError, match="query_range"):
        sp.VoxelQueryAndGroup((1, 1, 16), 8, vsize_xyz=vs, coors_range_xyz=rng)
    with pytest.raises(ValueError, match="nsample"):
        sp.VoxelQueryAndGroup((1, 1, 1), 0, vsize_xyz=vs, coors_range_xyz=rng)
    m = sp.VoxelQueryAndGroup((1, 2, 3), 16, 0.8, False, vsize_xyz=vs, coors_range_xyz=rng)
    assert m.query_range == [1, 2, 3] and m.nsample == 16 and m.use_xyz is False and "radius=0.8" in repr(m)


def test_group_voxels_refuses_a_gradient_without_groups():
    import torch
    from spconv_amd.pytorch import functional as F
    rows = torch.zeros((6, 8), dtype=torch.int32)
    nb = F.VoxelNeighbors(rows, torch.zeros((6,), dtype=torch.int32), None, None, 3)
    assert F.VoxelNeighbors._fields == ("rows", "count", "offsets", "groups", "num_voxels", "n_queries", "n_live")
    assert nb.groups is None and nb.n_queries is None and nb.n_live is None
    with pytest.raises(ValueError, match="with_groups"):
        F.group_voxels(torch.zeros((3, 4), requires_grad=True), nb)
    with pytest.raises(ValueError, match="one row per voxel"):
        F.group_voxels(torch.zeros((5, 4)), nb)
    with pytest.raises(NotImplementedError, match="float16, bfloat16, float32 or float64"):
        F.group_voxels(torch.zeros((3, 4), dtype=torch.int32), nb)
    with pytest.raises(NotImplementedError, match="MI355X"):
        F.group_voxels(torch.zeros((3, 4)), nb)


def test_squared_radius_is_one_float32_product():
    import numpy as np
    from spconv_amd.pytorch import _query
    for r in (0.5, 1.0, 0.8, 1.0 / 3.0, 2.4, 1e-3):
        assert _query.squared_radius(r) == float(np.float32(r) * np.float32(r))
    assert _query.squared_radius(None) is None


def test_new_names_and_signatures():
    import spconv_amd
    import spconv_amd.pytorch as sp
    for name in ("VoxelQueryAndGroup", "voxel_query", "group_voxels"):
        assert callable(getattr(sp, name)), name
    for name in ("VoxelNeighbors", "voxel_query", "voxel_query_into", "group_voxels"):
        assert hasattr(sp.functional, name), name
    vq = inspect.signature(sp.functional.voxel_query).parameters
    assert list(vq) == ["queries", "batch_ids", "x", "vsize_xyz", "coors_range_xyz", "query_range", "nsample", "radius",
                        "pad", "with_offsets", "n_queries", "with_groups"]
    assert vq["radius"].default is None and vq["pad"].default == "none" and vq["with_offsets"].default is False
    assert vq["n_queries"].default is None and vq["with_groups"].default is None
    assert list(inspect.signature(sp.functional.group_voxels).parameters) == ["vfeat", "nb"]
    init = inspect.signature(sp.VoxelQueryAndGroup.__init__).parameters
    assert list(init)[1:5] == ["query_range", "nsample", "radius", "use_xyz"]
    assert init["radius"].default is None and init["use_xyz"].default is True
    assert list(inspect.signature(sp.VoxelQueryAndGroup.forward).parameters)[1:] == ["x", "queries", "batch_ids"]
    for obj in (sp.functional.voxel_query, sp.functional.group_voxels, sp.VoxelQueryAndGroup):
        assert "no gradient with respect to the queries" in " ".join(obj.__doc__.lower().split()), obj
    spconv_amd.install_as_spconv()
    import spconv.pytorch as spconv
    for name in ("VoxelQueryAndGroup", "voxel_query", "group_voxels"):
        assert getattr(spconv, name) is getattr(sp, name), name
    assert spconv.functional.voxel_query is sp.functional.voxel_query
