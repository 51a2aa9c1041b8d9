"""CPU: the argument checks of the k-nearest-neighbour entry points (csrc/knn.hip) come before any pointer is looked at
(no kernel is launched in this file); the Python layer has the new names and refuses bad arguments.  (Declared,
exported and bound as declared: test_capi.py, for the whole header.)"""
import inspect

import pytest

from capi import fails as _fails
from spconv_amd import _lib


def test_max_k():
    from spconv_amd.pytorch import _knn
    assert _lib.load().spx_knn_max_k() == 64 == _knn.MAX_K == _knn.max_k()


def test_argument_checks_need_no_pointer():
    L = _lib.load()

    def knn(q_nfeat=3, m_cap=10, nfeat=4, n_cap=100, ndim=3, batch=2, k=3, width=4, eps=1e-8, flags=0):
        return L.spx_knn_query(None, q_nfeat, None, m_cap, None, None, nfeat, n_cap, ndim, None, None, batch, k, width, eps,
                               flags, None, None, None, None, None, None)
    _fails(knn(ndim=1), "ndim")
    _fails(knn(ndim=4), "ndim")
    _fails(knn(n_cap=-1), "counts")
    _fails(knn(m_cap=-1), "counts")
    _fails(knn(nfeat=2), "columns")
    _fails(knn(q_nfeat=2), "columns")
    _fails(knn(batch=0), "batch")
    _fails(knn(k=0), "k must")
    _fails(knn(k=65, width=65), "k must")
    _fails(knn(k=5, width=4), "width")
    _fails(knn(m_cap=1 << 29, k=3, width=4), "2^31")
    _fails(knn(m_cap=1 << 25, k=64, width=64), "2^31")
    _fails(knn(m_cap=1 << 25, k=3, width=64), "2^31")     # the stride counts, not k
    _fails(knn(flags=1), "flags")
    _fails(knn(flags=4), "flags")
    _fails(knn(eps=-1.0), "eps")
    _fails(knn(eps=float("nan")), "eps")
    _fails(knn(eps=float("inf")), "eps")
    assert knn(m_cap=0) == 0                            # no queries: nothing to do
    assert knn(m_cap=0, k=64, width=64, flags=2, ndim=2, nfeat=2, q_nfeat=2, eps=0.0) == 0
    _fails(knn(), "NULL")                               # data is required, the pointers are null: refused, no launch
    _fails(knn(n_cap=0), "NULL")


def test_launch_counter_key():
    L = _lib.load()
    assert L.spx_launch_count(b"sample/knn_query") >= 0
    for bad in ("sample/knn", "sample/knn_query/", "knn/query"):
        assert L.spx_launch_count(bad.encode()) == -1, bad


def test_python_argument_checks():
    import torch
    import spconv_amd.pytorch as sp
    from spconv_amd.pytorch import functional as F
    p, q = torch.zeros((20, 4)), torch.zeros((6, 3))
    bid = torch.zeros((20,), dtype=torch.int32)
    knn = lambda queries=q, qb=None, points=p, pb=bid, B=2, k=3, **kw: F.knn_query(queries, qb, points, pb, B, k, **kw)
    with pytest.raises(ValueError, match="float32"):
        knn(queries=q.double())
    with pytest.raises(ValueError, match="float32"):
        knn(points=torch.zeros((20,)))
    with pytest.raises(ValueError, match="float32"):
        knn(points=torch.zeros((20, 2)))
    with pytest.raises(ValueError, match="batch_ids"):
        knn(qb=torch.zeros((6,), dtype=torch.int64))
    with pytest.raises(ValueError, match="batch_ids"):
        knn(pb=bid[:5])
    for bad in (0, 65):
        with pytest.raises(ValueError, match="k must"):
            knn(k=bad)
    with pytest.raises(ValueError, match="width"):
        knn(k=5, width=4)
    with pytest.raises(ValueError, match="pad"):
        knn(pad="zero")
    for bad in (-1.0, float("nan"), float("inf"), None):
        with pytest.raises(ValueError, match="eps"):
            knn(eps=bad)
    with pytest.raises(ValueError, match="ndim"):
        knn(ndim=1)
    with pytest.raises(ValueError, match="batch_size"):
        knn(B=0)
    with pytest.raises(ValueError, match="scene_groups"):
        knn(groups=F.PointGroups(bid, None, None, 2))
    with pytest.raises(NotImplementedError, match="MI355X"):          # every check passed: there is no CPU path
        knn()
    with pytest.raises(NotImplementedError, match="MI355X"):
        F.three_nn(q, None, p, bid, 2)
    for fixed in ({"k": 3}, {"width": 8}, {"with_weights": False}):
        with pytest.raises(ValueError, match="fixed"):
            F.three_nn(q, None, p, bid, 2, **fixed)
    for bad in (0, 9):
        with pytest.raises(ValueError, match="k must"):
            sp.KNNInterpolate(bad)
    with pytest.raises(ValueError, match="eps"):
        sp.KNNInterpolate(3, -1e-8)
    with pytest.raises(ValueError, match="ndim"):
        sp.KNNInterpolate(3, ndim=4)
    for bad in (0, 65):
        with pytest.raises(ValueError, match="k must"):
            sp.KNNQueryAndGroup(bad)
    m = sp.KNNInterpolate()
    assert (m.k, m.eps, m.width) == (3, 1e-8, 4) and "k=3" in repr(m)
    assert [sp.KNNInterpolate(k).width for k in (1, 4, 5, 8)] == [4, 4, 8, 8]
    g = sp.KNNQueryAndGroup(16, False)
    assert g.k == 16 and g.use_xyz is False and "k=16" in repr(g)


def test_tables_refuse_a_wrong_width_or_missing_weights():
    import torch
    from spconv_amd.pytorch import functional as F

    def table(k, width, weights=True):
        rows = torch.full((5, width), -1, dtype=torch.int32)
        w = torch.zeros((5, width)) if weights else None
        return F.PointKNN(rows, torch.zeros((5,), dtype=torch.int32), None, w, None, None, k, 20)
    nb = table(5, 5, False).neighbors()
    assert isinstance(nb, F.VoxelNeighbors) and nb.num_voxels == 20 and nb.groups is None and nb.n_live is None
    with pytest.raises(ValueError, match="width k"):
        table(3, 4).neighbors()
    for k, width in ((3, 4), (4, 4), (5, 8), (8, 8)):
        c = table(k, width).corners()
        assert isinstance(c, F.PointCorners) and c.num_voxels == 20 and tuple(c.weights.shape) == (5, width)
    with pytest.raises(ValueError, match="with_weights"):
        table(3, 4, False).corners()
    for k, width in ((3, 3), (5, 5), (16, 16), (3, 6)):
        with pytest.raises(ValueError, match="width 4 or 8"):
            table(k, width).corners()
    with pytest.raises(ValueError, match="with_weights"):
        F.knn_interpolate(torch.zeros((20, 8)), table(3, 4, False))


def test_new_names_and_signatures():
    import spconv_amd
    import spconv_amd.pytorch as sp
    for name in ("KNNInterpolate", "KNNQueryAndGroup", "knn_query", "knn_interpolate", "three_nn"):
        assert callable(getattr(sp, name)), name
    for name in ("PointKNN", "knn_query", "knn_query_into", "knn_interpolate", "three_nn"):
        assert hasattr(sp.functional, name), name
    assert sp.functional.PointKNN._fields == ("rows", "count", "dist2", "weights", "offsets", "groups", "k", "num_points",
                                              "n_queries", "n_points")
    kq = inspect.signature(sp.functional.knn_query).parameters
    assert list(kq) == ["queries", "q_batch_ids", "points", "p_batch_ids", "batch_size", "k", "ndim", "width", "pad",
                        "with_dist2", "with_weights", "eps", "with_offsets", "n_queries", "n_points", "with_groups",
                        "groups"]
    assert kq["ndim"].default == 3 and kq["ndim"].kind is inspect.Parameter.KEYWORD_ONLY
    assert kq["width"].default is None and kq["pad"].default == "none" and kq["with_dist2"].default is True
    assert kq["with_weights"].default is False and kq["eps"].default == 1e-8 and kq["with_offsets"].default is False
    assert kq["with_groups"].default is False
    assert list(inspect.signature(sp.functional.knn_interpolate).parameters) == ["known_feats", "knn"]
    assert list(inspect.signature(sp.functional.three_nn).parameters)[:5] == [
        "unknown", "unknown_batch_ids", "known", "known_batch_ids", "batch_size"]
    init = inspect.signature(sp.KNNInterpolate.__init__).parameters
    assert list(init)[1:3] == ["k", "eps"] and init["k"].default == 3 and init["eps"].default == 1e-8
    assert list(inspect.signature(sp.KNNInterpolate.forward).parameters)[1:7] == [
        "known_points", "known_batch_ids", "known_feats", "unknown_points", "unknown_batch_ids", "batch_size"]
    init = inspect.signature(sp.KNNQueryAndGroup.__init__).parameters
    assert list(init)[1:3] == ["k", "use_xyz"] and init["use_xyz"].default is True
    assert list(inspect.signature(sp.KNNQueryAndGroup.forward).parameters)[1:7] == [
        "points", "p_batch_ids", "feats", "queries", "q_batch_ids", "batch_size"]
    for obj in (sp.functional.knn_query, sp.functional.knn_interpolate, sp.functional.three_nn, sp.KNNInterpolate,
                sp.KNNQueryAndGroup):
        assert "no gradient with respect to coordinates" in " ".join(obj.__doc__.lower().split()), obj
    spconv_amd.install_as_spconv()
    import spconv.pytorch as spconv
    for name in ("KNNInterpolate", "KNNQueryAndGroup", "knn_query", "knn_interpolate", "three_nn"):
        assert getattr(spconv, name) is getattr(sp, name), name
    assert spconv.functional.knn_query is sp.functional.knn_query
    from spconv.pytorch.spatial import KNNInterpolate
    assert KNNInterpolate is sp.KNNInterpolate
