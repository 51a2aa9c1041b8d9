"""CPU: the argument checks of the cell-query entry points (csrc/cellquery.hip) come before any pointer is looked at (no
kernel is launched in this file); the Python layer has the new names and refuses bad arguments."""
import pytest

from capi import fails as _fails
from spconv_amd import _lib


def test_argument_checks_need_no_pointer():
    L, I = _lib.load(), _lib.ints
    _fails(L.spx_cell_records(None, 2, None, 10, None, 1, None, None, None, None, None, None), "columns")
    _fails(L.spx_cell_records(None, 3, None, 10, None, 1, None, None, None, None, None, None), "range")

    def ball(m=10, grid=(8, 8, 8), vsize=0.5078125, nsample=16, r2=0.25, rm=1 << 20, lo=(0., 0., 0.)):
        import ctypes
        return L.spx_ball_query_cells(None, 3, None, m, None, None, 3, 10, 1, I(grid), (ctypes.c_float * 3)(*lo), vsize, None,
                                      None, rm, None, nsample, r2, 0, None, None, None, None)
    _fails(ball(grid=(8, (1 << 14) + 1, 8)), "grid axis 1")
    _fails(ball(nsample=129), "nsample")
    _fails(ball(r2=0.26), "cell edge")                                    # beyond the squared cell edge
    _fails(ball(r2=float("nan")), "radius")
    _fails(ball(rm=8), "rank map too small")
    _fails(ball(), "NULL")
    assert ball(m=0) == 0
    knn = lambda k=16, width=16: L.spx_knn_query_cells(None, 3, None, 10, None, None, 3, 10, 1, I((8, 8, 8)), None, 0.5, None,
                                                       None, 1 << 20, None, k, width, 0.25, 1e-8, 0, None, None, None, None,
                                                       None, None)
    _fails(knn(k=65, width=65), "k must be")
    _fails(knn(width=8), "width")


def test_python_argument_checks_and_names():
    import torch
    import spconv_amd.pytorch as sp
    F = sp.functional
    assert F.PointCellIndex._fields[:2] == ("plan", "points") and callable(F.point_cell_index_into)
    p, rng = torch.zeros((20, 3)), [0, 0, 0, 4, 4, 4]
    index = F.PointCellIndex(F.cluster_plan(0.5, rng, 1), p, None, None, None, None, 20)
    assert index.radius == 0.5
    for bad in (p.double(), p[:, :2], p.view(-1)):                        # float32 only, ndim 3 only
        with pytest.raises(ValueError, match="float32"):
            F.point_cell_index(bad, None, 1, 0.5, rng)
        with pytest.raises(ValueError, match="float32"):
            F.ball_query_cells(bad, None, index, 0.5, 16)
        with pytest.raises(ValueError, match="float32"):
            F.knn_query_cells(bad, None, index, 8, 0.5)
    with pytest.raises(ValueError, match="radius"):
        F.point_cell_index(p, None, 1, 0.0, rng)
    for bad in (0.5000001, 0.8, float("nan"), None, -1.0):                # float32(radius) <= the index's
        with pytest.raises(ValueError, match="radius"):
            F.ball_query_cells(p, None, index, bad, 16)
        with pytest.raises(ValueError, match="radius"):
            F.knn_query_cells(p, None, index, 8, bad)
    for bad in (0, 129):
        with pytest.raises(ValueError, match="nsample"):
            F.ball_query_cells(p, None, index, 0.5, bad)
    for bad in (0, 65):
        with pytest.raises(ValueError, match="k must be"):
            F.knn_query_cells(p, None, index, bad, 0.5)
    with pytest.raises(ValueError, match="pad"):
        F.ball_query_cells(p, None, index, 0.25, 16, pad="last")
    with pytest.raises(NotImplementedError, match="MI355X"):             # every check passed: there is no CPU path
        F.ball_query_cells(p, None, index, 0.25, 16)
    with pytest.raises(ValueError, match="ndim 3"):
        sp.BallQueryAndGroup(0.5, 16, ndim=2, coors_range_xyz=[0, 0, 0, 4, 4, 4])
    with pytest.raises(ValueError, match="come together"):
        sp.KNNQueryAndGroup(8, radius=0.5)
    assert sp.BallQueryAndGroup(0.5, 16).coors_range_xyz is None and sp.KNNQueryAndGroup(8).coors_range_xyz is None
    assert sp.KNNQueryAndGroup(8, radius=0.5, coors_range_xyz=rng).coors_range_xyz == (0, 0, 0, 4, 4, 4)
