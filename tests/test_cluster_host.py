"""CPU: the argument checks of the clustering entry points (csrc/cluster.hip) come before any pointer is looked at (no
kernel is launched in this file); the Python layer has the new names and refuses bad arguments and grids."""
import pytest

from capi import fails as _fails
from spconv_amd import _lib


def test_argument_checks_need_no_pointer():
    L, I = _lib.load(), _lib.ints
    assert L.spx_cluster_max_axis_cells() == 1 << 14
    ws = L.spx_cluster_ws_bytes
    assert ws(-1) == 0 and ws(1 << 30) == 0 and 0 < ws(0) < ws(1000) < ws(250_000) and ws(1000) >= 20 * 1000
    rec = lambda nfeat=3, n=10, batch=1: L.spx_cluster_records(None, nfeat, None, n, None, batch, None, None, None, None,
                                                               None, None, None, None, None, 0, None)
    _fails(rec(n=-1), "n_cap")
    _fails(rec(nfeat=2), "columns")
    _fails(rec(batch=0), "batch")
    _fails(rec(), "range")
    link = lambda n=10, batch=1, grid=(8, 8, 8), r2=0.25, rm=1 << 20: L.spx_cluster_link(
        n, batch, I(grid), None, None, None, rm, None, r2, None, None, None, 0, None)
    _fails(link(grid=(8, (1 << 14) + 1, 8)), "grid axis 1")
    _fails(link(grid=(0, 8, 8)), "grid axis 0")
    _fails(link(r2=float("nan")), "radius")
    _fails(link(batch=1 << 20, grid=(1 << 14, 1 << 14, 1 << 14)), "rank map")
    _fails(link(rm=8), "rank map too small")
    assert link(n=0) == 0
    _fails(link(), "NULL")
    num = lambda n=10, m=1, table=None, labels=0, cap=4: L.spx_cluster_number(n, None, None, None, m, table, labels, cap,
                                                                               None, None, None, 0, None)
    _fails(num(cap=0), "cap")
    _fails(num(m=0), "min_points")
    _fails(num(), "count")
    _fails(L.spx_cluster_roots(10, None, None, None), "NULL")
    assert L.spx_cluster_roots(0, None, None, None) == 0


def test_python_argument_checks_and_names():
    import torch
    import spconv_amd.pytorch as sp
    F = sp.functional
    assert F.PointClusters._fields == ("cluster_of_point", "root", "count", "groups", "status")
    assert sp.cluster_points is F.cluster_points and callable(F.cluster_points_into) and callable(sp.ClusterPoints)
    p, rng = torch.zeros((20, 3)), [0, 0, 0, 4, 4, 4]
    cl = lambda points=p, bid=None, B=1, radius=0.5, r=rng, **kw: F.cluster_points(points, bid, B, radius, r, **kw)
    for bad in (0.0, -1.0, float("nan"), float("inf"), None):
        with pytest.raises(ValueError, match="radius"):
            cl(radius=bad)
    for bad in ([0, 0, 0, 4, 4], [0, 0, 0, 4, 0, 4], [0, 0, 0, 4, float("nan"), 4]):
        with pytest.raises(ValueError, match="coors_range_xyz"):
            cl(r=bad)
    with pytest.raises(ValueError, match="cells per axis"):                # 2^14 cells of 0.5078125 end at 8320
        cl(r=[0, 0, 0, 8400, 4, 4])
    assert F.cluster_plan(0.5, [0, 0, 0, 8300, 4, 4], 1).grid_zyx == (8, 8, 16345)
    with pytest.raises(ValueError, match="rank map"):
        cl(r=[0, 0, 0, 2000, 2000, 2000])
    with pytest.raises(ValueError, match="batch_size"):
        cl(B=0)
    with pytest.raises(ValueError, match="float32"):
        cl(points=p.double())
    with pytest.raises(ValueError, match="labels"):
        cl(labels=torch.zeros((20,), dtype=torch.int64))
    with pytest.raises(ValueError, match="valid"):
        cl(valid=torch.zeros((5,), dtype=torch.bool))
    with pytest.raises(ValueError, match="min_points"):
        cl(min_points=0)
    with pytest.raises(ValueError, match="requires labels"):
        cl(min_points=torch.ones((3,)))
    with pytest.raises(NotImplementedError, match="MI355X"):               # every check passed: there is no CPU path
        cl()
    with pytest.raises(ValueError, match="min_points"):
        sp.ClusterPoints(0.5, rng, 0)
    assert "radius=0.5" in repr(sp.ClusterPoints(0.5, rng, 50))
    assert F.cluster_cap(1000, 50) == 20 and F.cluster_cap(10, 50) == 1 and F.cluster_cap(1000, torch.ones((3,))) == 1000
