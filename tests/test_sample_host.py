"""CPU: the argument checks of the sampling entry points (csrc/sample.hip) come before any pointer is looked at (no
kernel is launched in this file); the Python layer has the new names and refuses bad arguments.  (Declared, exported
and bound as declared: test_capi.py, for the whole header.)"""
import inspect

import pytest

from capi import fails as _fails
from spconv_amd import _lib


def test_resident_points_and_ws_bytes():
    L = _lib.load()
    resident = L.spx_fps_resident_points()
    assert resident >= 1024 and resident % 1024 == 0
    ws = L.spx_fps_ws_bytes
    ns = (0, 1, 1023, 1024, resident, resident + 1, 75_000, 300_000, 1 << 27)
    for ndim in (2, 3):
        sizes = [ws(n, 4, ndim) for n in ns]
        assert sizes == sorted(sizes) and sizes[-1] > sizes[5] > sizes[1] > 0, sizes
        assert all(s >= 16 * n for s, n in zip(sizes, ns))                     # a 16-byte record per point
        assert ws(75_000, 1, ndim) == ws(75_000, 64, ndim)
    assert ws(10, 4, 1) == 0 and ws(10, 4, 4) == 0 and ws(-1, 4, 3) == 0 and ws(10, 0, 3) == 0


def test_argument_checks_need_no_pointer():
    L = _lib.load()

    def fps(nfeat=4, n_cap=100, ndim=3, batch=2, K=16):
        return L.spx_fps(None, nfeat, n_cap, ndim, None, None, batch, K, None, None, None, 0, None)
    _fails(fps(ndim=1), "ndim")
    _fails(fps(ndim=4), "ndim")
    _fails(fps(n_cap=-1), "counts")
    _fails(fps(nfeat=2), "columns")
    _fails(fps(batch=0), "batch")
    _fails(fps(K=0), "num_samples")
    _fails(fps(K=65_537), "num_samples")
    _fails(fps(batch=1 << 15, K=65_536), "2^31")
    _fails(fps(), "NULL")                               # data is required, the pointers are null: refused, no launch
    _fails(fps(n_cap=0), "NULL")                        # (idx and count are written even for an empty cloud)

    def ball(q_nfeat=3, m_cap=10, nfeat=4, n_cap=100, ndim=3, batch=2, nsample=8, r2=1.0, flags=0):
        return L.spx_ball_query(None, q_nfeat, None, m_cap, None, None, nfeat, n_cap, ndim, None, None, batch, nsample, r2,
                                flags, None, None, None, None)
    _fails(ball(ndim=1), "ndim")
    _fails(ball(ndim=4), "ndim")
    _fails(ball(n_cap=-1), "counts")
    _fails(ball(m_cap=-1), "counts")
    _fails(ball(nfeat=2), "columns")
    _fails(ball(q_nfeat=2), "columns")
    _fails(ball(batch=0), "batch")
    _fails(ball(nsample=0), "nsample")
    _fails(ball(nsample=129), "nsample")
    _fails(ball(m_cap=1 << 28, nsample=8), "2^31")
    _fails(ball(m_cap=1 << 24, nsample=128), "2^31")
    _fails(ball(flags=1), "flags")
    _fails(ball(flags=4), "flags")
    _fails(ball(r2=-1.0), "radius")
    _fails(ball(r2=float("nan")), "radius")
    assert ball(m_cap=0) == 0                           # no queries: nothing to do
    assert ball(m_cap=0, nsample=128, flags=2, ndim=2, nfeat=2, q_nfeat=2) == 0
    _fails(ball(), "NULL")


def test_launch_counter_keys():
    L = _lib.load()
    for key in ("sample/fps", "sample/ball_query"):
        assert L.spx_launch_count(key.encode()) >= 0, key
    for bad in ("sample", "sample/", "sample/ball", "sample/fps/"):
        assert L.spx_launch_count(bad.encode()) == -1, bad


def test_python_argument_checks():
    import torch
    import spconv_amd.pytorch as sp
    from spconv_amd.pytorch import functional as F
    p, q = torch.zeros((20, 4)), torch.zeros((6, 3))
    bid = torch.zeros((20,), dtype=torch.int32)
    fps = lambda points=p, batch_ids=bid, B=2, K=4, **kw: F.farthest_point_sample(points, batch_ids, B, K, **kw)
    with pytest.raises(ValueError, match="float32"):
        fps(points=p.double())
    with pytest.raises(ValueError, match="float32"):
        fps(points=torch.zeros((20, 2)))
    with pytest.raises(ValueError, match="batch_ids"):
        fps(batch_ids=bid.long())
    with pytest.raises(ValueError, match="batch_ids"):
        fps(batch_ids=bid[:5])
    with pytest.raises(ValueError, match="ndim"):
        fps(ndim=4)
    with pytest.raises(ValueError, match="batch_size"):
        fps(B=0)
    for bad in (0, 65_537):
        with pytest.raises(ValueError, match="num_samples"):
            fps(K=bad)
    with pytest.raises(ValueError, match="scene_groups"):
        fps(groups=F.PointGroups(bid, None, None, 2))
    with pytest.raises(NotImplementedError, match="MI355X"):          # every check passed: there is no CPU path
        fps()
    ball = lambda queries=q, qb=None, points=p, pb=bid, B=2, radius=1.0, nsample=8, **kw: \
        F.ball_query(queries, qb, points, pb, B, radius, nsample, **kw)
    with pytest.raises(ValueError, match="float32"):
        ball(queries=q.double())
    with pytest.raises(ValueError, match="float32"):
        ball(points=torch.zeros((20,)))
    with pytest.raises(ValueError, match="batch_ids"):
        ball(qb=torch.zeros((6,), dtype=torch.int64))
    for bad in (0, 129):
        with pytest.raises(ValueError, match="nsample"):
            ball(nsample=bad)
    with pytest.raises(ValueError, match="pad"):
        ball(pad="zero")
    for bad in (-1.0, float("nan"), None):
        with pytest.raises(ValueError, match="radius"):
            ball(radius=bad)
    with pytest.raises(ValueError, match="ndim"):
        ball(ndim=1)
    with pytest.raises(NotImplementedError, match="MI355X"):
        ball()
    with pytest.raises(ValueError, match="num_samples"):
        sp.FarthestPointSample(0)
    with pytest.raises(ValueError, match="nsample"):
        sp.BallQueryAndGroup(0.8, 0)
    with pytest.raises(ValueError, match="radius"):
        sp.BallQueryAndGroup(-0.8, 16)
    m = sp.BallQueryAndGroup(0.8, 16, False)
    assert m.nsample == 16 and m.use_xyz is False and "radius=0.8" in repr(m)
    assert "num_samples=2048" in repr(sp.FarthestPointSample(2048))


def test_new_names_and_signatures():
    import spconv_amd
    import spconv_amd.pytorch as sp
    for name in ("FarthestPointSample", "BallQueryAndGroup", "farthest_point_sample", "gather_samples", "ball_query"):
        assert callable(getattr(sp, name)), name
    for name in ("PointSamples", "farthest_point_sample", "fps_into", "gather_samples", "ball_query", "ball_query_into",
                 "scene_groups"):
        assert hasattr(sp.functional, name), name
    assert sp.functional.PointSamples._fields == ("idx", "count", "batch_ids")
    fps = inspect.signature(sp.functional.farthest_point_sample).parameters
    assert list(fps) == ["points", "batch_ids", "batch_size", "num_samples", "ndim", "n_points", "groups"]
    assert fps["ndim"].default == 3 and fps["ndim"].kind is inspect.Parameter.KEYWORD_ONLY
    assert list(inspect.signature(sp.functional.gather_samples).parameters) == ["points", "samples"]
    bq = inspect.signature(sp.functional.ball_query).parameters
    assert list(bq) == ["queries", "q_batch_ids", "points", "p_batch_ids", "batch_size", "radius", "nsample", "ndim", "pad",
                        "with_offsets", "n_queries", "n_points", "with_groups", "groups"]
    assert bq["pad"].default == "none" and bq["with_offsets"].default is False and bq["with_groups"].default is False
    assert bq["ndim"].kind is inspect.Parameter.KEYWORD_ONLY
    assert list(inspect.signature(sp.FarthestPointSample.__init__).parameters)[1:2] == ["num_samples"]
    init = inspect.signature(sp.BallQueryAndGroup.__init__).parameters
    assert list(init)[1:4] == ["radius", "nsample", "use_xyz"] and init["use_xyz"].default is True
    assert list(inspect.signature(sp.BallQueryAndGroup.forward).parameters)[1:7] == [
        "points", "p_batch_ids", "feats", "queries", "q_batch_ids", "batch_size"]
    for obj in (sp.functional.farthest_point_sample, sp.functional.ball_query, sp.FarthestPointSample, sp.BallQueryAndGroup):
        assert "no gradient with respect to coordinates" in " ".join(obj.__doc__.lower().split()), obj
    spconv_amd.install_as_spconv()
    import spconv.pytorch as spconv
    for name in ("FarthestPointSample", "BallQueryAndGroup", "farthest_point_sample", "gather_samples", "ball_query"):
        assert getattr(spconv, name) is getattr(sp, name), name
    assert spconv.functional.ball_query is sp.functional.ball_query
    from spconv.pytorch.spatial import BallQueryAndGroup
    assert BallQueryAndGroup is sp.BallQueryAndGroup
