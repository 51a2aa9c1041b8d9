"""CPU: the argument checks of the entry points of csrc/roi.hip come before any pointer is looked at (no kernel is
launched in this file); the Python layer has the new names and refuses bad arguments before it refuses CPU tensors.
(Declared, exported and bound as declared: test_capi.py, for the whole header.)"""
import inspect
import os
import re

import pytest

from capi import fails as _fails
from spconv_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pad_codes_and_limits():
    from spconv_amd.pytorch import _roi
    text = open(os.path.join(ROOT, "include", "spconv_amd.h")).read()
    for name, code in (("SPX_ROI_PAD_NONE", _roi.PAD_NONE), ("SPX_ROI_PAD_FIRST", _roi.PAD_FIRST),
                       ("SPX_ROI_PAD_CYCLE", _roi.PAD_CYCLE)):
        assert re.search(r"#define %s %d\b" % (name, code), text), name
    assert (_roi.PAD_NONE, _roi.PAD_FIRST, _roi.PAD_CYCLE) == (0, 2, 4)
    L = _lib.load()
    assert L.spx_box_query_max_nsample() == 16384 == _roi.MAX_NSAMPLE == _roi.max_nsample()
    assert L.spx_box_query_waves() == 4 and L.spx_points_in_boxes_tile() == 128


def test_no_launch_counter_of_its_own():
    L = _lib.load()
    for key in ("roi", "roi/frames", "roi/points_in_boxes", "roi/box_query", "box/frames", "box/query"):
        assert L.spx_launch_count(key.encode()) == -1, key


def test_argument_checks_need_no_pointer():
    L = _lib.load()
    nan, inf = float("nan"), float("inf")

    def frames(nfeat=7, n=10, ex=0.0, ey=0.0, ez=0.0):
        return L.spx_boxes_to_frames(None, nfeat, n, None, ex, ey, ez, None, None)
    _fails(frames(n=-1), "counts")
    _fails(frames(nfeat=6), "columns")
    for bad in (-1.0, nan, inf):
        _fails(frames(ex=bad), "extra")
        _fails(frames(ey=bad), "extra")
        _fails(frames(ez=bad), "extra")
    assert frames(n=0) == 0 and frames(n=0, ex=0.5, ey=1.0, ez=2.0) == 0
    _fails(frames(), "NULL")                             # data is required, the pointers are null: refused, no launch

    def pib(nfeat=3, n=10, m=10, batch=1):
        return L.spx_points_in_boxes(None, nfeat, None, n, None, None, m, None, None, batch, None, None)
    _fails(pib(n=-1), "point counts")
    _fails(pib(m=-1), "box counts")
    _fails(pib(nfeat=2), "columns")
    _fails(pib(batch=0), "batch")
    assert pib(n=0) == 0 and pib(n=0, m=0) == 0
    _fails(pib(), "NULL")
    _fails(pib(m=0), "NULL")                             # out is written even without boxes

    def query(m=10, n=10, nfeat=3, batch=1, nsample=8, flags=0, grid=(0, 0, 0)):
        return L.spx_box_query(None, None, m, None, None, nfeat, n, None, None, batch, nsample, flags, grid[0], grid[1],
                               grid[2], None, None, None, None, None, None)
    for bad in (0, -1, 16385):
        _fails(query(nsample=bad), "nsample")
    for bad in (1, 3, 6, 8, -2):
        _fails(query(flags=bad), "flags")
    for bad in ((0, 1, 1), (1, 0, 1), (1, 1, 0), (65, 1, 1), (1, 65, 1), (1, 1, 65), (-1, -1, -1)):
        _fails(query(grid=bad), "grid")
    _fails(query(m=-1), "box counts")
    _fails(query(n=-1), "point counts")
    _fails(query(nfeat=2), "columns")
    _fails(query(batch=0), "batch")
    _fails(query(m=1 << 17, nsample=16384), "2^31")
    _fails(query(m=1 << 14, nsample=1, grid=(64, 64, 64)), "2^31")
    assert query(m=(1 << 17) - 1, nsample=16384, n=0) != 0             # fits: only the null pointers are refused
    assert "NULL" in L.spx_last_error().decode()
    for flags in (0, 2, 4):
        assert query(m=0, flags=flags) == 0 and query(m=0, flags=flags, grid=(12, 12, 12)) == 0
        _fails(query(flags=flags), "NULL")
    _fails(query(n=0), "NULL")                           # the tables are written even without points


def test_python_argument_checks():
    import torch
    import spconv_amd.pytorch as sp
    from spconv_amd.pytorch import functional as F
    boxes, pts, feats = torch.zeros((20, 7)), torch.zeros((50, 4)), torch.zeros((50, 8))
    bid, pid = torch.zeros((20,), dtype=torch.int32), torch.zeros((50,), dtype=torch.int32)
    frames = F.BoxFrames(torch.zeros((20, 8)), 20)
    for bad in (-0.1, float("nan"), float("inf"), (0.1, 0.2), (0.1, 0.2, -1.0), "wide", None):
        with pytest.raises(ValueError, match="extra_width"):
            F.boxes_to_frames(boxes, None, bad)
    with pytest.raises(ValueError, match="extra_width"):
        sp.RoIPointPool3d(512, -1.0)
    with pytest.raises(ValueError, match="float32"):
        F.boxes_to_frames(boxes.double())
    with pytest.raises(ValueError, match="float32"):
        F.boxes_to_frames(torch.zeros((20, 6)))
    with pytest.raises(ValueError, match="contiguous"):
        F.boxes_to_frames(torch.zeros((7, 20)).t())
    pib = lambda p=pts, pi=pid, b=boxes, bi=bid, B=1, **kw: F.points_in_boxes(p, pi, b, bi, B, **kw)
    query = lambda b=boxes, bi=bid, p=pts, pi=pid, B=1, ns=16, **kw: F.box_query(b, bi, p, pi, B, ns, **kw)
    for call in (pib, query):
        with pytest.raises(ValueError, match="float32"):
            call(p=pts.double())
        with pytest.raises(ValueError, match="float32"):
            call(p=torch.zeros((50, 2)))
        with pytest.raises(ValueError, match="float32"):
            call(b=boxes.half())
        with pytest.raises(ValueError, match="float32"):
            call(b=F.BoxFrames(torch.zeros((20, 7)), 20))
        with pytest.raises(ValueError, match="num_boxes"):
            call(b=F.BoxFrames(torch.zeros((20, 8)), 19))
        with pytest.raises(ValueError, match="batch_ids"):
            call(pi=pid.long())
        with pytest.raises(ValueError, match="batch_ids"):
            call(bi=bid[:5])
        with pytest.raises(ValueError, match="batch_size"):
            call(B=0)
        with pytest.raises(ValueError, match="extra_width"):
            call(extra_width=-1.0)
        with pytest.raises(ValueError, match="extra_width"):
            call(b=frames, extra_width=0.5)              # frames are enlarged already
    for bad in (0, -1, 16385, 1.5):
        with pytest.raises(ValueError, match="nsample"):
            query(ns=bad)
        with pytest.raises(ValueError, match="nsample"):
            sp.RoIPointPool3d(bad)
        with pytest.raises(ValueError, match="nsample"):
            sp.RoIAwarePool3d(12, bad)
    with pytest.raises(ValueError, match="pad"):
        query(pad="last")
    for bad in (0, 65, (1, 2), (1, 2, 0), (1, 2, 65), 1.5, "x"):
        with pytest.raises(ValueError, match="grid"):
            query(grid=bad)
        with pytest.raises(ValueError, match="grid"):
            sp.RoIAwarePool3d(bad)
        with pytest.raises(ValueError, match="grid"):
            F.roi_aware_pool(pts, pid, feats, boxes, bid, 1, bad)
    with pytest.raises(ValueError, match="grid"):
        F.roi_aware_pool(pts, pid, feats, boxes, bid, 1, None)
    with pytest.raises(ValueError, match="reduce"):
        F.roi_aware_pool(pts, pid, feats, boxes, bid, 1, 12, reduce="sum")
    with pytest.raises(ValueError, match="reduce"):
        sp.RoIAwarePool3d(12, reduce="sum")
    for pool in (lambda f: F.roi_point_pool(pts, pid, f, boxes, bid, 1), lambda f: F.roi_aware_pool(pts, pid, f, boxes, bid, 1, 4)):
        with pytest.raises(ValueError, match="one feature row per point"):
            pool(torch.zeros((49, 8)))
        with pytest.raises(ValueError, match="one feature row per point"):
            pool(torch.zeros((50,)))
    with pytest.raises(ValueError, match="nsample"):
        F.roi_point_pool(pts, pid, feats, boxes, bid, 1, 0)
    with pytest.raises(ValueError, match="nsample"):
        F.roi_aware_pool(pts, pid, feats, boxes, bid, 1, 4, 16385)
    with pytest.raises(ValueError, match="pad"):
        F.box_query_into(frames, bid, pts, None, "last", None, None, None)
    with pytest.raises(ValueError, match="cells and grid"):
        F.box_query_into(frames, bid, pts, None, "none", None, None, None, None, None, (2, 2, 2))
    # every check passed: there is no CPU path
    for call in (pib, query, lambda: pib(b=frames), lambda: query(b=frames, grid=12, pad="cycle", with_local=True),
                 lambda: F.boxes_to_frames(boxes, None, (0.1, 0.2, 0.3)),
                 lambda: F.roi_point_pool(pts, pid, feats, boxes, bid, 1),
                 lambda: F.roi_aware_pool(pts, pid, feats, boxes, bid, 1, 12, 128, "mean"),
                 lambda: sp.RoIPointPool3d(64, 0.5)(pts, pid, feats, boxes, bid, 1),
                 lambda: sp.RoIAwarePool3d((4, 4, 2))(pts, pid, feats, boxes, bid, 1)):
        with pytest.raises(NotImplementedError, match="MI355X"):
            call()
    m = sp.RoIAwarePool3d(12, 256, "mean")
    assert (m.out_size, m.max_pts_per_box, m.reduce) == ((12, 12, 12), 256, "mean") and "reduce=mean" in repr(m)
    m = sp.RoIPointPool3d(128, (0.1, 0.2, 0.3))
    assert (m.num_sampled_points, m.pool_extra_width) == (128, (0.1, 0.2, 0.3)) and "num_sampled_points=128" in repr(m)


def test_new_names_and_signatures():
    import spconv_amd
    import spconv_amd.pytorch as sp
    funcs = ("boxes_to_frames", "points_in_boxes", "box_query", "roi_point_pool", "roi_aware_pool")
    for name in funcs + ("RoIPointPool3d", "RoIAwarePool3d"):
        assert callable(getattr(sp, name)), name
    for name in funcs + ("BoxFrames", "BoxPoints", "box_query_into"):
        assert hasattr(sp.functional, name), name
    F = sp.functional
    assert F.BoxFrames._fields == ("frames", "num_boxes", "n_boxes")
    assert F.BoxPoints._fields == ("rows", "count", "hits", "local", "cells", "groups", "nsample", "num_points", "grid",
                                   "n_boxes", "n_points")
    assert callable(F.BoxPoints.neighbors)
    assert list(inspect.signature(F.boxes_to_frames).parameters) == ["boxes", "n_boxes", "extra_width"]
    pib = inspect.signature(F.points_in_boxes).parameters
    assert list(pib) == ["points", "p_batch_ids", "boxes", "b_batch_ids", "batch_size", "n_points", "n_boxes", "extra_width"]
    assert all(pib[k].kind is inspect.Parameter.KEYWORD_ONLY for k in list(pib)[5:])
    q = inspect.signature(F.box_query).parameters
    assert list(q)[:6] == ["boxes", "b_batch_ids", "points", "p_batch_ids", "batch_size", "nsample"]
    assert set(list(q)[6:]) >= {"pad", "with_local", "grid", "with_groups", "groups"}
    assert all(q[k].kind is inspect.Parameter.KEYWORD_ONLY for k in list(q)[6:])
    assert (q["pad"].default, q["with_local"].default, q["grid"].default, q["with_groups"].default) == ("none", False, None, False)
    rp = inspect.signature(F.roi_point_pool).parameters
    assert list(rp)[:8] == ["points", "p_batch_ids", "feats", "boxes", "b_batch_ids", "batch_size", "num_sampled_points",
                            "pool_extra_width"]
    assert (rp["num_sampled_points"].default, rp["pool_extra_width"].default) == (512, 0.0)
    ra = inspect.signature(F.roi_aware_pool).parameters
    assert list(ra)[:9] == ["points", "p_batch_ids", "feats", "boxes", "b_batch_ids", "batch_size", "out_size",
                            "max_pts_per_box", "reduce"]
    assert (ra["max_pts_per_box"].default, ra["reduce"].default) == (2048, "max")
    for obj in (F.boxes_to_frames, F.points_in_boxes, F.box_query, F.roi_point_pool, F.roi_aware_pool, sp.RoIPointPool3d,
                sp.RoIAwarePool3d):
        assert "no gradient" in " ".join(obj.__doc__.lower().split()), obj
    doc = " ".join(F.roi_aware_pool.__doc__.split())
    assert "PER BOX" in doc and "EVERY point that attains it" in doc          # the two differences from OpenPCDet
    spconv_amd.install_as_spconv()
    import spconv.pytorch as spconv
    for name in funcs + ("RoIPointPool3d", "RoIAwarePool3d"):
        assert getattr(spconv, name) is getattr(sp, name), name
    from spconv.pytorch.spatial import RoIAwarePool3d, RoIPointPool3d
    assert RoIAwarePool3d is sp.RoIAwarePool3d and RoIPointPool3d is sp.RoIPointPool3d
