"""CPU: the argument checks of the sectorised sampling entry points (csrc/sample.hip: spx_sector_ids, spx_fps_quota,
spx_fps_segments) come before any pointer is looked at (no kernel is launched in this file); the boundary table the
kernel is given is the one tests/refsector.py restates, entry for entry; the Python layer has the new names and refuses
bad arguments before it refuses CPU tensors.  (Declared, exported and bound as declared: test_capi.py.)"""
import ctypes
import inspect

import numpy as np
import pytest

import refsector as rsec
from capi import fails as _fails
from spconv_amd import _lib


def test_argument_checks_need_no_pointer():
    L = _lib.load()

    def ids(nfeat=4, n_cap=100, ndim=3, batch=2, S=6, cx=0.0, cy=0.0, filt=0, box_nfeat=7, m_cap=5, radius=1.0):
        return L.spx_sector_ids(None, nfeat, None, n_cap, None, ndim, batch, S, cx, cy, filt, None, box_nfeat, m_cap, None,
                                None, radius, None, None)
    _fails(ids(ndim=1), "ndim")
    _fails(ids(ndim=4), "ndim")
    _fails(ids(n_cap=-1), "counts")
    _fails(ids(nfeat=2), "columns")
    _fails(ids(batch=0), "batch")
    _fails(ids(S=0), "num_sectors")
    _fails(ids(S=65), "num_sectors")
    _fails(ids(batch=1 << 26, S=64), "2^31")
    _fails(ids(cx=float("nan")), "centre")
    _fails(ids(cy=float("inf")), "centre")
    _fails(ids(filt=2), "roi_filter")
    _fails(ids(filt=1, ndim=2, nfeat=2), "ndim 3")
    _fails(ids(filt=1, m_cap=-1), "box counts")
    _fails(ids(filt=1, box_nfeat=6), "7 columns")
    _fails(ids(filt=1, radius=-0.5), "radius")
    _fails(ids(filt=1, radius=float("nan")), "radius")
    _fails(ids(filt=1, radius=float("inf")), "radius")
    assert ids(n_cap=0) == 0 and ids(n_cap=0, filt=1, m_cap=0) == 0      # no points: nothing to do
    assert ids(box_nfeat=0, m_cap=-3, radius=-1.0, n_cap=0) == 0         # without a filter its arguments are not looked at
    _fails(ids(), "NULL")                                                # data is required, the pointers are null: no launch
    _fails(ids(filt=1), "NULL")

    def quota(n_cap=100, batch=2, S=6, K=16):
        return L.spx_fps_quota(None, n_cap, batch, S, K, None, None, None, None)
    _fails(quota(n_cap=-1), "counts")
    _fails(quota(batch=0), "batch")
    _fails(quota(S=0), "num_sectors")
    _fails(quota(S=65), "num_sectors")
    _fails(quota(K=0), "num_samples")
    _fails(quota(K=65_537), "num_samples")
    _fails(quota(batch=1 << 26, S=64), "2^31")
    _fails(quota(), "NULL")
    _fails(quota(n_cap=0), "NULL")                                       # (the outputs are written even for an empty cloud)

    def seg(nfeat=4, n_cap=100, ndim=3, groups=12, per_row=6, stride=21, cap=16, ws_bytes=0):
        return L.spx_fps_segments(None, nfeat, n_cap, ndim, None, None, groups, None, None, per_row, stride, cap, None, None,
                                  None, ws_bytes, None)
    _fails(seg(groups=0), "groups")
    _fails(seg(ndim=1), "ndim")
    _fails(seg(ndim=4), "ndim")
    _fails(seg(n_cap=-1), "counts")
    _fails(seg(nfeat=2), "columns")
    _fails(seg(per_row=0), "groups_per_row")
    _fails(seg(per_row=5), "groups_per_row")
    _fails(seg(cap=0), "max_quota")
    _fails(seg(cap=65_537), "max_quota")
    _fails(seg(stride=0), "row_stride")
    _fails(seg(groups=1 << 16, per_row=1, stride=1 << 15), "2^31")
    _fails(seg(), "NULL")
    _fails(seg(n_cap=0), "NULL")


def test_the_boundary_table_entry_for_entry():
    L = _lib.load()
    assert L.spx_sector_max() == 64 and L.spx_sector_box_tile() == 128
    from spconv_amd.pytorch import functional as F
    for S in range(1, 65):
        buf = (ctypes.c_float * (2 * S))()
        assert L.spx_sector_table(S, ctypes.cast(buf, ctypes.c_void_p)) == 0
        got = np.frombuffer(buf, dtype=np.float32).reshape(S, 2)
        assert np.array_equal(got.view(np.int32), rsec.table(S).view(np.int32)), S
        assert F.sector_table(S) == [(float(c), float(s)) for c, s in got]
    assert F.sector_table(4) == [(1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.0, -1.0)]
    assert F.sector_table(8)[2] == (0.0, 1.0) and F.sector_table(6)[3] == (-1.0, 0.0) and F.sector_table(1) == [(1.0, 0.0)]
    assert F.sector_table(6)[1] == (float(np.float32(0.5000000000000001)), float(np.float32(np.sqrt(3.0) / 2.0)))
    buf = (ctypes.c_float * 2)()
    _fails(L.spx_sector_table(0, ctypes.cast(buf, ctypes.c_void_p)), "num_sectors")
    _fails(L.spx_sector_table(65, ctypes.cast(buf, ctypes.c_void_p)), "num_sectors")
    _fails(L.spx_sector_table(6, None), "NULL")
    with pytest.raises(RuntimeError, match="num_sectors"):
        F.sector_table(0)


def test_the_launches_are_uncounted():
    """the key inventory of spx_launch_count stays as it is (tests/test_counters_host.py pins it): no key for these"""
    L = _lib.load()
    for key in ("sample/sector_ids", "sample/fps_quota", "sample/fps_segments", "sample/sector", "sector_ids"):
        assert L.spx_launch_count(key.encode()) == -1, key
    for key in ("sample/fps", "pointvoxel/groups"):
        assert L.spx_launch_count(key.encode()) >= 0, key


def test_python_argument_checks():
    import torch
    import spconv_amd.pytorch as sp
    from spconv_amd.pytorch import functional as F
    p = torch.zeros((20, 4))
    bid = torch.zeros((20,), dtype=torch.int32)
    rois, rbid = torch.zeros((5, 7)), torch.zeros((5,), dtype=torch.int32)

    def both(check):
        check(lambda points=p, batch_ids=bid, B=2, S=6, **kw: F.sector_ids(points, batch_ids, B, S, **kw))
        check(lambda points=p, batch_ids=bid, B=2, S=6, K=8, **kw: F.sector_fps(points, batch_ids, B, K, S, **kw))

    def shared(fn):
        with pytest.raises(ValueError, match="float32"):
            fn(points=p.double())
        with pytest.raises(ValueError, match="batch_ids"):
            fn(batch_ids=bid.long())
        with pytest.raises(ValueError, match="batch_size"):
            fn(B=0)
        with pytest.raises(ValueError, match="ndim"):
            fn(ndim=4)
        for bad in (0, 65, -1):
            with pytest.raises(ValueError, match="num_sectors"):
                fn(S=bad)
        for bad in ((0.0,), (0.0, float("nan")), (float("inf"), 0.0), None):
            with pytest.raises(ValueError, match="center"):
                fn(center=bad)
        with pytest.raises(ValueError, match="come together"):
            fn(rois=rois)
        with pytest.raises(ValueError, match="come together"):
            fn(roi_radius=1.6)
        with pytest.raises(ValueError, match="roi_batch_ids without rois"):
            fn(roi_batch_ids=rbid)
        with pytest.raises(ValueError, match="ndim 3"):
            fn(points=torch.zeros((20, 2)), ndim=2, rois=rois, roi_radius=1.6)
        for bad in (-1.0, float("nan"), float("inf")):
            with pytest.raises(ValueError, match="roi_radius"):
                fn(rois=rois, roi_radius=bad)
        with pytest.raises(ValueError, match=">= 7"):
            fn(rois=torch.zeros((5, 6)), roi_radius=1.6)
        with pytest.raises(ValueError, match="roi_batch_ids"):
            fn(rois=rois, roi_batch_ids=rbid[:3], roi_radius=1.6)
        with pytest.raises(NotImplementedError, match="MI355X"):       # every check passed: there is no CPU path
            fn()
        with pytest.raises(NotImplementedError, match="MI355X"):
            fn(rois=rois, roi_batch_ids=rbid, roi_radius=1.6)
    both(shared)
    fps = lambda B=2, K=8, S=6: F.sector_fps(p, bid, B, K, S)
    for bad in (0, 65_537):
        with pytest.raises(ValueError, match="num_samples"):
            fps(K=bad)
    with pytest.raises(ValueError, match="32-bit"):
        fps(B=1 << 15, K=65_536, S=2)
    with pytest.raises(ValueError, match="32-bit"):
        fps(B=(1 << 31) // (65_536 + 63) + 1, K=65_536, S=64)
    groups = F.PointGroups(bid, torch.zeros((3,), dtype=torch.int32), bid, 2)
    seg = lambda points=p, g=groups, K=4, cap=8, **kw: F.farthest_point_sample_segments(points, g, K, cap, **kw)
    with pytest.raises(ValueError, match="float32"):
        seg(points=p.double())
    with pytest.raises(ValueError, match="ndim"):
        seg(ndim=1)
    with pytest.raises(ValueError, match="offsets and list"):
        seg(g=F.PointGroups(bid, None, None, 2))
    with pytest.raises(ValueError, match="offsets and list"):
        seg(g=F.PointGroups(bid[:5], groups.offsets, bid[:5], 2))
    for bad in (0, 65_537):
        with pytest.raises(ValueError, match="max_samples"):
            seg(cap=bad)
    for bad in (-1, 9):
        with pytest.raises(ValueError, match="num_samples"):
            seg(K=bad)
    with pytest.raises(ValueError, match="num_samples"):
        seg(K=torch.zeros((3,), dtype=torch.int32))
    with pytest.raises(ValueError, match="num_samples"):
        seg(K=torch.zeros((2,), dtype=torch.int64))
    with pytest.raises(ValueError, match="32-bit"):
        seg(g=F.PointGroups(bid, groups.offsets, bid, 1 << 15), cap=65_536)
    with pytest.raises(NotImplementedError, match="MI355X"):
        seg()
    for kw, word in ((dict(num_samples=0), "num_samples"), (dict(num_samples=8, num_sectors=65), "num_sectors"),
                     (dict(num_samples=8, roi_radius=-1.0), "roi_radius"), (dict(num_samples=8, center=(1.0,)), "center")):
        with pytest.raises(ValueError, match=word):
            sp.SectorFPS(**kw)
    m = sp.SectorFPS(4096, roi_radius=1.6, center=(1, -2))
    assert (m.num_samples, m.num_sectors, m.roi_radius, m.center) == (4096, 6, 1.6, (1.0, -2.0))
    assert "num_samples=4096, num_sectors=6, roi_radius=1.6" in repr(m)
    with pytest.raises(ValueError, match="come together"):              # a module with a radius needs the RoIs
        m(p, bid, 2)


def test_new_names_and_signatures():
    import spconv_amd
    import spconv_amd.pytorch as sp
    for name in ("SectorFPS", "sector_ids", "sector_fps", "farthest_point_sample_segments"):
        assert callable(getattr(sp, name)), name
    for name in ("sector_ids", "sector_ids_into", "sector_fps", "sector_fps_into", "sector_buffers", "SectorBuffers",
                 "farthest_point_sample_segments", "fps_quota_into", "fps_segments_into", "sector_table"):
        assert hasattr(sp.functional, name), name
    ids = inspect.signature(sp.functional.sector_ids).parameters
    assert list(ids)[:10] == ["points", "batch_ids", "batch_size", "num_sectors", "center", "rois", "roi_batch_ids",
                              "roi_radius", "n_points", "n_rois"]
    assert ids["center"].default == (0., 0.) and ids["center"].kind is inspect.Parameter.KEYWORD_ONLY
    fps = inspect.signature(sp.functional.sector_fps).parameters
    assert list(fps)[:11] == ["points", "batch_ids", "batch_size", "num_samples", "num_sectors", "center", "rois",
                              "roi_batch_ids", "roi_radius", "n_points", "n_rois"] and "return_sectors" in fps
    assert fps["num_sectors"].default == 6 and fps["return_sectors"].default is False
    seg = inspect.signature(sp.functional.farthest_point_sample_segments).parameters
    assert list(seg) == ["points", "groups", "num_samples", "max_samples", "ndim"]
    assert seg["ndim"].default == 3 and seg["ndim"].kind is inspect.Parameter.KEYWORD_ONLY
    init = inspect.signature(sp.SectorFPS.__init__).parameters
    assert list(init)[1:] == ["num_samples", "num_sectors", "roi_radius", "center"]
    assert init["num_sectors"].default == 6 and init["roi_radius"].default is None and init["center"].default == (0., 0.)
    for obj in (sp.functional.sector_ids, sp.functional.sector_fps, sp.functional.farthest_point_sample_segments,
                sp.SectorFPS):
        assert "no gradient with respect to coordinates" in " ".join(obj.__doc__.lower().split()), obj
    spconv_amd.install_as_spconv()
    import spconv.pytorch as spconv
    for name in ("SectorFPS", "sector_ids", "sector_fps", "farthest_point_sample_segments"):
        assert getattr(spconv, name) is getattr(sp, name), name
    assert spconv.functional.sector_fps_into is sp.functional.sector_fps_into
    from spconv.pytorch.spatial import SectorFPS
    assert SectorFPS is sp.SectorFPS
