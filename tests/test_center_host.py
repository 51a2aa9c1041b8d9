"""CPU: the argument checks of the centre-head target entry points (csrc/center.hip: spx_box_centers,
spx_center_heatmap, spx_center_nearest, spx_center_heatmap_sparse) come before any pointer is looked at (no kernel is
launched in this file); the header's constants are the Python layer's; the Python layer has the new names and refuses
bad parameters before it refuses CPU tensors.  (Declared, exported and bound as declared: test_capi.py.)"""
import inspect
import os
import re

import pytest

from capi import HEADER, fails as _fails
from spconv_amd import _lib


def test_argument_checks_need_no_pointer():
    L = _lib.load()

    def rec(nfeat=7, cbytes=8, m_cap=10, batch=2, W=40, H=56, vx=0.1, vy=0.1, x0=0.0, y0=0.0, stride=1.0, C=3, objs=500,
            ov=0.1, rmin=2):
        return L.spx_box_centers(None, nfeat, None, None, cbytes, m_cap, None, None, None, batch, W, H, vx, vy, x0, y0, stride,
                                 C, objs, ov, rmin, None, None, None, None, None, None, None, None, None)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        _fails(rec(stride=bad), "stride")
    for bad in (0.0, 1.0, -0.1, float("nan")):
        _fails(rec(ov=bad), "min_overlap")
    _fails(rec(rmin=-1), "min_radius")
    _fails(rec(rmin=(1 << 20) + 1), "min_radius")
    _fails(rec(objs=0), "max_objs")
    _fails(rec(m_cap=-1), "box counts")
    _fails(rec(batch=0), "batch")
    _fails(rec(batch=65536), "batch")
    _fails(rec(W=0), "grid_size")
    _fails(rec(H=(1 << 23) + 1), "grid_size")
    _fails(rec(C=0), "num_classes")
    _fails(rec(C=65), "num_classes")
    _fails(rec(batch=4, C=64, W=4096, H=2048), "2^31")
    _fails(rec(batch=65535, objs=1 << 16), "max_objs")
    _fails(rec(vx=0.0), "voxel_size")
    _fails(rec(vy=float("inf")), "voxel_size")
    _fails(rec(x0=float("nan")), "range_min")
    _fails(rec(nfeat=6), "7 columns")
    _fails(rec(cbytes=2), "class ids")
    _fails(rec(), "NULL")                                 # every check passed, the pointers are null: no launch
    _fails(rec(m_cap=0), "NULL")                          # (the scene tables are written even without a box)

    def dense(m_cap=10, batch=2, W=40, H=56, C=3):
        return L.spx_center_heatmap(None, None, None, m_cap, None, None, batch, W, H, C, None, None)
    _fails(dense(m_cap=-1), "box counts")
    _fails(dense(batch=0), "batch")
    _fails(dense(W=0), "grid_size")
    _fails(dense(C=65), "num_classes")
    _fails(dense(batch=2, C=64, W=8192, H=2048), "2^31")
    _fails(dense(), "NULL")
    _fails(dense(m_cap=0), "NULL")

    def near(m_cap=10, n_cap=100, batch=2, W=40, H=56, objs=500):
        return L.spx_center_nearest(None, None, None, m_cap, None, n_cap, None, None, None, batch, W, H, None, None, objs,
                                    None, None, None, None)
    _fails(near(objs=0), "max_objs")
    _fails(near(m_cap=-1), "box counts")
    _fails(near(n_cap=-1), "row counts")
    _fails(near(batch=0), "batch")
    _fails(near(H=0), "grid_size")
    _fails(near(), "NULL")
    _fails(near(m_cap=0, n_cap=0), "NULL")

    def sparse(m_cap=10, n_cap=100, batch=2, W=40, H=56, C=3, anchor=0, cutoff=0):
        return L.spx_center_heatmap_sparse(None, None, None, None, None, m_cap, None, None, None, n_cap, None, batch, W, H, C,
                                           anchor, cutoff, None, None)
    _fails(sparse(anchor=2), "anchor")
    _fails(sparse(anchor=-1), "anchor")
    _fails(sparse(cutoff=2), "cutoff")
    _fails(sparse(m_cap=-1), "box counts")
    _fails(sparse(n_cap=-1), "row counts")
    _fails(sparse(C=0), "num_classes")
    _fails(sparse(n_cap=1 << 26, C=64), "2^31")
    assert sparse(n_cap=0) == 0                           # no rows: nothing to write
    _fails(sparse(), "NULL")
    _fails(sparse(anchor=1), "NULL")


def test_header_constants_are_the_python_constants():
    from spconv_amd.pytorch import _center
    L = _lib.load()
    defines = {k: int(v) for k, v in re.findall(r"#define\s+(SPX_CENTER_\w+)\s+(\d+)", HEADER)}
    assert defines == {"SPX_CENTER_MAX_CLASSES": _center.MAX_CLASSES, "SPX_CENTER_ANCHOR_CENTER": _center.ANCHOR_CENTER,
                       "SPX_CENTER_ANCHOR_NEAREST": _center.ANCHOR_NEAREST, "SPX_CENTER_CUTOFF_NONE": _center.CUTOFF_NONE,
                       "SPX_CENTER_CUTOFF_WINDOW": _center.CUTOFF_WINDOW}
    assert L.spx_center_max_classes() == _center.MAX_CLASSES == 64
    assert L.spx_center_tile() == 128 and _center.center_tile() == 128
    assert _center._ANCHORS == {"center": 0, "nearest": 1} and _center._CUTOFFS == {"none": 0, "window": 1}
    assert "center.o" in [os.path.basename(o) for o in _lib.linked_objects()]
    assert L.spx_launch_count(b"center/heatmap") == -1    # (uncounted: tests/test_counters_host.py pins the inventory)


def test_python_argument_checks():
    import torch
    import spconv_amd.pytorch as sp
    from spconv_amd.pytorch import functional as F
    boxes, bid, cls = torch.zeros((6, 8)), torch.zeros((6,), dtype=torch.int32), torch.zeros((6,), dtype=torch.int64)
    good = dict(grid_size=(40, 56), voxel_size=(0.1, 0.1), range_min=(0.0, -2.8), stride=2, num_classes=3)

    def rec(b=boxes, i=bid, c=cls, B=2, **kw):
        return F.box_centers(b, i, c, B, **{**good, **kw})
    # every bad parameter is refused although the tensors are on the CPU: the parameter checks come first
    for kw, word in ((dict(stride=0), "stride"), (dict(stride=-2.0), "stride"), (dict(stride=float("nan")), "stride"),
                     (dict(stride="a"), "stride"), (dict(min_overlap=0.0), "min_overlap"), (dict(min_overlap=1.0), "min_overlap"),
                     (dict(min_radius=-1), "min_radius"), (dict(min_radius=1.5), "min_radius"), (dict(max_objs=0), "max_objs"),
                     (dict(num_classes=0), "num_classes"), (dict(num_classes=65), "num_classes"),
                     (dict(grid_size=(40,)), "grid_size"), (dict(grid_size=(0, 56)), "grid_size"),
                     (dict(grid_size=(40.5, 56)), "grid_size"), (dict(voxel_size=(0.1, 0.0)), "voxel_size"),
                     (dict(voxel_size=0.1), "voxel_size"), (dict(range_min=(0.0, float("inf"))), "range_min"),
                     (dict(grid_size=(1 << 14, 1 << 14), num_classes=8), "32-bit"), (dict(B=0), "batch_size")):
        with pytest.raises(ValueError, match=word):
            rec(**kw)
    with pytest.raises(ValueError, match="float32"):
        rec(b=boxes.double())
    with pytest.raises(ValueError, match=">= 7"):
        rec(b=boxes[:, :6].contiguous())
    with pytest.raises(ValueError, match="b_batch_ids"):
        rec(i=bid.long())
    with pytest.raises(ValueError, match="class_ids"):
        rec(c=cls.float())
    with pytest.raises(ValueError, match="class_ids"):
        rec(c=cls[:4])
    with pytest.raises(NotImplementedError, match="MI355X"):          # every check passed: there is no CPU path
        rec()
    with pytest.raises(NotImplementedError, match="MI355X"):
        rec(i=None, c=None)
    for fn in (F.center_heatmap, lambda c: F.center_heatmap_sparse(c, torch.zeros((4, 3), dtype=torch.int32))):
        with pytest.raises(ValueError, match="BoxCenters"):
            fn(boxes)
    params = F.CenterParams((40, 56), (0.1, 0.1), (0.0, -2.8), 2.0, 3, 500, 0.1, 2, 2)
    i32 = lambda *s: torch.zeros(s, dtype=torch.int32)
    groups = F.PointGroups(i32(6), i32(3), i32(6), 2)
    centers = F.BoxCenters(torch.zeros((6, 2)), i32(6, 2), i32(6), i32(6), i32(6), i32(2, 500), i32(2, 500), i32(2, 500),
                           groups, params)
    with pytest.raises(ValueError, match="out is a contiguous float32"):
        F.center_heatmap(centers, torch.zeros((2, 3, 40, 56)))        # (H and W swapped)
    with pytest.raises(NotImplementedError, match="MI355X"):
        F.center_heatmap(centers)
    idx = i32(9, 3)
    with pytest.raises(ValueError, match="anchor"):
        F.center_heatmap_sparse(centers, idx, anchor="centre")
    with pytest.raises(ValueError, match="cutoff"):
        F.center_heatmap_sparse(centers, idx, cutoff="radius")
    with pytest.raises(ValueError, match="2-D"):
        F.center_heatmap_sparse(centers, i32(9, 4))
    with pytest.raises(ValueError, match="int32"):
        F.center_heatmap_sparse(centers, idx.long())
    with pytest.raises(ValueError, match="2-D"):
        F.center_heatmap_sparse(centers, sp.SparseConvTensor(torch.zeros((9, 4)), i32(9, 4), [4, 56, 40], 2))
    with pytest.raises(NotImplementedError, match="MI355X"):
        F.center_heatmap_sparse(centers, idx)
    for kw, word in ((dict(stride=0), "stride"), (dict(min_overlap=2), "min_overlap"), (dict(anchor="x"), "anchor"),
                     (dict(cutoff="x"), "cutoff"), (dict(max_objs=0), "max_objs")):
        with pytest.raises(ValueError, match=word):
            sp.CenterHeadTargets(**{**dict(num_classes=3, grid_size=(40, 56), voxel_size=(0.1, 0.1, 0.2),
                                           point_cloud_range=(0, -2.8, -3, 4, 2.8, 1), stride=2), **kw})
    import numpy as np
    from_arrays = sp.CenterHeadTargets(3, np.array([40, 56, 1]), np.array([0.1, 0.1, 0.2]),
                                       np.array([0, -2.8, -3, 4, 2.8, 1]), 2)       # the arrays of a data config
    assert (from_arrays.grid_size, from_arrays.voxel_size, from_arrays.range_min) == ((40, 56), (0.1, 0.1), (0.0, -2.8))
    with pytest.raises(ValueError, match="voxel_size"):
        sp.CenterHeadTargets(3, (40, 56), 0.1, (0, -2.8), 2)
    buf = F.center_buffers(6, params, "cpu")
    with pytest.raises(ValueError, match="b_batch_ids"):                # a scene list to build, and no ids to build it from
        F.box_centers_into(boxes, None, cls, None, buf, torch.zeros(64, dtype=torch.uint8))
    head = sp.CenterHeadTargets(3, (40, 56), (0.1, 0.1, 0.2), (0, -2.8, -3, 4, 2.8, 1), 2)
    assert (head.grid_size, head.voxel_size, head.range_min, head.stride) == ((40, 56), (0.1, 0.1), (0.0, -2.8), 2.0)
    assert (head.max_objs, head.min_overlap, head.min_radius, head.anchor, head.cutoff) == (500, 0.1, 2, "center", "none")
    assert "num_classes=3, grid_size=(40, 56)" in repr(head)
    with pytest.raises(NotImplementedError, match="MI355X"):
        head(boxes, bid, cls, 2)


def test_new_names_and_signatures():
    import spconv_amd
    import spconv_amd.pytorch as sp
    for name in ("CenterHeadTargets", "box_centers", "center_heatmap", "center_heatmap_sparse"):
        assert callable(getattr(sp, name)), name
    for name in ("box_centers", "box_centers_into", "center_buffers", "center_groups_ws", "center_heatmap",
                 "center_heatmap_into", "center_heatmap_sparse", "center_heatmap_sparse_into", "center_nearest_into",
                 "center_tile", "BoxCenters", "SparseCenters", "CenterParams"):
        assert hasattr(sp.functional, name), name
    rec = inspect.signature(sp.functional.box_centers).parameters
    assert list(rec) == ["boxes", "b_batch_ids", "class_ids", "batch_size", "grid_size", "voxel_size", "range_min", "stride",
                         "num_classes", "max_objs", "min_overlap", "min_radius", "n_boxes"]
    assert all(rec[k].kind is inspect.Parameter.KEYWORD_ONLY for k in list(rec)[4:])
    assert (rec["max_objs"].default, rec["min_overlap"].default, rec["min_radius"].default, rec["n_boxes"].default) == \
        (500, 0.1, 2, None)
    assert list(inspect.signature(sp.functional.center_heatmap).parameters) == ["centers", "out"]
    sparse = inspect.signature(sp.functional.center_heatmap_sparse).parameters
    assert list(sparse) == ["centers", "x", "anchor", "cutoff", "n_live"]
    assert (sparse["anchor"].default, sparse["cutoff"].default) == ("center", "none")
    assert sparse["anchor"].kind is inspect.Parameter.KEYWORD_ONLY
    init = inspect.signature(sp.CenterHeadTargets.__init__).parameters
    assert list(init)[1:] == ["num_classes", "grid_size", "voxel_size", "point_cloud_range", "stride", "max_objs",
                              "min_overlap", "min_radius", "anchor", "cutoff"]
    assert list(inspect.signature(sp.CenterHeadTargets.forward).parameters)[1:] == ["boxes", "b_batch_ids", "class_ids",
                                                                                   "batch_size", "x", "n_boxes"]
    assert sp.functional.BoxCenters._fields[:8] == ("center", "cell", "radius", "cls", "slot", "box_index", "mask", "inds")
    assert sp.functional.SparseCenters._fields == ("heat", "nearest", "inds", "mask")
    spconv_amd.install_as_spconv()
    import spconv.pytorch as spconv
    assert spconv.CenterHeadTargets is sp.CenterHeadTargets and spconv.functional.box_centers is sp.functional.box_centers
