"""CPU: the argument checks of the rotated-box entry points (csrc/box.hip) come before any pointer is looked at (no
kernel is launched in this file); the workspace size is monotone and 0 for refused arguments; the Python layer has the
new names and refuses bad arguments.  (Declared, exported and bound as declared: test_capi.py, for the whole header.)"""
import inspect
import os
import re

import pytest

from capi import fails as _fails
from spconv_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_mode_codes_and_limits():
    from spconv_amd.pytorch import _box
    text = open(os.path.join(ROOT, "include", "spconv_amd.h")).read()
    for name, code in (("SPX_BOX_OVERLAP_BEV", _box.MODE_OVERLAP_BEV), ("SPX_BOX_IOU_BEV", _box.MODE_IOU_BEV),
                       ("SPX_BOX_IOU_3D", _box.MODE_IOU_3D)):
        assert re.search(r"#define %s %d\b" % (name, code), text), name
    assert _lib.load().spx_nms_max_pre() == 16384 == _box.MAX_PRE == _box.max_pre()


def test_nms_ws_bytes_is_monotone_and_zero_for_refused_arguments():
    ws = _lib.load().spx_nms_ws_bytes
    for bad in ((-1, 1, 64), (10, 0, 64), (10, -1, 64), (10, 1 << 30, 64), (10, 1, 0), (10, 1, -5), (10, 1, 16385)):
        assert ws(*bad) == 0, bad
    assert ws(0, 1, 1) > 0 and ws(0, 7, 16384) > 0
    ns = (0, 1, 63, 64, 65, 1000, 4096, 4097, 16384, 16385, 100000, 1 << 20)
    batches = (1, 2, 3, 4, 7, 8, 64, 1000)
    pres = (1, 63, 64, 65, 100, 4096, 4097, 8192, 8193, 16384)
    for b in batches:
        for p in pres:
            sizes = [ws(n, b, p) for n in ns]
            assert all(v > 0 for v in sizes) and sizes == sorted(sizes), (b, p, sizes)
    for n in ns:
        for p in pres:
            sizes = [ws(n, b, p) for b in batches]
            assert sizes == sorted(sizes), (n, p, sizes)
        for b in batches:
            sizes = [ws(n, b, p) for p in pres]
            assert sizes == sorted(sizes), (n, b, sizes)
    # the mask is what grows: 16384 candidates of one scene are 16384 rows of 256 words
    assert ws(16384, 1, 16384) >= 16384 * 256 * 8
    assert ws(1 << 20, 4, 4096) < (4 * 4096 * 64 * 8) + (1 << 20) * 64      # rows by scene, not by box


def test_argument_checks_need_no_pointer():
    L = _lib.load()

    def corners(nfeat=7, n=10):
        return L.spx_boxes_to_corners(None, nfeat, n, None, None, None, None)
    _fails(corners(n=-1), "counts")
    _fails(corners(nfeat=6), "columns")
    assert corners(n=0) == 0
    _fails(corners(), "NULL")                            # data is required, the pointers are null: refused, no launch

    def overlap(m=10, n=10, mode=1):
        return L.spx_boxes_overlap(None, None, m, None, None, None, n, None, mode, None, None)
    _fails(overlap(mode=-1), "mode")
    _fails(overlap(mode=3), "mode")
    _fails(overlap(m=-1), "counts")
    _fails(overlap(n=-1), "counts")
    _fails(overlap(n=65535 * 256 + 1), "columns")
    assert overlap(m=0) == 0 and overlap(n=0) == 0 and overlap(m=0, n=0, mode=2) == 0
    for mode in (0, 1, 2):
        _fails(overlap(mode=mode), "NULL")

    def aligned(n=10, mode=2):
        return L.spx_boxes_overlap_aligned(None, None, None, None, None, None, n, mode, None, None)
    _fails(aligned(mode=5), "mode")
    _fails(aligned(n=-1), "counts")
    assert aligned(n=0) == 0
    _fails(aligned(), "NULL")

    def nms(n=10, batch=1, thresh=0.5, use=0, st=0.0, pre=64, post=16, ws_bytes=0):
        return L.spx_nms_rotated(None, None, None, None, n, None, batch, thresh, use, st, pre, post, None, None, None,
                                 ws_bytes, None)
    _fails(nms(n=-1), "counts")
    _fails(nms(batch=0), "batch")
    _fails(nms(batch=1 << 30), "batch")
    _fails(nms(pre=0), "pre_max")
    _fails(nms(pre=16385, post=1), "pre_max")
    _fails(nms(post=0), "post_max")
    _fails(nms(pre=64, post=65), "post_max")
    _fails(nms(thresh=float("nan")), "thresh")
    _fails(nms(use=2), "use_score_thresh")
    _fails(nms(use=1, st=float("nan")), "score_thresh")
    assert "score_thresh" not in (nms(use=0, st=float("nan")), L.spx_last_error().decode())[1]   # (not given: not looked at)
    _fails(nms(), "NULL")
    _fails(nms(n=0), "NULL")                            # keep and count are written even without boxes


def test_launch_counter_keys():
    L = _lib.load()
    for key in ("box/corners", "box/pairs", "box/aligned", "box/key", "box/mask", "box/reduce"):
        assert L.spx_launch_count(key.encode()) >= 0, key
    for bad in ("box", "box/", "box/nms", "box/mask/", "boxes/mask"):
        assert L.spx_launch_count(bad.encode()) == -1, bad


def test_python_argument_checks():
    import torch
    import spconv_amd.pytorch as sp
    from spconv_amd.pytorch import functional as F
    boxes, scores = torch.zeros((20, 7)), torch.zeros((20,))
    ids = torch.zeros((20,), dtype=torch.int32)
    nms = lambda b=boxes, s=scores, t=0.5, **kw: F.nms_rotated(b, s, t, **kw)
    for bad in (0, -1, 16385, 1.5):
        with pytest.raises(ValueError, match="pre_max"):
            nms(pre_max=bad, post_max=1)
        with pytest.raises(ValueError, match="pre_max"):
            sp.RotatedNMS(0.5, bad, 1)
    for pre, post in ((64, 65), (64, 0), (4096, 4097)):
        with pytest.raises(ValueError, match="post_max"):
            nms(pre_max=pre, post_max=post)
        with pytest.raises(ValueError, match="post_max"):
            sp.RotatedNMS(0.5, pre, post)
    for bad in (None, float("nan")):
        with pytest.raises(ValueError, match="thresh"):
            nms(t=bad)
    with pytest.raises(ValueError, match="score_thresh"):
        nms(score_thresh=float("nan"))
    with pytest.raises(ValueError, match="batch_size"):
        nms(batch_size=0)
    with pytest.raises(ValueError, match="float32"):                  # wrong dtypes and shapes
        nms(b=boxes.double())
    with pytest.raises(ValueError, match="float32"):
        nms(b=torch.zeros((20, 6)))
    with pytest.raises(ValueError, match="float32"):
        nms(s=scores.half())
    with pytest.raises(ValueError, match="float32"):
        nms(s=torch.zeros((19,)))
    with pytest.raises(ValueError, match="batch_ids"):
        nms(batch_ids=ids.long())
    with pytest.raises(ValueError, match="class_ids"):
        nms(class_ids=ids[:5])
    with pytest.raises(ValueError, match="contiguous"):               # non-contiguous inputs
        nms(b=torch.zeros((7, 20)).t())
    with pytest.raises(ValueError, match="contiguous"):
        nms(s=torch.zeros((40,))[::2])
    with pytest.raises(ValueError, match="contiguous"):
        nms(batch_ids=torch.zeros((40,), dtype=torch.int32)[::2])
    with pytest.raises(ValueError, match="contiguous"):
        F.boxes_iou_bev(torch.zeros((7, 20)).t(), boxes)
    with pytest.raises(ValueError, match="float32"):
        F.boxes_iou3d(boxes, boxes.int())
    with pytest.raises(ValueError, match="float32"):
        F.boxes_to_corners(torch.zeros((20,)))
    bev, z = torch.zeros((20, 4, 2)), torch.zeros((20, 2))
    with pytest.raises(ValueError, match="float32"):
        F.boxes_iou_bev(F.BoxCorners(torch.zeros((20, 8)), z, 20), boxes)
    with pytest.raises(ValueError, match="float32"):
        F.boxes_iou_bev(F.BoxCorners(bev, torch.zeros((19, 2)), 20), boxes)
    with pytest.raises(ValueError, match="num_boxes"):
        F.boxes_iou_bev(F.BoxCorners(bev, z, 19), boxes)
    with pytest.raises(ValueError, match="zrange"):
        F.boxes_iou3d(F.BoxCorners(bev, None, 20), boxes)
    with pytest.raises(ValueError, match="one box of b per box of a"):
        F.boxes_iou3d_aligned(F.BoxCorners(bev, z, 20), F.BoxCorners(bev[:5], z[:5], 5))
    # every check passed: there is no CPU path
    for call in (nms, lambda: F.boxes_to_corners(boxes), lambda: F.boxes_overlap_bev(boxes, boxes),
                 lambda: F.boxes_iou_bev(F.BoxCorners(bev, None, 20), boxes), lambda: F.boxes_iou3d(boxes, boxes),
                 lambda: F.boxes_iou3d_aligned(boxes, F.BoxCorners(bev, z, 20)),
                 lambda: sp.RotatedNMS(0.7)(boxes, scores)):
        with pytest.raises(NotImplementedError, match="MI355X"):
            call()
    keep, count, ws = torch.zeros((1, 8), dtype=torch.int32), torch.zeros((1,), dtype=torch.int32), torch.zeros(64, dtype=torch.uint8)
    into = lambda k=keep, c=count, **kw: F.nms_rotated_into(F.BoxCorners(bev, None, 20), scores, 0.5, k, c, ws, **kw)
    with pytest.raises(ValueError, match="keep"):
        into(k=keep.long())
    with pytest.raises(ValueError, match="keep"):
        into(batch_size=2)
    with pytest.raises(ValueError, match="count"):
        into(c=torch.zeros((2,), dtype=torch.int32))
    with pytest.raises(ValueError, match="post_max"):
        into(pre_max=4)                                                # (post_max is the width of keep)
    with pytest.raises(NotImplementedError, match="MI355X"):
        into()
    m = sp.RotatedNMS(0.7, 1000, 100, 0.1)
    assert (m.thresh, m.pre_max, m.post_max, m.score_thresh) == (0.7, 1000, 100, 0.1) and "pre_max=1000" in repr(m)


def test_new_names_and_signatures():
    import spconv_amd
    import spconv_amd.pytorch as sp
    funcs = ("boxes_to_corners", "boxes_overlap_bev", "boxes_iou_bev", "boxes_iou3d", "boxes_iou3d_aligned", "nms_rotated")
    for name in funcs + ("RotatedNMS",):
        assert callable(getattr(sp, name)), name
    for name in funcs + ("BoxCorners", "BoxNMS", "nms_rotated_into", "nms_ws_bytes"):
        assert hasattr(sp.functional, name), name
    F = sp.functional
    assert F.BoxCorners._fields == ("bev", "zrange", "num_boxes", "n_boxes")
    assert F.BoxNMS._fields[:2] == ("keep", "count") and callable(F.BoxNMS.indices)
    assert list(inspect.signature(F.BoxNMS.indices).parameters) == ["self", "scene"]
    assert list(inspect.signature(F.boxes_to_corners).parameters) == ["boxes", "n_boxes"]
    nms = inspect.signature(F.nms_rotated).parameters
    assert list(nms) == ["boxes", "scores", "thresh", "batch_ids", "batch_size", "class_ids", "pre_max", "post_max",
                         "score_thresh", "n_boxes"]
    assert all(nms[k].kind is inspect.Parameter.KEYWORD_ONLY for k in list(nms)[3:])
    assert (nms["batch_ids"].default, nms["batch_size"].default, nms["class_ids"].default, nms["pre_max"].default,
            nms["post_max"].default, nms["score_thresh"].default, nms["n_boxes"].default) == (None, 1, None, 4096, 512,
                                                                                               None, None)
    for name in ("boxes_overlap_bev", "boxes_iou_bev", "boxes_iou3d", "boxes_iou3d_aligned"):
        assert list(inspect.signature(getattr(F, name)).parameters) == ["a", "b", "n_a", "n_b"], name
    init = inspect.signature(sp.RotatedNMS.__init__).parameters
    assert list(init)[1:] == ["thresh", "pre_max", "post_max", "score_thresh"] and init["score_thresh"].default is None
    for obj in (F.boxes_to_corners, F.boxes_overlap_bev, F.boxes_iou_bev, F.boxes_iou3d, F.boxes_iou3d_aligned,
                F.nms_rotated, sp.RotatedNMS):
        assert "no gradient" in " ".join(obj.__doc__.lower().split()), obj
    spconv_amd.install_as_spconv()
    import spconv.pytorch as spconv
    for name in funcs + ("RotatedNMS",):
        assert getattr(spconv, name) is getattr(sp, name), name
    from spconv.pytorch.spatial import RotatedNMS
    assert RotatedNMS is sp.RotatedNMS
