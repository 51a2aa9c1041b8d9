"""CPU: the argument checks of the gradient entry points (csrc/boxgrad.hip) come before any pointer is looked at (no
kernel is launched in this file); the Python layer has the new names and refuses bad arguments before any GPU work."""
import inspect
import os
import re

import pytest

from capi import fails as _fails
from spconv_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_penalty_codes():
    from spconv_amd.pytorch import _boxgrad
    text = open(os.path.join(ROOT, "include", "spconv_amd.h")).read()
    for name, code in (("SPX_BOX_PENALTY_NONE", _boxgrad.PENALTIES["none"]), ("SPX_BOX_PENALTY_DIOU", _boxgrad.PENALTIES["diou"])):
        assert re.search(r"#define %s %d\b" % (name, code), text), name
    assert sorted(_boxgrad.PENALTIES) == ["diou", "none"]


def test_argument_checks_need_no_pointer():
    L = _lib.load()

    def pairs(n=10, mode=2, penalty=0):
        return L.spx_boxes_iou_aligned_grad(None, None, None, None, None, None, n, mode, penalty, None, None, None, None,
                                            None, None, None)
    for mode in (-1, 0, 3):                              # (0, the bare overlap, has no IoU to differentiate)
        _fails(pairs(mode=mode), "mode")
    for penalty in (-1, 2):
        _fails(pairs(penalty=penalty), "penalty")
    _fails(pairs(n=-1), "counts")
    for mode in (1, 2):
        for penalty in (0, 1):
            assert pairs(n=0, mode=mode, penalty=penalty) == 0          # nothing to do: no launch, no pointer looked at
            _fails(pairs(mode=mode, penalty=penalty), "NULL")          # data is required, the tables are null

    def corners(nfeat=7, n=10):
        return L.spx_boxes_to_corners_bwd(None, nfeat, n, None, None, None, None, None)
    _fails(corners(n=-1), "counts")
    _fails(corners(nfeat=6), "columns")
    assert corners(n=0) == 0
    _fails(corners(), "NULL")


def test_no_launch_counter_key_was_added():
    L = _lib.load()
    for bad in ("box/grad", "box/pair_grad", "box/corners_bwd", "boxgrad", "boxgrad/pairs"):
        assert L.spx_launch_count(bad.encode()) == -1, bad


def test_python_argument_checks():
    import torch
    import spconv_amd.pytorch as sp
    from spconv_amd.pytorch import functional as F
    boxes = torch.zeros((20, 7))
    bev, z = torch.zeros((20, 4, 2)), torch.zeros((20, 2))
    for fn in (F.boxes_iou_bev_diff, F.boxes_iou3d_diff):
        with pytest.raises(ValueError, match="penalty"):
            fn(boxes, boxes, penalty="giou")
        with pytest.raises(ValueError, match="penalty"):
            fn(boxes, boxes, penalty=1)
        with pytest.raises(ValueError, match="float32"):
            fn(boxes.double(), boxes)
        with pytest.raises(ValueError, match="float32"):
            fn(boxes, torch.zeros((20, 6)))
        with pytest.raises(ValueError, match="contiguous"):
            fn(torch.zeros((7, 20)).t(), boxes)
        with pytest.raises(ValueError, match="one box of b per box of a"):
            fn(boxes, boxes[:5])
        with pytest.raises(ValueError, match="num_boxes"):
            fn(F.BoxCorners(bev, z, 19), boxes)
        with pytest.raises(ValueError, match="float32"):
            fn(F.BoxCorners(torch.zeros((20, 8)), z, 20), boxes)
        for call in (lambda: fn(boxes, boxes), lambda: fn(boxes.clone().requires_grad_(), F.BoxCorners(bev, z, 20)),
                     lambda: fn(boxes, boxes, penalty="diou")):
            with pytest.raises(NotImplementedError, match="MI355X"):        # every check passed: there is no CPU path
                call()
    with pytest.raises(ValueError, match="zrange"):
        F.boxes_iou3d_diff(F.BoxCorners(bev, None, 20), boxes)
    with pytest.raises(NotImplementedError, match="MI355X"):
        F.boxes_iou_bev_diff(F.BoxCorners(bev, None, 20), boxes)            # (the plane needs no z range)
    into = lambda a=F.BoxCorners(bev, z, 20), b=F.BoxCorners(bev, z, 20), mode=2, **kw: \
        F.boxes_iou_aligned_grad_into(a, b, mode, **kw)
    with pytest.raises(ValueError, match="mode"):
        into(mode=0)
    with pytest.raises(ValueError, match="penalty"):
        into(penalty="ciou")
    with pytest.raises(ValueError, match="one box of b per box of a"):
        into(b=F.BoxCorners(bev[:5], z[:5], 5))
    with pytest.raises(ValueError, match="gbev_a"):
        into(gbev_a=torch.zeros((20, 8)))
    with pytest.raises(ValueError, match="gz_b"):
        into(gz_b=torch.zeros((19, 2)))
    with pytest.raises(ValueError, match="value"):
        into(value=torch.zeros((20,), dtype=torch.float64))
    with pytest.raises(ValueError, match="grad_out"):
        into(grad_out=torch.zeros((40,))[::2])
    with pytest.raises(ValueError, match="zrange"):
        into(a=F.BoxCorners(bev, None, 20))
    with pytest.raises(NotImplementedError, match="MI355X"):
        into(value=torch.zeros((20,)))
    bwd = lambda b=boxes, g=bev, gz=z, out=torch.zeros((20, 7)): F.boxes_to_corners_bwd_into(b, None, g, gz, out)
    with pytest.raises(ValueError, match="boxes"):
        bwd(b=torch.zeros((20, 6)))
    with pytest.raises(ValueError, match="gbev"):
        bwd(g=torch.zeros((19, 4, 2)))
    with pytest.raises(ValueError, match="gzrange"):
        bwd(gz=torch.zeros((20, 3)))
    with pytest.raises(ValueError, match="gboxes"):
        bwd(out=torch.zeros((20, 9)))
    with pytest.raises(NotImplementedError, match="MI355X"):
        bwd()
    for bad in ({"mode": "giou"}, {"reduction": "avg"}):
        with pytest.raises(ValueError, match=list(bad)[0]):
            sp.RotatedIoU3DLoss(**bad)
    with pytest.raises(ValueError, match="avg_factor"):
        sp.RotatedIoU3DLoss(reduction="sum")(boxes, boxes, avg_factor=4.0)
    m = sp.RotatedIoU3DLoss("diou", plane=True, reduction="none", loss_weight=2.0)
    assert (m.mode, m.plane, m.reduction, m.loss_weight) == ("diou", True, "none", 2.0) and "mode=diou" in repr(m)


def test_new_names_and_signatures():
    import spconv_amd
    import spconv_amd.pytorch as sp
    F = sp.functional
    for name in ("boxes_iou_bev_diff", "boxes_iou3d_diff", "RotatedIoU3DLoss"):
        assert callable(getattr(sp, name)), name
    for name in ("boxes_iou_bev_diff", "boxes_iou3d_diff", "boxes_iou_aligned_grad_into", "boxes_to_corners_bwd_into"):
        assert hasattr(F, name), name
    for fn in (F.boxes_iou_bev_diff, F.boxes_iou3d_diff):
        p = inspect.signature(fn).parameters
        assert list(p) == ["a", "b", "penalty", "n_a", "n_b"]
        assert all(p[k].kind is inspect.Parameter.KEYWORD_ONLY for k in list(p)[2:])
        assert (p["penalty"].default, p["n_a"].default, p["n_b"].default) == ("none", None, None)
        assert "gradient" in fn.__doc__
    init = inspect.signature(sp.RotatedIoU3DLoss.__init__).parameters
    assert list(init)[1:] == ["mode", "plane", "reduction", "loss_weight"]
    assert [init[k].default for k in list(init)[1:]] == ["iou", False, "mean", 1.0]
    fwd = inspect.signature(sp.RotatedIoU3DLoss.forward).parameters
    assert list(fwd)[1:] == ["pred", "target", "weight", "avg_factor"]
    # the functions without a gradient still say so
    for obj in (F.boxes_iou_bev, F.boxes_iou3d, F.boxes_iou3d_aligned):
        assert "no gradient" in " ".join(obj.__doc__.lower().split()), obj
    spconv_amd.install_as_spconv()
    import spconv.pytorch as spconv
    assert spconv.RotatedIoU3DLoss is sp.RotatedIoU3DLoss and spconv.boxes_iou3d_diff is sp.boxes_iou3d_diff
