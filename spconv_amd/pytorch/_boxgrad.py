"""Differentiable rotated IoU on the HIP kernels of csrc/boxgrad.hip: the IoU of aligned (prediction, target) pairs in the
plane and in space, with or without the DIoU penalty, and its gradient with respect to the boxes or their corners
(``functional.boxes_iou_bev_diff`` / ``boxes_iou3d_diff``, ``spatial.RotatedIoU3DLoss``).  Not part of the reference;
the code bases users port call it as mmcv's ``diff_iou_rotated_3d`` under mmdet3d's ``RotatedIoU3DLoss``.

  * forward    the corners launch of _box.py for an argument given as boxes, then ``spx_boxes_iou_aligned_grad`` with
               no gradient table: without a penalty the bits of ``boxes_iou3d_aligned``
  * backward   the same entry with ``grad_out`` and the gradient tables autograd asks for (the edge integral of the
               header: no atomics, identical bits run to run), then ``spx_boxes_to_corners_bwd`` for boxes
  * ``_into``  the two C calls over buffers the caller owns: capturable

Differentiable once.  tests/refboxgrad.py restates every output of the pair entry in numpy float32.
"""
from __future__ import annotations

from typing import Optional

import torch
from torch.autograd.function import once_differentiable

from spconv_amd import _lib
from spconv_amd.pytorch._box import (MODE_IOU_3D, MODE_IOU_BEV, BoxCorners, Boxes, _check_arg, _check_f32, corners_into)
from spconv_amd.pytorch._rulebook import _check_count, _ptr, _require_gpu, _stream

PENALTIES = {"none": 0, "diou": 1}                       # SPX_BOX_PENALTY_*


def _check_penalty(op: str, penalty) -> int:
    if not isinstance(penalty, str) or penalty not in PENALTIES:
        raise ValueError(f"{op}: penalty must be 'none' or 'diou', got {penalty!r}")
    return PENALTIES[penalty]


def _check_table(op: str, what: str, t: Optional[torch.Tensor], shape) -> None:
    """An optional fp32 table of the `_into` forms: its dtype, shape and contiguity."""
    if t is not None:
        _check_f32(op, what, t, lambda x: tuple(x.shape) == tuple(shape), str(list(shape)))


def _require_all_gpu(*tables) -> None:
    """The refusal of CPU tensors comes behind every ValueError."""
    for what, t in tables:
        if t is not None:
            _require_gpu(t, what)


def boxes_iou_aligned_grad_into(a: BoxCorners, b: BoxCorners, mode: int, *, penalty: str = "none",
                                grad_out: Optional[torch.Tensor] = None, value: Optional[torch.Tensor] = None,
                                gbev_a: Optional[torch.Tensor] = None, gz_a: Optional[torch.Tensor] = None,
                                gbev_b: Optional[torch.Tensor] = None, gz_b: Optional[torch.Tensor] = None) -> None:
    """The one C call of the pair entry into buffers the caller owns (no allocation, nothing read back: capturable).  a /
    b: ``BoxCorners`` of the same length N (their n_boxes are the device counts); mode: 1 (the plane) or 2 (space);
    grad_out fp32 [N] or None (ones).  Each output is None or written in full: value [N], gbev_a / gbev_b [N, 4, 2],
    gz_a / gz_b [N, 2]."""
    op = "boxes_iou_aligned_grad_into"
    pen = _check_penalty(op, penalty)
    if mode not in (MODE_IOU_BEV, MODE_IOU_3D):
        raise ValueError(f"{op}: mode must be 1 (the plane) or 2 (space), got {mode}")
    N = int(a.num_boxes)
    if int(b.num_boxes) != N:
        raise ValueError(f"{op}: one box of b per box of a, got {a.num_boxes} and {b.num_boxes}")
    tables = (("bev_a", a.bev, (N, 4, 2)), ("bev_b", b.bev, (N, 4, 2)), ("grad_out", grad_out, (N,)),
              ("value", value, (N,)), ("gbev_a", gbev_a, (N, 4, 2)), ("gz_a", gz_a, (N, 2)), ("gbev_b", gbev_b, (N, 4, 2)),
              ("gz_b", gz_b, (N, 2)))
    space = mode == MODE_IOU_3D
    if space:
        if a.zrange is None or b.zrange is None:
            raise ValueError(f"{op}: the corners carry no zrange; an overlap in space needs one")
        tables += (("zrange_a", a.zrange, (N, 2)), ("zrange_b", b.zrange, (N, 2)))
    for what, t, shape in tables:
        _check_table(op, what, t, shape)
    _require_all_gpu(*((what, t) for what, t, _ in tables))
    _check_count(a.n_boxes, f"{op}: n_a")
    _check_count(b.n_boxes, f"{op}: n_b")
    _lib.check(_lib.load().spx_boxes_iou_aligned_grad(
        a.bev.data_ptr(), _ptr(a.zrange) if space else None, _ptr(a.n_boxes), b.bev.data_ptr(),
        _ptr(b.zrange) if space else None, _ptr(b.n_boxes), N, int(mode), pen, _ptr(grad_out), _ptr(value), _ptr(gbev_a),
        _ptr(gz_a), _ptr(gbev_b), _ptr(gz_b), _stream(a.bev)))


def boxes_to_corners_bwd_into(boxes: torch.Tensor, n_boxes: Optional[torch.Tensor], gbev: torch.Tensor,
                              gzrange: Optional[torch.Tensor], gboxes: torch.Tensor) -> None:
    """The backward of ``boxes_to_corners`` into a buffer the caller owns (capturable): boxes fp32 [N, F >= 7], gbev fp32
    [N, 4, 2], gzrange fp32 [N, 2] or None (zeros) -> gboxes fp32 [N, F], every element written (zeros beyond the
    seventh column and in the row of an invalid box)."""
    op = "boxes_to_corners_bwd_into"
    _check_f32(op, "boxes", boxes, lambda t: t.dim() == 2 and t.shape[1] >= 7, "[N, >= 7]")
    N = int(boxes.shape[0])
    if gbev is None or gboxes is None:
        raise ValueError(f"{op}: gbev and gboxes are required")
    _check_table(op, "gbev", gbev, (N, 4, 2))
    _check_table(op, "gzrange", gzrange, (N, 2))
    _check_table(op, "gboxes", gboxes, tuple(boxes.shape))
    _require_all_gpu(("boxes", boxes), ("gbev", gbev), ("gzrange", gzrange), ("gboxes", gboxes))
    _check_count(n_boxes, f"{op}: n_boxes")
    _lib.check(_lib.load().spx_boxes_to_corners_bwd(boxes.data_ptr(), int(boxes.shape[1]), N, _ptr(n_boxes),
                                                    gbev.data_ptr(), _ptr(gzrange), gboxes.data_ptr(), _stream(boxes)))


class _Corners(torch.autograd.Function):
    """boxes -> (bev, zrange): the corners launch, its backward the corners-backward launch."""

    @staticmethod
    def forward(ctx, boxes, n_boxes):
        N, dev = int(boxes.shape[0]), boxes.device
        bev = torch.empty((N, 4, 2), dtype=torch.float32, device=dev)
        zrange = torch.empty((N, 2), dtype=torch.float32, device=dev)
        if N > 0:
            with torch.cuda.device(dev):
                corners_into(boxes, n_boxes, bev, zrange)
        ctx.save_for_backward(boxes, n_boxes)
        ctx.set_materialize_grads(False)
        return bev, zrange

    @staticmethod
    @once_differentiable
    def backward(ctx, gbev, gzrange):
        boxes, n_boxes = ctx.saved_tensors
        if gbev is None and gzrange is None:
            return None, None
        if gbev is None:                                 # (only the z range was used)
            gbev = torch.zeros((boxes.shape[0], 4, 2), dtype=torch.float32, device=boxes.device)
        gboxes = torch.empty_like(boxes)
        if boxes.shape[0] > 0:
            with torch.cuda.device(boxes.device):
                boxes_to_corners_bwd_into(boxes, n_boxes, gbev.contiguous(),
                                          None if gzrange is None else gzrange.contiguous(), gboxes)
        return gboxes, None


class _Pairs(torch.autograd.Function):
    """(bev_a, zrange_a, bev_b, zrange_b) -> value [N]; the forward saves its inputs only, the backward runs the pair
    entry again with grad_out and the tables autograd needs."""

    @staticmethod
    def forward(ctx, bev_a, z_a, bev_b, z_b, n_a, n_b, mode, penalty):
        N, dev = int(bev_a.shape[0]), bev_a.device
        value = torch.empty((N,), dtype=torch.float32, device=dev)
        if N > 0:
            with torch.cuda.device(dev):
                boxes_iou_aligned_grad_into(BoxCorners(bev_a, z_a, N, n_a), BoxCorners(bev_b, z_b, N, n_b), mode,
                                            penalty=penalty, value=value)
        ctx.save_for_backward(bev_a, z_a, bev_b, z_b, n_a, n_b)
        ctx.mode, ctx.penalty = mode, penalty
        return value

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        bev_a, z_a, bev_b, z_b, n_a, n_b = ctx.saved_tensors
        N = int(bev_a.shape[0])
        outs = [torch.empty_like(t) if want and t is not None else None
                for t, want in zip((bev_a, z_a, bev_b, z_b), ctx.needs_input_grad[:4])]
        if N > 0 and any(o is not None for o in outs):
            with torch.cuda.device(bev_a.device):
                boxes_iou_aligned_grad_into(BoxCorners(bev_a, z_a, N, n_a), BoxCorners(bev_b, z_b, N, n_b), ctx.mode,
                                            penalty=ctx.penalty, grad_out=g.contiguous(), gbev_a=outs[0], gz_a=outs[1],
                                            gbev_b=outs[2], gz_b=outs[3])
        # (the plane is handed no z range: it has none to give a gradient to)
        return outs[0], outs[1], outs[2], outs[3], None, None, None, None


def _diff_corners(op: str, x: Boxes, n_boxes: Optional[torch.Tensor], need_z: bool) -> BoxCorners:
    """The corners form of a checked argument, on the autograd tape when it asks for a gradient."""
    if isinstance(x, BoxCorners):
        _require_gpu(x.bev, "bev")
        if x.zrange is not None:
            _require_gpu(x.zrange, "zrange")
        count = n_boxes if n_boxes is not None else x.n_boxes
        _check_count(count, f"{op}: n_boxes")
        return BoxCorners(x.bev, x.zrange, x.num_boxes, count)
    _require_gpu(x, "boxes")
    _check_count(n_boxes, f"{op}: n_boxes")
    bev, zrange = _Corners.apply(x, n_boxes)
    return BoxCorners(bev, zrange, int(x.shape[0]), n_boxes)


def _iou_diff(op: str, a: Boxes, b: Boxes, mode: int, penalty, n_a, n_b) -> torch.Tensor:
    space = mode == MODE_IOU_3D
    _check_penalty(op, penalty)
    na, nb = _check_arg(op, a, space), _check_arg(op, b, space)
    if na != nb:
        raise ValueError(f"{op}: one box of b per box of a, got {na} and {nb}")
    ca, cb = _diff_corners(op, a, n_a, space), _diff_corners(op, b, n_b, space)
    if ca.bev.device != cb.bev.device:
        raise ValueError(f"{op}: a is on {ca.bev.device}, b on {cb.bev.device}")
    return _Pairs.apply(ca.bev, ca.zrange if space else None, cb.bev, cb.zrange if space else None, ca.n_boxes,
                        cb.n_boxes, mode, penalty)


def boxes_iou_bev_diff(a: Boxes, b: Boxes, *, penalty: str = "none", n_a: Optional[torch.Tensor] = None,
                       n_b: Optional[torch.Tensor] = None) -> torch.Tensor:
    """fp32 [N]: the bird's-eye IoU of the aligned pairs (a[i], b[i]) -- ``boxes_iou_bev(a, b)[i, i]`` to the bit -- WITH
    a gradient.  a / b: boxes fp32 [N, >= 7] (the gradient arrives in the seven columns, zeros in the others) or
    ``BoxCorners`` (the gradient arrives in ``bev`` when it requires grad).  penalty: "none", or "diou": minus the
    squared distance of the centres over the squared diagonal of the axis-aligned rectangle around both, so that pairs
    that do not overlap still move.  A pair with an invalid box (NaN / Inf, a size <= 0, at or beyond *n_a / *n_b) has
    value 0 and no gradient.  The gradient of the shared area is the boundary integral over the parts of each quad's
    edges inside the other (not a derivative of the clip): one launch, one lane per pair, no atomics, identical bits
    run to run.  With no input requiring grad the call is the forward launch alone.  Differentiable once."""
    return _iou_diff("boxes_iou_bev_diff", a, b, MODE_IOU_BEV, penalty, n_a, n_b)


def boxes_iou3d_diff(a: Boxes, b: Boxes, *, penalty: str = "none", n_a: Optional[torch.Tensor] = None,
                     n_b: Optional[torch.Tensor] = None) -> torch.Tensor:
    """fp32 [N]: the IoU in space of the aligned pairs (a[i], b[i]) -- the bits of ``boxes_iou3d_aligned`` -- WITH a
    gradient (mmcv's ``diff_iou_rotated_3d``).  Arguments and rules as ``boxes_iou_bev_diff``; ``BoxCorners`` receive
    their gradient in ``bev`` and ``zrange``; the DIoU penalty measures centres and the enclosing box in space.  The
    shared height sends its gradient to the table that attains the min / max (a tie: a)."""
    return _iou_diff("boxes_iou3d_diff", a, b, MODE_IOU_3D, penalty, n_a, n_b)
