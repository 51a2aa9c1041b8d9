"""Rotated boxes on the HIP kernels of csrc/box.hip: corners, pairwise overlap and IoU in the plane and in space, and a
non-maximum suppression that stays on the device (``functional.boxes_to_corners`` / ``boxes_overlap_bev`` /
``boxes_iou_bev`` / ``boxes_iou3d`` / ``boxes_iou3d_aligned`` / ``nms_rotated`` / ``nms_rotated_into``,
``spatial.RotatedNMS``).  Not part of the reference (its ``spconv.utils`` box ops are CPU only, behind an optional
build); the code bases users port call them as the ``iou3d_nms`` CUDA extension of OpenPCDet / mmdet3d
(``boxes_iou_bev``, ``boxes_iou3d_gpu``, ``nms_gpu``), whose NMS copies its mask to the host.

  * boxes            OpenPCDet's 7-vectors, fp32 ``[N, >= 7]`` = (x, y, z, dx, dy, dz, heading), z the centre
  * ``BoxCorners``   the four bird's-eye corners and the z range of every box (``spx_boxes_to_corners``: one launch), or
                     the caller's own corners in either orientation; an invalid box holds NaN
  * overlap / IoU    one launch over the (M, N) grid, every element written; the subject is the first argument
  * ``nms_rotated``  key, sort (``spx_serialize``), mask and reduce launches; nothing read back: capturable

No function of this module has a gradient; the IoU of aligned pairs has one in _boxgrad.py (``boxes_iou3d_diff``, DESIGN
section 3.36).  tests/refbox.py restates every output in numpy float32.
"""
from __future__ import annotations

from typing import NamedTuple, Optional, Union

import torch

from spconv_amd import _lib
from spconv_amd.pytorch._rulebook import _check_count, _ptr, _require_gpu, _stream, _ws

MAX_PRE = 16384
MODE_OVERLAP_BEV, MODE_IOU_BEV, MODE_IOU_3D = 0, 1, 2     # SPX_BOX_*


class BoxCorners(NamedTuple):
    """bev fp32 [N, 4, 2] (the corners in the plane, counter-clockwise from ``boxes_to_corners``; either orientation
    when built by hand), zrange fp32 [N, 2] = (zmin, zmax) or None (a table for the plane only), num_boxes (N),
    n_boxes (device int32 or None: boxes at or beyond it do not exist).  A box with a corner that is not finite is
    invalid."""
    bev: torch.Tensor
    zrange: Optional[torch.Tensor]
    num_boxes: int
    n_boxes: Optional[torch.Tensor] = None


class BoxNMS(NamedTuple):
    """keep int32 [batch_size, post_max] (original box indices in rank order, -1 behind them), count int32
    [batch_size], post_max."""
    keep: torch.Tensor
    count: torch.Tensor
    post_max: int

    def indices(self, scene: int = 0) -> torch.Tensor:
        """The kept indices of one scene, trimmed: the 1-D tensor ``nms_gpu`` returns.  One read-back (the eager
        convenience; not capturable)."""
        return self.keep[int(scene), :int(self.count[int(scene)].item())]


Boxes = Union[torch.Tensor, BoxCorners]


def max_pre() -> int:
    return int(_lib.load().spx_nms_max_pre())


def nms_ws_bytes(n: int, batch_size: int, pre_max: int) -> int:
    return int(_lib.load().spx_nms_ws_bytes(int(n), int(batch_size), int(pre_max)))


def _check_f32(op: str, what: str, t: torch.Tensor, shape_ok, shape_text: str) -> None:
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or not shape_ok(t):
        got = f"{tuple(t.shape)} {t.dtype}" if isinstance(t, torch.Tensor) else type(t).__name__
        raise ValueError(f"{op}: {what} is a float32 tensor {shape_text}, got {got}")
    if not t.is_contiguous():
        raise ValueError(f"{op}: {what} must be contiguous")


def _check_ids(op: str, what: str, t: Optional[torch.Tensor], n: int) -> None:
    if t is None:
        return
    if t.dtype != torch.int32 or tuple(t.shape) != (n,):
        raise ValueError(f"{op}: {what} is an int32 tensor [{n}], got {tuple(t.shape)} {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{op}: {what} must be contiguous")


def _check_boxes(op: str, boxes: torch.Tensor) -> int:
    _check_f32(op, "boxes", boxes, lambda t: t.dim() == 2 and t.shape[1] >= 7,
               "[N, >= 7] (x, y, z, dx, dy, dz, heading)")
    return int(boxes.shape[0])


def _check_corners(op: str, c: BoxCorners, need_z: bool) -> int:
    _check_f32(op, "bev", c.bev, lambda t: t.dim() == 3 and tuple(t.shape[1:]) == (4, 2), "[N, 4, 2]")
    n = int(c.bev.shape[0])
    if c.zrange is None:
        if need_z:
            raise ValueError(f"{op}: the corners carry no zrange; an overlap in space needs one")
    else:
        _check_f32(op, "zrange", c.zrange, lambda t: tuple(t.shape) == (n, 2), f"[{n}, 2]")
    if int(c.num_boxes) != n:
        raise ValueError(f"{op}: num_boxes is {c.num_boxes}, bev holds {n} boxes")
    return n


def corners_into(boxes: torch.Tensor, n_boxes: Optional[torch.Tensor], bev: torch.Tensor, zrange: torch.Tensor) -> None:
    """The one C call into buffers the caller owns (capturable): bev fp32 [N, 4, 2], zrange fp32 [N, 2]."""
    _lib.check(_lib.load().spx_boxes_to_corners(boxes.data_ptr(), int(boxes.shape[1]), int(boxes.shape[0]), _ptr(n_boxes),
                                                bev.data_ptr(), zrange.data_ptr(), _stream(boxes)))


def boxes_to_corners(boxes: torch.Tensor, n_boxes: Optional[torch.Tensor] = None) -> BoxCorners:
    """boxes fp32 [N, >= 7] = (x, y, z, dx, dy, dz, heading) -> ``BoxCorners``: bev [N, 4, 2], the corners (+, +), (-, +),
    (-, -), (+, -) of (dx / 2, dy / 2) turned by the heading (``cosf`` / ``sinf``) and moved to (x, y), counter-clockwise;
    zrange [N, 2] = (z - dz * 0.5, z + dz * 0.5).  A box is valid when it lies below *n_boxes, its seven numbers are
    finite and dx, dy, dz > 0; an invalid box gets NaN everywhere, and every later step treats it as absent.  One launch,
    nothing read back.  No gradient."""
    N = _check_boxes("boxes_to_corners", boxes)
    _require_gpu(boxes, "boxes")
    _check_count(n_boxes, "boxes_to_corners: n_boxes")
    dev = boxes.device
    with torch.cuda.device(dev), torch.no_grad():
        bev = torch.empty((N, 4, 2), dtype=torch.float32, device=dev)
        zrange = torch.empty((N, 2), dtype=torch.float32, device=dev)
        if N > 0:
            corners_into(boxes.detach(), n_boxes, bev, zrange)
    return BoxCorners(bev, zrange, N, n_boxes)


def _check_arg(op: str, b: Boxes, need_z: bool) -> int:
    """The ValueErrors of a boxes-or-corners argument; they come before the refusal of a CPU tensor."""
    return _check_corners(op, b, need_z) if isinstance(b, BoxCorners) else _check_boxes(op, b)


def _as_corners(op: str, b: Boxes, n_boxes: Optional[torch.Tensor], need_z: bool) -> BoxCorners:
    """The corners form of a checked argument: as given, or the corners launch over boxes."""
    if isinstance(b, BoxCorners):
        _require_gpu(b.bev, "bev")
        if b.zrange is not None:
            _require_gpu(b.zrange, "zrange")
        count = n_boxes if n_boxes is not None else b.n_boxes
        _check_count(count, f"{op}: n_boxes")
        return BoxCorners(b.bev, b.zrange, b.num_boxes, count)
    _require_gpu(b, "boxes")
    _check_count(n_boxes, f"{op}: n_boxes")
    return boxes_to_corners(b, n_boxes)


def overlap_into(a: BoxCorners, b: BoxCorners, mode: int, out: torch.Tensor) -> None:
    """The one C call of the matrix forms into a buffer the caller owns (capturable): out fp32 [M, N]."""
    _lib.check(_lib.load().spx_boxes_overlap(a.bev.data_ptr(), _ptr(a.zrange), int(a.num_boxes), _ptr(a.n_boxes),
                                             b.bev.data_ptr(), _ptr(b.zrange), int(b.num_boxes), _ptr(b.n_boxes),
                                             int(mode), out.data_ptr(), _stream(out)))


def _pairs(op: str, a: Boxes, b: Boxes, mode: int, n_a, n_b) -> torch.Tensor:
    _check_arg(op, a, mode == MODE_IOU_3D)
    _check_arg(op, b, mode == MODE_IOU_3D)
    ca = _as_corners(op, a, n_a, mode == MODE_IOU_3D)
    cb = _as_corners(op, b, n_b, mode == MODE_IOU_3D)
    if ca.bev.device != cb.bev.device:
        raise ValueError(f"{op}: a is on {ca.bev.device}, b on {cb.bev.device}")
    dev = ca.bev.device
    with torch.cuda.device(dev), torch.no_grad():
        out = torch.empty((ca.num_boxes, cb.num_boxes), dtype=torch.float32, device=dev)
        if out.numel() > 0:
            overlap_into(ca, cb, mode, out)
    return out


def boxes_overlap_bev(a: Boxes, b: Boxes, *, n_a: Optional[torch.Tensor] = None,
                      n_b: Optional[torch.Tensor] = None) -> torch.Tensor:
    """fp32 [M, N]: the area the bird's-eye quads of a[i] and b[j] share (``boxes_overlap_bev_gpu``).  a / b: boxes
    fp32 [*, >= 7] or ``BoxCorners``; the boxes form is the corners launch followed by the corners form (identical
    bits).  Sutherland-Hodgman of a[i] (the subject) against the edges of b[j] behind a bounding-rectangle reject, in
    fp32 with every operation rounded on its own, clamped to the smaller of the two areas.  A pair with an invalid box,
    a row at or beyond *n_a and a column at or beyond *n_b give 0; every element is written.  One launch over the
    (M, N) grid.  No gradient."""
    return _pairs("boxes_overlap_bev", a, b, MODE_OVERLAP_BEV, n_a, n_b)


def boxes_iou_bev(a: Boxes, b: Boxes, *, n_a: Optional[torch.Tensor] = None,
                  n_b: Optional[torch.Tensor] = None) -> torch.Tensor:
    """fp32 [M, N]: ``inter / max((area_a + area_b) - inter, 1e-8)`` over the overlap of ``boxes_overlap_bev``
    (``boxes_iou_bev``).  At most 1; a box with itself gives exactly 1.  No gradient."""
    return _pairs("boxes_iou_bev", a, b, MODE_IOU_BEV, n_a, n_b)


def boxes_iou3d(a: Boxes, b: Boxes, *, n_a: Optional[torch.Tensor] = None,
                n_b: Optional[torch.Tensor] = None) -> torch.Tensor:
    """fp32 [M, N]: the IoU in space (``boxes_iou3d_gpu``): the overlap in the plane times the shared height ``max(
    min(zmax_a, zmax_b) - max(zmin_a, zmin_b), 0)``, over ``max((vol_a + vol_b) - inter3d, 1e-6)`` with vol = area *
    (zmax - zmin).  No gradient."""
    return _pairs("boxes_iou3d", a, b, MODE_IOU_3D, n_a, n_b)


def boxes_iou3d_aligned(a: Boxes, b: Boxes, *, n_a: Optional[torch.Tensor] = None,
                        n_b: Optional[torch.Tensor] = None) -> torch.Tensor:
    """fp32 [N]: ``boxes_iou3d(a, b)[i, i]`` for two tables of the same length, one value per pair, one launch.  No
    gradient."""
    op = "boxes_iou3d_aligned"
    na, nb = _check_arg(op, a, True), _check_arg(op, b, True)
    if na != nb:
        raise ValueError(f"{op}: one box of b per box of a, got {na} and {nb}")
    ca, cb = _as_corners(op, a, n_a, True), _as_corners(op, b, n_b, True)
    if ca.bev.device != cb.bev.device:
        raise ValueError(f"{op}: a is on {ca.bev.device}, b on {cb.bev.device}")
    dev, N = ca.bev.device, ca.num_boxes
    with torch.cuda.device(dev), torch.no_grad():
        out = torch.empty((N,), dtype=torch.float32, device=dev)
        if N > 0:
            _lib.check(_lib.load().spx_boxes_overlap_aligned(
                ca.bev.data_ptr(), _ptr(ca.zrange), _ptr(ca.n_boxes), cb.bev.data_ptr(), _ptr(cb.zrange), _ptr(cb.n_boxes),
                N, MODE_IOU_3D, out.data_ptr(), _stream(out)))
    return out


def _check_nms(op: str, thresh, pre_max, post_max, score_thresh, batch_size) -> None:
    if int(batch_size) < 1:
        raise ValueError(f"{op}: batch_size must be >= 1, got {batch_size}")
    if int(pre_max) != pre_max or not 1 <= int(pre_max) <= MAX_PRE:
        raise ValueError(f"{op}: pre_max must be in 1 .. {MAX_PRE}, got {pre_max}")
    if int(post_max) != post_max or not 1 <= int(post_max) <= int(pre_max):
        raise ValueError(f"{op}: post_max must be in 1 .. pre_max = {pre_max}, got {post_max}")
    if thresh is None or float(thresh) != float(thresh):
        raise ValueError(f"{op}: thresh must be a number, got {thresh}")
    if score_thresh is not None and float(score_thresh) != float(score_thresh):
        raise ValueError(f"{op}: score_thresh must be None or a number, got {score_thresh}")


def nms_rotated_into(corners: BoxCorners, scores: torch.Tensor, thresh: float, keep: torch.Tensor, count: torch.Tensor,
                     ws: torch.Tensor, *, batch_ids: Optional[torch.Tensor] = None, batch_size: int = 1,
                     class_ids: Optional[torch.Tensor] = None, pre_max: int = 4096,
                     score_thresh: Optional[float] = None) -> None:
    """``nms_rotated`` into buffers the caller owns (no allocation: capturable).  corners: a ``BoxCorners`` (its n_boxes
    is the device count); keep int32 [batch_size, post_max] (post_max is its width), count int32 [batch_size], ws:
    uint8, at least ``nms_ws_bytes(N, batch_size, pre_max)`` bytes, handed over in any state."""
    op = "nms_rotated_into"
    N = _check_corners(op, corners, False)
    if keep.dim() != 2 or keep.dtype != torch.int32 or int(keep.shape[0]) != int(batch_size) or not keep.is_contiguous():
        raise ValueError(f"{op}: keep is a contiguous int32 tensor [batch_size, post_max], got {tuple(keep.shape)} "
                         f"{keep.dtype}")
    post_max = int(keep.shape[1])
    _check_nms(op, thresh, pre_max, post_max, score_thresh, batch_size)
    if count.dtype != torch.int32 or tuple(count.shape) != (int(batch_size),) or not count.is_contiguous():
        raise ValueError(f"{op}: count is a contiguous int32 tensor [{int(batch_size)}], got {tuple(count.shape)} "
                         f"{count.dtype}")
    _check_f32(op, "scores", scores, lambda t: tuple(t.shape) == (N,), f"[{N}]")
    _check_ids(op, "batch_ids", batch_ids, N)
    _check_ids(op, "class_ids", class_ids, N)
    for t, what in ((corners.bev, "bev"), (scores, "scores"), (keep, "keep"), (count, "count"), (ws, "ws")):
        _require_gpu(t, what)
    for t, what in ((batch_ids, "batch_ids"), (class_ids, "class_ids")):
        if t is not None:
            _require_gpu(t, what)
    _check_count(corners.n_boxes, f"{op}: n_boxes")
    if ws.dtype != torch.uint8 or not ws.is_contiguous():
        raise ValueError(f"{op}: ws is a contiguous uint8 tensor")
    _lib.check(_lib.load().spx_nms_rotated(
        corners.bev.data_ptr(), scores.data_ptr(), _ptr(batch_ids), _ptr(class_ids), N, _ptr(corners.n_boxes),
        int(batch_size), float(thresh), 0 if score_thresh is None else 1,
        0.0 if score_thresh is None else float(score_thresh), int(pre_max), post_max, keep.data_ptr(), count.data_ptr(),
        ws.data_ptr(), ws.numel(), _stream(scores)))


def nms_rotated(boxes: Boxes, scores: torch.Tensor, thresh: float, *, batch_ids: Optional[torch.Tensor] = None,
                batch_size: int = 1, class_ids: Optional[torch.Tensor] = None, pre_max: int = 4096, post_max: int = 512,
                score_thresh: Optional[float] = None, n_boxes: Optional[torch.Tensor] = None) -> BoxNMS:
    """Rotated non-maximum suppression per scene, wholly on the device (``nms_gpu``, batched).  boxes: fp32 [N, >= 7] or
    ``BoxCorners``; scores fp32 [N]; batch_ids / class_ids int32 [N] or None (all scene 0 / one class).  A candidate is
    a valid box below *n_boxes whose batch id is in [0, batch_size), whose score is not NaN and, with `score_thresh`,
    is above it.  Per scene the candidates are ranked by (score descending, index ascending) and only the first
    `pre_max` (1 .. 16384) take part.  A candidate is kept if and only if no earlier-ranked KEPT candidate of its scene
    -- with class_ids: and of its class -- has ``iou_bev(earlier, it) > thresh`` (strict, the earlier one the subject);
    a scene stops at `post_max` (1 .. pre_max) kept boxes.  Returns ``BoxNMS``: keep int32 [batch_size, post_max] (box
    indices in rank order, -1 behind them) and count int32 [batch_size], every element written; ``.indices(scene)`` is
    the trimmed 1-D tensor at the price of one read-back.  Launches: key, the radix sort of ``serialize``, mask,
    reduce; nothing read back.  No gradient."""
    op = "nms_rotated"
    _check_nms(op, thresh, pre_max, post_max, score_thresh, batch_size)
    if isinstance(boxes, BoxCorners):
        N = _check_corners(op, boxes, False)
    else:
        N = _check_boxes(op, boxes)
    _check_f32(op, "scores", scores, lambda t: tuple(t.shape) == (N,), f"[{N}]")
    _check_ids(op, "batch_ids", batch_ids, N)
    _check_ids(op, "class_ids", class_ids, N)
    corners = _as_corners(op, boxes, n_boxes, False)
    dev = corners.bev.device
    B = int(batch_size)
    with torch.cuda.device(dev), torch.no_grad():
        keep = torch.empty((B, int(post_max)), dtype=torch.int32, device=dev)
        count = torch.empty((B,), dtype=torch.int32, device=dev)
        ws = _ws(nms_ws_bytes(N, B, pre_max), dev)
        nms_rotated_into(corners, scores.detach(), thresh, keep, count, ws, batch_ids=batch_ids, batch_size=B,
                         class_ids=class_ids, pre_max=int(pre_max), score_thresh=score_thresh)
    return BoxNMS(keep, count, int(post_max))
