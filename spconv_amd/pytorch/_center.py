"""Training targets of the centre heads on the HIP kernels of csrc/center.hip (``functional.box_centers`` /
``center_heatmap`` / ``center_heatmap_sparse`` and their ``_into`` forms, ``spatial.CenterHeadTargets``).  Not part of the
reference; the detectors users port (CenterPoint, VoxelNeXt, TransFusion, DSVT, HEDNet, SAFDNet) build them in
OpenPCDet's ``CenterHead.assign_target_of_single_head`` -- a Python loop over the ground-truth boxes with a read-back per
box.

  * ``box_centers``            per box its centre in cells, cell, Gaussian radius, class plane and slot, per scene the
                               tables ``box_index`` / ``mask`` / ``inds`` [B, max_objs] (``spx_box_centers``: one launch
                               behind the scene list of the boxes), as a ``BoxCenters``
  * ``center_heatmap``         the dense maps [B, C, H, W] (``spx_center_heatmap``: a lane per cell, no atomics, no fill)
  * ``center_heatmap_sparse``  the heat of the rows of a sparse 2-D level [N, C] with the nearest row of every box
                               (``spx_center_nearest``, ``spx_center_heatmap_sparse``), as a ``SparseCenters``

Nothing is read back, every output element is written by the call that owns it, results are identical run to run, and
every call has an ``_into`` form over buffers the caller owns: the chain replays from a captured graph with other
device-side counts.  Targets have no gradient.  tests/refcenter.py restates every table in numpy float32.
"""
from __future__ import annotations

import math
from typing import NamedTuple, Optional, Tuple

import torch

from spconv_amd import _lib
from spconv_amd.pytorch import _pointvoxel
from spconv_amd.pytorch._box import _check_boxes, _check_ids
from spconv_amd.pytorch._pointvoxel import PointGroups
from spconv_amd.pytorch._rulebook import _check_count, _ptr, _require_gpu, _stream, _ws
from spconv_amd.pytorch._sample import scene_groups

MAX_CLASSES, MAX_EXTENT, MAX_RADIUS = 64, 1 << 23, 1 << 20        # SPX_CENTER_MAX_CLASSES, the limits of the header
ANCHOR_CENTER, ANCHOR_NEAREST = 0, 1                               # SPX_CENTER_ANCHOR_*
CUTOFF_NONE, CUTOFF_WINDOW = 0, 1                                  # SPX_CENTER_CUTOFF_*
_ANCHORS = {"center": ANCHOR_CENTER, "nearest": ANCHOR_NEAREST}
_CUTOFFS = {"none": CUTOFF_NONE, "window": CUTOFF_WINDOW}


class CenterParams(NamedTuple):
    """The host parameters of a centre head's map: grid_size (W, H), voxel_size (vx, vy), range_min (x0, y0), stride,
    num_classes (C), max_objs, min_overlap, min_radius, batch_size (B)."""
    grid_size: Tuple[int, int]
    voxel_size: Tuple[float, float]
    range_min: Tuple[float, float]
    stride: float
    num_classes: int
    max_objs: int
    min_overlap: float
    min_radius: int
    batch_size: int


class BoxCenters(NamedTuple):
    """What ``box_centers`` writes.  Per box: center fp32 [M, 2] (cx, cy in cells), cell int32 [M, 2] (ix, iy), radius
    int32 [M] (zeros for a box without a valid geometry), cls int32 [M] (the class plane, -1: the box takes no part),
    slot int32 [M] (its position among the boxes of its scene, -1: none).  Per scene: box_index int32 [B, max_objs] (-1
    past the scene's boxes), mask int32 [B, max_objs], inds int32 [B, max_objs] (``iy * W + ix``, 0 where the mask is
    0).  groups: the ``scene_groups`` of the box batch ids; params: a ``CenterParams``; n_boxes: the device box count
    or None."""
    center: torch.Tensor
    cell: torch.Tensor
    radius: torch.Tensor
    cls: torch.Tensor
    slot: torch.Tensor
    box_index: torch.Tensor
    mask: torch.Tensor
    inds: torch.Tensor
    groups: PointGroups
    params: CenterParams
    n_boxes: Optional[torch.Tensor] = None


class SparseCenters(NamedTuple):
    """What ``center_heatmap_sparse`` writes: heat fp32 [N, C], nearest int32 [M] (per box that takes part the nearest
    live row of its scene, -1: none), inds int32 [B, max_objs] (that row for the box of every slot -- a GLOBAL row
    index --, 0 where the mask is 0), mask int32 [B, max_objs] (the box takes part and has a nearest row)."""
    heat: torch.Tensor
    nearest: torch.Tensor
    inds: torch.Tensor
    mask: torch.Tensor


def center_tile() -> int:
    """Box records a heat kernel stages at a time."""
    return int(_lib.load().spx_center_tile())


def _pair(op: str, name: str, value, kind):
    try:
        out = tuple(kind(v) for v in value)
        exact = all(kind(v) == v for v in value)
    except (TypeError, ValueError):
        out, exact = (), False
    if len(out) != 2 or not exact:
        raise ValueError(f"{op}: {name} is two {'ints' if kind is int else 'floats'}, got {value!r}")
    return out


def check_params(op: str, batch_size, grid_size, voxel_size, range_min, stride, num_classes, max_objs, min_overlap,
                 min_radius) -> CenterParams:
    """Every ValueError of the host parameters (they come before any tensor is looked at)."""
    B = int(batch_size)
    if B < 1 or B > 65535:
        raise ValueError(f"{op}: batch_size must be in 1 .. 65535, got {batch_size}")
    W, H = _pair(op, "grid_size", grid_size, int)
    if not (1 <= W <= MAX_EXTENT and 1 <= H <= MAX_EXTENT):
        raise ValueError(f"{op}: grid_size is two extents (W, H) in 1 .. {MAX_EXTENT}, got {grid_size!r}")
    vx, vy = _pair(op, "voxel_size", voxel_size, float)
    if not (0. < vx < math.inf and 0. < vy < math.inf):
        raise ValueError(f"{op}: voxel_size is two positive finite floats, got {voxel_size!r}")
    x0, y0 = _pair(op, "range_min", range_min, float)
    if not (abs(x0) < math.inf and abs(y0) < math.inf):
        raise ValueError(f"{op}: range_min is two finite floats, got {range_min!r}")
    try:
        s = float(stride)
    except (TypeError, ValueError):
        s = math.nan
    if not 0. < s < math.inf:
        raise ValueError(f"{op}: stride must be a positive finite float, got {stride!r}")
    if int(num_classes) != num_classes or not 1 <= int(num_classes) <= MAX_CLASSES:
        raise ValueError(f"{op}: num_classes must be in 1 .. {MAX_CLASSES}, got {num_classes!r}")
    if int(max_objs) != max_objs or int(max_objs) < 1 or B * int(max_objs) >= 1 << 31:
        raise ValueError(f"{op}: max_objs must be >= 1 (and batch_size * max_objs below 2^31), got {max_objs!r}")
    if not 0. < float(min_overlap) < 1.:
        raise ValueError(f"{op}: min_overlap must lie inside (0, 1), got {min_overlap!r}")
    if int(min_radius) != min_radius or not 0 <= int(min_radius) <= MAX_RADIUS:
        raise ValueError(f"{op}: min_radius must be in 0 .. {MAX_RADIUS}, got {min_radius!r}")
    if B * int(num_classes) * H * W >= 1 << 31:
        raise ValueError(f"{op}: {B} x {int(num_classes)} x {H} x {W} elements do not fit 32-bit entries")
    return CenterParams((W, H), (vx, vy), (x0, y0), s, int(num_classes), int(max_objs), float(min_overlap),
                        int(min_radius), B)


def _check_classes(op: str, class_ids: Optional[torch.Tensor], M: int) -> None:
    if class_ids is None:
        return
    if not isinstance(class_ids, torch.Tensor) or class_ids.dtype not in (torch.int32, torch.int64) or \
            tuple(class_ids.shape) != (M,):
        got = f"{tuple(class_ids.shape)} {class_ids.dtype}" if isinstance(class_ids, torch.Tensor) else type(class_ids).__name__
        raise ValueError(f"{op}: class_ids is an int32 or int64 tensor [{M}], got {got}")
    if not class_ids.is_contiguous():
        raise ValueError(f"{op}: class_ids must be contiguous")


def _check_centers(op: str, centers) -> None:
    if not isinstance(centers, BoxCenters):
        raise ValueError(f"{op}: centers is the BoxCenters of box_centers, got {type(centers).__name__}")


def center_buffers(num_boxes: int, params: CenterParams, device) -> BoxCenters:
    """The tables of ``box_centers_into`` for M boxes (allocated here, once) with the buffers of the scene list; the
    ``groups`` field carries rows / offsets / list, the scratch of the list is ``center_groups_ws``."""
    M, B = int(num_boxes), params.batch_size
    i32 = dict(dtype=torch.int32, device=device)
    e = lambda *shape: torch.empty(shape, **i32)
    groups = PointGroups(e(M), e(B + 1), e(M), B)
    return BoxCenters(torch.empty((M, 2), dtype=torch.float32, device=device), e(M, 2), e(M), e(M), e(M),
                      e(B, params.max_objs), e(B, params.max_objs), e(B, params.max_objs), groups, params)


def center_groups_ws(num_boxes: int, batch_size: int, device) -> torch.Tensor:
    """The scratch ``box_centers_into`` hands to the scene list of M box batch ids."""
    return _ws(_lib.load().spx_point_groups_ws_bytes(int(num_boxes), int(batch_size)), device)


def box_centers_into(boxes: torch.Tensor, b_batch_ids: Optional[torch.Tensor], class_ids: Optional[torch.Tensor],
                     n_boxes: Optional[torch.Tensor], out: BoxCenters, groups_ws: Optional[torch.Tensor] = None) -> BoxCenters:
    """The capturable form, into ``center_buffers``: the scene list of the box batch ids (with `groups_ws` from
    ``center_groups_ws``, which needs int32 `b_batch_ids`: ValueError without them; without `groups_ws` ``out.groups``
    is taken as built) and the records.  No allocation, nothing read back.  Returns `out` with the device count
    attached."""
    p = out.params
    M = int(boxes.shape[0])
    if groups_ws is not None:
        if b_batch_ids is None:
            raise ValueError("box_centers_into: the scene list is built from int32 b_batch_ids; without them leave "
                             "groups_ws out and hand over out.groups as built")
        if M > 0:
            _pointvoxel.point_groups_into(b_batch_ids, p.batch_size, n_boxes, out.groups.rows, out.groups.offsets,
                                          out.groups.list, groups_ws)
        else:
            out.groups.offsets.zero_()                    # no box: every scene is the empty range (a fill: capturable)
    _lib.check(_lib.load().spx_box_centers(
        _ptr(boxes), int(boxes.shape[1]), _ptr(b_batch_ids), _ptr(class_ids),
        8 if class_ids is not None and class_ids.dtype == torch.int64 else 4, M, _ptr(n_boxes),
        out.groups.offsets.data_ptr(), _ptr(out.groups.list), p.batch_size, p.grid_size[0], p.grid_size[1],
        p.voxel_size[0], p.voxel_size[1], p.range_min[0], p.range_min[1], p.stride, p.num_classes, p.max_objs,
        p.min_overlap, p.min_radius, _ptr(out.center), _ptr(out.cell), _ptr(out.radius), _ptr(out.cls), _ptr(out.slot),
        out.box_index.data_ptr(), out.mask.data_ptr(), out.inds.data_ptr(), _stream(out.box_index)))
    return out._replace(n_boxes=n_boxes)


def box_centers(boxes: torch.Tensor, b_batch_ids: Optional[torch.Tensor], class_ids: Optional[torch.Tensor],
                batch_size: int, *, grid_size, voxel_size, range_min, stride, num_classes: int, max_objs: int = 500,
                min_overlap: float = 0.1, min_radius: int = 2, n_boxes: Optional[torch.Tensor] = None) -> BoxCenters:
    """The records of the ground-truth boxes of a centre head.  boxes fp32 [M, >= 7] = OpenPCDet's (x, y, z, dx, dy,
    dz, heading), b_batch_ids int32 [M] or None (all scene 0), class_ids int32 / int64 [M] 0-based planes or None (all
    class 0); grid_size (W, H) cells of voxel_size (vx, vy) * stride from range_min (x0, y0).  Per box, in float32 with
    every operation rounded on its own: ``cx = ((x - x0) / vx) / stride`` clamped to [0, W - 0.5] (a centre outside the
    range lands on the border, as in OpenPCDet), ``ix = int(cx)``, likewise y against H; ``w = (dx / vx) / stride``,
    ``h = (dy / vy) / stride`` and ``radius = max(int(gaussian_radius(h, w, min_overlap)), min_radius)`` with CornerNet's
    formula (the header of ``spx_box_centers`` spells it).  A box takes part when it lies below *n_boxes, its batch id
    is in [0, batch_size) and its class in [0, num_classes), its seven numbers are finite, dx, dy, dz > 0 and the
    radius is finite and below 2^20.  Its slot is its position among the boxes of its scene in ascending box index,
    counting every box of the scene below *n_boxes, taking part or not: a padded [B, max, 8] tensor flattened keeps
    OpenPCDet's slots, and a box of another head (class -1) keeps its slot with mask 0.  A slot at or beyond `max_objs`
    does not exist: that box takes no part.  Returns a ``BoxCenters``.  Launches: the scene list of the boxes, the
    records; nothing read back.  No gradient."""
    op = "box_centers"
    params = check_params(op, batch_size, grid_size, voxel_size, range_min, stride, num_classes, max_objs, min_overlap,
                          min_radius)
    M = _check_boxes(op, boxes)
    _check_ids(op, "b_batch_ids", b_batch_ids, M)
    _check_classes(op, class_ids, M)
    _require_gpu(boxes, "boxes")
    if b_batch_ids is not None:
        _require_gpu(b_batch_ids, "b_batch_ids")
    if class_ids is not None:
        _require_gpu(class_ids, "class_ids")
    _check_count(n_boxes, f"{op}: n_boxes")
    dev = boxes.device
    with torch.cuda.device(dev), torch.no_grad():
        out = center_buffers(M, params, dev)
        out = out._replace(groups=scene_groups(b_batch_ids, M, params.batch_size, n_boxes, dev))
        return box_centers_into(boxes.detach(), b_batch_ids, class_ids, n_boxes, out)


def center_heatmap_into(centers: BoxCenters, out: torch.Tensor) -> torch.Tensor:
    """The one C call into a buffer the caller owns (capturable): out fp32 [B, C, H, W], every element written."""
    p = centers.params
    _lib.check(_lib.load().spx_center_heatmap(
        _ptr(centers.cell), _ptr(centers.radius), _ptr(centers.cls), int(centers.cls.shape[0]),
        centers.groups.offsets.data_ptr(), _ptr(centers.groups.list), p.batch_size, p.grid_size[0], p.grid_size[1],
        p.num_classes, out.data_ptr(), _stream(out)))
    return out


def center_heatmap(centers: BoxCenters, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """fp32 [B, C, H, W]: element (b, c, y, x) is the maximum, over the boxes of scene b and class c that take part
    with ``|x - ix| <= radius`` and ``|y - iy| <= radius``, of ``expf(-(ddx * ddx + ddy * ddy) / (2 * sigma * sigma))``
    with ``sigma = (2 * radius + 1) / 6`` and the integers ddx = x - ix, ddy = y - iy; 0 where no box reaches
    (``draw_gaussian_to_heatmap`` over every box of ``assign_target_of_single_head``).  A lane per cell gathers the
    boxes of its scene: no atomics, no zero fill, every element of `out` (given or allocated) written once, identical
    run to run and for any order of the boxes that keeps their slots.  One launch, nothing read back.  No gradient."""
    op = "center_heatmap"
    _check_centers(op, centers)
    p = centers.params
    shape = (p.batch_size, p.num_classes, p.grid_size[1], p.grid_size[0])
    if out is not None and (not isinstance(out, torch.Tensor) or out.dtype != torch.float32 or tuple(out.shape) != shape
                            or not out.is_contiguous()):
        raise ValueError(f"{op}: out is a contiguous float32 tensor {list(shape)}")
    _require_gpu(centers.cls, "centers")
    if out is not None:
        _require_gpu(out, "out")
    dev = centers.cls.device
    with torch.cuda.device(dev), torch.no_grad():
        if out is None:
            out = torch.empty(shape, dtype=torch.float32, device=dev)
        return center_heatmap_into(centers, out)


def center_nearest_into(centers: BoxCenters, indices: torch.Tensor, row_groups: PointGroups,
                        n_live: Optional[torch.Tensor], nearest: torch.Tensor, inds: torch.Tensor,
                        mask: torch.Tensor) -> None:
    """The one C call into buffers the caller owns (capturable): nearest int32 [M], inds / mask int32 [B, max_objs].
    row_groups: ``point_groups(indices[:, 0], B, n_live)``.  The scene of a box is ``centers.groups.rows``."""
    p = centers.params
    _lib.check(_lib.load().spx_center_nearest(
        _ptr(centers.center), _ptr(centers.cls), _ptr(centers.groups.rows), int(centers.cls.shape[0]), _ptr(indices),
        int(indices.shape[0]), _ptr(n_live), row_groups.offsets.data_ptr(), _ptr(row_groups.list), p.batch_size,
        p.grid_size[0], p.grid_size[1], centers.box_index.data_ptr(), centers.mask.data_ptr(), p.max_objs,
        _ptr(nearest), inds.data_ptr(), mask.data_ptr(), _stream(inds)))


def center_heatmap_sparse_into(centers: BoxCenters, indices: torch.Tensor, n_live: Optional[torch.Tensor],
                               nearest: Optional[torch.Tensor], anchor: str, cutoff: str, heat: torch.Tensor) -> None:
    """The one C call into a buffer the caller owns (capturable): heat fp32 [N, C]; nearest (of ``center_nearest_into``)
    is needed for anchor="nearest" only."""
    p = centers.params
    _lib.check(_lib.load().spx_center_heatmap_sparse(
        _ptr(centers.center), _ptr(centers.cell), _ptr(centers.radius), _ptr(centers.cls), _ptr(nearest),
        int(centers.cls.shape[0]), centers.groups.offsets.data_ptr(), _ptr(centers.groups.list), _ptr(indices),
        int(indices.shape[0]), _ptr(n_live), p.batch_size, p.grid_size[0], p.grid_size[1], p.num_classes,
        _ANCHORS[anchor], _CUTOFFS[cutoff], heat.data_ptr(), _stream(heat)))


def _level(op: str, x):
    """(indices, n_live of the tensor) of a SparseConvTensor or an index tensor; the ValueErrors of its shape."""
    n_live = None
    if hasattr(x, "indices") and hasattr(x, "spatial_shape"):
        if len(x.spatial_shape) != 2:
            raise ValueError(f"{op}: a centre head sits on a 2-D level (behind SparseCollapse), got ndim "
                             f"{len(x.spatial_shape)}")
        n_live = getattr(x, "n_live_dev", None)
        x = x.indices
    if not isinstance(x, torch.Tensor) or x.dim() != 2 or x.dtype != torch.int32:
        got = f"{tuple(x.shape)} {x.dtype}" if isinstance(x, torch.Tensor) else type(x).__name__
        raise ValueError(f"{op}: indices is an int32 tensor [N, 3] = (b, y, x), got {got}")
    if int(x.shape[1]) != 3:
        raise ValueError(f"{op}: a centre head sits on a 2-D level: indices [N, 3] = (b, y, x), got ndim "
                         f"{int(x.shape[1]) - 1}")
    return x, n_live


def center_heatmap_sparse(centers: BoxCenters, x, *, anchor: str = "center", cutoff: str = "none",
                          n_live: Optional[torch.Tensor] = None) -> SparseCenters:
    """The heat of the rows of a sparse 2-D level (VoxelNeXt's head behind ``SparseCollapse``).  x: a 2-D
    SparseConvTensor (its n_live_dev is the device row count) or indices int32 [N, 3] = (b, y, x).  A row is live when it lies below *n_live, its batch id
    is in [0, B) and its cell inside W x H.  For every box that takes part, ``nearest`` is the live row of its scene
    with the least ``d2 = (float(vx) - cx) ** 2 + (float(vy) - cy) ** 2`` (float32, the x term first), ties to the
    lowest row, -1 for a scene without live rows.  ``heat[i, c]`` is the maximum over the boxes of row i's scene and
    class c of ``expf(-d / (2 * sigma * sigma))`` with sigma as in ``center_heatmap``: anchor="center" (VoxelNeXt's
    ``gt_center``) takes d = d2 and centres the window on the box's cell, anchor="nearest" the integer squared distance
    to the nearest row's cell and centres the window there (a box without a nearest row draws nothing);
    cutoff="window" keeps the dense rule ``|.| <= radius``, cutoff="none" (VoxelNeXt) lets a box reach every live row
    of its scene.  Rows that are not live get zeros.  Returns a ``SparseCenters``; its inds are GLOBAL row indices.
    Launches: the scene list of the rows, the nearest rows and their tables, the heat; nothing read back.  No
    gradient."""
    op = "center_heatmap_sparse"
    _check_centers(op, centers)
    if anchor not in _ANCHORS:
        raise ValueError(f"{op}: anchor is 'center' or 'nearest', got {anchor!r}")
    if cutoff not in _CUTOFFS:
        raise ValueError(f"{op}: cutoff is 'none' or 'window', got {cutoff!r}")
    indices, live = _level(op, x)
    n_live = live if n_live is None else n_live
    M, N = int(centers.cls.shape[0]), int(indices.shape[0])
    p = centers.params
    if N * p.num_classes >= 1 << 31:
        raise ValueError(f"{op}: {N} rows x {p.num_classes} classes do not fit 32-bit entries")
    _require_gpu(centers.cls, "centers")
    _require_gpu(indices, "indices")
    _check_count(n_live, f"{op}: n_live")
    dev = indices.device
    with torch.cuda.device(dev), torch.no_grad():
        indices = indices.contiguous()
        i32 = dict(dtype=torch.int32, device=dev)
        rows = scene_groups(indices[:, 0].contiguous() if N > 0 else None, N, p.batch_size, n_live, dev)
        nearest = torch.empty((M,), **i32)
        inds, mask = torch.empty((p.batch_size, p.max_objs), **i32), torch.empty((p.batch_size, p.max_objs), **i32)
        heat = torch.empty((N, p.num_classes), dtype=torch.float32, device=dev)
        center_nearest_into(centers, indices, rows, n_live, nearest, inds, mask)
        if N > 0:
            center_heatmap_sparse_into(centers, indices, n_live, nearest, anchor, cutoff, heat)
    return SparseCenters(heat, nearest, inds, mask)
