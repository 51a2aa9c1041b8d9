"""Points in rotated boxes, RoI point pooling and RoI-aware pooling on the HIP kernels of csrc/roi.hip
(``functional.boxes_to_frames`` / ``points_in_boxes`` / ``box_query`` / ``box_query_into`` / ``roi_point_pool`` /
``roi_aware_pool``, ``spatial.RoIPointPool3d`` / ``RoIAwarePool3d``).  Not part of the reference; the two-stage
detectors users port call them as the ``roiaware_pool3d`` / ``roipoint_pool3d`` CUDA extensions of OpenPCDet / mmdet3d
(``points_in_boxes_gpu``: PV-RCNN's keypoint labels, PointRCNN's and Part-A2's segmentation targets, ground-truth
sampling; ``roipoint_pool3d``: PointRCNN's second stage; ``roiaware_pool3d``: Part-A2's).

  * ``BoxFrames``        centre, enlarged half sizes, cosine and sine of every box (``spx_boxes_to_frames``: one launch),
                         or the caller's own; an invalid box holds NaN and contains nothing
  * ``points_in_boxes``  per point the lowest box index of its scene that contains it (``spx_points_in_boxes``)
  * ``box_query``        per box the first ``nsample`` points of its scene inside it, in ascending point index, with the
                         total, the points in the box's frame and their cells of a grid over the box
                         (``spx_box_query``), as a ``BoxPoints``
  * ``BoxPoints.neighbors()``  the ``VoxelNeighbors`` that ``group_voxels`` and its gradient take
  * ``roi_point_pool`` / ``roi_aware_pool``  compositions of the query with ``group_voxels``, ``point_groups`` and
                         ``points_to_voxels``: no kernel of their own, the gradients are the existing fixed-order ones

There is no gradient with respect to coordinates or boxes.  tests/refroi.py restates every table in numpy float32.
"""
from __future__ import annotations

import math
from typing import NamedTuple, Optional, Sequence, Tuple, Union

import torch

from spconv_amd import _lib
from spconv_amd.pytorch._box import _check_boxes, _check_f32, _check_ids
from spconv_amd.pytorch._level import flat_groups
from spconv_amd.pytorch._pointvoxel import PointGroups, point_groups, points_to_voxels
from spconv_amd.pytorch._query import VoxelNeighbors, group_voxels
from spconv_amd.pytorch._rulebook import _check_count, _float_code, _ptr, _require_gpu, _stream
from spconv_amd.pytorch._sample import _check_cloud, _check_groups, _require_cloud, scene_groups

MAX_NSAMPLE, MAX_GRID = 16384, 64
PAD_NONE, PAD_FIRST, PAD_CYCLE = 0, 2, 4                  # SPX_ROI_PAD_*
_PADS = {"none": PAD_NONE, "first": PAD_FIRST, "cycle": PAD_CYCLE}


class BoxFrames(NamedTuple):
    """frames fp32 [M, 8] = (x, y, z, hx, hy, hz, c, s): the centre, the enlarged half sizes and the cosine and sine of
    the heading (from ``boxes_to_frames``, or built by hand), num_boxes (M), n_boxes (device int32 or None: boxes at or
    beyond it do not exist).  A frame with a NaN contains nothing."""
    frames: torch.Tensor
    num_boxes: int
    n_boxes: Optional[torch.Tensor] = None


class BoxPoints(NamedTuple):
    """The points of every box: rows int32 [M, nsample] (point index, -1: none), count int32 [M] = min(hits, nsample),
    hits int32 [M] (all points inside, uncapped), local fp32 [M, nsample, 3] (the kept points in the box's frame) or
    None, cells int32 [M, nsample] (global cell id ``m * ox * oy * oz + (ix * oy + iy) * oz + iz``, -1: none) or None,
    groups (a ``PointGroups`` over the FLATTENED rows -- entry e = m * nsample + s -- or None: only a gradient needs
    it), nsample, num_points (N), grid ((ox, oy, oz) or None), n_boxes / n_points (device int32 or None: boxes / points
    at or beyond them do not exist)."""
    rows: torch.Tensor
    count: torch.Tensor
    hits: torch.Tensor
    local: Optional[torch.Tensor]
    cells: Optional[torch.Tensor]
    groups: Optional[PointGroups]
    nsample: int
    num_points: int
    grid: Optional[Tuple[int, int, int]] = None
    n_boxes: Optional[torch.Tensor] = None
    n_points: Optional[torch.Tensor] = None

    def neighbors(self) -> VoxelNeighbors:
        """The table as ``group_voxels(point_feats, ...)`` takes it (num_voxels = N, n_live = n_points; nsample <= 128,
        the widest table ``spx_group_fwd`` accepts: ``gather`` has no such limit); its offsets are the points in the
        box's frame."""
        return VoxelNeighbors(self.rows, self.count, self.local, self.groups, self.num_points, self.n_boxes,
                              self.n_points)

    def gather(self, feats: torch.Tensor) -> torch.Tensor:
        """[N, C] point rows -> [M, nsample, C]: ``group_voxels`` over the table taken as M * nsample queries of one slot
        each.  ``spx_group_fwd`` refuses more than 128 slots per query, and a gather does not care where a query ends:
        the entries e = m * nsample + s, the groups over them and the fixed-order gradient are the same, for any
        nsample."""
        M, S = (int(v) for v in self.rows.shape)
        nb = VoxelNeighbors(self.rows.reshape(M * S, 1), self.count, None, self.groups, self.num_points, None,
                            self.n_points)
        return group_voxels(feats, nb).reshape(M, S, int(feats.shape[1]))


Boxes = Union[torch.Tensor, BoxFrames]


def max_nsample() -> int:
    return int(_lib.load().spx_box_query_max_nsample())


def _extra(op: str, extra_width) -> Tuple[float, float, float]:
    """The three extra widths of a float or a 3-tuple: finite and >= 0."""
    try:
        e = tuple(float(v) for v in extra_width) if isinstance(extra_width, (tuple, list)) else (float(extra_width),) * 3
    except (TypeError, ValueError):
        e = ()
    if len(e) != 3 or not all(0.0 <= v < math.inf for v in e):
        raise ValueError(f"{op}: extra_width is a float or three floats, finite and >= 0, got {extra_width!r}")
    return e


def _check_frames(op: str, f: BoxFrames) -> int:
    _check_f32(op, "frames", f.frames, lambda t: t.dim() == 2 and t.shape[1] == 8, "[M, 8]")
    if int(f.num_boxes) != int(f.frames.shape[0]):
        raise ValueError(f"{op}: num_boxes is {f.num_boxes}, frames holds {int(f.frames.shape[0])} boxes")
    return int(f.frames.shape[0])


def _check_arg(op: str, b: Boxes, extra_width) -> int:
    """The ValueErrors of a boxes-or-frames argument; they come before the refusal of a CPU tensor."""
    if isinstance(b, BoxFrames):
        if extra_width is not None:
            raise ValueError(f"{op}: extra_width belongs to boxes_to_frames; these frames are enlarged already")
        return _check_frames(op, b)
    _extra(op, 0.0 if extra_width is None else extra_width)
    return _check_boxes(op, b)


def _check_nsample(op: str, nsample, M: int) -> int:
    if int(nsample) != nsample or not 1 <= int(nsample) <= MAX_NSAMPLE:
        raise ValueError(f"{op}: nsample must be in 1 .. {MAX_NSAMPLE}, got {nsample}")
    if M * int(nsample) >= 1 << 31:
        raise ValueError(f"{op}: {M} boxes x {nsample} entries each do not fit 32-bit entries")
    return int(nsample)


def _check_grid(op: str, grid, M: int) -> Optional[Tuple[int, int, int]]:
    if grid is None:
        return None
    try:
        g = tuple(int(v) for v in grid) if isinstance(grid, (tuple, list)) else (int(grid),) * 3
        exact = all(int(v) == v for v in (grid if isinstance(grid, (tuple, list)) else (grid,)))
    except (TypeError, ValueError):
        g, exact = (), False
    if len(g) != 3 or not exact or not all(1 <= v <= MAX_GRID for v in g):
        raise ValueError(f"{op}: the grid is an int or three ints in 1 .. {MAX_GRID}, got {grid!r}")
    if M * g[0] * g[1] * g[2] >= 1 << 31:
        raise ValueError(f"{op}: {M} boxes x {g[0] * g[1] * g[2]} cells each do not fit 32-bit cell ids")
    return g


def frames_into(boxes: torch.Tensor, n_boxes: Optional[torch.Tensor], extra: Sequence[float], frames: torch.Tensor) -> None:
    """The one C call into a buffer the caller owns (capturable): frames fp32 [M, 8]; extra: three floats."""
    _lib.check(_lib.load().spx_boxes_to_frames(boxes.data_ptr(), int(boxes.shape[1]), int(boxes.shape[0]), _ptr(n_boxes),
                                               float(extra[0]), float(extra[1]), float(extra[2]), frames.data_ptr(),
                                               _stream(boxes)))


def boxes_to_frames(boxes: torch.Tensor, n_boxes: Optional[torch.Tensor] = None, extra_width=0.) -> BoxFrames:
    """boxes fp32 [M, >= 7] = (x, y, z, dx, dy, dz, heading) -> ``BoxFrames``: frames [M, 8] = (x, y, z, hx, hy, hz, c,
    s) with ``hx = dx * 0.5 + ex`` (likewise y and z; `extra_width` is a float or a 3-tuple, finite and >= 0:
    OpenPCDet's ``pool_extra_width`` / ``enlarge_box3d`` per side), ``c = cosf(heading)``, ``s = sinf(heading)``.  A
    box is valid by the rule of ``boxes_to_corners`` -- below *n_boxes, seven finite numbers, dx, dy, dz > 0 before
    enlargement -- and an invalid box gets eight NaNs: it contains nothing.  One launch, nothing read back.  No
    gradient."""
    extra = _extra("boxes_to_frames", extra_width)
    M = _check_boxes("boxes_to_frames", boxes)
    _require_gpu(boxes, "boxes")
    _check_count(n_boxes, "boxes_to_frames: n_boxes")
    dev = boxes.device
    with torch.cuda.device(dev), torch.no_grad():
        frames = torch.empty((M, 8), dtype=torch.float32, device=dev)
        if M > 0:
            frames_into(boxes.detach(), n_boxes, extra, frames)
    return BoxFrames(frames, M, n_boxes)


def _as_frames(op: str, b: Boxes, n_boxes: Optional[torch.Tensor], extra_width) -> BoxFrames:
    """The frames form of a checked argument: as given, or the frames launch over boxes."""
    if isinstance(b, BoxFrames):
        _require_gpu(b.frames, "frames")
        count = n_boxes if n_boxes is not None else b.n_boxes
        _check_count(count, f"{op}: n_boxes")
        return BoxFrames(b.frames, b.num_boxes, count)
    return boxes_to_frames(b, n_boxes, 0.0 if extra_width is None else extra_width)


def points_in_boxes(points: torch.Tensor, p_batch_ids: Optional[torch.Tensor], boxes: Boxes,
                    b_batch_ids: Optional[torch.Tensor], batch_size: int, *, n_points: Optional[torch.Tensor] = None,
                    n_boxes: Optional[torch.Tensor] = None, extra_width=None) -> torch.Tensor:
    """int32 [N]: for every point the LOWEST box index of its own scene that contains it, -1 for none
    (``points_in_boxes_gpu``, over stacked scenes).  points fp32 [N, >= 3] (x, y, z first), boxes fp32 [M, >= 7] or
    ``BoxFrames``, p_batch_ids / b_batch_ids int32 or None (all scene 0).  With the frame of ``boxes_to_frames`` and
    every fp32 operation rounded on its own: ``sx = px - x, sy = py - y, lz = pz - z, lx = sx * c + sy * s, ly = sy * c
    - sx * s`` and the point is inside when ``|lz| <= hz and -hx < lx < hx and -hy < ly < hy``: inclusive in z, strict
    in the plane (``check_pt_in_box3d``).  -1 as well for a point with a coordinate that is not finite, at or beyond
    *n_points or with a batch id outside [0, batch_size); an invalid box, one at or beyond *n_boxes and one with a
    foreign batch id contain nothing.  Every element is written; the result does not depend on how points or boxes are
    ordered across scenes.  Launches: the frames (for boxes), the scene list of the boxes, the query; nothing read
    back.  No gradient."""
    op = "points_in_boxes"
    B = int(batch_size)
    N = _check_cloud(op, "points", points, p_batch_ids, B, 3)
    M = _check_arg(op, boxes, extra_width)
    _check_ids(op, "b_batch_ids", b_batch_ids, M)
    _require_cloud(op, "points", points, p_batch_ids, n_points)
    if b_batch_ids is not None:
        _require_gpu(b_batch_ids, "b_batch_ids")
    fr = _as_frames(op, boxes, n_boxes, extra_width)
    dev = points.device
    if fr.frames.device != dev:
        raise ValueError(f"{op}: the boxes are on {fr.frames.device}, the points on {dev}")
    with torch.cuda.device(dev), torch.no_grad():
        points = points.detach().contiguous()
        p_batch_ids = None if p_batch_ids is None else p_batch_ids.contiguous()
        out = torch.empty((N,), dtype=torch.int32, device=dev)
        if N > 0:
            bg = scene_groups(b_batch_ids, M, B, fr.n_boxes, dev)
            _lib.check(_lib.load().spx_points_in_boxes(
                points.data_ptr(), int(points.shape[1]), _ptr(p_batch_ids), N, _ptr(n_points), _ptr(fr.frames), M,
                bg.offsets.data_ptr(), _ptr(bg.list), B, out.data_ptr(), _stream(points)))
    return out


def box_query_into(frames: BoxFrames, b_batch_ids: Optional[torch.Tensor], points: torch.Tensor, groups: PointGroups,
                   pad: str, rows: torch.Tensor, count: torch.Tensor, hits: torch.Tensor,
                   local: Optional[torch.Tensor] = None, cells: Optional[torch.Tensor] = None,
                   grid: Optional[Sequence[int]] = None) -> None:
    """The C call into buffers the caller owns (no allocation, no workspace: capturable).  frames: a ``BoxFrames`` (its
    n_boxes is the device count); groups: the ``scene_groups`` of the points; rows int32 [M, nsample] (nsample is its
    width), count / hits int32 [M], local fp32 [M, nsample, 3] or None, cells int32 [M, nsample] together with grid
    (ox, oy, oz), or both None."""
    if pad not in _PADS:
        raise ValueError(f"box_query_into: pad is 'none', 'first' or 'cycle', got {pad!r}")
    if (cells is None) != (grid is None):
        raise ValueError("box_query_into: cells and grid come together")
    g = (0, 0, 0) if grid is None else tuple(int(v) for v in grid)
    _lib.check(_lib.load().spx_box_query(
        _ptr(frames.frames), _ptr(b_batch_ids), int(frames.num_boxes), _ptr(frames.n_boxes), points.data_ptr(),
        int(points.shape[1]), int(points.shape[0]), groups.offsets.data_ptr(), groups.list.data_ptr(),
        int(groups.num_voxels), int(rows.shape[1]), _PADS[pad], g[0], g[1], g[2], rows.data_ptr(), count.data_ptr(),
        hits.data_ptr(), _ptr(local), _ptr(cells), _stream(points)))


def box_query(boxes: Boxes, b_batch_ids: Optional[torch.Tensor], points: torch.Tensor,
              p_batch_ids: Optional[torch.Tensor], batch_size: int, nsample: int, *, pad: str = "none",
              with_local: bool = False, grid=None, with_groups: bool = False, groups: Optional[PointGroups] = None,
              n_boxes: Optional[torch.Tensor] = None, n_points: Optional[torch.Tensor] = None,
              extra_width=None) -> BoxPoints:
    """The first `nsample` (1 .. 16384) points of its scene inside each box, by the test of ``points_in_boxes``.  boxes
    fp32 [M, >= 7] or ``BoxFrames``, points fp32 [N, >= 3] (x, y, z first), b_batch_ids / p_batch_ids int32 or None
    (all scene 0).  A box's hits are the valid points of ITS scene (below *n_points, a batch id in [0, batch_size),
    finite coordinates) inside it; they are visited in ASCENDING POINT INDEX and the first nsample are kept: rows
    [M, nsample], count [M] = min(hits, nsample), hits [M] (all of them, uncapped), with with_local the kept points in
    the box's frame (lx, ly, lz) [M, nsample, 3] (PointRCNN's canonical transform), and with `grid` (an int or three
    ints in 1 .. 64) their cells [M, nsample]: ``wx = (hx + hx) / ox, ix = min(max(int((lx + hx) / wx), 0), ox - 1)``,
    likewise y and z, the entry the GLOBAL id ``m * ox * oy * oz + (ix * oy + iy) * oz + iz``.  Slots at or beyond
    count hold -1 / 0; pad="first" repeats slot 0 there, pad="cycle" writes slot ``s % count`` (``roipoint_pool3d``),
    both only when count > 0.  An invalid box, one at or beyond *n_boxes and one with a foreign batch id have count =
    hits = 0.  The result does not depend on how boxes or points are ordered across scenes.  Returns a ``BoxPoints``;
    with_groups builds the transposed list the gradient of ``group_voxels`` walks.  `groups`: a ready ``scene_groups``
    of the points.  Launches: the frames (for boxes), the scene list (unless given), the query, and for a pad a second
    launch over the padded slots; nothing read back.  No gradient with respect to coordinates or boxes."""
    op = "box_query"
    B = int(batch_size)
    M = _check_arg(op, boxes, extra_width)
    _check_ids(op, "b_batch_ids", b_batch_ids, M)
    N = _check_cloud(op, "points", points, p_batch_ids, B, 3)
    nsample = _check_nsample(op, nsample, M)
    if pad not in _PADS:
        raise ValueError(f"{op}: pad is 'none', 'first' or 'cycle', got {pad!r}")
    grid = _check_grid(op, grid, M)
    if groups is not None:
        _check_groups(op, groups, N, B)
        n_points = groups.n_points if n_points is None else n_points
    _require_cloud(op, "points", points, p_batch_ids, n_points)
    if b_batch_ids is not None:
        _require_gpu(b_batch_ids, "b_batch_ids")
    fr = _as_frames(op, boxes, n_boxes, extra_width)
    dev = points.device
    if fr.frames.device != dev:
        raise ValueError(f"{op}: the boxes are on {fr.frames.device}, the points on {dev}")
    with torch.cuda.device(dev), torch.no_grad():
        points = points.detach().contiguous()
        if groups is None:
            groups = scene_groups(None if p_batch_ids is None else p_batch_ids.contiguous(), N, B, n_points, dev)
        rows = torch.empty((M, nsample), dtype=torch.int32, device=dev)
        count = torch.empty((M,), dtype=torch.int32, device=dev)
        hits = torch.empty((M,), dtype=torch.int32, device=dev)
        local = torch.empty((M, nsample, 3), dtype=torch.float32, device=dev) if with_local else None
        cells = torch.empty((M, nsample), dtype=torch.int32, device=dev) if grid is not None else None
        if M > 0:
            box_query_into(fr, b_batch_ids, points, groups, pad, rows, count, hits, local, cells, grid)
        flat = flat_groups(rows, N, n_points) if with_groups else None
    return BoxPoints(rows, count, hits, local, cells, flat, nsample, N, grid, fr.n_boxes, n_points)


def _check_feats(op: str, feats: torch.Tensor, N: int) -> None:
    if not isinstance(feats, torch.Tensor) or feats.dim() != 2 or int(feats.shape[0]) != N:
        got = tuple(feats.shape) if isinstance(feats, torch.Tensor) else type(feats).__name__
        raise ValueError(f"{op}: one feature row per point ([{N}, C]), got {got}")
    _float_code(feats, op)


def roi_point_pool(points: torch.Tensor, p_batch_ids: Optional[torch.Tensor], feats: torch.Tensor, boxes: Boxes,
                   b_batch_ids: Optional[torch.Tensor], batch_size: int, num_sampled_points: int = 512,
                   pool_extra_width=0., *, n_points: Optional[torch.Tensor] = None,
                   n_boxes: Optional[torch.Tensor] = None, groups: Optional[PointGroups] = None):
    """``roipoint_pool3d`` over stacked scenes: (pooled [M, S, 3 + C], empty int32 [M]) with S = `num_sampled_points`.
    Row (m, s) is the xyz of a point inside box m -- enlarged by `pool_extra_width` per side, a float or a 3-tuple --
    cast to the dtype of feats, followed by its C features: the first S points of the box's scene inside it in
    ascending point index, and with fewer than S slot s holds slot ``s % count`` again (``box_query(pad="cycle")``
    followed by ``group_voxels`` over xyz and over feats, entry by entry: ``BoxPoints.gather``).  A box without a point is all zeros and has empty = 1.
    Differentiable in feats (the segment sum of ``group_voxels``, in ascending entry, no atomics: identical run to
    run); there is no gradient with respect to coordinates or boxes.  Nothing read back."""
    op = "roi_point_pool"
    N = _check_cloud(op, "points", points, p_batch_ids, int(batch_size), 3)
    _check_feats(op, feats, N)
    extra = None if isinstance(boxes, BoxFrames) and pool_extra_width in (0, 0.0, None) else pool_extra_width
    needs_grad = bool(feats.requires_grad and torch.is_grad_enabled())
    bp = box_query(boxes, b_batch_ids, points, p_batch_ids, batch_size, num_sampled_points, pad="cycle",
                   with_groups=needs_grad, groups=groups, n_boxes=n_boxes, n_points=n_points, extra_width=extra)
    with torch.no_grad():
        xyz = bp.gather(points.detach()[:, :3].contiguous())
    grouped = bp.gather(feats)
    pooled = torch.cat([xyz.to(grouped.dtype), grouped], dim=2)
    return pooled, (bp.count == 0).to(torch.int32)


def roi_aware_pool(points: torch.Tensor, p_batch_ids: Optional[torch.Tensor], feats: torch.Tensor, boxes: Boxes,
                   b_batch_ids: Optional[torch.Tensor], batch_size: int, out_size, max_pts_per_box: int = 2048,
                   reduce: str = "max", *, n_points: Optional[torch.Tensor] = None,
                   n_boxes: Optional[torch.Tensor] = None, groups: Optional[PointGroups] = None) -> torch.Tensor:
    """``roiaware_pool3d`` over stacked scenes: [M, ox, oy, oz, C], the max or the mean of the features of the points
    in every cell of an `out_size` (an int or three ints in 1 .. 64) grid over each box; an empty cell is zeros.  A
    composite without a kernel of its own: ``box_query(grid=out_size, nsample=max_pts_per_box)``, ``point_groups`` over
    the flattened cells (the id -1 of an empty slot belongs to no cell), ``group_voxels``, ``points_to_voxels``.  Two
    differences from OpenPCDet: the cap is PER BOX -- the first `max_pts_per_box` (1 .. 16384) points of a box in
    ascending point index take part, not 128 per cell -- and on a tie of a max the gradient goes to EVERY point that
    attains it, not to one.  Differentiable in feats (both gradients are the existing fixed-order ones: no atomics,
    identical run to run); there is no gradient with respect to coordinates or boxes.  Nothing read back."""
    op = "roi_aware_pool"
    if reduce not in ("max", "mean"):
        raise ValueError(f"{op}: reduce must be 'max' or 'mean', got {reduce!r}")
    N = _check_cloud(op, "points", points, p_batch_ids, int(batch_size), 3)
    _check_feats(op, feats, N)
    if out_size is None:
        raise ValueError(f"{op}: the grid is an int or three ints in 1 .. {MAX_GRID}, got None")
    needs_grad = bool(feats.requires_grad and torch.is_grad_enabled())
    bp = box_query(boxes, b_batch_ids, points, p_batch_ids, batch_size, max_pts_per_box, grid=out_size,
                   with_groups=needs_grad, groups=groups, n_boxes=n_boxes, n_points=n_points)
    M, S = (int(v) for v in bp.rows.shape)
    ox, oy, oz = bp.grid
    C = int(feats.shape[1])
    if M == 0:
        return feats.new_zeros((0, ox, oy, oz, C))
    with torch.cuda.device(feats.device):
        cell_groups = point_groups(bp.cells.reshape(-1), M * ox * oy * oz)
    grouped = bp.gather(feats)
    out = points_to_voxels(grouped.reshape(M * S, C), cell_groups, reduce)
    return out.reshape(M, ox, oy, oz, C)
