"""Farthest-point sampling and ball query over raw points on the HIP kernels of csrc/sample.hip
(``functional.farthest_point_sample`` / ``gather_samples`` / ``ball_query``, ``spatial.FarthestPointSample`` /
``BallQueryAndGroup``).  Not part of the reference; the point-voxel detectors (PV-RCNN, PV-RCNN++, Voxel R-CNN's raw-point
source) call them as the ``furthest_point_sample`` / ``ball_query`` CUDA extensions of ``pointnet2_stack``.

  * scenes                  the points of scene b are ``list[offsets[b] : offsets[b + 1]]`` of ``point_groups`` over the
                            batch ids: any input order, ascending point index inside a scene; both operations accept a
                            ready ``PointGroups`` (``scene_groups``) so a caller builds it once
  * ``farthest_point_sample``  K samples per scene (``spx_fps``: one workgroup per scene, one launch), ties to the lowest
                            point index, distinct indices, -1 past the scene's valid points
  * ``gather_samples``      the sampled rows, NaN in dead slots (``gather_rows``): a dead slot is an invalid query for
                            ``voxel_query``, ``point_corners`` and ``ball_query`` alike
  * ``ball_query``          per query the first ``nsample`` points of its scene inside a radius, in ascending point
                            index (``spx_ball_query``), as the ``VoxelNeighbors`` that ``group_voxels`` and its
                            gradient take, the points standing where a level's rows do
  * ``sector_fps``          sectorised, proposal-centric sampling (``sector_ids`` -> ``point_groups`` -> quotas ->
                            ``farthest_point_sample_segments``, the FPS kernel with K read per group): one workgroup
                            per sector of every scene, samples packed sector by sector (the section at the end)

There is no gradient with respect to coordinates: raw coordinates need none.
"""
from __future__ import annotations

from typing import NamedTuple, Optional

import torch

from spconv_amd import _lib
from spconv_amd.pytorch import _pointvoxel
from spconv_amd.pytorch._level import flat_groups
from spconv_amd.pytorch._pointvoxel import PointGroups, gather_rows
from spconv_amd.pytorch._query import MAX_NSAMPLE, VoxelNeighbors, squared_radius
from spconv_amd.pytorch._rulebook import _check_count, _ptr, _require_gpu, _stream, _ws

MAX_SAMPLES = 1 << 16
_FLAG_PAD_FIRST = 2


class PointSamples(NamedTuple):
    """The samples of every scene: idx int32 [B, K] (point index, -1 at or beyond count[b]), count int32 [B] =
    min(valid points of b, K), batch_ids int32 [B * K] (b for every slot of scene b: the batch ids of the gathered
    samples as queries)."""
    idx: torch.Tensor
    count: torch.Tensor
    batch_ids: torch.Tensor


def resident_points() -> int:
    """The largest scene ``spx_fps`` keeps in registers; a larger one streams staged records from scratch."""
    return int(_lib.load().spx_fps_resident_points())


def fps_ws_bytes(n_cap: int, batch_size: int, ndim: int) -> int:
    return int(_lib.load().spx_fps_ws_bytes(int(n_cap), int(batch_size), int(ndim)))


def _check_cloud(op: str, noun: str, points: torch.Tensor, batch_ids: Optional[torch.Tensor], batch_size: int,
                 ndim: int) -> int:
    """The ValueErrors of a cloud (`noun`: what `op` calls it); they come before the refusal of a CPU tensor
    (``_require_cloud``)."""
    if ndim not in (2, 3):
        raise ValueError(f"{op}: ndim must be 2 or 3, got {ndim}")
    if int(batch_size) < 1:
        raise ValueError(f"{op}: batch_size must be >= 1, got {batch_size}")
    if points.dim() != 2 or points.dtype != torch.float32 or points.shape[1] < ndim:
        raise ValueError(f"{op}: {noun} is a float32 tensor [N, >= {ndim}], got {tuple(points.shape)} {points.dtype}")
    N = int(points.shape[0])
    if batch_ids is not None and (batch_ids.shape != (N,) or batch_ids.dtype != torch.int32):
        raise ValueError(f"{op}: the batch_ids of the {noun} are a CUDA int32 tensor [N]")
    return N


def _require_cloud(op: str, noun: str, points: torch.Tensor, batch_ids: Optional[torch.Tensor],
                   count: Optional[torch.Tensor]) -> None:
    _require_gpu(points, noun)
    if batch_ids is not None:
        _require_gpu(batch_ids, "batch_ids")
    _check_count(count, f"{op}: n_{noun}")


def _check_groups(op: str, groups: PointGroups, N: int, batch_size: int) -> None:
    if groups.offsets is None or groups.list is None or groups.num_voxels != int(batch_size) or groups.list.shape[0] != N:
        raise ValueError(f"{op}: groups are the point_groups of the {N} batch ids over {batch_size} scenes "
                         f"(scene_groups), got {groups.num_voxels} groups over {tuple(groups.rows.shape)} points")


def scene_groups(batch_ids: Optional[torch.Tensor], n: int, batch_size: int, n_points: Optional[torch.Tensor] = None,
                 device=None) -> PointGroups:
    """The points of every scene: ``point_groups(batch_ids, batch_size, n_points)``, all scene 0 for batch_ids None.
    Ids outside [0, batch_size) and rows at or beyond *n_points belong to no scene."""
    dev = batch_ids.device if batch_ids is not None else device
    with torch.cuda.device(dev):
        if int(n) == 0:
            empty = torch.empty((0,), dtype=torch.int32, device=dev)
            return PointGroups(empty, torch.zeros((int(batch_size) + 1,), dtype=torch.int32, device=dev), empty,
                               int(batch_size), n_points, None)
        ids = batch_ids if batch_ids is not None else torch.zeros((int(n),), dtype=torch.int32, device=dev)
        return _pointvoxel.point_groups(ids, int(batch_size), n_points)


def sample_batch_ids(batch_size: int, num_samples: int, device) -> torch.Tensor:
    """int32 [B * K]: b for every slot of scene b (built from host values; nothing is read)."""
    b = torch.arange(int(batch_size), dtype=torch.int32, device=device)
    return b.view(-1, 1).expand(int(batch_size), int(num_samples)).reshape(-1)


def fps_into(points: torch.Tensor, groups: PointGroups, num_samples: int, ndim: int, idx: torch.Tensor,
             count: torch.Tensor, ws: Optional[torch.Tensor]) -> None:
    """The one C call into buffers the caller owns (no allocation: capturable).  idx int32 [B, K], count int32 [B], ws:
    ``fps_ws_bytes`` bytes (needed once the cloud holds more than ``resident_points()`` points)."""
    _lib.check(_lib.load().spx_fps(points.data_ptr(), int(points.shape[1]), int(points.shape[0]), int(ndim),
                                   groups.offsets.data_ptr(), groups.list.data_ptr(), int(groups.num_voxels),
                                   int(num_samples), idx.data_ptr(), count.data_ptr(), _ptr(ws),
                                   0 if ws is None else ws.numel(), _stream(points)))


def farthest_point_sample(points: torch.Tensor, batch_ids: Optional[torch.Tensor], batch_size: int, num_samples: int, *,
                          ndim: int = 3, n_points: Optional[torch.Tensor] = None,
                          groups: Optional[PointGroups] = None) -> PointSamples:
    """`num_samples` (K, 1 .. 65 536, the same for every scene) points of every scene by farthest-point sampling.
    points fp32 [N, >= ndim] (x, y, z first), batch_ids int32 [N] or None (all scene 0); rows at or beyond *n_points and
    ids outside [0, batch_size) belong to no scene, a point with a coordinate that is not finite is never a sample.
    Slot 0 of a scene is its lowest valid point index; every valid point keeps t (+inf at first); a step sets ``t[i] =
    d2 < t[i] ? d2 : t[i]`` with d2 the fp32 squared distance to the last sample, every operation rounded on its own,
    and picks the not-yet-chosen point with the largest t, ties to the LOWEST point index.  A chosen point stops being a
    candidate: the indices of a scene are distinct (pointnet2 repeats one once only duplicates are left; for distinct
    points the sequences agree).  Returns PointSamples(idx [B, K] with -1 at or beyond count[b], count [B] = min(valid
    points, K), batch_ids [B * K]).  `groups`: a ready ``scene_groups`` of the cloud.  One launch, nothing read back.
    No gradient with respect to coordinates."""
    K, B = int(num_samples), int(batch_size)
    N = _check_cloud("farthest_point_sample", "points", points, batch_ids, B, ndim)
    if not 1 <= K <= MAX_SAMPLES:
        raise ValueError(f"farthest_point_sample: num_samples must be in 1 .. {MAX_SAMPLES}, got {num_samples}")
    if B * K >= 1 << 31:
        raise ValueError(f"farthest_point_sample: {B} scenes x {K} samples do not fit 32-bit entries")
    if groups is not None:
        _check_groups("farthest_point_sample", groups, N, B)
    _require_cloud("farthest_point_sample", "points", points, batch_ids, n_points)
    dev = points.device
    with torch.cuda.device(dev), torch.no_grad():
        points = points.detach().contiguous()
        if groups is None:
            groups = scene_groups(None if batch_ids is None else batch_ids.contiguous(), N, B, n_points, dev)
        idx = torch.empty((B, K), dtype=torch.int32, device=dev)
        count = torch.empty((B,), dtype=torch.int32, device=dev)
        ws = _ws(fps_ws_bytes(N, B, ndim), dev) if N > resident_points() else None
        fps_into(points, groups, K, ndim, idx, count, ws)
        return PointSamples(idx, count, sample_batch_ids(B, K, dev))


def gather_samples(points: torch.Tensor, samples: PointSamples) -> torch.Tensor:
    """[B * K, nfeat]: the rows of the samples, NaN in the slots at or beyond count[b] -- an invalid query for
    ``voxel_query``, ``point_corners`` and ``ball_query`` alike (``gather_rows``: one launch)."""
    if points.dim() != 2 or not points.dtype.is_floating_point:
        raise ValueError(f"gather_samples: points is a floating tensor [N, nfeat], got {tuple(points.shape)} {points.dtype}")
    _require_gpu(points, "points")
    with torch.cuda.device(points.device), torch.no_grad():
        return gather_rows(points.detach(), samples.idx.reshape(-1), float("nan"))


def _check_pad(op: str, pad: str) -> None:
    if pad not in ("none", "first"):
        raise ValueError(f"{op}: pad is 'none' or 'first', got {pad!r}")


def _check_ball(nsample: int, pad: str) -> int:
    if not 1 <= int(nsample) <= MAX_NSAMPLE:
        raise ValueError(f"ball_query: nsample must be in 1 .. {MAX_NSAMPLE}, got {nsample}")
    _check_pad("ball_query", pad)
    return int(nsample)


def _scene_query(op: str, queries: torch.Tensor, q_batch_ids: Optional[torch.Tensor], points: torch.Tensor,
                 p_batch_ids: Optional[torch.Tensor], batch_size: int, ndim: int, entries: int,
                 n_queries: Optional[torch.Tensor], n_points: Optional[torch.Tensor], groups: Optional[PointGroups]):
    """The prologue of ``ball_query`` and ``knn_query`` (`entries` slots per query): every ValueError, then the refusal
    of CPU tensors, then the inputs detached and contiguous and the scene groups of the points (built when none are
    given).  Returns (queries, q_batch_ids, points, groups, n_points, M, N, dev)."""
    B = int(batch_size)
    M = _check_cloud(op, "queries", queries, q_batch_ids, B, ndim)
    N = _check_cloud(op, "points", points, p_batch_ids, B, ndim)
    if M * entries >= 1 << 31:
        raise ValueError(f"{op}: {M} queries x {entries} entries each do not fit 32-bit entries")
    if groups is not None:
        _check_groups(op, groups, N, B)
        n_points = groups.n_points if n_points is None else n_points
    _require_cloud(op, "queries", queries, q_batch_ids, n_queries)
    _require_cloud(op, "points", points, p_batch_ids, n_points)
    dev = queries.device
    queries, points = queries.detach().contiguous(), points.detach().contiguous()     # (on their own device, no graph)
    q_batch_ids = None if q_batch_ids is None else q_batch_ids.contiguous()
    if groups is None:
        groups = scene_groups(None if p_batch_ids is None else p_batch_ids.contiguous(), N, B, n_points, dev)
    return queries, q_batch_ids, points, groups, n_points, M, N, dev


def ball_query_into(queries: torch.Tensor, q_batch_ids: Optional[torch.Tensor], n_queries: Optional[torch.Tensor],
                    points: torch.Tensor, groups: PointGroups, ndim: int, nsample: int, r2: float, pad_first: bool,
                    rows: torch.Tensor, count: torch.Tensor, offsets: Optional[torch.Tensor]) -> None:
    """The one C call into buffers the caller owns (no allocation: capturable).  r2: ``squared_radius``; rows int32
    [M, nsample], count int32 [M], offsets fp32 [M, nsample, ndim] or None."""
    _lib.check(_lib.load().spx_ball_query(
        queries.data_ptr(), int(queries.shape[1]), _ptr(q_batch_ids), int(queries.shape[0]), _ptr(n_queries),
        points.data_ptr(), int(points.shape[1]), int(points.shape[0]), int(ndim), groups.offsets.data_ptr(),
        groups.list.data_ptr(), int(groups.num_voxels), int(nsample), float(r2), _FLAG_PAD_FIRST if pad_first else 0,
        rows.data_ptr(), count.data_ptr(), _ptr(offsets), _stream(queries)))


def ball_query(queries: torch.Tensor, q_batch_ids: Optional[torch.Tensor], points: torch.Tensor,
               p_batch_ids: Optional[torch.Tensor], batch_size: int, radius: float, nsample: int, *, ndim: int = 3,
               pad: str = "none", with_offsets: bool = False, n_queries: Optional[torch.Tensor] = None,
               n_points: Optional[torch.Tensor] = None, with_groups: bool = False,
               groups: Optional[PointGroups] = None) -> VoxelNeighbors:
    """The first `nsample` (1 .. 128) points of its scene inside `radius` of each query.  queries fp32 [M, >= ndim],
    points fp32 [N, >= ndim] (x, y, z first), q_batch_ids / p_batch_ids int32 or None (all scene 0).  A query's hits are
    the valid points of ITS scene (a point below *n_points, with a batch id in [0, batch_size) and finite coordinates)
    with ``d2 < float32(radius) ** 2``, d = point - query and d2 in fp32 with every operation rounded on its own; they
    are visited in ASCENDING POINT INDEX and the first nsample are kept: rows [M, nsample] (point indices), count [M] =
    min(hits, nsample), and with with_offsets the point-minus-query vectors [M, nsample, ndim].  Slots at or beyond
    count hold -1 / 0; pad="first" repeats slot 0 there when count > 0, as pointnet2 does.  A query with a NaN
    coordinate, with a batch id outside [0, batch_size) or at or beyond *n_queries has count 0.  The result does not
    depend on how queries or points are ordered across scenes.  Returns the ``VoxelNeighbors`` of the points
    (num_voxels = N, n_live = n_points): ``group_voxels(point_feats, nb)`` and its gradient work on [N, C] point
    features; with_groups builds the transposed list that gradient walks.  `groups`: a ready ``scene_groups`` of the
    points.  One launch, nothing read back.  No gradient with respect to coordinates."""
    nsample = _check_ball(nsample, pad)
    if radius is None:
        raise ValueError("ball_query: radius must be >= 0, got None")
    r2 = squared_radius(radius)
    queries, q_batch_ids, points, groups, n_points, M, N, dev = _scene_query(
        "ball_query", queries, q_batch_ids, points, p_batch_ids, batch_size, ndim, nsample, n_queries, n_points, groups)
    with torch.cuda.device(dev), torch.no_grad():
        rows = torch.empty((M, nsample), dtype=torch.int32, device=dev)
        count = torch.empty((M,), dtype=torch.int32, device=dev)
        offsets = torch.empty((M, nsample, ndim), dtype=torch.float32, device=dev) if with_offsets else None
        if M > 0:
            ball_query_into(queries, q_batch_ids, n_queries, points, groups, ndim, nsample, r2, pad == "first", rows, count,
                            offsets)
        flat = flat_groups(rows, N, n_points) if with_groups else None
    return VoxelNeighbors(rows, count, offsets, flat, N, n_queries, n_points)


# ------------------------------------------------------------------------------------------------ sectorised sampling
#
# PV-RCNN++'s ``sectorized_proposal_centric_sampling`` and pointnet2_stack's ``stack_farthest_point_sample``: a per-point
# segment id (``sector_ids``: scene * S + azimuth sector, -1 for a point the RoI filter turns down), ``point_groups``
# over it, a quota per segment (``spx_fps_quota``) and the sampling kernel with K read per segment
# (``spx_fps_segments``): B * S workgroups on B * S CUs, none waiting for another, nothing read back.

MAX_SECTORS = 64


class SectorBuffers(NamedTuple):
    """What ``sector_fps_into`` writes, allocated once by ``sector_buffers``: seg int32 [N], the groups of seg (rows,
    offsets [B * S + 1], list, their scratch), quota / slot / seg_count int32 [B * S], count int32 [B], idx int32
    [B, K + S - 1], and the scratch of the sampling kernel (None for a cloud of up to ``resident_points()`` points)."""
    seg: torch.Tensor
    rows: torch.Tensor
    offsets: torch.Tensor
    list: torch.Tensor
    groups_ws: torch.Tensor
    quota: torch.Tensor
    slot: torch.Tensor
    seg_count: torch.Tensor
    count: torch.Tensor
    idx: torch.Tensor
    ws: Optional[torch.Tensor]


def sector_table(num_sectors: int):
    """[(c_k, s_k)] of the S sector boundaries as the kernel uses them (``spx_sector_table``): (cos, sin)(2 pi k / S)
    computed in float64 and rounded to float32, exact on the axes.  Host only."""
    import ctypes
    S = int(num_sectors)
    table = (ctypes.c_float * (2 * max(S, 1)))()
    _lib.check(_lib.load().spx_sector_table(S, ctypes.cast(table, ctypes.c_void_p)))
    return [(float(table[2 * k]), float(table[2 * k + 1])) for k in range(S)]


def _check_sectors(op: str, num_sectors: int, center) -> tuple:
    if not 1 <= int(num_sectors) <= MAX_SECTORS:
        raise ValueError(f"{op}: num_sectors must be in 1 .. {MAX_SECTORS}, got {num_sectors}")
    try:
        cx, cy = (float(v) for v in center)
    except (TypeError, ValueError):
        raise ValueError(f"{op}: center is two finite floats (x, y), got {center!r}") from None
    if not (abs(cx) < float("inf") and abs(cy) < float("inf")):
        raise ValueError(f"{op}: center is two finite floats (x, y), got {center!r}")
    return cx, cy


def _check_rois(op: str, rois: Optional[torch.Tensor], roi_batch_ids: Optional[torch.Tensor], roi_radius, batch_size: int,
                ndim: int) -> Optional[float]:
    """The ValueErrors of the RoI filter; the radius as a float, None without a filter."""
    if (rois is None) != (roi_radius is None):
        raise ValueError(f"{op}: rois and roi_radius come together, got rois {'given' if rois is not None else 'None'} "
                         f"and roi_radius {roi_radius!r}")
    if rois is None:
        if roi_batch_ids is not None:
            raise ValueError(f"{op}: roi_batch_ids without rois")
        return None
    if ndim != 3:
        raise ValueError(f"{op}: the RoI filter needs ndim 3, got {ndim}")
    radius = float(roi_radius)
    if not 0. <= radius < float("inf"):
        raise ValueError(f"{op}: roi_radius must be finite and >= 0, got {roi_radius!r}")
    if rois.dim() != 2 or rois.dtype != torch.float32 or rois.shape[1] < 7:
        raise ValueError(f"{op}: rois is a float32 tensor [M, >= 7] (x, y, z, dx, dy, dz, heading), got "
                         f"{tuple(rois.shape)} {rois.dtype}")
    if roi_batch_ids is not None and (roi_batch_ids.shape != (int(rois.shape[0]),) or roi_batch_ids.dtype != torch.int32):
        raise ValueError(f"{op}: the roi_batch_ids are a CUDA int32 tensor [M]")
    return radius


def _check_sector_fps(op: str, batch_size: int, num_samples: int, num_sectors: int) -> None:
    K, S, B = int(num_samples), int(num_sectors), int(batch_size)
    if not 1 <= K <= MAX_SAMPLES:
        raise ValueError(f"{op}: num_samples must be in 1 .. {MAX_SAMPLES}, got {num_samples}")
    if B * (K + S - 1) >= 1 << 31:
        raise ValueError(f"{op}: {B} scenes x {K + S - 1} slots do not fit 32-bit entries")


def sector_ids_into(points: torch.Tensor, batch_ids: Optional[torch.Tensor], n_points: Optional[torch.Tensor], ndim: int,
                    batch_size: int, num_sectors: int, center, rois: Optional[torch.Tensor],
                    roi_groups: Optional[PointGroups], roi_radius: Optional[float], seg: torch.Tensor) -> None:
    """The one C call into a buffer the caller owns (no allocation: capturable).  roi_groups: ``scene_groups`` of the
    roi batch ids (with the device box count); rois None: no filter."""
    filt = rois is not None
    _lib.check(_lib.load().spx_sector_ids(
        points.data_ptr(), int(points.shape[1]), _ptr(batch_ids), int(points.shape[0]), _ptr(n_points), int(ndim),
        int(batch_size), int(num_sectors), float(center[0]), float(center[1]), 1 if filt else 0, _ptr(rois),
        int(rois.shape[1]) if filt else 0, int(rois.shape[0]) if filt else 0, roi_groups.offsets.data_ptr() if filt else None,
        roi_groups.list.data_ptr() if filt else None, float(roi_radius) if filt else 0., seg.data_ptr(), _stream(points)))


def _sector_inputs(op: str, points, batch_ids, batch_size, num_sectors, center, rois, roi_batch_ids, roi_radius, n_points,
                   n_rois, ndim, num_samples=None):
    """The prologue of ``sector_ids`` and ``sector_fps`` (the one with `num_samples`): every ValueError, then the
    refusal of CPU tensors.  Returns (N, centre, radius)."""
    N = _check_cloud(op, "points", points, batch_ids, int(batch_size), ndim)
    centre = _check_sectors(op, num_sectors, center)
    if num_samples is not None:
        _check_sector_fps(op, batch_size, num_samples, num_sectors)
    radius = _check_rois(op, rois, roi_batch_ids, roi_radius, int(batch_size), ndim)
    _require_cloud(op, "points", points, batch_ids, n_points)
    if rois is not None:
        _require_cloud(op, "rois", rois, roi_batch_ids, n_rois)
    return N, centre, radius


def _roi_groups(rois, roi_batch_ids, batch_size, n_rois, dev):
    if rois is None:
        return None, None
    rois = rois.detach().contiguous()
    ids = None if roi_batch_ids is None else roi_batch_ids.contiguous()
    return rois, scene_groups(ids, int(rois.shape[0]), int(batch_size), n_rois, dev)


def sector_ids(points: torch.Tensor, batch_ids: Optional[torch.Tensor], batch_size: int, num_sectors: int, *,
               center=(0., 0.), rois: Optional[torch.Tensor] = None, roi_batch_ids: Optional[torch.Tensor] = None,
               roi_radius: Optional[float] = None, n_points: Optional[torch.Tensor] = None,
               n_rois: Optional[torch.Tensor] = None, ndim: int = 3) -> torch.Tensor:
    """int32 [N]: ``b * S + sector`` for a valid point of scene b, -1 for a point in no segment -- a row at or beyond
    *n_points, a batch id outside [0, batch_size), a coordinate that is not finite, a point the RoI filter turns down.
    The sector (S = `num_sectors` in 1 .. 64, about `center`) is OpenPCDet's ``floor((atan2(y, x) + pi) / (2 pi / S))``,
    decided by the sign of one float32 cross product per boundary (the header of ``spx_sector_ids`` has the rule); two
    deliberate differences: a point on the negative x axis with y = +0 is sector 0 (OpenPCDet gives it the index S and
    so drops it), and the origin is sector 0 (there S / 2).  With `rois` fp32 [M, >= 7] (OpenPCDet 7-vectors),
    `roi_batch_ids` int32 [M] or None, `roi_radius` and an optional device `n_rois`, a point is kept when its distance
    to the NEAREST valid box centre of its scene is below that box's half diagonal plus the radius
    (``sample_points_with_roi``: only the nearest centre's size counts); a scene without a valid box keeps nothing.
    One launch (and the scene groups of the boxes), nothing read back.  No gradient with respect to coordinates."""
    N, centre, radius = _sector_inputs("sector_ids", points, batch_ids, batch_size, num_sectors, center, rois,
                                       roi_batch_ids, roi_radius, n_points, n_rois, ndim)
    dev = points.device
    with torch.cuda.device(dev), torch.no_grad():
        rois, roi_groups = _roi_groups(rois, roi_batch_ids, batch_size, n_rois, dev)
        seg = torch.empty((N,), dtype=torch.int32, device=dev)
        sector_ids_into(points.detach().contiguous(), None if batch_ids is None else batch_ids.contiguous(), n_points, ndim,
                        batch_size, num_sectors, centre, rois, roi_groups, radius, seg)
    return seg


def fps_quota_into(groups: PointGroups, batch_size: int, num_sectors: int, num_samples: int, quota: torch.Tensor,
                   slot: torch.Tensor, count: torch.Tensor) -> None:
    """The one C call (capturable): per segment of the B * S groups its share of K, the exclusive prefix of the shares
    inside its scene, and per scene their sum (``spx_fps_quota``)."""
    _lib.check(_lib.load().spx_fps_quota(groups.offsets.data_ptr(), int(groups.list.shape[0]), int(batch_size),
                                         int(num_sectors), int(num_samples), quota.data_ptr(), slot.data_ptr(),
                                         count.data_ptr(), _stream(quota)))


def fps_segments_into(points: torch.Tensor, groups: PointGroups, quota: torch.Tensor, slot: Optional[torch.Tensor],
                      groups_per_row: int, row_stride: int, max_quota: int, ndim: int, idx: torch.Tensor,
                      count: torch.Tensor, ws: Optional[torch.Tensor]) -> None:
    """The one C call into buffers the caller owns (capturable): idx int32 [G / groups_per_row, row_stride], count int32
    [G], ws as ``fps_into``."""
    _lib.check(_lib.load().spx_fps_segments(
        points.data_ptr(), int(points.shape[1]), int(points.shape[0]), int(ndim), groups.offsets.data_ptr(),
        groups.list.data_ptr(), int(groups.num_voxels), quota.data_ptr(), _ptr(slot), int(groups_per_row), int(row_stride),
        int(max_quota), idx.data_ptr(), count.data_ptr(), _ptr(ws), 0 if ws is None else ws.numel(), _stream(points)))


def farthest_point_sample_segments(points: torch.Tensor, groups: PointGroups, num_samples, max_samples: int, *,
                                   ndim: int = 3) -> PointSamples:
    """Farthest-point sampling per GROUP with its own K (``stack_farthest_point_sample``).  `groups`: any
    ``point_groups`` of the cloud with G groups (``scene_groups``, the groups of ``sector_ids``, ...); `num_samples`: an
    int32 device tensor [G], read by the kernel and clamped to 0 .. `max_samples` (1 .. 65 536), or an int for every
    group.  The rule inside a group is ``farthest_point_sample``'s: with an int K = max_samples over ``scene_groups``
    the result is equal to it.  Returns PointSamples(idx [G, max_samples] with -1 at or beyond count[g], count [G] =
    min(valid points, num_samples[g], max_samples), batch_ids [G * max_samples] = g).  One workgroup per group, two
    launches, nothing read back.  No gradient with respect to coordinates."""
    op = "farthest_point_sample_segments"
    if ndim not in (2, 3):
        raise ValueError(f"{op}: ndim must be 2 or 3, got {ndim}")
    if points.dim() != 2 or points.dtype != torch.float32 or points.shape[1] < ndim:
        raise ValueError(f"{op}: points is a float32 tensor [N, >= {ndim}], got {tuple(points.shape)} {points.dtype}")
    N, M = int(points.shape[0]), int(max_samples)
    if groups.offsets is None or groups.list is None or groups.list.shape[0] != N:
        raise ValueError(f"{op}: groups are point_groups of the {N} points with their offsets and list")
    G = int(groups.num_voxels)
    if not 1 <= M <= MAX_SAMPLES:
        raise ValueError(f"{op}: max_samples must be in 1 .. {MAX_SAMPLES}, got {max_samples}")
    if G * M >= 1 << 31:
        raise ValueError(f"{op}: {G} groups x {M} samples do not fit 32-bit entries")
    per_group = isinstance(num_samples, torch.Tensor)
    if per_group:
        if num_samples.shape != (G,) or num_samples.dtype != torch.int32:
            raise ValueError(f"{op}: num_samples is an int or a CUDA int32 tensor [{G}], got {tuple(num_samples.shape)} "
                             f"{num_samples.dtype}")
    elif not 0 <= int(num_samples) <= M:
        raise ValueError(f"{op}: num_samples must be in 0 .. max_samples = {M}, got {num_samples}")
    _require_gpu(points, "points")
    if per_group:
        _require_gpu(num_samples, "num_samples")
    dev = points.device
    with torch.cuda.device(dev), torch.no_grad():
        points = points.detach().contiguous()
        quota = num_samples.contiguous() if per_group else torch.full((G,), int(num_samples), dtype=torch.int32, device=dev)
        idx = torch.empty((G, M), dtype=torch.int32, device=dev)
        count = torch.empty((G,), dtype=torch.int32, device=dev)
        ws = _ws(fps_ws_bytes(N, G, ndim), dev) if N > resident_points() else None
        fps_segments_into(points, groups, quota, None, 1, M, M, ndim, idx, count, ws)
        return PointSamples(idx, count, sample_batch_ids(G, M, dev))


def sector_buffers(n: int, batch_size: int, num_samples: int, num_sectors: int, ndim: int, device) -> SectorBuffers:
    """The buffers of ``sector_fps_into`` for a cloud of n points (allocated here, once)."""
    B, S, G = int(batch_size), int(num_sectors), int(batch_size) * int(num_sectors)
    i32 = dict(dtype=torch.int32, device=device)
    e = lambda *shape: torch.empty(shape, **i32)
    return SectorBuffers(e(n), e(n), e(G + 1), e(n), _ws(_lib.load().spx_point_groups_ws_bytes(int(n), G), device), e(G), e(G),
                         e(G), e(B), e(B, int(num_samples) + S - 1),
                         _ws(fps_ws_bytes(n, G, ndim), device) if n > resident_points() else None)


def sector_fps_into(points: torch.Tensor, batch_ids: Optional[torch.Tensor], n_points: Optional[torch.Tensor],
                    batch_size: int, num_samples: int, num_sectors: int, center, rois: Optional[torch.Tensor],
                    roi_groups: Optional[PointGroups], roi_radius: Optional[float], ndim: int, buf: SectorBuffers) -> None:
    """The capturable composition, into ``sector_buffers``: segment ids -> their groups -> quotas -> segmented sampling.
    Four C calls, no allocation, nothing read back."""
    B, K, S = int(batch_size), int(num_samples), int(num_sectors)
    sector_ids_into(points, batch_ids, n_points, ndim, B, S, center, rois, roi_groups, roi_radius, buf.seg)
    _pointvoxel.point_groups_into(buf.seg, B * S, None, buf.rows, buf.offsets, buf.list, buf.groups_ws)
    groups = PointGroups(buf.rows, buf.offsets, buf.list, B * S)
    fps_quota_into(groups, B, S, K, buf.quota, buf.slot, buf.count)
    fps_segments_into(points, groups, buf.quota, buf.slot, S, K + S - 1, K, ndim, buf.idx, buf.seg_count, buf.ws)


def sector_fps(points: torch.Tensor, batch_ids: Optional[torch.Tensor], batch_size: int, num_samples: int,
               num_sectors: int = 6, *, center=(0., 0.), rois: Optional[torch.Tensor] = None,
               roi_batch_ids: Optional[torch.Tensor] = None, roi_radius: Optional[float] = None,
               n_points: Optional[torch.Tensor] = None, n_rois: Optional[torch.Tensor] = None, ndim: int = 3,
               return_sectors: bool = False):
    """PV-RCNN++'s sectorised proposal-centric keypoint sampling: the points ``sector_ids`` keeps are cut into S =
    `num_sectors` azimuth sectors per scene, sector k of a scene with n_k of its n kept points gets the quota ``min(n_k,
    ceil(n_k * K / n))`` (exact integers; K = `num_samples` in 1 .. 65 536), and every sector is sampled on its own by
    farthest-point sampling (the rule of ``farthest_point_sample``), one workgroup per sector.  Returns
    PointSamples(idx [B, K + S - 1], count [B], batch_ids [B * (K + S - 1)]): the samples of scene b are packed sector
    by sector in ascending sector, in sampling order inside a sector, count[b] = the sum of its quotas (<= K + S - 1), -1
    at or beyond it -- what ``gather_samples``, ``ball_query``, ``knn_query``, ``voxel_query`` and ``point_corners`` take
    unchanged.  `return_sectors` adds (seg [N], quota [B * S]).  Unlike OpenPCDet, a scene whose filter keeps nothing has
    count 0 (there: its first point), the indices of a scene are distinct, and the quota is the integer ceiling, not one
    in Python floats.  The sample set is NOT that of ``farthest_point_sample``: sectors are sampled independently.
    Nothing is read back.  No gradient with respect to coordinates."""
    N, centre, radius = _sector_inputs("sector_fps", points, batch_ids, batch_size, num_sectors, center, rois,
                                       roi_batch_ids, roi_radius, n_points, n_rois, ndim, num_samples)
    B, K, S = int(batch_size), int(num_samples), int(num_sectors)
    width = K + S - 1
    dev = points.device
    with torch.cuda.device(dev), torch.no_grad():
        rois, roi_groups = _roi_groups(rois, roi_batch_ids, B, n_rois, dev)
        buf = sector_buffers(N, B, K, S, ndim, dev)
        sector_fps_into(points.detach().contiguous(), None if batch_ids is None else batch_ids.contiguous(), n_points, B, K,
                        S, centre, rois, roi_groups, radius, ndim, buf)
        samples = PointSamples(buf.idx, buf.count, sample_batch_ids(B, width, dev))
    return (samples, buf.seg, buf.quota) if return_sectors else samples
