"""Cell-indexed ball query and radius-limited k-nearest neighbours over raw points on the HIP kernels of
csrc/cellquery.hip (``functional.point_cell_index`` / ``ball_query_cells`` / ``knn_query_cells`` and their ``_into``
forms; ``spatial.BallQueryAndGroup`` / ``KNNQueryAndGroup`` with ``coors_range_xyz``).  Not part of the reference.

  * ``point_cell_index``   the spatial index ``cluster_points`` builds for itself, as an object: the static voxeliser in
                           key order over cells of edge ``radius * (1 + 2**-6)`` (cell rows, rank map), ``point_groups``
                           over the cell of every point, and the points as 16-byte records in cell order
                           (``spx_cell_records``).  One index serves every query radius up to its own.
  * ``ball_query_cells``   ``ball_query``'s tables, bit for bit, from the records of the 27 cells round a query
                           (``spx_ball_query_cells``); a point outside the index's range is never a hit
  * ``knn_query_cells``    the k smallest under (d2, point index) among the points with d2 < r2
                           (``spx_knn_query_cells``): the leading entries of ``knn_query`` that lie inside the radius

The ``_into`` forms allocate nothing and read nothing back: they can be recorded in a stream capture.  There is no
gradient with respect to coordinates.
"""
from __future__ import annotations

import ctypes
from typing import NamedTuple, Optional, Sequence

import torch

from spconv_amd import _lib
from spconv_amd.pytorch import _pointvoxel
from spconv_amd.pytorch._cluster import ClusterPlan, cluster_plan
from spconv_amd.pytorch._knn import PointKNN, _check_knn
from spconv_amd.pytorch._level import flat_groups
from spconv_amd.pytorch._pointvoxel import PointGroups
from spconv_amd.pytorch._query import MAX_NSAMPLE, VoxelNeighbors, squared_radius
from spconv_amd.pytorch._rulebook import _check_count, _ptr, _require_gpu, _stream, _ws
from spconv_amd.pytorch._sample import _FLAG_PAD_FIRST, _check_pad


class PointCellIndex(NamedTuple):
    """The cell index of a cloud: plan (``cluster_plan``: radius, r2, cell edge, grid, range), points fp32 [N, >= 3]
    (read again for the offsets), indices int32 [N, 4] ({batch, z, y, x} of every cell row), rankmap, cells (the
    ``PointGroups`` of the cells: rows = the cell of every point, offsets [N + 1], list), records fp32 [N, 4] (the
    points as {x, y, z, index bits} in cell order, x = NaN for a point that takes no part), num_points (N as the
    tables report it), n_points (device int32 or None)."""
    plan: ClusterPlan
    points: torch.Tensor
    indices: torch.Tensor
    rankmap: torch.Tensor
    cells: PointGroups
    records: torch.Tensor
    num_points: int
    n_points: Optional[torch.Tensor] = None

    @property
    def radius(self) -> float:
        return self.plan.radius


class CellIndexBuffers(NamedTuple):
    """What ``point_cell_index_into`` writes, allocated once by ``cell_index_buffers`` for clouds of up to n points."""
    n_all: torch.Tensor             # int32 [1] = n: the point count of a call without n_points
    indices: torch.Tensor
    num_per_cell: torch.Tensor
    pc_cell_id: torch.Tensor
    n_cells: torch.Tensor
    rankmap: torch.Tensor
    voxel_ws: torch.Tensor
    cells: PointGroups
    groups_ws: torch.Tensor
    records: torch.Tensor


def _check_points(op: str, noun: str, t: torch.Tensor, batch_ids: Optional[torch.Tensor]) -> int:
    if t.dim() != 2 or t.dtype != torch.float32 or t.shape[1] < 3:
        raise ValueError(f"{op}: {noun} is a float32 tensor [N, >= 3] (ndim is 3, coordinates are float32), got "
                         f"{tuple(t.shape)} {t.dtype}")
    n = int(t.shape[0])
    if batch_ids is not None and (batch_ids.shape != (n,) or batch_ids.dtype != torch.int32):
        raise ValueError(f"{op}: the batch_ids of the {noun} are a CUDA int32 tensor [N]")
    return n


def cell_index_buffers(n: int, plan: ClusterPlan, device) -> CellIndexBuffers:
    """The buffers of ``point_cell_index_into`` for clouds of n >= 1 points (allocated here, once)."""
    L, n = _lib.load(), int(n)
    i32 = dict(dtype=torch.int32, device=device)
    e = lambda *shape: torch.empty(shape, **i32)
    voxel_bytes = int(L.spx_point2voxel_static_ws_bytes(n, n, 3, plan.batch_size, plan.host[2], 1))
    if voxel_bytes == 0:
        raise ValueError(f"point_cell_index: no key-ordered voxeliser for {plan.batch_size} x {list(plan.grid_zyx)} cells")
    return CellIndexBuffers(
        torch.full((1,), n, **i32), e(n, 4), e(n), torch.empty((n,), dtype=torch.int64, device=device), e(2),
        e(plan.rank_bytes // 4), _ws(voxel_bytes, device), PointGroups(e(n), e(n + 1), e(n), n),
        _ws(L.spx_point_groups_ws_bytes(n, n), device), torch.empty((n, 4), dtype=torch.float32, device=device))


def point_cell_index_into(points: torch.Tensor, batch_ids: Optional[torch.Tensor], n_points: Optional[torch.Tensor],
                          plan: ClusterPlan, buf: CellIndexBuffers) -> PointCellIndex:
    """The capturable composition, into ``cell_index_buffers``: cells -> their points -> records.  Three C calls, no
    allocation, nothing read back.  points fp32 [n, >= 3] contiguous, batch_ids int32 [n] or None."""
    L, n, s = _lib.load(), int(points.shape[0]), _stream(points)
    vsize, range_zyx, grid, range_xyz = plan.host
    count_dev = buf.n_all if n_points is None else n_points
    _lib.check(L.spx_point2voxel_static(
        points.data_ptr(), _ptr(batch_ids), n, count_dev.data_ptr(), int(points.shape[1]), 3, vsize, range_zyx, grid,
        plan.batch_size, n, 1, 0, 1, None, buf.indices.data_ptr(), buf.num_per_cell.data_ptr(), buf.pc_cell_id.data_ptr(),
        buf.n_cells.data_ptr(), None, 0, buf.rankmap.data_ptr(), buf.rankmap.numel() * 4, buf.voxel_ws.data_ptr(),
        buf.voxel_ws.numel(), s))
    cells = buf.cells
    _pointvoxel.point_groups_into(buf.pc_cell_id, n, count_dev, cells.rows, cells.offsets, cells.list, buf.groups_ws)
    _lib.check(L.spx_cell_records(
        points.data_ptr(), int(points.shape[1]), _ptr(batch_ids), n, count_dev.data_ptr(), plan.batch_size, range_xyz,
        cells.rows.data_ptr(), cells.offsets.data_ptr(), cells.list.data_ptr(), buf.records.data_ptr(), s))
    return PointCellIndex(plan, points, buf.indices, buf.rankmap, cells, buf.records, n, n_points)


def point_cell_index(points: torch.Tensor, batch_ids: Optional[torch.Tensor], batch_size: int, radius: float,
                     coors_range_xyz: Sequence[float], *, n_points: Optional[torch.Tensor] = None) -> PointCellIndex:
    """The cell index of a cloud for queries of up to `radius`.  points fp32 [N, >= 3] (x, y, z first), batch_ids int32
    [N] or None (all scene 0), n_points a device int32 or None.  A point TAKES PART when it lies below *n_points, its
    batch id is in [0, batch_size), its coordinates are finite and it lies inside `coors_range_xyz` (low <= p < high);
    every other point is never a hit.  The geometry is ``cluster_plan``'s, with its ValueErrors: cells of edge
    ``float32(radius * (1 + 2**-6))``, at most 2^14 per axis, a key space the rank map holds.  ndim is 3 and
    coordinates are float32.  Nothing is read back."""
    plan = cluster_plan(radius, coors_range_xyz, batch_size)
    N = _check_points("point_cell_index", "points", points, batch_ids)
    if N > (1 << 30) - 8:
        raise ValueError(f"point_cell_index: at most 2^30 - 8 points, got {N}")
    _require_gpu(points, "points")
    if batch_ids is not None:
        _require_gpu(batch_ids, "batch_ids")
    _check_count(n_points, "point_cell_index: n_points")
    dev = points.device
    with torch.cuda.device(dev), torch.no_grad():
        points = points.detach().contiguous()
        batch_ids = None if batch_ids is None else batch_ids.contiguous()
        if N == 0:      # one row that does not exist: the kernels meet an index without records
            points = torch.full((1, int(points.shape[1])), float("nan"), dtype=torch.float32, device=dev)
            batch_ids, n_points = None, torch.zeros((1,), dtype=torch.int32, device=dev)
        index = point_cell_index_into(points, batch_ids, n_points, plan, cell_index_buffers(max(N, 1), plan, dev))
        return index._replace(num_points=N)


def _query_r2(op: str, radius, index: PointCellIndex) -> float:
    """r2 of a query radius, which must not exceed the index's (both as float32)."""
    if radius is None:
        raise ValueError(f"{op}: radius must be >= 0, got None")
    r2 = squared_radius(radius)
    if not ctypes.c_float(float(radius)).value <= index.plan.radius:
        raise ValueError(f"{op}: radius {radius} exceeds the index's {index.plan.radius}: build the index at the largest "
                         f"radius it serves")
    return r2


def _check_queries(op: str, queries, q_batch_ids, index: PointCellIndex, entries: int, n_queries):
    M = _check_points(op, "queries", queries, q_batch_ids)
    if M * entries >= 1 << 31:
        raise ValueError(f"{op}: {M} queries x {entries} entries each do not fit 32-bit entries")
    _require_gpu(queries, "queries")
    if q_batch_ids is not None:
        _require_gpu(q_batch_ids, "batch_ids")
    _check_count(n_queries, f"{op}: n_queries")
    return M, queries.detach().contiguous(), None if q_batch_ids is None else q_batch_ids.contiguous()


def _index_args(index: PointCellIndex) -> tuple:
    plan, pts = index.plan, index.points
    lo = (ctypes.c_float * 3)(*plan.coors_range_xyz[:3])
    return (pts.data_ptr(), int(pts.shape[1]), int(pts.shape[0]), plan.batch_size, plan.host[2], lo, plan.vsize,
            index.cells.offsets.data_ptr(), index.rankmap.data_ptr(), index.rankmap.numel() * 4, index.records.data_ptr())


def ball_query_cells_into(queries: torch.Tensor, q_batch_ids: Optional[torch.Tensor], n_queries: Optional[torch.Tensor],
                          index: PointCellIndex, nsample: int, r2: float, pad_first: bool, rows: torch.Tensor,
                          count: torch.Tensor, offsets: Optional[torch.Tensor]) -> None:
    """The one C call into buffers the caller owns (no allocation: capturable).  r2: ``squared_radius`` of a radius up
    to the index's; rows int32 [M, nsample], count int32 [M], offsets fp32 [M, nsample, 3] or None."""
    _lib.check(_lib.load().spx_ball_query_cells(
        queries.data_ptr(), int(queries.shape[1]), _ptr(q_batch_ids), int(queries.shape[0]), _ptr(n_queries),
        *_index_args(index), int(nsample), float(r2), _FLAG_PAD_FIRST if pad_first else 0, rows.data_ptr(),
        count.data_ptr(), _ptr(offsets), _stream(queries)))


def knn_query_cells_into(queries: torch.Tensor, q_batch_ids: Optional[torch.Tensor], n_queries: Optional[torch.Tensor],
                         index: PointCellIndex, k: int, r2: float, eps: float, pad_first: bool, rows: torch.Tensor,
                         count: torch.Tensor, dist2: Optional[torch.Tensor] = None,
                         weights: Optional[torch.Tensor] = None, offsets: Optional[torch.Tensor] = None) -> None:
    """The one C call into buffers the caller owns (no allocation: capturable).  rows int32 [M, width] (width >= k),
    count int32 [M], dist2 / weights fp32 [M, width] or None, offsets fp32 [M, width, 3] or None."""
    _lib.check(_lib.load().spx_knn_query_cells(
        queries.data_ptr(), int(queries.shape[1]), _ptr(q_batch_ids), int(queries.shape[0]), _ptr(n_queries),
        *_index_args(index), int(k), int(rows.shape[1]), float(r2), float(eps), _FLAG_PAD_FIRST if pad_first else 0,
        rows.data_ptr(), count.data_ptr(), _ptr(dist2), _ptr(weights), _ptr(offsets), _stream(queries)))


def ball_query_cells(queries: torch.Tensor, q_batch_ids: Optional[torch.Tensor], index: PointCellIndex, radius: float,
                     nsample: int, *, pad: str = "none", with_offsets: bool = False,
                     n_queries: Optional[torch.Tensor] = None, with_groups: bool = False) -> VoxelNeighbors:
    """``ball_query`` over a ``point_cell_index``: the first `nsample` (1 .. 128) points inside `radius` of each query,
    in ascending point index, among the points that take part in the index.  `radius` is any value with
    ``float32(radius) <= index.radius`` (a larger one is a ValueError): one index built at the largest radius serves
    several.  Rows, count and offsets EQUAL ``ball_query``'s over the same cloud, bit for bit, for every point inside
    the index's range; a point outside the range is never a hit (the one difference).  A query may lie anywhere, the
    range included or not; one with a NaN coordinate, a batch id outside [0, batch_size) or at or beyond *n_queries has
    count 0.  Returns the ``VoxelNeighbors`` of the points, as ``ball_query`` does.  One launch that reads the records
    of at most 27 cells per query, nothing read back.  No gradient with respect to coordinates."""
    op = "ball_query_cells"
    if not 1 <= int(nsample) <= MAX_NSAMPLE:
        raise ValueError(f"{op}: nsample must be in 1 .. {MAX_NSAMPLE}, got {nsample}")
    _check_pad(op, pad)
    r2, nsample = _query_r2(op, radius, index), int(nsample)
    M, queries, q_batch_ids = _check_queries(op, queries, q_batch_ids, index, nsample, n_queries)
    dev, N = queries.device, index.num_points
    with torch.cuda.device(dev), torch.no_grad():
        rows = torch.empty((M, nsample), dtype=torch.int32, device=dev)
        count = torch.empty((M,), dtype=torch.int32, device=dev)
        offsets = torch.empty((M, nsample, 3), dtype=torch.float32, device=dev) if with_offsets else None
        if M > 0:
            ball_query_cells_into(queries, q_batch_ids, n_queries, index, nsample, r2, pad == "first", rows, count, offsets)
        flat = flat_groups(rows, N, index.n_points) if with_groups else None
    return VoxelNeighbors(rows, count, offsets, flat, N, n_queries, index.n_points)


def knn_query_cells(queries: torch.Tensor, q_batch_ids: Optional[torch.Tensor], index: PointCellIndex, k: int,
                    radius: float, *, width: Optional[int] = None, pad: str = "none", eps: float = 1e-8,
                    with_offsets: bool = False, n_queries: Optional[torch.Tensor] = None,
                    with_groups: bool = False) -> PointKNN:
    """``knn_query`` limited to `radius`, over a ``point_cell_index``: per query the `k` (1 .. 64) smallest under the
    total order (d2, point index) among the points of the index with ``d2 < float32(radius) ** 2`` -- the leading
    entries of ``knn_query``'s result that lie inside the radius.  count [M] = min(points inside the radius, k).
    `radius` as ``ball_query_cells`` takes it; `width`, `pad`, `eps`, the tables (rows, dist2, weights -- normalised
    over the kept entries --, offsets on request) and the validity of a query (finite coordinates) are ``knn_query``'s.
    A k-NN without a radius is not this kernel's: use ``knn_query``.  Returns a ``PointKNN``.  One launch, nothing read
    back.  No gradient with respect to coordinates or weights."""
    op = "knn_query_cells"
    k, width = _check_knn(op, k, width, pad, eps)
    r2 = _query_r2(op, radius, index)
    M, queries, q_batch_ids = _check_queries(op, queries, q_batch_ids, index, width, n_queries)
    dev, N = queries.device, index.num_points
    with torch.cuda.device(dev), torch.no_grad():
        rows = torch.empty((M, width), dtype=torch.int32, device=dev)
        count = torch.empty((M,), dtype=torch.int32, device=dev)
        dist2 = torch.empty((M, width), dtype=torch.float32, device=dev)
        weights = torch.empty((M, width), dtype=torch.float32, device=dev)
        offsets = torch.empty((M, width, 3), dtype=torch.float32, device=dev) if with_offsets else None
        if M > 0:
            knn_query_cells_into(queries, q_batch_ids, n_queries, index, k, r2, eps, pad == "first", rows, count, dist2,
                                 weights, offsets)
        flat = flat_groups(rows, N, index.n_points) if with_groups else None
    return PointKNN(rows, count, dist2, weights, offsets, flat, k, N, n_queries, index.n_points)
