"""Instance clustering on the HIP kernels of csrc/cluster.hip (``functional.cluster_points`` / ``cluster_points_into``,
``spatial.ClusterPoints``): the connected components of the radius graph of a point cloud.  Not part of the reference;
the bottom-up instance-segmentation networks over sparse U-Nets (PointGroup, HAIS, SoftGroup, SSTNet, ISBNet's grouping
branch) call it as ``ballquery_batch_p`` + ``bfs_cluster`` of ``pointgroup_ops`` / ``softgroup.ops``, the second a
breadth-first search on the CPU behind a copy to the host.

  * index    existing pieces, composed here: the static voxeliser in key order over cells of edge ``radius * (1 +
             2**-6)`` (``spx_point2voxel_static``: cell rows and the level's rank map) and ``point_groups`` over its
             ``pc_voxel_id`` (the points of every cell)
  * records  the points as 16-byte records in cell order (``spx_cluster_records``)
  * link     every pair of the radius graph united in a lock-free union-find (``spx_cluster_link``)
  * roots    ``root[i]`` = the smallest point index of i's component (``spx_cluster_roots``)
  * number   sizes from ``point_groups`` over the roots, kept components numbered by ascending root
             (``spx_cluster_number``), and ``point_groups`` over the numbers: the clusters as ``PointGroups``

Nothing is read back; ``cluster_points_into`` allocates nothing and can be recorded in a stream capture.  There are no
gradients: every output is an integer.
"""
from __future__ import annotations

import ctypes
import math
from typing import NamedTuple, Optional, Sequence

import torch

from spconv_amd import _lib
from spconv_amd.pytorch import _pointvoxel
from spconv_amd.pytorch._pointvoxel import PointGroups
from spconv_amd.pytorch._query import squared_radius
from spconv_amd.pytorch._rulebook import _check_count, _ptr, _require_gpu, _stream, _ws

CELL_WIDEN = 1.0 + 2.0 ** -6


class PointClusters(NamedTuple):
    """The clusters of a cloud: cluster_of_point int32 [N] (-1: the point takes no part or its component was filtered),
    root int32 [N] (the smallest point index of the point's component, -1: takes no part), count (device int32 [1]: the
    clusters kept), groups (a ``PointGroups`` over cluster ids: rows = cluster_of_point, offsets [cap + 1], list with
    the members of every cluster in ascending point index, n_live = count), status (device int32 [1]: 0, or the bits of
    ``spx_cluster_link`` for a loop that left through its iteration cap -- nothing reads it on the hot path)."""
    cluster_of_point: torch.Tensor
    root: torch.Tensor
    count: torch.Tensor
    groups: PointGroups
    status: torch.Tensor

    @property
    def cap(self) -> int:
        return self.groups.num_voxels


class ClusterPlan(NamedTuple):
    """The host side of a clustering, made once by ``cluster_plan``: r2 (``squared_radius``), the cell edge, the grid in
    zyx order, the range, and the host arrays the C calls take."""
    radius: float
    r2: float
    vsize: float
    batch_size: int
    grid_zyx: tuple
    coors_range_xyz: tuple
    rank_bytes: int
    host: tuple             # (vsize_zyx, coors_range_zyx, grid_zyx, range_xyz) as ctypes arrays


class ClusterBuffers(NamedTuple):
    """What ``cluster_points_into`` writes, allocated once by ``cluster_buffers`` for clouds of up to n points."""
    n_all: torch.Tensor             # int32 [1] = n: the point count of a call without n_points
    indices: torch.Tensor           # the voxeliser's outputs: cell rows [n, 4], counts, the cell of every point, {kept, found}
    num_per_cell: torch.Tensor
    pc_cell_id: torch.Tensor
    n_cells: torch.Tensor
    rankmap: torch.Tensor
    voxel_ws: torch.Tensor
    cells: PointGroups              # the points of every cell
    groups_ws: torch.Tensor         # scratch of the three point_groups calls
    root: torch.Tensor
    status: torch.Tensor
    ws: torch.Tensor
    sizes: PointGroups              # point_groups over the roots: offsets give the sizes
    cluster_id: torch.Tensor
    count: torch.Tensor
    groups: PointGroups             # the result


def max_axis_cells() -> int:
    """The most cells per axis the widened cell edge is proven for."""
    return int(_lib.load().spx_cluster_max_axis_cells())


def _f32(v: float) -> float:
    return ctypes.c_float(float(v)).value


def cluster_plan(radius: float, coors_range_xyz: Sequence[float], batch_size: int) -> ClusterPlan:
    """Every ValueError of the geometry: a finite radius > 0, a finite, non-empty range of six floats, a grid of cells
    of edge ``float32(radius * (1 + 2**-6))`` that covers the range with at most ``max_axis_cells()`` cells per axis and
    a key space (batch_size x grid) the rank map holds."""
    op = "cluster_points"
    if int(batch_size) < 1:
        raise ValueError(f"{op}: batch_size must be >= 1, got {batch_size}")
    try:
        r = _f32(radius)
    except (TypeError, ValueError):
        raise ValueError(f"{op}: radius must be finite and > 0, got {radius!r}") from None
    if not 0. < r < float("inf"):
        raise ValueError(f"{op}: radius must be finite and > 0, got {radius!r}")
    rng = [_f32(v) for v in coors_range_xyz]
    if len(rng) != 6 or not all(math.isfinite(v) for v in rng) or not all(rng[j] < rng[3 + j] for j in range(3)):
        raise ValueError(f"{op}: coors_range_xyz is six finite floats (lows, then highs) with low < high, got "
                         f"{list(coors_range_xyz)}")
    vsize = _f32(r * CELL_WIDEN)
    # cells that cover [lo, hi): floorf((p - lo) / vsize) of a point below hi is at most that of hi, rounding being
    # monotone; the quotient of two float32 rounded through double is the float32 quotient
    grid_xyz = [int(math.floor(_f32(_f32(rng[3 + j] - rng[j]) / vsize))) + 1 for j in range(3)]
    limit = max_axis_cells()
    if max(grid_xyz) > limit:
        raise ValueError(f"{op}: the range holds {grid_xyz} cells of edge {vsize} (xyz); the cell search is exact up to "
                         f"{limit} cells per axis: cluster a smaller range or with a larger radius")
    grid_zyx = grid_xyz[::-1]
    rank_bytes = int(_lib.load().spx_rankmap_bytes(3, int(batch_size), _lib.ints(grid_zyx)))
    if rank_bytes == 0 or rank_bytes > 1 << 30:
        raise ValueError(f"{op}: {batch_size} x {grid_zyx} cells are beyond what a rank map holds (2^31 cells, 1 GiB): "
                         f"cluster a smaller range or with a larger radius")
    f = lambda v: (ctypes.c_float * len(v))(*v)
    host = (f([vsize] * 3), f(rng[:3][::-1] + rng[3:][::-1]), _lib.ints(grid_zyx), f(rng))
    return ClusterPlan(r, squared_radius(r), vsize, int(batch_size), tuple(grid_zyx), tuple(rng), rank_bytes, host)


def _check_inputs(points, batch_ids, labels, valid, n_points, min_points) -> int:
    op = "cluster_points"
    if points.dim() != 2 or points.dtype != torch.float32 or points.shape[1] < 3:
        raise ValueError(f"{op}: points is a float32 tensor [N, >= 3], got {tuple(points.shape)} {points.dtype}")
    N = int(points.shape[0])
    if N > (1 << 30) - 8:
        raise ValueError(f"{op}: at most 2^30 - 8 points, got {N}")
    for name, t in (("batch_ids", batch_ids), ("labels", labels)):
        if t is not None and (t.shape != (N,) or t.dtype != torch.int32):
            raise ValueError(f"{op}: {name} is a CUDA int32 tensor [N]")
    if valid is not None and (valid.shape != (N,) or valid.dtype not in (torch.bool, torch.uint8)):
        raise ValueError(f"{op}: valid is a CUDA bool or uint8 tensor [N]")
    if isinstance(min_points, torch.Tensor):
        if min_points.dim() != 1 or min_points.dtype != torch.float32 or min_points.numel() < 1:
            raise ValueError(f"{op}: a min_points table is a CUDA float32 tensor [num_labels]")
        if labels is None:
            raise ValueError(f"{op}: a min_points table is indexed by the component's label: it requires labels")
    elif int(min_points) < 1:
        raise ValueError(f"{op}: min_points must be >= 1, got {min_points}")
    for name, t in (("points", points), ("batch_ids", batch_ids), ("labels", labels), ("valid", valid),
                    ("min_points", min_points if isinstance(min_points, torch.Tensor) else None)):
        if t is not None:
            _require_gpu(t, name)
    _check_count(n_points, f"{op}: n_points")
    return N


def cluster_cap(n: int, min_points) -> int:
    """The host-known bound on the clusters of n points: n // min_points, n for the table form (1 at the least)."""
    return max(1, int(n) if isinstance(min_points, torch.Tensor) else int(n) // int(min_points))


def cluster_buffers(n: int, plan: ClusterPlan, cap: int, device) -> ClusterBuffers:
    """The buffers of ``cluster_points_into`` for clouds of n >= 1 points and up to `cap` clusters (allocated here,
    once)."""
    L, n, cap = _lib.load(), int(n), int(cap)
    i32 = dict(dtype=torch.int32, device=device)
    e = lambda *shape: torch.empty(shape, **i32)
    voxel_bytes = int(L.spx_point2voxel_static_ws_bytes(n, n, 3, plan.batch_size, plan.host[2], 1))
    if voxel_bytes == 0:
        raise ValueError(f"cluster_points: no key-ordered voxeliser for {plan.batch_size} x {list(plan.grid_zyx)} cells")
    return ClusterBuffers(
        torch.full((1,), n, **i32), e(n, 4), e(n), torch.empty((n,), dtype=torch.int64, device=device), e(2),
        e(plan.rank_bytes // 4), _ws(voxel_bytes, device), PointGroups(e(n), e(n + 1), e(n), n),
        _ws(L.spx_point_groups_ws_bytes(n, n), device), e(n), e(1), _ws(L.spx_cluster_ws_bytes(n), device),
        PointGroups(e(n), e(n + 1), e(n), n), e(n), e(1), PointGroups(e(n), e(cap + 1), e(n), cap))


def cluster_points_into(points: torch.Tensor, batch_ids: Optional[torch.Tensor], n_points: Optional[torch.Tensor],
                        plan: ClusterPlan, labels: Optional[torch.Tensor], valid: Optional[torch.Tensor], min_points,
                        buf: ClusterBuffers, stage=None) -> PointClusters:
    """The capturable composition, into ``cluster_buffers``: cells -> their points -> records -> link -> roots -> sizes
    -> numbers -> the clusters' points.  Eight C calls, no allocation, nothing read back.  points fp32 [n, >= 3]
    contiguous, the other tensors as ``cluster_points`` takes them (valid as uint8).  `stage(name)`: called behind the
    launches of every item (a probe's clock), never on the hot path."""
    L, n, s = _lib.load(), int(points.shape[0]), _stream(points)
    vsize, range_zyx, grid, range_xyz = plan.host
    count_dev = buf.n_all if n_points is None else n_points
    mark = stage if stage is not None else (lambda name: None)
    _lib.check(L.spx_point2voxel_static(
        points.data_ptr(), _ptr(batch_ids), n, count_dev.data_ptr(), int(points.shape[1]), 3, vsize, range_zyx, grid,
        plan.batch_size, n, 1, 0, 1, None, buf.indices.data_ptr(), buf.num_per_cell.data_ptr(), buf.pc_cell_id.data_ptr(),
        buf.n_cells.data_ptr(), None, 0, buf.rankmap.data_ptr(), buf.rankmap.numel() * 4, buf.voxel_ws.data_ptr(),
        buf.voxel_ws.numel(), s))
    cells = buf.cells
    _pointvoxel.point_groups_into(buf.pc_cell_id, n, count_dev, cells.rows, cells.offsets, cells.list, buf.groups_ws)
    mark("index")
    _lib.check(L.spx_cluster_records(
        points.data_ptr(), int(points.shape[1]), _ptr(batch_ids), n, count_dev.data_ptr(), plan.batch_size, _ptr(labels),
        _ptr(valid), range_xyz, cells.rows.data_ptr(), cells.offsets.data_ptr(), cells.list.data_ptr(), buf.root.data_ptr(),
        buf.status.data_ptr(), buf.ws.data_ptr(), buf.ws.numel(), s))
    mark("records")
    _lib.check(L.spx_cluster_link(
        n, plan.batch_size, grid, buf.indices.data_ptr(), cells.offsets.data_ptr(), buf.rankmap.data_ptr(),
        buf.rankmap.numel() * 4, _ptr(labels), plan.r2, buf.root.data_ptr(), buf.status.data_ptr(), buf.ws.data_ptr(),
        buf.ws.numel(), s))
    mark("link")
    _lib.check(L.spx_cluster_roots(n, buf.root.data_ptr(), buf.status.data_ptr(), s))
    sizes = buf.sizes
    _pointvoxel.point_groups_into(buf.root, n, count_dev, sizes.rows, sizes.offsets, sizes.list, buf.groups_ws)
    table = min_points if isinstance(min_points, torch.Tensor) else None
    cap = buf.groups.num_voxels
    _lib.check(L.spx_cluster_number(
        n, buf.root.data_ptr(), sizes.offsets.data_ptr(), _ptr(labels), 1 if table is not None else int(min_points),
        _ptr(table), 0 if table is None else int(table.numel()), cap, buf.cluster_id.data_ptr(), buf.count.data_ptr(),
        buf.ws.data_ptr(), buf.ws.numel(), s))
    mark("flatten")
    g = buf.groups
    _pointvoxel.point_groups_into(buf.cluster_id, cap, count_dev, g.rows, g.offsets, g.list, buf.groups_ws)
    mark("groups")
    groups = PointGroups(g.rows, g.offsets, g.list, cap, n_points, buf.count)
    return PointClusters(g.rows, buf.root, buf.count, groups, buf.status)


def cluster_points(points: torch.Tensor, batch_ids: Optional[torch.Tensor], batch_size: int, radius: float,
                   coors_range_xyz: Sequence[float], *, labels: Optional[torch.Tensor] = None,
                   valid: Optional[torch.Tensor] = None, min_points=1,
                   n_points: Optional[torch.Tensor] = None) -> PointClusters:
    """The clusters of a cloud: the connected components of its radius graph (PointGroup's ``ballquery_batch_p`` +
    ``bfs_cluster``).  points fp32 [N, >= 3] (x, y, z first), batch_ids / labels int32 [N] or None, valid bool / uint8
    [N] or None, n_points a device int32 or None.  Point i TAKES PART when i < *n_points, its batch id is in [0,
    batch_size), its coordinates are finite and inside `coors_range_xyz` (low <= p < high), it passes `valid` and its
    label is >= 0.  Two points that take part are LINKED when they share the scene and the label and ``d2 < r2`` under
    ``ball_query``'s float32 predicate (r2 = ``squared_radius(radius)``; distance exactly `radius` does not link): a
    cluster is a connected component of the graph ``ball_query`` would return with an unbounded nsample.  The ROOT of a
    component is its smallest point index; a component is kept when its size is >= `min_points` -- an int, or a device
    float32 table [num_labels] indexed by the component's label (SoftGroup's ``class_numpoint_mean * npoint_thr``; it
    requires labels, and a label at or beyond the table keeps nothing) --, and kept components are numbered 0, 1, ...
    by ascending root, the order ``bfs_cluster`` discovers them in.  Returns PointClusters(cluster_of_point, root,
    count, groups, status); ``points_to_voxels(feat, clusters.groups, "max" | "mean" | "sum")`` and
    ``voxels_to_points`` work on clusters unchanged, with cap = N // min_points (N for the table form) cluster rows of
    which *count are live.  Unlike upstream, the members of a cluster are listed in ascending point index, not in
    breadth-first order, and a point outside the range takes no part.  The result is identical run to run.  Nothing is
    read back.  No gradients: every output is an integer."""
    plan = cluster_plan(radius, coors_range_xyz, batch_size)
    N = _check_inputs(points, batch_ids, labels, valid, n_points, min_points)
    dev, cap = points.device, cluster_cap(N, min_points)
    with torch.cuda.device(dev), torch.no_grad():
        if N == 0:
            i32 = dict(dtype=torch.int32, device=dev)
            empty, zero = torch.empty((0,), **i32), torch.zeros((1,), **i32)
            groups = PointGroups(empty, torch.zeros((cap + 1,), **i32), empty, cap, n_points, zero)
            return PointClusters(empty, empty, zero, groups, torch.zeros((1,), **i32))
        contiguous = lambda t: None if t is None else t.contiguous()
        if valid is not None:
            valid = valid.contiguous().view(torch.uint8)
        return cluster_points_into(points.detach().contiguous(), contiguous(batch_ids), n_points, plan, contiguous(labels),
                                   valid, contiguous(min_points) if isinstance(min_points, torch.Tensor) else min_points,
                                   cluster_buffers(N, plan, cap, dev))
