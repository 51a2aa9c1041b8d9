"""k-nearest-neighbour query and inverse-distance interpolation over raw points on the HIP kernel of csrc/knn.hip
(``functional.knn_query`` / ``knn_query_into`` / ``knn_interpolate`` / ``three_nn``, ``spatial.KNNInterpolate`` /
``KNNQueryAndGroup``).  Not part of the reference; the code bases users port call them as the ``three_nn`` /
``three_interpolate`` CUDA extensions of ``pointnet2_stack`` / ``pointnet2_batch`` (every PointNet++ feature-propagation
layer, PointRCNN, 3DSSD, IA-SSD, the point heads of the PV-RCNN family) and the ``knn_query`` of ``pointops`` (Point
Transformer grouping, unpooling interpolation, DGCNN-style edge features).

  * ``knn_query``        per query the k points of its scene that come first under the total order (squared distance,
                         point index), in that order (``spx_knn_query``: one launch), with optional squared distances,
                         normalised inverse-distance weights and point-minus-query vectors, as a ``PointKNN``
  * ``PointKNN.neighbors()``  the ``VoxelNeighbors`` that ``group_voxels`` and its gradient take (width == k)
  * ``PointKNN.corners()``    the ``PointCorners`` that ``voxels_to_points_trilinear`` and its gradient take (weights and
                         a width of 4 or 8), the points standing where a level's rows do
  * ``knn_interpolate``  ``out[i] = sum_s w[i, s] * feats[rows[i, s]]`` under the name users look for

There is no gradient with respect to coordinates or weights: raw coordinates need none (pointnet2's three_interpolate
gives none either).
"""
from __future__ import annotations

import math
from typing import NamedTuple, Optional

import torch

from spconv_amd import _lib
from spconv_amd.pytorch._interp import PointCorners, voxels_to_points_trilinear
from spconv_amd.pytorch._level import flat_groups
from spconv_amd.pytorch._pointvoxel import PointGroups
from spconv_amd.pytorch._query import VoxelNeighbors
from spconv_amd.pytorch._rulebook import _ptr, _stream
from spconv_amd.pytorch._sample import _FLAG_PAD_FIRST, _check_pad, _scene_query

MAX_K = 64


class PointKNN(NamedTuple):
    """The nearest-neighbour table of a set of queries over a point cloud: rows int32 [M, width] (point index, -1:
    none), count int32 [M] = min(valid points of the query's scene, k), dist2 / weights fp32 [M, width] or None,
    offsets fp32 [M, width, ndim] (point minus query) or None, groups (a ``PointGroups`` over the FLATTENED rows --
    entry e = m * width + s -- or None: only a gradient needs it), k, num_points (N), n_queries / n_points (device
    int32 or None: queries / points at or beyond them do not exist)."""
    rows: torch.Tensor
    count: torch.Tensor
    dist2: Optional[torch.Tensor]
    weights: Optional[torch.Tensor]
    offsets: Optional[torch.Tensor]
    groups: Optional[PointGroups]
    k: int
    num_points: int
    n_queries: Optional[torch.Tensor] = None
    n_points: Optional[torch.Tensor] = None

    def neighbors(self) -> VoxelNeighbors:
        """The table as ``group_voxels(point_feats, ...)`` takes it (num_voxels = N, n_live = n_points)."""
        if int(self.rows.shape[1]) != self.k:
            raise ValueError(f"PointKNN.neighbors: grouping takes a table of width k, got width {int(self.rows.shape[1])} "
                             f"for k = {self.k}; call knn_query with width=None")
        return VoxelNeighbors(self.rows, self.count, self.offsets, self.groups, self.num_points, self.n_queries,
                              self.n_points)

    def corners(self) -> PointCorners:
        """The table as ``voxels_to_points_trilinear(known_feats, ...)`` takes it (num_voxels = N, the queries standing
        where the points of a corner table do)."""
        if self.weights is None:
            raise ValueError("PointKNN.corners: a blend needs the weights; call knn_query with with_weights=True")
        if int(self.rows.shape[1]) not in (4, 8):
            raise ValueError(f"PointKNN.corners: the blend takes a table of width 4 or 8, got {int(self.rows.shape[1])}; "
                             f"call knn_query with width=4 or width=8")
        return PointCorners(self.rows, self.weights, self.groups, self.num_points, self.n_queries, self.n_points)


def max_k() -> int:
    return int(_lib.load().spx_knn_max_k())


def _check_knn(op: str, k: int, width: Optional[int], pad: str, eps: float) -> tuple:
    if not 1 <= int(k) <= MAX_K:
        raise ValueError(f"{op}: k must be in 1 .. {MAX_K}, got {k}")
    width = int(k) if width is None else int(width)
    if width < int(k):
        raise ValueError(f"{op}: width must be >= k, got {width} < {k}")
    _check_pad(op, pad)
    if eps is None or not (0.0 <= float(eps) < math.inf):
        raise ValueError(f"{op}: eps must be finite and >= 0, got {eps}")
    return int(k), width


def knn_query_into(queries: torch.Tensor, q_batch_ids: Optional[torch.Tensor], n_queries: Optional[torch.Tensor],
                   points: torch.Tensor, groups: PointGroups, ndim: int, k: int, eps: float, pad_first: bool,
                   rows: torch.Tensor, count: torch.Tensor, dist2: Optional[torch.Tensor] = None,
                   weights: Optional[torch.Tensor] = None, offsets: Optional[torch.Tensor] = None) -> None:
    """The one C call into buffers the caller owns (no allocation, no workspace: capturable).  groups: the
    ``scene_groups`` of the points; rows int32 [M, width] (width >= k), count int32 [M], dist2 / weights fp32
    [M, width] or None, offsets fp32 [M, width, ndim] or None."""
    _lib.check(_lib.load().spx_knn_query(
        queries.data_ptr(), int(queries.shape[1]), _ptr(q_batch_ids), int(queries.shape[0]), _ptr(n_queries),
        points.data_ptr(), int(points.shape[1]), int(points.shape[0]), int(ndim), groups.offsets.data_ptr(),
        groups.list.data_ptr(), int(groups.num_voxels), int(k), int(rows.shape[1]), float(eps),
        _FLAG_PAD_FIRST if pad_first else 0, rows.data_ptr(), count.data_ptr(), _ptr(dist2), _ptr(weights),
        _ptr(offsets), _stream(queries)))


def knn_query(queries: torch.Tensor, q_batch_ids: Optional[torch.Tensor], points: torch.Tensor,
              p_batch_ids: Optional[torch.Tensor], batch_size: int, k: int, *, ndim: int = 3, width: Optional[int] = None,
              pad: str = "none", with_dist2: bool = True, with_weights: bool = False, eps: float = 1e-8,
              with_offsets: bool = False, n_queries: Optional[torch.Tensor] = None,
              n_points: Optional[torch.Tensor] = None, with_groups: bool = False,
              groups: Optional[PointGroups] = None) -> PointKNN:
    """The `k` (1 .. 64) nearest points of its scene for each query.  queries fp32 [M, >= ndim], points fp32
    [N, >= ndim] (x, y, z first), q_batch_ids / p_batch_ids int32 or None (all scene 0).  A point is valid when it lies
    below *n_points, its batch id is in [0, batch_size) and its first ndim coordinates are finite; a query when it lies
    below *n_queries, its batch id is in [0, batch_size) and its first ndim coordinates are finite.  With d = point -
    query and d2 in fp32, every operation rounded on its own, a query keeps the count = min(valid points of ITS scene,
    k) candidates that come first under the TOTAL ORDER (d2, point index), in that order: equal distances go to the
    lower point index, and the result does not depend on how queries or points are ordered across scenes.  `width`
    (default k, >= k) is the row stride of every table: rows [M, width], count [M], and on request dist2 [M, width],
    weights [M, width] and the point-minus-query vectors [M, width, ndim].  Slots in [count, k) hold -1 / 0, or with
    pad="first" and count > 0 slot 0 again with weight 0; slots in [k, width) always hold -1 / 0; an invalid query has
    count 0.  The weights are pointnet2's: ``r = 1 / (sqrt(d2) + eps)``, ``w = r / sum(r)`` over the kept slots in
    ascending slot, in fp32.  Returns a ``PointKNN``; with_groups builds the transposed list the gradients of
    ``group_voxels`` / ``knn_interpolate`` walk.  `groups`: a ready ``scene_groups`` of the points.  One launch, nothing
    read back.  No gradient with respect to coordinates or weights."""
    k, width = _check_knn("knn_query", k, width, pad, eps)
    queries, q_batch_ids, points, groups, n_points, M, N, dev = _scene_query(
        "knn_query", queries, q_batch_ids, points, p_batch_ids, batch_size, ndim, width, n_queries, n_points, groups)
    with torch.cuda.device(dev), torch.no_grad():
        rows = torch.empty((M, width), dtype=torch.int32, device=dev)
        count = torch.empty((M,), dtype=torch.int32, device=dev)
        dist2 = torch.empty((M, width), dtype=torch.float32, device=dev) if with_dist2 else None
        weights = torch.empty((M, width), dtype=torch.float32, device=dev) if with_weights else None
        offsets = torch.empty((M, width, ndim), dtype=torch.float32, device=dev) if with_offsets else None
        if M > 0:
            knn_query_into(queries, q_batch_ids, n_queries, points, groups, ndim, k, eps, pad == "first", rows, count,
                           dist2, weights, offsets)
        flat = flat_groups(rows, N, n_points) if with_groups else None
    return PointKNN(rows, count, dist2, weights, offsets, flat, k, N, n_queries, n_points)


def three_nn(unknown: torch.Tensor, unknown_batch_ids: Optional[torch.Tensor], known: torch.Tensor,
             known_batch_ids: Optional[torch.Tensor], batch_size: int, **kwargs) -> PointKNN:
    """pointnet2's ``three_nn`` with its weights: ``knn_query(unknown, ..., known, ..., k=3, width=4,
    with_weights=True)`` -- the table ``knn_interpolate`` blends.  Further keywords are ``knn_query``'s.  No gradient
    with respect to coordinates or weights."""
    for fixed in ("k", "width", "with_weights"):
        if fixed in kwargs:
            raise ValueError(f"three_nn: {fixed} is fixed (k=3, width=4, with_weights=True); use knn_query")
    return knn_query(unknown, unknown_batch_ids, known, known_batch_ids, batch_size, 3, width=4, with_weights=True,
                     **kwargs)


def knn_interpolate(known_feats: torch.Tensor, knn: PointKNN) -> torch.Tensor:
    """[N, C] features of the known points -> [M, C]: row m is ``sum_s weights[m, s] * known_feats[rows[m, s]]``, added
    in ascending slot in fp32 (fp64 for float64) and rounded once; zeros for a query without a neighbour
    (``voxels_to_points_trilinear(known_feats, knn.corners())``: pointnet2's ``three_interpolate``).  Differentiable in
    known_feats (a segment sum in ascending entry, no atomics: identical run to run; the table needs its groups);
    there is no gradient with respect to coordinates or weights."""
    return voxels_to_points_trilinear(known_feats, knn.corners())
