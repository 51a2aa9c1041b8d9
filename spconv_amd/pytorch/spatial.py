"""``spconv.pytorch.spatial`` (reference ``spconv/pytorch/spatial.py:28-45``), and ``SparseCollapse``: the hand-over
from a 3-D backbone to a sparse 2-D head on the kernels of csrc/collapse.hip; ``SparsePrune`` (csrc/select.hip);
``TrilinearDevoxelize``: a sparse level read out at points (csrc/interp.hip); ``VoxelQueryAndGroup``: the voxels around
query points, gathered (csrc/query.hip); ``FarthestPointSample`` / ``BallQueryAndGroup``: keypoints of a raw cloud and the
raw points around query points, gathered (csrc/sample.hip); ``KNNInterpolate`` / ``KNNQueryAndGroup``: features carried
to many points from their nearest few, and the nearest raw points of query points, gathered (csrc/knn.hip);
``RotatedNMS``: rotated non-maximum suppression that stays on the device (csrc/box.hip); ``RotatedIoU3DLoss``: the
rotated-IoU regression loss of aligned boxes, with a gradient (csrc/boxgrad.hip); ``RoIPointPool3d`` /
``RoIAwarePool3d``: the points of every RoI, gathered or reduced per cell of a grid over the box (csrc/roi.hip);
``CenterHeadTargets``: the Gaussian heatmaps and regression rows of a centre head (csrc/center.hip)."""
from typing import NamedTuple, Optional, Sequence

import torch

from spconv_amd.pytorch.core import SparseConvTensor
from spconv_amd.pytorch.modules import SparseModule


def _group(feats: torch.Tensor, nb, use_xyz: bool):
    """([M, nsample, (ndim +) C], count [M]): the rows of `nb`, with `use_xyz` behind the offsets cast to their dtype."""
    from spconv_amd.pytorch import functional as F
    grouped = F.group_voxels(feats, nb)
    if use_xyz:
        grouped = torch.cat([nb.offsets.to(grouped.dtype), grouped], dim=2)
    return grouped, nb.count


class RemoveDuplicate(SparseModule):
    """Keeps one row per (batch, coordinate): the FIRST one in row order, which is also the row the
    rulebook's hash keeps for a duplicated coordinate (csrc/sparse/indices.py:1672).  The reference
    linearises the indices and takes ``torch.unique`` of the keys; so does this, with the row order
    made explicit."""

    def forward(self, x: SparseConvTensor) -> SparseConvTensor:
        inds = x.indices
        key = inds[:, 0].to(torch.int64)
        for d, size in enumerate(x.spatial_shape):
            key = key * int(size) + inds[:, d + 1].to(torch.int64)
        uniq, inverse = torch.unique(key, return_inverse=True)
        rows = torch.arange(inds.shape[0], device=inds.device)
        first = torch.full((uniq.shape[0],), inds.shape[0], dtype=rows.dtype, device=inds.device)
        first.scatter_reduce_(0, inverse, rows, reduce="amin")
        first = first.sort().values                      # keep the surviving rows in their order
        return SparseConvTensor(x.features[first], inds[first].contiguous(), x.spatial_shape,
                                x.batch_size, x.grid)


class SparseCollapse(SparseModule):
    """Drops the spatial axes ``axes`` (0 = the first: z of a zyx tensor) and merges the rows that land on one
    (batch, kept axes) cell by ``reduce`` = "sum" | "mean" | "max": the height compression of the fully sparse
    detectors (``functional.sparse_collapse``).  ``axes = ()`` merges duplicate coordinates.  The result is a fresh
    tensor over the kept extents with rows in key order and the level's rank map attached, so ``SubMConv2d`` /
    ``SparseConv2d`` carry on in key order; the rows of a cell are reduced in ascending input row, without atomics:
    results are identical run to run.

    Static shapes (an input with ``n_live_dev``: inside StaticInference / StaticTrainingStep) take the sync-free
    build; ``static_num_out`` bounds its rows (None: the input's rows, which always suffices).  The counters of the last
    call {cells found, 0, live rows} stay on the device in ``_static_n_out_dev``; a module with an explicit bound is
    part of the runners' ``overflowed()``."""

    def __init__(self, axes: Sequence[int], reduce: str = "sum", static_num_out: Optional[int] = None,
                 name: Optional[str] = None):
        super().__init__(name=name)
        self.axes = tuple(int(a) for a in axes)
        if len(set(self.axes)) != len(self.axes) or any(a < 0 for a in self.axes):
            raise ValueError(f"SparseCollapse: axes {self.axes} must be distinct and >= 0")
        if reduce not in ("sum", "mean", "max"):
            raise ValueError(f"SparseCollapse: reduce must be 'sum', 'mean' or 'max', got {reduce!r}")
        self.reduce = reduce
        self.static_num_out = None if static_num_out is None else int(static_num_out)
        self._static_n_out_dev = None

    def forward(self, x: SparseConvTensor) -> SparseConvTensor:
        from spconv_amd.pytorch import functional as F
        return F.sparse_collapse(x, self.axes, self.reduce, self.static_num_out, self)

    def extra_repr(self) -> str:
        return f"axes={self.axes}, reduce={self.reduce!r}, static_num_out={self.static_num_out}"


class SparsePrune(SparseModule):
    """Spatial voxel pruning (``functional.sparse_prune``): keeps the ``k`` live rows with the largest score, or
    ``int(ratio * live rows)`` of them -- exactly one of ``ratio`` and ``k`` is given -- on the kernels of
    csrc/select.hip.  ``score`` = "absmean" | "absmax" of the row's features.  Of equal scores the lowest rows stay:
    the selection is identical run to run.  The result is a fresh tensor over the same grid, rows in the input's
    order; when the input's rows are in key order (its index tensor carries the level's rank map) the result's rank map
    is attached, and the ``SubMConv`` layers behind build their rulebooks from it.  ``return_dropped=True`` returns
    ``(kept, dropped)``.

    Static shapes (an input with ``n_live_dev``: inside StaticInference / StaticTrainingStep) take the sync-free form;
    ``static_num_out`` bounds the kept rows (None: the bound that follows from ``ratio`` / ``k`` and the input's rows,
    which always suffices).  The counters of the last call {rows found, 0, live rows} stay on the device in
    ``_static_n_out_dev``; a module with an explicit bound is part of the runners' ``overflowed()``."""

    def __init__(self, ratio: Optional[float] = None, k: Optional[int] = None, score: str = "absmean",
                 return_dropped: bool = False, static_num_out: Optional[int] = None, name: Optional[str] = None):
        super().__init__(name=name)
        from spconv_amd.pytorch import _select
        _select.check_count(k, ratio, "SparsePrune")
        if score not in _select.OPS:
            raise ValueError(f"SparsePrune: score must be 'absmean' or 'absmax', got {score!r}")
        self.ratio = None if ratio is None else float(ratio)
        self.k = None if k is None else int(k)
        self.score = score
        self.return_dropped = bool(return_dropped)
        self.static_num_out = None if static_num_out is None else int(static_num_out)
        self._static_n_out_dev = None

    def forward(self, x: SparseConvTensor):
        from spconv_amd.pytorch import functional as F
        return F.sparse_prune(x, self.ratio, self.k, self.score, self.return_dropped, self.static_num_out, self)

    def extra_repr(self) -> str:
        return (f"ratio={self.ratio}, k={self.k}, score={self.score!r}, return_dropped={self.return_dropped}, "
                f"static_num_out={self.static_num_out}")


class TrilinearDevoxelize(torch.nn.Module):
    """Per-point features out of a sparse level by trilinear interpolation (``functional.point_corners`` +
    ``functional.voxels_to_points_trilinear``, the kernels of csrc/interp.hip): every point blends the rows of the
    2^ndim voxels whose centres surround it -- the devoxelize of SPVCNN / PVCNN.  Not part of the reference.

    ``vsize_xyz`` / ``coors_range_xyz`` as the voxelisers take them; the voxel size is that of the level being read (a
    level behind strided layers: the voxeliser's size times the stride).  ``normalize=True`` divides a point's weights
    by the sum of those whose voxel exists.  ``forward(x, points, batch_ids, n_points=None) -> [N, C]``: points fp32
    [N, >= ndim], batch_ids int32 [N] or None, n_points a device int32 or None.  A point outside the range or without
    any voxel around it gets zeros.  Key-ordered levels (an index tensor that carries its rank map) are looked up
    without a hash table.  The gradient goes to x's features only, added in a fixed order without atomics; there is
    no gradient with respect to the points."""

    def __init__(self, vsize_xyz: Sequence[float], coors_range_xyz: Sequence[float], normalize: bool = True):
        super().__init__()
        from spconv_amd.pytorch import _level
        _level._geometry(vsize_xyz, coors_range_xyz)
        self.vsize_xyz = [float(v) for v in vsize_xyz]
        self.coors_range_xyz = [float(v) for v in coors_range_xyz]
        self.normalize = bool(normalize)

    def forward(self, x: SparseConvTensor, points: torch.Tensor, batch_ids: Optional[torch.Tensor] = None,
                n_points: Optional[torch.Tensor] = None) -> torch.Tensor:
        from spconv_amd.pytorch import functional as F
        corners = F.point_corners(points, batch_ids, x, self.vsize_xyz, self.coors_range_xyz, self.normalize, n_points)
        return F.voxels_to_points_trilinear(x.features, corners)

    def extra_repr(self) -> str:
        return f"vsize_xyz={self.vsize_xyz}, coors_range_xyz={self.coors_range_xyz}, normalize={self.normalize}"


class VoxelQueryAndGroup(torch.nn.Module):
    """The voxels of a sparse level around query points, gathered for a shared MLP (``functional.voxel_query`` +
    ``functional.group_voxels``, the kernels of csrc/query.hip): the ``voxel_query_wrapper`` / ``grouping_operation``
    pair of Voxel R-CNN's Voxel RoI pooling and of the PV-RCNN family's voxel set abstraction.  Not part of the
    reference.

    ``query_range``: ndim ints in index-column (zyx) order, each in 0 .. 15: the window of cells around a query's own
    cell; ``nsample`` in 1 .. 128: the first so many voxels of the window, in ascending linear key, are kept;
    ``radius``: None, or the distance below which a voxel centre must lie; ``vsize_xyz`` / ``coors_range_xyz`` as the
    voxelisers take them, the voxel size being that of the level being read (a level behind strided layers: the
    voxeliser's size times the stride).  ``forward(x, queries, batch_ids) -> ([M, nsample, C (+ ndim)], count [M])``:
    queries fp32 [M, >= ndim], batch_ids int32 [M] or None.  With ``use_xyz`` the offsets from the query to the voxel
    centres, cast to the feature dtype, come in front of the C feature columns.  Empty slots repeat slot 0
    (pad="first"), so the caller's MLP and a plain ``max(1)`` follow in torch; a query without any voxel gets zeros and
    count 0.  Key-ordered levels (an index tensor that carries its rank map) are looked up without a hash table.  The
    gradient goes to x's features only, added in a fixed order without atomics; there is no gradient with respect to
    the queries."""

    def __init__(self, query_range: Sequence[int], nsample: int, radius: Optional[float] = None, use_xyz: bool = True, *,
                 vsize_xyz: Sequence[float], coors_range_xyz: Sequence[float]):
        super().__init__()
        from spconv_amd.pytorch import _level, _query
        ndim, _, _ = _level._geometry(vsize_xyz, coors_range_xyz, "VoxelQueryAndGroup")
        self.query_range = _query._check_window(query_range, nsample, ndim, "first")
        _query.squared_radius(radius)
        self.nsample = int(nsample)
        self.radius = None if radius is None else float(radius)
        self.use_xyz = bool(use_xyz)
        self.vsize_xyz = [float(v) for v in vsize_xyz]
        self.coors_range_xyz = [float(v) for v in coors_range_xyz]

    def forward(self, x: SparseConvTensor, queries: torch.Tensor, batch_ids: Optional[torch.Tensor] = None):
        from spconv_amd.pytorch import functional as F
        nb = F.voxel_query(queries, batch_ids, x, self.vsize_xyz, self.coors_range_xyz, self.query_range, self.nsample,
                           self.radius, "first", self.use_xyz)
        return _group(x.features, nb, self.use_xyz)

    def extra_repr(self) -> str:
        return (f"query_range={self.query_range}, nsample={self.nsample}, radius={self.radius}, use_xyz={self.use_xyz}, "
                f"vsize_xyz={self.vsize_xyz}, coors_range_xyz={self.coors_range_xyz}")


class FarthestPointSample(torch.nn.Module):
    """Keypoints of a raw cloud by farthest-point sampling (``functional.farthest_point_sample``, the kernel of
    csrc/sample.hip): the ``furthest_point_sample`` of ``pointnet2_stack``.  Not part of the reference.

    ``num_samples`` in 1 .. 65 536: samples per scene, the same for every scene.  ``forward(points, batch_ids,
    batch_size, n_points=None, groups=None) -> PointSamples(idx [B, K], count [B], batch_ids [B * K])``: points fp32
    [N, >= ndim], batch_ids int32 [N] or None.  Ties go to the lowest point index, the indices of a scene are distinct,
    slots beyond a scene's valid points hold -1.  ``functional.gather_samples(points, samples)`` gives the sampled rows
    (NaN in dead slots).  No gradient with respect to coordinates."""

    def __init__(self, num_samples: int, ndim: int = 3):
        super().__init__()
        from spconv_amd.pytorch import _sample
        if not 1 <= int(num_samples) <= _sample.MAX_SAMPLES:
            raise ValueError(f"FarthestPointSample: num_samples must be in 1 .. {_sample.MAX_SAMPLES}, got {num_samples}")
        if ndim not in (2, 3):
            raise ValueError(f"FarthestPointSample: ndim must be 2 or 3, got {ndim}")
        self.num_samples, self.ndim = int(num_samples), int(ndim)

    def forward(self, points: torch.Tensor, batch_ids: Optional[torch.Tensor], batch_size: int,
                n_points: Optional[torch.Tensor] = None, groups=None):
        from spconv_amd.pytorch import functional as F
        return F.farthest_point_sample(points, batch_ids, batch_size, self.num_samples, ndim=self.ndim, n_points=n_points,
                                       groups=groups)

    def extra_repr(self) -> str:
        return f"num_samples={self.num_samples}, ndim={self.ndim}"


class SectorFPS(torch.nn.Module):
    """Keypoints of a raw cloud by sectorised (and, with RoIs, proposal-centric) farthest-point sampling
    (``functional.sector_fps``, the kernels of csrc/sample.hip): PV-RCNN++'s ``sectorized_proposal_centric_sampling``.
    Not part of the reference.

    ``num_samples`` in 1 .. 65 536: K per scene, shared among ``num_sectors`` (1 .. 64) azimuth sectors about ``center``
    in proportion to their points; ``roi_radius`` (None: no filter) keeps the points within the nearest RoI's half
    diagonal plus that radius.  ``forward(points, batch_ids, batch_size, rois=None, roi_batch_ids=None, n_points=None,
    n_rois=None) -> PointSamples(idx [B, K + S - 1], count [B], batch_ids [B * (K + S - 1)])``, packed sector by sector;
    `rois` are required exactly when ``roi_radius`` is set.  One workgroup per sector.  No gradient with respect to
    coordinates."""

    def __init__(self, num_samples: int, num_sectors: int = 6, roi_radius: Optional[float] = None, center=(0., 0.)):
        super().__init__()
        from spconv_amd.pytorch import _sample
        self.center = _sample._check_sectors("SectorFPS", num_sectors, center)
        _sample._check_sector_fps("SectorFPS", 1, num_samples, num_sectors)
        if roi_radius is not None and not 0. <= float(roi_radius) < float("inf"):
            raise ValueError(f"SectorFPS: roi_radius must be finite and >= 0, got {roi_radius!r}")
        self.num_samples, self.num_sectors = int(num_samples), int(num_sectors)
        self.roi_radius = None if roi_radius is None else float(roi_radius)

    def forward(self, points: torch.Tensor, batch_ids: Optional[torch.Tensor], batch_size: int,
                rois: Optional[torch.Tensor] = None, roi_batch_ids: Optional[torch.Tensor] = None,
                n_points: Optional[torch.Tensor] = None, n_rois: Optional[torch.Tensor] = None):
        from spconv_amd.pytorch import functional as F
        return F.sector_fps(points, batch_ids, batch_size, self.num_samples, self.num_sectors, center=self.center,
                            rois=rois, roi_batch_ids=roi_batch_ids, roi_radius=self.roi_radius, n_points=n_points,
                            n_rois=n_rois)

    def extra_repr(self) -> str:
        return (f"num_samples={self.num_samples}, num_sectors={self.num_sectors}, roi_radius={self.roi_radius}, "
                f"center={self.center}")


class BallQueryAndGroup(torch.nn.Module):
    """The raw points around query points, gathered for a shared MLP (``functional.ball_query`` +
    ``functional.group_voxels``, the kernels of csrc/sample.hip and csrc/query.hip): the ``ball_query`` /
    ``grouping_operation`` pair of ``pointnet2_stack``'s set abstraction over the raw-point source.  Not part of the
    reference.

    ``radius`` >= 0; ``nsample`` in 1 .. 128: the first so many points of the query's scene inside the radius, in
    ascending point index, are kept.  ``forward(points, p_batch_ids, feats, queries, q_batch_ids, batch_size) -> ([M,
    nsample, (ndim +) C], count [M])``: points fp32 [N, >= ndim], feats [N, C], queries fp32 [M, >= ndim], batch ids
    int32 or None.  With ``use_xyz`` the offsets from the query to the points, cast to the feature dtype, come in front of
    the C feature columns.  Empty slots repeat slot 0 (pad="first"), so the caller's MLP and a plain ``max(1)`` follow
    in torch; a query without any point gets zeros and count 0.  The gradient goes to feats only, added in a fixed order
    without atomics; there is no gradient with respect to coordinates."""

    def __init__(self, radius: float, nsample: int, use_xyz: bool = True, ndim: int = 3):
        super().__init__()
        from spconv_amd.pytorch import _query, _sample
        if radius is None:
            raise ValueError("BallQueryAndGroup: radius must be >= 0, got None")
        _query.squared_radius(radius)
        self.nsample = _sample._check_ball(nsample, "first")
        if ndim not in (2, 3):
            raise ValueError(f"BallQueryAndGroup: ndim must be 2 or 3, got {ndim}")
        self.radius, self.use_xyz, self.ndim = float(radius), bool(use_xyz), int(ndim)

    def forward(self, points: torch.Tensor, p_batch_ids: Optional[torch.Tensor], feats: torch.Tensor, queries: torch.Tensor,
                q_batch_ids: Optional[torch.Tensor], batch_size: int, n_queries: Optional[torch.Tensor] = None,
                n_points: Optional[torch.Tensor] = None, groups=None):
        from spconv_amd.pytorch import functional as F
        nb = F.ball_query(queries, q_batch_ids, points, p_batch_ids, batch_size, self.radius, self.nsample, ndim=self.ndim,
                          pad="first", with_offsets=self.use_xyz, n_queries=n_queries, n_points=n_points,
                          with_groups=bool(feats.requires_grad and torch.is_grad_enabled()), groups=groups)
        return _group(feats, nb, self.use_xyz)

    def extra_repr(self) -> str:
        return f"radius={self.radius}, nsample={self.nsample}, use_xyz={self.use_xyz}, ndim={self.ndim}"


class KNNInterpolate(torch.nn.Module):
    """Features carried from few known points to many unknown ones by inverse-distance interpolation over the k nearest
    (``functional.knn_query`` + ``functional.knn_interpolate``, the kernels of csrc/knn.hip and csrc/interp.hip): the
    ``three_nn`` / ``three_interpolate`` pair of pointnet2's feature propagation at k = 3.  Not part of the reference.

    ``k`` in 1 .. 8 (the blend takes a table of 4 entries for k <= 4 and of 8 otherwise); ``eps`` >= 0: ``w = 1 /
    (sqrt(d2) + eps)``, normalised over the kept neighbours.  ``forward(known_points, known_batch_ids, known_feats,
    unknown_points, unknown_batch_ids, batch_size) -> [M, C]``: known_points fp32 [N, >= ndim], known_feats [N, C],
    unknown_points fp32 [M, >= ndim], batch ids int32 or None.  Equal distances go to the lower point index; an unknown
    point whose scene holds no valid known point gets zeros.  The gradient goes to known_feats only, added in a fixed
    order without atomics; there is no gradient with respect to coordinates or weights."""

    def __init__(self, k: int = 3, eps: float = 1e-8, ndim: int = 3):
        super().__init__()
        from spconv_amd.pytorch import _knn
        if not 1 <= int(k) <= 8:
            raise ValueError(f"KNNInterpolate: k must be in 1 .. 8 (the blend is at most 8 wide), got {k}")
        _knn._check_knn("KNNInterpolate", k, None, "none", eps)
        if ndim not in (2, 3):
            raise ValueError(f"KNNInterpolate: ndim must be 2 or 3, got {ndim}")
        self.k, self.eps, self.ndim = int(k), float(eps), int(ndim)
        self.width = 4 if self.k <= 4 else 8

    def forward(self, known_points: torch.Tensor, known_batch_ids: Optional[torch.Tensor], known_feats: torch.Tensor,
                unknown_points: torch.Tensor, unknown_batch_ids: Optional[torch.Tensor], batch_size: int,
                n_unknown: Optional[torch.Tensor] = None, n_known: Optional[torch.Tensor] = None, groups=None):
        from spconv_amd.pytorch import functional as F
        knn = F.knn_query(unknown_points, unknown_batch_ids, known_points, known_batch_ids, batch_size, self.k,
                          ndim=self.ndim, width=self.width, with_dist2=False, with_weights=True, eps=self.eps,
                          n_queries=n_unknown, n_points=n_known,
                          with_groups=bool(known_feats.requires_grad and torch.is_grad_enabled()), groups=groups)
        return F.knn_interpolate(known_feats, knn)

    def extra_repr(self) -> str:
        return f"k={self.k}, eps={self.eps}, ndim={self.ndim}"


class KNNQueryAndGroup(torch.nn.Module):
    """The k nearest raw points of every query, gathered for a shared MLP (``functional.knn_query`` +
    ``functional.group_voxels``, the kernels of csrc/knn.hip and csrc/query.hip): the ``knn_query`` / ``grouping`` pair
    of pointops.  Not part of the reference.

    ``k`` in 1 .. 64: the points of the query's scene that come first under (squared distance, point index).
    ``forward(points, p_batch_ids, feats, queries, q_batch_ids, batch_size) -> ([M, k, (ndim +) C], count [M])``:
    points fp32 [N, >= ndim], feats [N, C], queries fp32 [M, >= ndim], batch ids int32 or None.  With ``use_xyz`` the
    offsets from the query to the points, cast to the feature dtype, come in front of the C feature columns.  Slots
    beyond a scene's valid points repeat slot 0 (pad="first"), mirroring ``BallQueryAndGroup``; a query without any
    point gets zeros and count 0.  The gradient goes to feats only, added in a fixed order without atomics; there is
    no gradient with respect to coordinates."""

    def __init__(self, k: int, use_xyz: bool = True, ndim: int = 3):
        super().__init__()
        from spconv_amd.pytorch import _knn
        self.k, _ = _knn._check_knn("KNNQueryAndGroup", k, None, "first", 0.0)
        if ndim not in (2, 3):
            raise ValueError(f"KNNQueryAndGroup: ndim must be 2 or 3, got {ndim}")
        self.use_xyz, self.ndim = bool(use_xyz), int(ndim)

    def forward(self, points: torch.Tensor, p_batch_ids: Optional[torch.Tensor], feats: torch.Tensor, queries: torch.Tensor,
                q_batch_ids: Optional[torch.Tensor], batch_size: int, n_queries: Optional[torch.Tensor] = None,
                n_points: Optional[torch.Tensor] = None, groups=None):
        from spconv_amd.pytorch import functional as F
        knn = F.knn_query(queries, q_batch_ids, points, p_batch_ids, batch_size, self.k, ndim=self.ndim, pad="first",
                          with_dist2=False, with_offsets=self.use_xyz, n_queries=n_queries, n_points=n_points,
                          with_groups=bool(feats.requires_grad and torch.is_grad_enabled()), groups=groups)
        return _group(feats, knn.neighbors(), self.use_xyz)

    def extra_repr(self) -> str:
        return f"k={self.k}, use_xyz={self.use_xyz}, ndim={self.ndim}"


class RotatedNMS(torch.nn.Module):
    """Rotated non-maximum suppression per scene, wholly on the device (``functional.nms_rotated``, the kernels of
    csrc/box.hip): the ``nms_gpu`` every OpenPCDet / mmdet3d head ends in.  Not part of the reference.

    ``thresh``: a box is dropped when a kept, higher-scored box of its scene (with ``class_ids``: and class) overlaps it
    with a bird's-eye IoU above it; ``pre_max`` (1 .. 16384) candidates per scene take part, ``post_max`` (1 ..
    pre_max) are kept at most; ``score_thresh``: only scores above it are candidates.
    ``forward(boxes, scores, batch_ids=None, batch_size=1, class_ids=None, n_boxes=None) -> BoxNMS(keep [batch_size,
    post_max], count [batch_size])``: boxes fp32 [N, >= 7] = (x, y, z, dx, dy, dz, heading) or a ``BoxCorners``, scores
    fp32 [N], ids int32 [N] or None.  Nothing is read back, so the module can sit inside a captured graph once its
    buffers are owned by the caller (``functional.nms_rotated_into``).  There is no gradient."""

    def __init__(self, thresh: float, pre_max: int = 4096, post_max: int = 512, score_thresh: Optional[float] = None):
        super().__init__()
        from spconv_amd.pytorch import _box
        _box._check_nms("RotatedNMS", thresh, pre_max, post_max, score_thresh, 1)
        self.thresh, self.pre_max, self.post_max = float(thresh), int(pre_max), int(post_max)
        self.score_thresh = None if score_thresh is None else float(score_thresh)

    def forward(self, boxes, scores: torch.Tensor, batch_ids: Optional[torch.Tensor] = None, batch_size: int = 1,
                class_ids: Optional[torch.Tensor] = None, n_boxes: Optional[torch.Tensor] = None):
        from spconv_amd.pytorch import functional as F
        return F.nms_rotated(boxes, scores, self.thresh, batch_ids=batch_ids, batch_size=batch_size, class_ids=class_ids,
                             pre_max=self.pre_max, post_max=self.post_max, score_thresh=self.score_thresh,
                             n_boxes=n_boxes)

    def extra_repr(self) -> str:
        return (f"thresh={self.thresh}, pre_max={self.pre_max}, post_max={self.post_max}, "
                f"score_thresh={self.score_thresh}")


class RotatedIoU3DLoss(torch.nn.Module):
    """``1 - IoU`` of aligned (prediction, target) boxes, rotated, with a gradient (``functional.boxes_iou3d_diff`` /
    ``boxes_iou_bev_diff``: the kernels of csrc/boxgrad.hip): mmdet3d's ``RotatedIoU3DLoss`` over mmcv's
    ``diff_iou_rotated_3d``, the regression loss of FCAF3D / TR3D-style heads.  Not part of the reference.

    ``mode``: "iou", or "diou" (minus the squared centre distance over the squared diagonal of the enclosing
    axis-aligned box: pairs that do not overlap still move); ``plane``: the bird's-eye IoU instead of the IoU in
    space; ``reduction``: "none", "mean" or "sum"; ``loss_weight`` scales the result.
    ``forward(pred, target, weight=None, avg_factor=None)``: pred / target fp32 [N, >= 7] = (x, y, z, dx, dy, dz,
    heading) or ``BoxCorners``; weight: None or [N], multiplied in before the reduction; avg_factor: with "mean" the
    sum is divided by ``avg_factor + eps`` (eps of float32) instead of N, with "none" it is ignored, with "sum" it is
    refused -- mmdet's ``weight_reduce_loss``.  The reduction is plain torch.  A pair with an invalid box has loss 1
    and no gradient."""

    def __init__(self, mode: str = "iou", plane: bool = False, reduction: str = "mean", loss_weight: float = 1.0):
        super().__init__()
        if mode not in ("iou", "diou"):
            raise ValueError(f"RotatedIoU3DLoss: mode must be 'iou' or 'diou', got {mode!r}")
        if reduction not in ("none", "mean", "sum"):
            raise ValueError(f"RotatedIoU3DLoss: reduction must be 'none', 'mean' or 'sum', got {reduction!r}")
        self.mode, self.plane, self.reduction, self.loss_weight = mode, bool(plane), reduction, float(loss_weight)

    def forward(self, pred, target, weight: Optional[torch.Tensor] = None, avg_factor=None):
        from spconv_amd.pytorch import functional as F
        if avg_factor is not None and self.reduction == "sum":
            raise ValueError("RotatedIoU3DLoss: avg_factor can not be used with reduction='sum'")
        iou = (F.boxes_iou_bev_diff if self.plane else F.boxes_iou3d_diff)(
            pred, target, penalty="diou" if self.mode == "diou" else "none")
        if weight is not None and tuple(weight.shape) != tuple(iou.shape):
            raise ValueError(f"RotatedIoU3DLoss: weight is None or {list(iou.shape)}, got {list(weight.shape)}")
        loss = 1.0 - iou
        if weight is not None:
            loss = loss * weight
        if self.reduction == "sum":
            loss = loss.sum()
        elif self.reduction == "mean":
            loss = loss.mean() if avg_factor is None else loss.sum() / (avg_factor + torch.finfo(torch.float32).eps)
        return self.loss_weight * loss

    def extra_repr(self) -> str:
        return f"mode={self.mode}, plane={self.plane}, reduction={self.reduction}, loss_weight={self.loss_weight}"


class RoIPointPool3d(torch.nn.Module):
    """The points of every RoI with their features, a fixed number per box (``functional.roi_point_pool``: the kernels
    of csrc/roi.hip and csrc/query.hip): the ``roipoint_pool3d`` of PointRCNN's second stage.  Not part of the
    reference.

    ``num_sampled_points`` (1 .. 16384) slots per box; ``pool_extra_width`` (a float or a 3-tuple, >= 0) enlarges every
    box per side.  ``forward(points, p_batch_ids, feats, boxes, b_batch_ids, batch_size) -> (pooled [M, S, 3 + C],
    empty int32 [M])``: points fp32 [N, >= 3], feats [N, C], boxes fp32 [M, >= 7] = (x, y, z, dx, dy, dz, heading),
    batch ids int32 or None.  The first S points inside a box in ascending point index, repeated cyclically when there
    are fewer; a box without a point is zeros with empty = 1.  The gradient goes to feats only, added in a fixed order
    without atomics; there is no gradient with respect to coordinates or boxes."""

    def __init__(self, num_sampled_points: int = 512, pool_extra_width=0.):
        super().__init__()
        from spconv_amd.pytorch import _roi
        self.num_sampled_points = _roi._check_nsample("RoIPointPool3d", num_sampled_points, 1)
        self.pool_extra_width = _roi._extra("RoIPointPool3d", pool_extra_width)

    def forward(self, points: torch.Tensor, p_batch_ids: Optional[torch.Tensor], feats: torch.Tensor, boxes: torch.Tensor,
                b_batch_ids: Optional[torch.Tensor], batch_size: int, n_points: Optional[torch.Tensor] = None,
                n_boxes: Optional[torch.Tensor] = None, groups=None):
        from spconv_amd.pytorch import functional as F
        return F.roi_point_pool(points, p_batch_ids, feats, boxes, b_batch_ids, batch_size, self.num_sampled_points,
                                self.pool_extra_width, n_points=n_points, n_boxes=n_boxes, groups=groups)

    def extra_repr(self) -> str:
        return f"num_sampled_points={self.num_sampled_points}, pool_extra_width={self.pool_extra_width}"


class RoIAwarePool3d(torch.nn.Module):
    """The features of the points of every RoI reduced per cell of a grid over the box (``functional.roi_aware_pool``:
    the kernels of csrc/roi.hip, csrc/query.hip, csrc/pointvoxel.hip and csrc/collapse.hip): the ``roiaware_pool3d``
    of Part-A2's second stage.  Not part of the reference.

    ``out_size`` (an int or three ints in 1 .. 64) cells per box; ``max_pts_per_box`` (1 .. 16384): the first so many
    points of a box in ascending point index take part (OpenPCDet caps 128 per cell instead); ``reduce``: "max" or
    "mean".  ``forward(points, p_batch_ids, feats, boxes, b_batch_ids, batch_size) -> [M, ox, oy, oz, C]``, zeros in an
    empty cell.  The gradient goes to feats only, in a fixed order without atomics (a max tie: to every point that
    attains it); there is no gradient with respect to coordinates or boxes."""

    def __init__(self, out_size, max_pts_per_box: int = 2048, reduce: str = "max"):
        super().__init__()
        from spconv_amd.pytorch import _roi
        if out_size is None:
            raise ValueError("RoIAwarePool3d: the grid is an int or three ints in 1 .. 64, got None")
        self.out_size = _roi._check_grid("RoIAwarePool3d", out_size, 1)
        self.max_pts_per_box = _roi._check_nsample("RoIAwarePool3d", max_pts_per_box, 1)
        if reduce not in ("max", "mean"):
            raise ValueError(f"RoIAwarePool3d: reduce must be 'max' or 'mean', got {reduce!r}")
        self.reduce = reduce

    def forward(self, points: torch.Tensor, p_batch_ids: Optional[torch.Tensor], feats: torch.Tensor, boxes: torch.Tensor,
                b_batch_ids: Optional[torch.Tensor], batch_size: int, n_points: Optional[torch.Tensor] = None,
                n_boxes: Optional[torch.Tensor] = None, groups=None):
        from spconv_amd.pytorch import functional as F
        return F.roi_aware_pool(points, p_batch_ids, feats, boxes, b_batch_ids, batch_size, self.out_size,
                                self.max_pts_per_box, self.reduce, n_points=n_points, n_boxes=n_boxes, groups=groups)

    def extra_repr(self) -> str:
        return f"out_size={self.out_size}, max_pts_per_box={self.max_pts_per_box}, reduce={self.reduce}"


class CenterTargets(NamedTuple):
    """What ``CenterHeadTargets`` returns: heatmap fp32 [B, C, H, W] (dense) or [N, C] (over the rows of a sparse
    level), target_boxes fp32 [B, max_objs, 8 + extra], inds int32 [B, max_objs] (``iy * W + ix``; over a sparse level
    the GLOBAL row index of the nearest row), mask int32 [B, max_objs]."""
    heatmap: torch.Tensor
    target_boxes: torch.Tensor
    inds: torch.Tensor
    mask: torch.Tensor


class CenterHeadTargets(torch.nn.Module):
    """The training targets of one centre head (``functional.box_centers`` / ``center_heatmap`` /
    ``center_heatmap_sparse``, the kernels of csrc/center.hip): OpenPCDet's ``CenterHead.assign_target_of_single_head``
    and VoxelNeXt's sparse twin without their Python loop over the boxes.  Not part of the reference.

    ``grid_size``: (W, H) of the HEAD's map (OpenPCDet's ``grid_size[:2] // stride``); ``voxel_size`` (vx, vy[, vz]) and
    ``point_cloud_range`` (x0, y0, ...) as in the data config; ``stride``: the map's stride over the voxels;
    ``anchor`` / ``cutoff``: the sparse form's (``center_heatmap_sparse``).  ``forward(boxes, b_batch_ids, class_ids,
    batch_size, x=None, n_boxes=None) -> CenterTargets``: boxes fp32 [M, >= 7], class_ids 0-based planes (None: class 0);
    with `x` (a 2-D SparseConvTensor or indices [N, 3]) the heatmap is over its rows and inds are row indices.  A row of
    target_boxes is (offset x, offset y, z, log dx, log dy, log dz, cos heading, sin heading, any columns beyond the
    seventh as they are) of the box in that slot, the offset being the centre in cells minus the cell (over a sparse
    level: minus the cell of the nearest row), all multiplied by the mask: plain torch over ``box_index``.  For several
    heads call one module per head with the class ids of the other heads mapped to -1: those boxes keep their slots with
    mask 0.  Nothing is read back.  Targets have no gradient."""

    def __init__(self, num_classes: int, grid_size, voxel_size, point_cloud_range, stride, max_objs: int = 500,
                 min_overlap: float = 0.1, min_radius: int = 2, anchor: str = "center", cutoff: str = "none"):
        super().__init__()
        from spconv_amd.pytorch import _center
        op = "CenterHeadTargets"

        def first2(v):
            """the x and y entries of a tuple, list or array as the data config has it ((x, y, z), a 6-entry range)"""
            try:
                return tuple(v.tolist() if hasattr(v, "tolist") else v)[:2]
            except TypeError:
                return v                                  # (not a sequence: check_params says what it should be)

        _center.check_params(op, 1, first2(grid_size), first2(voxel_size), first2(point_cloud_range), stride, num_classes,
                             max_objs, min_overlap, min_radius)
        if anchor not in ("center", "nearest"):
            raise ValueError(f"{op}: anchor is 'center' or 'nearest', got {anchor!r}")
        if cutoff not in ("none", "window"):
            raise ValueError(f"{op}: cutoff is 'none' or 'window', got {cutoff!r}")
        self.num_classes, self.max_objs, self.min_radius = int(num_classes), int(max_objs), int(min_radius)
        self.grid_size = tuple(int(v) for v in first2(grid_size))
        self.voxel_size = tuple(float(v) for v in first2(voxel_size))
        self.range_min = tuple(float(v) for v in first2(point_cloud_range))
        self.stride, self.min_overlap = float(stride), float(min_overlap)
        self.anchor, self.cutoff = anchor, cutoff

    def forward(self, boxes: torch.Tensor, b_batch_ids: Optional[torch.Tensor], class_ids: Optional[torch.Tensor],
                batch_size: int, x=None, n_boxes: Optional[torch.Tensor] = None) -> CenterTargets:
        from spconv_amd.pytorch import _center
        from spconv_amd.pytorch import functional as F
        centers = F.box_centers(boxes, b_batch_ids, class_ids, batch_size, grid_size=self.grid_size,
                                voxel_size=self.voxel_size, range_min=self.range_min, stride=self.stride,
                                num_classes=self.num_classes, max_objs=self.max_objs, min_overlap=self.min_overlap,
                                min_radius=self.min_radius, n_boxes=n_boxes)
        with torch.no_grad():
            cell = centers.cell
            if x is None:
                heat, inds, mask = F.center_heatmap(centers), centers.inds, centers.mask
            else:
                sc = F.center_heatmap_sparse(centers, x, anchor=self.anchor, cutoff=self.cutoff)
                heat, inds, mask = sc.heat, sc.inds, sc.mask
                indices, _ = _center._level("CenterHeadTargets", x)     # (a Tensor has an `indices` method of its own)
                if int(indices.shape[0]) > 0:       # the cell (x, y) of every box's nearest row; unused where there is none
                    cell = indices[sc.nearest.clamp(min=0).long()][:, [2, 1]]
            M = int(boxes.shape[0])
            width = 8 + int(boxes.shape[1]) - 7
            if M == 0:
                target = boxes.new_zeros((int(batch_size), self.max_objs, width))
            else:
                b = boxes.detach()
                rows = torch.cat([centers.center - cell.to(torch.float32), b[:, 2:3], b[:, 3:6].log(), b[:, 6:7].cos(),
                                  b[:, 6:7].sin(), b[:, 7:]], dim=1)
                target = rows[centers.box_index.clamp(min=0).long()]
                target = torch.where((mask != 0).unsqueeze(-1), target, torch.zeros_like(target))
        return CenterTargets(heat, target, inds, mask)

    def extra_repr(self) -> str:
        return (f"num_classes={self.num_classes}, grid_size={self.grid_size}, voxel_size={self.voxel_size}, "
                f"range_min={self.range_min}, stride={self.stride}, max_objs={self.max_objs}, "
                f"min_overlap={self.min_overlap}, min_radius={self.min_radius}, anchor={self.anchor}, cutoff={self.cutoff}")
