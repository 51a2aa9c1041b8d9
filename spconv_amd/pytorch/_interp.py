"""Trilinear devoxelisation on the HIP kernels of csrc/interp.hip: voxel rows of a sparse level interpolated to points
(``functional.point_corners`` / ``voxels_to_points_trilinear`` / ``spatial.TrilinearDevoxelize``).  Not part of the
reference; the point-voxel networks (SPVCNN / PVCNN, Cylinder3D's point refinement, the keypoint interpolation of the
PV-RCNN family) write it as K hash queries, ``index_select`` / ``mul`` / ``sum`` and an ``index_add_`` backward.

  * ``point_corners``              per point the K = 2^ndim voxels whose centres surround it, as rows of the level and
                                   weights (``spx_point_corners``): through the level's rank map when its index tensor
                                   carries one (key-ordered rows, one load per corner), through a hash table built from
                                   the rows otherwise; nothing read back
  * ``voxels_to_points_trilinear`` ``out[i] = sum_c w[i, c] * vfeat[rows[i, c]]`` (``spx_interp_fwd``); its gradient in
                                   ``vfeat`` is a segment sum over the transposed corner list (``spx_point_groups`` over
                                   the flattened corner table, ``spx_interp_bwd``): no atomics, identical run to run

There is no gradient with respect to the points or the weights: raw coordinates need none (torchsparse's devoxelize
gives none either).
"""
from __future__ import annotations

import ctypes
from typing import NamedTuple, Optional, Sequence

import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from spconv_amd import _lib
from spconv_amd.pytorch import _pointvoxel
from spconv_amd.pytorch._pointvoxel import PointGroups
from spconv_amd.pytorch._rulebook import _check_count, _float_code, _ptr, _rankmap_of, _require_gpu, _stream, _ws


class PointCorners(NamedTuple):
    """The corner table of a point cloud over one level: rows int32 [N, K] (row of the level, -1: none), weights fp32
    [N, K] (0 where the row is -1), groups (a ``PointGroups`` over the FLATTENED table -- entry e = i * K + c -- or None:
    only a gradient needs it), num_voxels (rows of the level), n_points / n_live (device int32 or None: points / voxel
    rows at or beyond them do not exist)."""
    rows: torch.Tensor
    weights: torch.Tensor
    groups: Optional[PointGroups]
    num_voxels: int
    n_points: Optional[torch.Tensor] = None
    n_live: Optional[torch.Tensor] = None


def _floats(values):
    return (ctypes.c_float * len(values))(*values)


def _geometry(vsize_xyz: Sequence[float], coors_range_xyz: Sequence[float], what: str = "point_corners"):
    from spconv_amd.pytorch.utils import calc_point2voxel_meta_data
    ndim = len(vsize_xyz)
    if ndim not in (2, 3):
        raise ValueError(f"{what}: ndim must be 2 or 3, got {ndim}")
    if len(coors_range_xyz) != 2 * ndim:
        raise ValueError(f"{what}: coors_range_xyz holds {2 * ndim} values for ndim = {ndim}")
    if not min(float(v) for v in vsize_xyz) > 0:
        raise ValueError(f"{what}: voxel sizes must be positive, got {list(vsize_xyz)}")
    vsize, _, _, coors_range = calc_point2voxel_meta_data(list(vsize_xyz), list(coors_range_xyz))
    return ndim, vsize, coors_range


def level_rankmap(indices: torch.Tensor, batch_size: int, spatial_shape) -> Optional[torch.Tensor]:
    """The rank map attached to exactly this index tensor, if it describes this level and the tensor has not been
    written since (``_rulebook._rankmap_of``'s validation).  That function also gates on a layer's kernel volume, which
    means nothing for a lookup: 27 is passed only because it is inside the gate."""
    return _rankmap_of(indices, int(batch_size), spatial_shape, int(indices.shape[0]), 27)


def corners_ws_bytes(n_cap: int, ndim: int, n: int) -> int:
    return int(_lib.load().spx_point_corners_ws_bytes(int(n_cap), int(ndim), int(n)))


def point_corners_into(points: torch.Tensor, batch_ids: Optional[torch.Tensor], n_points: Optional[torch.Tensor],
                       vsize_zyx, coors_range_zyx, indices: torch.Tensor, n_live: Optional[torch.Tensor], batch_size: int,
                       spatial_shape: Sequence[int], rankmap: Optional[torch.Tensor], normalize: bool, rows: torch.Tensor,
                       weights: torch.Tensor, ws: Optional[torch.Tensor]) -> None:
    """The one C call into buffers the caller owns (no allocation: capturable).  vsize_zyx / coors_range_zyx: ctypes
    float arrays in zyx order (``calc_point2voxel_meta_data``); rankmap: the level's rank map or None (hash form, which
    needs `ws` of ``corners_ws_bytes``)."""
    ndim = len(spatial_shape)
    _lib.check(_lib.load().spx_point_corners(
        points.data_ptr(), int(points.shape[1]), _ptr(batch_ids), int(points.shape[0]), _ptr(n_points), ndim, vsize_zyx,
        coors_range_zyx, indices.data_ptr(), int(indices.shape[0]), _ptr(n_live), int(batch_size),
        _lib.ints(spatial_shape), _ptr(rankmap), 0 if rankmap is None else rankmap.numel() * rankmap.element_size(),
        int(bool(normalize)), rows.data_ptr(), weights.data_ptr(), _ptr(ws), 0 if ws is None else ws.numel(),
        _stream(points)))


def corner_groups(rows: torch.Tensor, num_voxels: int, n_live: Optional[torch.Tensor] = None) -> Optional[PointGroups]:
    """The transposed corner list: ``spx_point_groups`` over the flattened table (None for an empty table or level)."""
    if rows.numel() == 0 or num_voxels < 1:
        return None
    return _pointvoxel.point_groups(rows.reshape(-1), num_voxels, None, n_live)


def point_corners(points: torch.Tensor, batch_ids: Optional[torch.Tensor], x, vsize_xyz: Sequence[float],
                  coors_range_xyz: Sequence[float], normalize: bool = True, n_points: Optional[torch.Tensor] = None,
                  with_groups: Optional[bool] = None) -> PointCorners:
    """The K = 2^ndim voxels of the level `x` (a SparseConvTensor) whose centres surround each point, and their
    multilinear weights.  points fp32 [N, >= ndim] (x, y, z first), batch_ids int32 [N] or None (all batch 0);
    vsize_xyz / coors_range_xyz as the voxelisers take them, the voxel size being that of x's level (a strided level:
    the stride times the voxeliser's).  A point outside the range, with a NaN coordinate, with a batch id outside
    [0, batch_size) or at or beyond *n_points gets rows -1 and weights 0; so does a corner outside the grid or one that no
    live row of x holds.  normalize=True divides the weights of a point by the sum of those present.  fp32 arithmetic,
    every operation rounded on its own.  x's rank map is used when its index tensor carries one (rows in key order),
    the hash table otherwise; a static tensor's n_live_dev is passed through.  with_groups (default: x's features
    require a gradient) builds the transposed list the gradient in the voxel rows walks.  No gradient with respect to
    the points: raw coordinates need none."""
    _require_gpu(points, "points")
    ndim, vsize, coors_range = _geometry(vsize_xyz, coors_range_xyz)
    indices, spatial_shape, B = x.indices, [int(v) for v in x.spatial_shape], int(x.batch_size)
    _require_gpu(indices, "indices")
    if len(spatial_shape) != ndim:
        raise ValueError(f"point_corners: the level has {len(spatial_shape)} spatial axes, vsize_xyz {ndim}")
    if points.dim() != 2 or points.dtype != torch.float32 or points.shape[1] < ndim:
        raise ValueError(f"point_corners: points is a float32 tensor [N, >= {ndim}], got {tuple(points.shape)} {points.dtype}")
    if indices.dtype != torch.int32 or indices.dim() != 2 or indices.shape[1] != ndim + 1:
        raise ValueError(f"point_corners: indices is an int32 tensor [n, {ndim + 1}]")
    N, n, K = int(points.shape[0]), int(indices.shape[0]), 1 << ndim
    if N * K >= 1 << 31:
        raise ValueError(f"point_corners: {N} points x {K} corners do not fit 32-bit entries")
    if batch_ids is not None:
        if batch_ids.shape != (N,) or batch_ids.dtype != torch.int32 or not batch_ids.is_cuda:
            raise ValueError("point_corners: batch_ids is a CUDA int32 tensor [N]")
        batch_ids = batch_ids.contiguous()
    _check_count(n_points, "point_corners: n_points")
    n_live = getattr(x, "n_live_dev", None)
    _check_count(n_live, "point_corners: n_live")
    if with_groups is None:
        with_groups = bool(x.features.requires_grad and torch.is_grad_enabled())
    dev = points.device
    with torch.cuda.device(dev), torch.no_grad():
        points = points.detach().contiguous()
        rankmap = level_rankmap(indices, B, spatial_shape)
        indices = indices.contiguous()
        rows = torch.empty((N, K), dtype=torch.int32, device=dev)
        weights = torch.empty((N, K), dtype=torch.float32, device=dev)
        if N > 0:
            ws = None if rankmap is not None else _ws(corners_ws_bytes(N, ndim, n), dev)
            point_corners_into(points, batch_ids, n_points, _floats(vsize), _floats(coors_range), indices, n_live, B,
                               spatial_shape, rankmap, normalize, rows, weights, ws)
        groups = corner_groups(rows, n, n_live) if with_groups else None
    return PointCorners(rows, weights, groups, n, n_points, n_live)


def interp_fwd(vfeat: torch.Tensor, corners: PointCorners) -> torch.Tensor:
    """out[i] = sum_c weights[i, c] * vfeat[rows[i, c]] (spx_interp_fwd: one launch)."""
    dt = _float_code(vfeat, "voxels_to_points_trilinear")
    vfeat = vfeat.contiguous()
    N, K = (int(v) for v in corners.rows.shape)
    n, C = int(vfeat.shape[0]), int(vfeat.shape[1])
    out = torch.empty((N, C), dtype=vfeat.dtype, device=vfeat.device)
    if N > 0 and C > 0:
        _lib.check(_lib.load().spx_interp_fwd(vfeat.data_ptr(), n, corners.rows.data_ptr(), corners.weights.data_ptr(), N,
                                              K.bit_length() - 1, C, dt, out.data_ptr(), _stream(vfeat)))
    return out


def interp_bwd(dout: torch.Tensor, corners: PointCorners) -> torch.Tensor:
    """dvfeat[v] = sum over the entries e of voxel v's group of weights_flat[e] * dout[e // K], in ascending e
    (spx_interp_bwd: one launch, no atomics); zeros for an empty group and for rows at or beyond *n_live."""
    dt = _float_code(dout, "voxels_to_points_trilinear")
    dout = dout.contiguous()
    N, K = (int(v) for v in corners.rows.shape)
    n, C = corners.num_voxels, int(dout.shape[1])
    g = corners.groups
    if n == 0 or C == 0 or N == 0:
        return torch.zeros((n, C), dtype=dout.dtype, device=dout.device)
    if g is None or g.offsets is None:
        raise ValueError("voxels_to_points_trilinear: a gradient needs the corner groups; call point_corners with "
                         "with_groups=True")
    dvfeat = torch.empty((n, C), dtype=dout.dtype, device=dout.device)
    _lib.check(_lib.load().spx_interp_bwd(dout.data_ptr(), N, K.bit_length() - 1, corners.weights.data_ptr(),
                                          g.offsets.data_ptr(), g.list.data_ptr(), n, _ptr(corners.n_live), C, dt,
                                          dvfeat.data_ptr(), _stream(dout)))
    return dvfeat


class TrilinearFunction(Function):
    """spx_interp_fwd / spx_interp_bwd.  The gradient is the one in the voxel rows; points and weights get none."""

    @staticmethod
    def forward(ctx, vfeat, corners):
        ctx.corners = corners
        return interp_fwd(vfeat.detach(), corners)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_output):
        return interp_bwd(grad_output, ctx.corners), None


def voxels_to_points_trilinear(vfeat: torch.Tensor, corners: PointCorners) -> torch.Tensor:
    """[num_voxels, C] voxel rows -> [N, C]: row i is the weighted sum of the rows of point i's corners, added in
    ascending corner index in fp32 (fp64 for float64) and rounded once; zeros for a point without a corner.
    Differentiable in vfeat (a segment sum over the transposed corner list, in ascending entry: identical run to run);
    there is no gradient with respect to the points or the weights."""
    _require_gpu(vfeat, "voxel features")
    _float_code(vfeat, "voxels_to_points_trilinear")
    if vfeat.dim() != 2 or vfeat.shape[0] != corners.num_voxels:
        raise ValueError(f"voxels_to_points_trilinear: one row per voxel ([{corners.num_voxels}, C]), got "
                         f"{tuple(vfeat.shape)}")
    with torch.cuda.device(vfeat.device):
        if not (vfeat.requires_grad and torch.is_grad_enabled()):
            return interp_fwd(vfeat, corners)
        if corners.groups is None and corners.rows.numel() > 0 and corners.num_voxels > 0:
            raise ValueError("voxels_to_points_trilinear: a gradient needs the corner groups; call point_corners with "
                             "with_groups=True")
        return TrilinearFunction.apply(vfeat, corners)
