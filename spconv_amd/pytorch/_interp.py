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

from typing import NamedTuple, Optional, Sequence

import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from spconv_amd import _lib
from spconv_amd.pytorch._level import _floats, _geometry, check_points, flat_groups, grad_rows, groups_missing
from spconv_amd.pytorch._level import flat_groups as corner_groups  # noqa: F401  (the name tests and tools reach)
from spconv_amd.pytorch._pointvoxel import PointGroups
from spconv_amd.pytorch._rulebook import _float_code, _ptr, _require_gpu, _stream, _ws


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
    ndim, vsize, coors_range = _geometry(vsize_xyz, coors_range_xyz)
    K = 1 << ndim
    indices, spatial_shape, B, n_live, rankmap, with_groups = check_points("point_corners", "points", points, batch_ids,
                                                                           n_points, x, ndim, K, with_groups)
    N, n, dev = int(points.shape[0]), int(indices.shape[0]), points.device
    with torch.cuda.device(dev), torch.no_grad():
        points = points.detach().contiguous()
        batch_ids = None if batch_ids is None else batch_ids.contiguous()
        rows = torch.empty((N, K), dtype=torch.int32, device=dev)
        weights = torch.empty((N, K), dtype=torch.float32, device=dev)
        if N > 0:
            ws = None if rankmap is not None else _ws(corners_ws_bytes(N, ndim, n), dev)
            point_corners_into(points, batch_ids, n_points, _floats(vsize), _floats(coors_range), indices, n_live, B,
                               spatial_shape, rankmap, normalize, rows, weights, ws)
        groups = flat_groups(rows, n, n_live) if with_groups else None
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
    dt, dout, dvfeat, g = grad_rows("voxels_to_points_trilinear", dout, corners, "corner", "point_corners")
    if g is not None:
        N, K = corners.rows.shape
        _lib.check(_lib.load().spx_interp_bwd(dout.data_ptr(), N, K.bit_length() - 1, corners.weights.data_ptr(),
                                              g.offsets.data_ptr(), g.list.data_ptr(), corners.num_voxels,
                                              _ptr(corners.n_live), int(dout.shape[1]), dt, dvfeat.data_ptr(),
                                              _stream(dout)))
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
            raise groups_missing("voxels_to_points_trilinear", "corner", "point_corners")
        return TrilinearFunction.apply(vfeat, corners)
