"""A sparse level as something points look cells up in, the Python side of csrc/lookup.h: what the wrappers of
csrc/interp.hip (``_interp.py``) and csrc/query.hip (``_query.py``) share -- the geometry the voxelisers take and the
level's rank map, the checks of points against a level, the transposed list of a flattened [N, K] table of rows and
the prologue of the two segment-sum backwards that walk it."""
from __future__ import annotations

import ctypes
from typing import Optional, Sequence

import torch

from spconv_amd.pytorch import _pointvoxel
from spconv_amd.pytorch._pointvoxel import PointGroups
from spconv_amd.pytorch._rulebook import _check_count, _float_code, _rankmap_of, _require_gpu
from spconv_amd.pytorch.utils import calc_point2voxel_meta_data


def _floats(values):
    return (ctypes.c_float * len(values))(*values)


def _geometry(vsize_xyz: Sequence[float], coors_range_xyz: Sequence[float], what: str = "point_corners"):
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


def check_points(op: str, noun: str, points: torch.Tensor, batch_ids: Optional[torch.Tensor],
                 n_points: Optional[torch.Tensor], x, ndim: int, per_point: int, with_groups: Optional[bool]):
    """`points` (`noun`: what `op` calls them -- fp32 [N, >= ndim], x y z first), batch_ids (int32 [N] or None) and the
    device count n_points against the level `x` (a SparseConvTensor), `per_point` table entries each.  Every
    ValueError comes before the refusal of a CPU tensor.  Returns (indices -- contiguous --, spatial_shape, batch_size,
    n_live -- a static tensor's n_live_dev or None --, the rank map of x's index tensor or None, with_groups -- None
    resolved to "x's features require a gradient", asked here, outside the caller's no_grad block)."""
    indices, spatial_shape, B = x.indices, [int(v) for v in x.spatial_shape], int(x.batch_size)
    if len(spatial_shape) != ndim:
        raise ValueError(f"{op}: the level has {len(spatial_shape)} spatial axes, vsize_xyz {ndim} (ndim mismatch)")
    if points.dim() != 2 or points.dtype != torch.float32 or points.shape[1] < ndim:
        raise ValueError(f"{op}: {noun} is a float32 tensor [N, >= {ndim}], got {tuple(points.shape)} {points.dtype}")
    if indices.dtype != torch.int32 or indices.dim() != 2 or indices.shape[1] != ndim + 1:
        raise ValueError(f"{op}: indices is an int32 tensor [n, {ndim + 1}]")
    N = int(points.shape[0])
    if N * per_point >= 1 << 31:
        raise ValueError(f"{op}: {N} {noun} x {per_point} entries each do not fit 32-bit entries")
    if batch_ids is not None and (batch_ids.shape != (N,) or batch_ids.dtype != torch.int32):
        raise ValueError(f"{op}: batch_ids is a CUDA int32 tensor [N]")
    _require_gpu(points, noun)
    _require_gpu(indices, "indices")
    if batch_ids is not None:
        _require_gpu(batch_ids, "batch_ids")
    _check_count(n_points, f"{op}: n_{noun}")
    n_live = getattr(x, "n_live_dev", None)
    _check_count(n_live, f"{op}: n_live")
    rankmap = level_rankmap(indices, B, spatial_shape)          # (of exactly this tensor: before .contiguous())
    if with_groups is None:
        with_groups = bool(x.features.requires_grad and torch.is_grad_enabled())
    return indices.contiguous(), spatial_shape, B, n_live, rankmap, with_groups


def flat_groups(rows: torch.Tensor, num_voxels: int, n_live: Optional[torch.Tensor] = None) -> Optional[PointGroups]:
    """The transposed list of a table of rows [N, K]: ``spx_point_groups`` over the flattened table, entry e = i * K + c
    (None for an empty table or level)."""
    if rows.numel() == 0 or num_voxels < 1:
        return None
    return _pointvoxel.point_groups(rows.reshape(-1), num_voxels, None, n_live)


def groups_missing(op: str, what: str, maker: str) -> ValueError:
    return ValueError(f"{op}: a gradient needs the {what} groups; call {maker} with with_groups=True")


def grad_rows(op: str, dout: torch.Tensor, table, what: str, maker: str):
    """The prologue of a segment-sum backward over `table` (a PointCorners / VoxelNeighbors): (dtype code, dout
    contiguous, dvfeat [num_voxels, C], groups).  groups None: nothing to launch, dvfeat is the finished gradient
    (zeros: no rows, no channels or no entries)."""
    dt = _float_code(dout, op)
    dout = dout.contiguous()
    n, C = table.num_voxels, int(dout.shape[-1])
    if n == 0 or C == 0 or table.rows.shape[0] == 0:
        return dt, dout, torch.zeros((n, C), dtype=dout.dtype, device=dout.device), None
    g = table.groups
    if g is None or g.offsets is None:
        raise groups_missing(op, what, maker)
    return dt, dout, torch.empty((n, C), dtype=dout.dtype, device=dout.device), g
