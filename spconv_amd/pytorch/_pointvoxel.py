"""Point <-> voxel features on the HIP kernels of csrc/pointvoxel.hip and csrc/collapse.hip: what a learned voxel
feature encoder (``vfe.DynamicVFE``) runs between a voxeliser and the first sparse layer.  Not part of the reference,
whose users write these steps with ``torch_scatter``.

  * ``point_groups``      the points of every voxel as {rows, offsets, list} (``spx_point_groups``: one C call, nothing
                          read back), from the ``pc_voxel_id`` a voxeliser returns
  * ``points_to_voxels``  sum / mean / max of the point rows of every voxel over ALL its points, in ascending point
                          index, fp32 (fp64) accumulation, one rounding, no atomics (``spx_collapse_fwd`` / ``_bwd``)
  * ``voxels_to_points``  voxel rows back to their points (``spx_voxel_to_point``); its gradient is the segment sum over
                          the same groups -- identical run to run, where ``index_add_`` is not
  * ``decorate_points``   the input row of the per-point MLP (``spx_point_decorate``)
"""
from __future__ import annotations

import ctypes
from typing import NamedTuple, Optional, Sequence

import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from spconv_amd import _lib
from spconv_amd.pytorch import _collapse
from spconv_amd.pytorch._rulebook import _float_code, _ptr, _require_gpu, _stream, _ws

_OUT_DTYPES = {torch.float32: _lib.DTYPE_F32, torch.float16: _lib.DTYPE_F16, torch.bfloat16: _lib.DTYPE_BF16}
_BITS = {1: torch.int8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


class PointGroups(NamedTuple):
    """The points of every voxel: rows int32 [n] (voxel of each point, -1: none), offsets int32 [num_voxels + 1] and
    list int32 [n] (group v = list[offsets[v] : offsets[v + 1]], ascending point index), n_points (device int32 or None:
    rows at or beyond it are no points), n_live (device int32 or None: voxel rows at or beyond it are dead).  offsets and
    list are None for groups that only carry rows (a forward gather needs no more)."""
    rows: torch.Tensor
    offsets: Optional[torch.Tensor]
    list: Optional[torch.Tensor]
    num_voxels: int
    n_points: Optional[torch.Tensor] = None
    n_live: Optional[torch.Tensor] = None

    @property
    def n_out(self) -> int:             # (the name _collapse.fwd / bwd read)
        return self.num_voxels


def _check_ids(ids: torch.Tensor, num_voxels: int) -> int:
    if ids.dim() != 1 or ids.dtype not in (torch.int64, torch.int32):
        raise ValueError(f"point_groups: pc_voxel_id is a 1-d int64 or int32 tensor, got {tuple(ids.shape)} {ids.dtype}")
    if int(num_voxels) < 1:
        raise ValueError(f"point_groups: num_voxels must be >= 1, got {num_voxels}")
    return 8 if ids.dtype == torch.int64 else 4


def point_groups_into(ids: torch.Tensor, num_voxels: int, n_points: Optional[torch.Tensor], rows: torch.Tensor,
                      offsets: torch.Tensor, lst: torch.Tensor, ws: torch.Tensor) -> None:
    """The one C call into buffers the caller owns (no allocation: capturable)."""
    _lib.check(_lib.load().spx_point_groups(ids.data_ptr(), _check_ids(ids, num_voxels), int(ids.shape[0]), _ptr(n_points),
                                            int(num_voxels), rows.data_ptr(), offsets.data_ptr(), lst.data_ptr(),
                                            ws.data_ptr(), ws.numel(), _stream(ids)))


def point_groups(pc_voxel_id: torch.Tensor, num_voxels: int, n_points: Optional[torch.Tensor] = None,
                 n_live: Optional[torch.Tensor] = None) -> PointGroups:
    """Groups the points by voxel.  `pc_voxel_id` [N] int64 / int32 is what a voxeliser returns: the voxel row of every
    point, also of points past the per-voxel cap; an id outside [0, num_voxels) (-1: dropped) belongs to no voxel."""
    _require_gpu(pc_voxel_id, "pc_voxel_id")
    _check_ids(pc_voxel_id, num_voxels)
    ids = pc_voxel_id.contiguous()
    n, dev = int(ids.shape[0]), ids.device
    with torch.cuda.device(dev):
        i32 = dict(dtype=torch.int32, device=dev)
        rows, lst = torch.empty((n,), **i32), torch.empty((n,), **i32)
        offsets = torch.empty((int(num_voxels) + 1,), **i32)
        ws = _ws(_lib.load().spx_point_groups_ws_bytes(n, int(num_voxels)), dev)
        point_groups_into(ids, num_voxels, n_points, rows, offsets, lst, ws)
    return PointGroups(rows, offsets, lst, int(num_voxels), n_points, n_live)


def _check_rows(feat: torch.Tensor, groups: PointGroups, what: str) -> None:
    if feat.dim() != 2 or feat.shape[0] != groups.rows.shape[0]:
        raise ValueError(f"{what}: one feature row per point ([{groups.rows.shape[0]}, C]), got {tuple(feat.shape)}")


class PointsToVoxelsFunction(Function):
    """out[v] = sum / mean / max of feat[list[offsets[v] : offsets[v + 1]]] in list order (spx_collapse_fwd); the backward
    is one launch as well (a gather for sum, spx_collapse_bwd for mean and max)."""

    @staticmethod
    def forward(ctx, feat, groups, reduce):
        out = _collapse.fwd(feat.detach(), groups, reduce, groups.n_live)
        ctx.groups, ctx.reduce = groups, reduce
        if reduce == "max":
            ctx.save_for_backward(feat, out)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_output):
        feat, out = ctx.saved_tensors if ctx.reduce == "max" else (None, None)
        return _collapse.bwd(grad_output, ctx.groups, ctx.reduce, feat, out), None, None


def points_to_voxels(feat: torch.Tensor, groups: PointGroups, reduce: str = "max") -> torch.Tensor:
    """[N, C] point rows -> [num_voxels, C] voxel rows.  An empty voxel and every voxel row at or beyond *groups.n_live
    is zeros.  Gradient of max: every point that attains the maximum receives the voxel's gradient (ties all receive,
    as spx_maxpool_bwd; torch_scatter picks one of them)."""
    if reduce not in _collapse.OPS:
        raise ValueError(f"points_to_voxels: reduce must be 'sum', 'mean' or 'max', got {reduce!r}")
    _require_gpu(feat, "features")
    _float_code(feat, "points_to_voxels")
    _check_rows(feat, groups, "points_to_voxels")
    if groups.offsets is None:
        raise ValueError("points_to_voxels: these groups carry rows only; build them with point_groups")
    with torch.cuda.device(feat.device):
        return PointsToVoxelsFunction.apply(feat, groups, reduce)


def _fill_bits(value, dtype: torch.dtype) -> int:
    one = torch.tensor([value], dtype=dtype)
    return int(one.view(_BITS[one.element_size()]).item())


def gather_rows(vfeat: torch.Tensor, rows: torch.Tensor, invalid_value=0) -> torch.Tensor:
    """out[i] = vfeat[rows[i]] or the fill (spx_voxel_to_point); any dtype of 1, 2, 4 or 8 bytes per element."""
    vfeat = vfeat.contiguous()
    n, C = int(rows.shape[0]), int(vfeat.shape[1])
    out = torch.empty((n, C), dtype=vfeat.dtype, device=vfeat.device)
    if n == 0 or C == 0:
        return out
    _lib.check(_lib.load().spx_voxel_to_point(vfeat.data_ptr(), int(vfeat.shape[0]), rows.data_ptr(), n, C,
                                              vfeat.element_size(), _fill_bits(invalid_value, vfeat.dtype),
                                              out.data_ptr(), _stream(vfeat)))
    return out


class VoxelsToPointsFunction(Function):
    """out[i] = vfeat[rows[i]] or the fill; dvfeat[v] = the rows of dout of voxel v's points added in ascending point
    index in fp32 (fp64), rounded once (spx_collapse_fwd, sum): no atomics, identical run to run."""

    @staticmethod
    def forward(ctx, vfeat, groups, invalid_value):
        ctx.groups = groups
        return gather_rows(vfeat.detach(), groups.rows, invalid_value)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_output):
        return _collapse.fwd(grad_output, ctx.groups, "sum", None), None, None


def voxels_to_points(vfeat: torch.Tensor, groups: PointGroups, invalid_value=0) -> torch.Tensor:
    """[num_voxels, C] voxel rows -> [N, C]: row i is the row of point i's voxel, `invalid_value` for a point without
    one.  Differentiable in vfeat for the floating dtypes."""
    _require_gpu(vfeat, "voxel features")
    if vfeat.dim() != 2 or vfeat.shape[0] != groups.num_voxels:
        raise ValueError(f"voxels_to_points: one row per voxel ([{groups.num_voxels}, C]), got {tuple(vfeat.shape)}")
    if vfeat.is_quantized or vfeat.element_size() not in _BITS or vfeat.is_complex():
        raise NotImplementedError(f"voxels_to_points: unsupported dtype {vfeat.dtype}")
    with torch.cuda.device(vfeat.device):
        if not (vfeat.requires_grad and torch.is_grad_enabled()):
            return gather_rows(vfeat, groups.rows, invalid_value)
        _float_code(vfeat, "voxels_to_points (with a gradient)")
        if groups.offsets is None:
            raise ValueError("voxels_to_points: a gradient needs full groups; build them with point_groups")
        return VoxelsToPointsFunction.apply(vfeat, groups, invalid_value)


def decorate_points(points: torch.Tensor, groups: PointGroups, indices: torch.Tensor, vsize_xyz: Sequence[float],
                    coors_range_xyz: Sequence[float], cluster: bool = True, center: bool = True,
                    dtype: torch.dtype = torch.float32, pad_to: Optional[int] = None) -> torch.Tensor:
    """The input rows of a dynamic VFE: [N, nfeat (+ ndim with `cluster`) (+ ndim with `center`)], padded with zero
    columns to `pad_to`.  points fp32 [N, nfeat] (x, y, z first), indices = the voxel index rows (batch index, then
    zyx), vsize_xyz / coors_range_xyz as the voxelisers take them.  A point without a voxel gets zeros.  fp32
    arithmetic, every operation rounded on its own, one rounding into `dtype`.  No gradient: raw points need none."""
    from spconv_amd.pytorch.utils import calc_point2voxel_meta_data
    _require_gpu(points, "points")
    ndim = len(vsize_xyz)
    if points.dim() != 2 or points.dtype != torch.float32 or points.shape[1] < ndim:
        raise ValueError(f"decorate_points: points is a float32 tensor [N, >= {ndim}], got {tuple(points.shape)} {points.dtype}")
    _check_rows(points, groups, "decorate_points")
    if dtype not in _OUT_DTYPES:
        raise ValueError(f"decorate_points: dtype must be float32, float16 or bfloat16, got {dtype}")
    if not (indices.dtype == torch.int32 and indices.dim() == 2 and indices.shape[1] == ndim + 1
            and indices.shape[0] >= groups.num_voxels):
        raise ValueError(f"decorate_points: indices is an int32 tensor [>= {groups.num_voxels}, {ndim + 1}]")
    vsize, _, _, coors_range = calc_point2voxel_meta_data(list(vsize_xyz), list(coors_range_xyz))
    n, nfeat = int(points.shape[0]), int(points.shape[1])
    width = nfeat + ndim * (int(bool(cluster)) + int(bool(center)))
    C_out = width if pad_to is None else int(pad_to)
    if C_out < width:
        raise ValueError(f"decorate_points: pad_to = {pad_to} is narrower than the decorated row ({width} columns)")
    with torch.cuda.device(points.device), torch.no_grad():
        points, indices = points.detach().contiguous(), indices.contiguous()
        mean = None
        if cluster:
            if groups.offsets is None:
                raise ValueError("decorate_points: the cluster offset needs full groups; build them with point_groups")
            mean = _collapse.fwd(points, groups, "mean", groups.n_live)
        out = torch.empty((n, C_out), dtype=dtype, device=points.device)
        if n > 0:
            f = lambda v: (ctypes.c_float * len(v))(*v)
            _lib.check(_lib.load().spx_point_decorate(
                points.data_ptr(), nfeat, n, groups.rows.data_ptr(), indices.data_ptr(), ndim, f(vsize), f(coors_range),
                _ptr(mean), int(bool(cluster)) | (int(bool(center)) << 1), out.data_ptr(), _OUT_DTYPES[dtype], C_out,
                _stream(points)))
    return out
