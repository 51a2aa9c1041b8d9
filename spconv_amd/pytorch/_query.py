"""Voxel query and neighbour grouping on the HIP kernels of csrc/query.hip (``functional.voxel_query`` /
``group_voxels`` / ``spatial.VoxelQueryAndGroup``).  Not part of the reference; the two-stage detectors over sparse
backbones (Voxel R-CNN's Voxel RoI pooling, the voxel set abstraction of the PV-RCNN family) call them as the
``voxel_query`` / ``grouping_operation`` CUDA extensions of ``pointnet2_stack``.

  * ``voxel_query``   per query point the first ``nsample`` voxels of a level inside a window of cells (and a radius),
                      as rows of the level (``spx_voxel_query``): through the level's rank map when its index tensor
                      carries one (key-ordered rows, one or two loads per window line), through a hash table built
                      from the rows otherwise; nothing read back
  * ``group_voxels``  ``out[m, s] = vfeat[rows[m, s]]`` (``spx_group_fwd``); its gradient in ``vfeat`` is a segment sum
                      over the transposed list (``spx_point_groups`` over the flattened rows, ``spx_group_bwd``): no
                      atomics, identical run to run

There is no gradient with respect to the queries: raw coordinates need none.
"""
from __future__ import annotations

import ctypes
from typing import NamedTuple, Optional, Sequence

import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from spconv_amd import _lib
from spconv_amd.pytorch._level import _floats, _geometry, check_points, flat_groups, grad_rows, groups_missing
from spconv_amd.pytorch._level import flat_groups as neighbor_groups, level_rankmap  # noqa: F401  (names tests and tools reach)
from spconv_amd.pytorch._pointvoxel import PointGroups
from spconv_amd.pytorch._rulebook import _float_code, _ptr, _require_gpu, _stream, _ws

MAX_RANGE, MAX_NSAMPLE = 15, 128
_FLAG_RADIUS, _FLAG_PAD_FIRST = 1, 2


class VoxelNeighbors(NamedTuple):
    """The neighbour table of a set of queries over one level: rows int32 [M, nsample] (row of the level, -1: none),
    count int32 [M] (kept hits), offsets fp32 [M, nsample, ndim] (voxel centre minus query, xyz) or None, groups (a
    ``PointGroups`` over the FLATTENED rows -- entry e = m * nsample + s -- or None: only a gradient needs it),
    num_voxels (rows of the level), n_queries / n_live (device int32 or None: queries / voxel rows at or beyond them do
    not exist)."""
    rows: torch.Tensor
    count: torch.Tensor
    offsets: Optional[torch.Tensor]
    groups: Optional[PointGroups]
    num_voxels: int
    n_queries: Optional[torch.Tensor] = None
    n_live: Optional[torch.Tensor] = None


def _check_window(query_range: Sequence[int], nsample: int, ndim: int, pad: str):
    query_range = [int(v) for v in query_range]
    if len(query_range) != ndim:
        raise ValueError(f"voxel_query: query_range holds {ndim} values (zyx) for ndim = {ndim}, got {query_range}")
    if min(query_range) < 0 or max(query_range) > MAX_RANGE:
        raise ValueError(f"voxel_query: every query_range must be in 0 .. {MAX_RANGE}, got {query_range}")
    if not 1 <= int(nsample) <= MAX_NSAMPLE:
        raise ValueError(f"voxel_query: nsample must be in 1 .. {MAX_NSAMPLE}, got {nsample}")
    if pad not in ("none", "first"):
        raise ValueError(f"voxel_query: pad is 'none' or 'first', got {pad!r}")
    return query_range


def squared_radius(radius: Optional[float]) -> Optional[float]:
    """float32(radius) * float32(radius), rounded to float32: the r2 the kernel compares with"""
    if radius is None:
        return None
    r = ctypes.c_float(float(radius)).value
    if not r >= 0:
        raise ValueError(f"voxel_query: radius must be >= 0, got {radius}")
    return ctypes.c_float(r * r).value          # (the product of two float32 is exact in double: one rounding)


def query_ws_bytes(n_cap: int, nsample: int, ndim: int, n: int, ranked: bool) -> int:
    return int(_lib.load().spx_voxel_query_ws_bytes(int(n_cap), int(nsample), int(ndim), int(n), int(bool(ranked))))


def voxel_query_into(queries: torch.Tensor, batch_ids: Optional[torch.Tensor], n_queries: Optional[torch.Tensor],
                     vsize_zyx, coors_range_zyx, indices: torch.Tensor, n_live: Optional[torch.Tensor], batch_size: int,
                     spatial_shape: Sequence[int], rankmap: Optional[torch.Tensor], query_range: Sequence[int],
                     nsample: int, r2: Optional[float], pad_first: bool, rows: torch.Tensor, count: torch.Tensor,
                     offsets: Optional[torch.Tensor], ws: Optional[torch.Tensor], group_width: int = 0) -> None:
    """The one C call into buffers the caller owns (no allocation: capturable).  vsize_zyx / coors_range_zyx: ctypes
    float arrays in zyx order (``calc_point2voxel_meta_data``); rankmap: the level's rank map or None (hash form, which
    needs `ws` of ``query_ws_bytes``); r2: ``squared_radius`` or None; group_width: 0 (chosen from the window) or the
    lanes per query, a power of two up to 64 -- the result does not depend on it."""
    ndim = len(spatial_shape)
    flags = (_FLAG_RADIUS if r2 is not None else 0) | (_FLAG_PAD_FIRST if pad_first else 0)
    if group_width:
        if group_width not in (1, 2, 4, 8, 16, 32, 64):
            raise ValueError(f"voxel_query: group_width is a power of two up to 64, got {group_width}")
        flags |= int(group_width).bit_length() << 8
    _lib.check(_lib.load().spx_voxel_query(
        queries.data_ptr(), int(queries.shape[1]), _ptr(batch_ids), int(queries.shape[0]), _ptr(n_queries), ndim, vsize_zyx,
        coors_range_zyx, indices.data_ptr(), int(indices.shape[0]), _ptr(n_live), int(batch_size),
        _lib.ints(spatial_shape), _ptr(rankmap), 0 if rankmap is None else rankmap.numel() * rankmap.element_size(),
        _lib.ints(query_range), int(nsample), 0.0 if r2 is None else float(r2), flags, rows.data_ptr(), count.data_ptr(),
        _ptr(offsets), _ptr(ws), 0 if ws is None else ws.numel(), _stream(queries)))


def voxel_query(queries: torch.Tensor, batch_ids: Optional[torch.Tensor], x, vsize_xyz: Sequence[float],
                coors_range_xyz: Sequence[float], query_range: Sequence[int], nsample: int,
                radius: Optional[float] = None, pad: str = "none", with_offsets: bool = False,
                n_queries: Optional[torch.Tensor] = None, with_groups: Optional[bool] = None) -> VoxelNeighbors:
    """The first `nsample` voxels of the level `x` (a SparseConvTensor, ndim 2 or 3) around each query.  queries fp32
    [M, >= ndim] (x, y, z first), batch_ids int32 [M] or None (all batch 0); vsize_xyz / coors_range_xyz as
    ``point_corners`` takes them, the voxel size being that of x's level; query_range: ndim ints in index-column (zyx)
    order, each in 0 .. 15; nsample in 1 .. 128.  A query's own cell is ``floorf((q - lo) / vsize)``; the candidates
    are the cells within query_range of it, visited in ascending linear key (z outermost, x innermost -- ascending row
    for a key-ordered level).  A candidate is a hit when it lies inside the grid, a live row of x holds it and, with a
    radius, the squared distance between its centre and the query, in fp32 with every operation rounded on its own,
    is below ``float32(radius) ** 2``.  The first nsample hits are kept: rows [M, nsample], count [M] =
    min(hits, nsample), and with with_offsets the centre-minus-query vectors [M, nsample, ndim] (xyz).  Slots at or
    beyond count hold row -1 and offsets 0; pad="first" repeats slot 0 there (rows and offsets) when count > 0, as
    pointnet2 does, so a plain ``max(1)`` behind the MLP is correct.  A query outside the range, with a NaN
    coordinate, with a batch id outside [0, batch_size) or at or beyond *n_queries has count 0 and rows -1.  x's rank
    map is used when its index tensor carries one (rows in key order), the hash table otherwise; a static tensor's
    n_live_dev is passed through.  with_groups (default: x's features require a gradient) builds the transposed list
    the gradient of ``group_voxels`` walks.  No gradient with respect to the queries: raw coordinates need none."""
    ndim, vsize, coors_range = _geometry(vsize_xyz, coors_range_xyz, "voxel_query")
    query_range = _check_window(query_range, nsample, ndim, pad)
    r2 = squared_radius(radius)
    nsample = int(nsample)
    indices, spatial_shape, B, n_live, rankmap, with_groups = check_points("voxel_query", "queries", queries, batch_ids,
                                                                           n_queries, x, ndim, nsample, with_groups)
    M, n, dev = int(queries.shape[0]), int(indices.shape[0]), queries.device
    with torch.cuda.device(dev), torch.no_grad():
        queries = queries.detach().contiguous()
        batch_ids = None if batch_ids is None else batch_ids.contiguous()
        rows = torch.empty((M, nsample), dtype=torch.int32, device=dev)
        count = torch.empty((M,), dtype=torch.int32, device=dev)
        offsets = torch.empty((M, nsample, ndim), dtype=torch.float32, device=dev) if with_offsets else None
        if M > 0:
            ws = None if rankmap is not None else _ws(query_ws_bytes(M, nsample, ndim, n, False), dev)
            voxel_query_into(queries, batch_ids, n_queries, _floats(vsize), _floats(coors_range), indices, n_live, B,
                             spatial_shape, rankmap, query_range, nsample, r2, pad == "first", rows, count, offsets, ws)
        groups = flat_groups(rows, n, n_live) if with_groups else None
    return VoxelNeighbors(rows, count, offsets, groups, n, n_queries, n_live)


def group_fwd(vfeat: torch.Tensor, nb: VoxelNeighbors) -> torch.Tensor:
    """out[m, s] = vfeat[rows[m, s]], zeros for -1 (spx_group_fwd: one launch)."""
    dt = _float_code(vfeat, "group_voxels")
    vfeat = vfeat.contiguous()
    M, S = (int(v) for v in nb.rows.shape)
    n, C = int(vfeat.shape[0]), int(vfeat.shape[1])
    out = torch.empty((M, S, C), dtype=vfeat.dtype, device=vfeat.device)
    if M > 0 and C > 0:
        _lib.check(_lib.load().spx_group_fwd(vfeat.data_ptr(), n, nb.rows.data_ptr(), M, S, C, dt, out.data_ptr(),
                                             _stream(vfeat)))
    return out


def group_bwd(dout: torch.Tensor, nb: VoxelNeighbors) -> torch.Tensor:
    """dvfeat[v] = sum of dout[e] over the entries e of voxel v's group, in ascending e (spx_group_bwd: one launch, no
    atomics); zeros for an empty group and for rows at or beyond *n_live."""
    dt, dout, dvfeat, g = grad_rows("group_voxels", dout, nb, "neighbour", "voxel_query")
    if g is not None:
        M, S = nb.rows.shape
        _lib.check(_lib.load().spx_group_bwd(dout.data_ptr(), M, S, g.offsets.data_ptr(), g.list.data_ptr(), nb.num_voxels,
                                             _ptr(nb.n_live), int(dout.shape[-1]), dt, dvfeat.data_ptr(), _stream(dout)))
    return dvfeat


class GroupFunction(Function):
    """spx_group_fwd / spx_group_bwd.  The gradient is the one in the voxel rows; the queries get none."""

    @staticmethod
    def forward(ctx, vfeat, nb):
        ctx.nb = nb
        return group_fwd(vfeat.detach(), nb)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_output):
        return group_bwd(grad_output, ctx.nb), None


def group_voxels(vfeat: torch.Tensor, nb: VoxelNeighbors) -> torch.Tensor:
    """[num_voxels, C] voxel rows -> [M, nsample, C]: slot (m, s) is a copy of row ``nb.rows[m, s]``, zeros where that
    is -1.  Differentiable in vfeat (a segment sum over the transposed list, in ascending entry, fp32 accumulation --
    fp64 for float64 -- rounded once: identical run to run); there is no gradient with respect to the queries."""
    if vfeat.dim() != 2 or vfeat.shape[0] != nb.num_voxels:
        raise ValueError(f"group_voxels: one row per voxel ([{nb.num_voxels}, C]), got {tuple(vfeat.shape)}")
    _float_code(vfeat, "group_voxels")
    needs_grad = vfeat.requires_grad and torch.is_grad_enabled()
    if needs_grad and nb.groups is None and nb.rows.numel() > 0 and nb.num_voxels > 0:
        raise groups_missing("group_voxels", "neighbour", "voxel_query")
    _require_gpu(vfeat, "voxel features")
    with torch.cuda.device(vfeat.device):
        if not needs_grad:
            return group_fwd(vfeat, nb)
        return GroupFunction.apply(vfeat, nb)
