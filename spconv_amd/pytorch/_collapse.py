"""Axis collapse on the HIP kernels of csrc/collapse.hip: drop spatial axes of a sparse tensor and merge the rows that
land on one cell of the projected grid (``functional.sparse_collapse`` / ``spatial.SparseCollapse``).

``sparse_collapse_build`` numbers the projected cells through the rank map of the PROJECTED level and lists the rows of
each (include/spconv_amd.h, axis collapse):

  * eager form: count (the call's one D->H read: cells found, live input rows) + fill
  * static form (the input carries ``n_live`` or a ``static_num_out`` is given): room for ``static_num_out`` rows,
    nothing read back -- the call can sit inside a captured graph; ``n_out_dev`` = {found, 0, live rows}
  * output rows in ascending key order of the projected grid, ``out_indices`` leaves with the rank map attached -- the
    SubM layers behind take ``spx_subm_rulebook_ranked``; the rows of a group are listed in ascending input row
  * a projected key space that does not fit a rank map raises NotImplementedError: there is no composite to fall
    back to

``fwd`` / ``bwd`` are the two reduction launches; the gradient of a sum is ``_union.add_bwd`` with one operand.
"""
from __future__ import annotations

import ctypes
from typing import List, NamedTuple, Optional, Sequence, Tuple

import torch

from spconv_amd import _lib
from spconv_amd.pytorch._rulebook import _float_code, _ptr, _require_gpu, _stream, _tag_rank_map, _ws

OPS = {"sum": _lib.COLLAPSE_SUM, "mean": _lib.COLLAPSE_MEAN, "max": _lib.COLLAPSE_MAX}


class Collapse(NamedTuple):
    """What a collapse build leaves: out_indices [n_out, kept + 1] (key order, rank map attached), rows int32 [n]
    (output row of each input row, -1: dead or dropped), offsets int32 [n_out + 1] and list int32 [n] (group r =
    list[offsets[r] : offsets[r + 1]], ascending input row), spatial_shape (the kept extents), n_out_dev (static
    form: device {found, 0, live rows}), live_rows (eager form: live input rows)."""
    out_indices: torch.Tensor
    rows: torch.Tensor
    offsets: torch.Tensor
    list: torch.Tensor
    n_out: int
    spatial_shape: List[int]
    n_out_dev: Optional[torch.Tensor]
    live_rows: Optional[int]


def check_axes(axes: Sequence[int], ndim: int) -> Tuple[int, ...]:
    """The sorted, distinct axes to remove (0 = first spatial axis); at least one axis stays."""
    axes = tuple(int(a) for a in axes)
    if len(set(axes)) != len(axes):
        raise ValueError(f"sparse_collapse: axes {axes} are not distinct")
    if any(a < 0 or a >= ndim for a in axes):
        raise ValueError(f"sparse_collapse: axes {axes} outside [0, ndim = {ndim})")
    if len(axes) >= ndim:
        raise ValueError(f"sparse_collapse: axes {axes} remove every axis of {ndim}: at least one stays")
    return tuple(sorted(axes))


def sparse_collapse_build(indices: torch.Tensor, batch_size: int, spatial_shape: Sequence[int], axes: Sequence[int],
                          n_live: Optional[torch.Tensor] = None, static_num_out: Optional[int] = None) -> Collapse:
    """Groups the live rows of `indices` (int32 [n, ndim + 1], batch index first) by batch index + the axes NOT in
    `axes`.  Static form when `static_num_out` is given or `n_live` is a tensor."""
    _require_gpu(indices, "indices")
    spatial_shape = [int(v) for v in spatial_shape]
    ndim = len(spatial_shape)
    if not 1 <= ndim <= 4:
        raise ValueError(f"sparse_collapse: ndim must be in [1, 4], got {ndim}")
    axes = check_axes(axes, ndim)
    if not (indices.dtype == torch.int32 and indices.dim() == 2 and indices.shape[1] == ndim + 1):
        raise ValueError("sparse_collapse: indices is a CUDA int32 tensor [n, ndim + 1]")
    with torch.cuda.device(indices.device):         # (kernels, fills and scratch belong to the device of the data)
        return _build(indices.contiguous(), int(batch_size), spatial_shape, axes, n_live, static_num_out)


def _build(indices, B, spatial_shape, axes, n_live, static_num_out) -> Collapse:
    L = _lib.load()
    ndim, n, dev = len(spatial_shape), int(indices.shape[0]), indices.device
    kept = [s for d, s in enumerate(spatial_shape) if d not in axes]
    mask = sum(1 << a for a in axes)
    sp = _lib.ints(spatial_shape)
    nbytes = int(L.spx_rankmap_bytes(len(kept), B, _lib.ints(kept))) if min(spatial_shape) >= 1 else 0
    ws_bytes = int(L.spx_collapse_ws_bytes(ndim, B, sp, mask, n))
    if nbytes <= 0 or ws_bytes <= 0:
        raise NotImplementedError(
            f"sparse_collapse: the projected key space (batch {B} x {kept}) does not fit a rank map (2^31 cells) or the "
            f"grid {spatial_shape} is empty; there is no composite path to fall back to")
    i32 = dict(dtype=torch.int32, device=dev)
    cells = torch.empty((nbytes // 4,), **i32)
    ws = _ws(ws_bytes, dev)
    rows = torch.empty((n,), **i32)
    lst = torch.empty((n,), **i32)
    head = (indices.data_ptr(), n, _ptr(n_live), ndim, B, sp, mask)
    tail = (cells.data_ptr(), nbytes, ws.data_ptr(), ws.numel())
    stream = _stream(indices)
    if static_num_out is not None or n_live is not None:
        cap = int(static_num_out) if static_num_out else max(n, 1)
        out_indices = torch.empty((cap, len(kept) + 1), **i32)
        offsets = torch.empty((cap + 1,), **i32)
        n_out_dev = torch.empty((3,), **i32)
        _lib.check(L.spx_collapse_static(*head, cap, out_indices.data_ptr(), rows.data_ptr(), offsets.data_ptr(),
                                         lst.data_ptr(), n_out_dev.data_ptr(), *tail, stream))
        _tag_rank_map(out_indices, cells, B, kept, cap)
        return Collapse(out_indices, rows, offsets, lst, cap, kept, n_out_dev, None)
    result = (ctypes.c_int * 2)()
    _lib.check(L.spx_collapse_count(*head, *tail, result, stream))
    n_out, live_rows = int(result[0]), int(result[1])
    out_indices = torch.empty((n_out, len(kept) + 1), **i32)
    offsets = torch.empty((n_out + 1,), **i32)
    _lib.check(L.spx_collapse_fill(*head, n_out, out_indices.data_ptr(), rows.data_ptr(), offsets.data_ptr(),
                                   lst.data_ptr(), *tail, stream))
    if n_out > 0:
        _tag_rank_map(out_indices, cells, B, kept, n_out)
    return Collapse(out_indices, rows, offsets, lst, n_out, kept, None, live_rows)


def _op(reduce: str) -> int:
    try:
        return OPS[reduce]
    except KeyError:
        raise ValueError(f"sparse_collapse: reduce must be 'sum', 'mean' or 'max', got {reduce!r}") from None


def fwd(feat: torch.Tensor, c: Collapse, reduce: str = "sum", n_live: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[r] = reduce of feat[list[offsets[r] : offsets[r + 1]]] in list order (spx_collapse_fwd); rows at or beyond
    *n_live are zeros."""
    _require_gpu(feat, "features")
    op, dt = _op(reduce), _float_code(feat, "sparse_collapse")
    feat = feat.contiguous()
    C = int(feat.shape[1])
    out = torch.empty((c.n_out, C), dtype=feat.dtype, device=feat.device)
    if c.n_out == 0 or C == 0:
        return out
    _lib.check(_lib.load().spx_collapse_fwd(feat.data_ptr(), feat.shape[0], c.offsets.data_ptr(), c.list.data_ptr(),
                                            c.n_out, C, dt, op, out.data_ptr(), _ptr(n_live), _stream(out)))
    return out


def bwd(dout: torch.Tensor, c: Collapse, reduce: str, feat: Optional[torch.Tensor] = None,
        out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Gradient of `fwd` with respect to feat: sum -> din[i] = dout[rows[i]] (spx_union_add_bwd, one operand); mean and
    max -> spx_collapse_bwd (max needs the forward's feat and out).  Dead and dropped rows get zeros."""
    op, dt = _op(reduce), _float_code(dout, "sparse_collapse")
    dout = dout.contiguous()
    if reduce == "sum":
        from spconv_amd.pytorch import _union
        return _union.add_bwd(dout, [c.rows], [True])[0]
    n, C = int(c.rows.shape[0]), int(dout.shape[1])
    din = torch.empty((n, C), dtype=dout.dtype, device=dout.device)
    if n == 0 or C == 0:
        return din
    if reduce == "max":
        assert feat is not None and out is not None, "the gradient of max needs the forward's feat and out"
        feat, out = feat.contiguous(), out.contiguous()
    _lib.check(_lib.load().spx_collapse_bwd(_ptr(feat), _ptr(out), dout.data_ptr(), c.rows.data_ptr(),
                                            c.offsets.data_ptr(), n, c.n_out, C, dt, op, din.data_ptr(), _stream(dout)))
    return din
