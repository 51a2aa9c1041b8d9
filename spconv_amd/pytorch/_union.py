"""Misaligned add on the HIP kernels of csrc/union.hip: the union of up to eight coordinate sets and the merge of
their feature rows (``functional.sparse_add_hash_based`` / ``sparse_add`` / ``tables.AddTableMisaligned``).

``sparse_union`` numbers the union through the level's rank map (include/spconv_amd.h, misaligned add):

  * eager form: count (the call's one D->H read: union size, duplicate flag, live rows per operand) + fill.  When one
    operand already holds every coordinate of the union the result keeps THAT operand's numbering (``base``), so its
    index tensor and its cached rulebooks stay valid; otherwise the rows come out in ascending key order and
    ``out_indices`` leaves with the rank map attached -- the SubM layers behind take ``spx_subm_rulebook_ranked``
  * static form (any operand carries ``n_live``): key order, room for ``static_num_out`` rows, nothing read back --
    the call can sit inside a captured graph; ``n_out_dev`` = {found, duplicate flag, live rows}
  * a coordinate twice within one operand (the composite sums such rows, a src table cannot say that) is reported:
    the eager form returns None and the caller keeps the composite

``SparseUnionAddFunction`` is the autograd function over the two merge kernels.
"""
from __future__ import annotations

import ctypes
from typing import List, NamedTuple, Optional, Sequence

import torch

from spconv_amd import _lib
from spconv_amd.pytorch import _rulebook
from spconv_amd.pytorch._rulebook import _DTYPES, _cells, _ptr, _stream, _tag_rank_map, _ws

MAX_OPERANDS = 8


class Union(NamedTuple):
    """What a union build leaves: out_indices [n_out, ndim + 1] (None with base >= 0: the result's indices are operand
    `base`'s), rows[t] int32 [n_t] (output row of each input row, -1: dead or dropped), src int32 [T, n_out] (row of
    operand t at each output row, -1: absent), base (-1: key order), n_out_dev (static form: device {found, duplicate
    flag, live rows}), live (eager form: live rows per operand)."""
    out_indices: Optional[torch.Tensor]
    rows: List[torch.Tensor]
    src: torch.Tensor
    n_out: int
    base: int
    n_out_dev: Optional[torch.Tensor]
    live: Optional[List[int]]


def fits(total_rows: int, batch_size: int, spatial_shape) -> int:
    """Bytes of the level's rank map when the native path applies to a union over `total_rows` rows, else 0 (the size
    gates of ops.attach_rank_map: same environment switch)."""
    spatial_shape = [int(v) for v in spatial_shape]
    if not 1 <= len(spatial_shape) <= 4:
        return 0
    nbytes = int(_lib.load().spx_rankmap_bytes(len(spatial_shape), int(batch_size), _lib.ints(spatial_shape)))
    return nbytes if _rulebook._rankmap_fits(nbytes, _cells(batch_size, spatial_shape), total_rows) else 0


def _check_operands(indices: Sequence[torch.Tensor], ndim: int) -> None:
    if not 1 <= len(indices) <= MAX_OPERANDS:
        raise ValueError(f"sparse_union: 1 to {MAX_OPERANDS} operands, got {len(indices)}")
    dev = indices[0].device
    for t in indices:
        if not (t.is_cuda and t.dtype == torch.int32 and t.dim() == 2 and t.shape[1] == ndim + 1 and t.device == dev):
            raise ValueError("sparse_union: every operand is a CUDA int32 tensor [n, ndim + 1] on one device")


def sparse_union(indices: Sequence[torch.Tensor], batch_size: int, spatial_shape: Sequence[int],
                 n_live: Optional[Sequence[Optional[torch.Tensor]]] = None, static_num_out: Optional[int] = None,
                 base: Optional[int] = None, gate: bool = True) -> Optional[Union]:
    """Union of the coordinate sets `indices[t]` (int32 [n_t, ndim + 1], batch index first).  Static form when
    `static_num_out` is given or any `n_live[t]` is a tensor.  base: None = the covering operand if there is one
    (the largest, then the first), else key order; -1 forces key order.  Returns None when the native path does not
    apply: the size gate (gate=False skips all of it but the hard limit of the key space), or -- eager form -- a
    coordinate that occurs twice within one operand."""
    spatial_shape = [int(v) for v in spatial_shape]
    _check_operands(indices, len(spatial_shape))
    with torch.cuda.device(indices[0].device):      # (kernels, fills and scratch belong to the device of the data)
        return _sparse_union(indices, int(batch_size), spatial_shape, n_live, static_num_out, base, gate)


def _sparse_union(indices, B, spatial_shape, n_live, static_num_out, base, gate) -> Optional[Union]:
    ndim, T = len(spatial_shape), len(indices)
    L = _lib.load()
    indices = [t.contiguous() for t in indices]
    dev = indices[0].device
    ns = [int(t.shape[0]) for t in indices]
    total = sum(ns)
    sp = _lib.ints(spatial_shape)
    nbytes = fits(total, B, spatial_shape) if gate else int(L.spx_rankmap_bytes(ndim, B, sp))
    ws_bytes = int(L.spx_union_ws_bytes(ndim, B, sp, T, total))
    if nbytes <= 0 or ws_bytes <= 0:
        return None
    i32 = dict(dtype=torch.int32, device=dev)
    lives = list(n_live) if n_live is not None else [None] * T
    static = static_num_out is not None or any(v is not None for v in lives)
    cells = torch.empty((nbytes // 4,), **i32)
    ws = _ws(ws_bytes, dev)
    rows = [torch.empty((n,), **i32) for n in ns]
    head = (_lib.ptrs([t.data_ptr() for t in indices]), _lib.ints(ns), _lib.ptrs([_ptr(v) for v in lives]), T, ndim, B, sp)
    tail = (cells.data_ptr(), nbytes, ws.data_ptr(), ws.numel())
    stream = _stream(indices[0])
    row_ptrs = _lib.ptrs([r.data_ptr() for r in rows])
    if static:
        cap = int(static_num_out) if static_num_out else max(total, 1)
        out_indices = torch.empty((cap, ndim + 1), **i32)
        src = torch.empty((T, cap), **i32)
        n_out_dev = torch.empty((3,), **i32)
        _lib.check(L.spx_union_static(*head, cap, out_indices.data_ptr(), row_ptrs, src.data_ptr(), n_out_dev.data_ptr(),
                                      *tail, stream))
        _tag_rank_map(out_indices, cells, B, spatial_shape, cap)
        return Union(out_indices, rows, src, cap, -1, n_out_dev, None)
    result = (ctypes.c_int * (2 + T))()
    _lib.check(L.spx_union_count(*head, *tail, result, stream))
    size, dup, live = int(result[0]), int(result[1]), [int(v) for v in result[2:2 + T]]
    if dup:
        return None
    if base is None:
        cover = [t for t in range(T) if live[t] == size]
        base = max(cover, key=lambda t: ns[t]) if cover else -1        # (max keeps the first of equals)
    elif base >= 0 and live[base] != size:
        raise ValueError(f"sparse_union: operand {base} holds {live[base]} of the union's {size} coordinates")
    n_out = ns[base] if base >= 0 else size
    out_indices = torch.empty((n_out, ndim + 1), **i32) if base < 0 else None
    src = torch.empty((T, n_out), **i32)
    _lib.check(L.spx_union_fill(*head, n_out, base, _ptr(out_indices), row_ptrs, src.data_ptr(), *tail, stream))
    if base < 0 and n_out > 0:
        _tag_rank_map(out_indices, cells, B, spatial_shape, n_out)
    return Union(out_indices, rows, src, n_out, base, None, live)


def add_fwd(feats: Sequence[torch.Tensor], src: torch.Tensor, n_out: int,
            n_live: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[r] = sum of feats[t][src[t, r]] over the operands present at r (spx_union_add_fwd)."""
    feats = [f.contiguous() for f in feats]
    C, dt = int(feats[0].shape[1]), feats[0].dtype
    out = torch.empty((n_out, C), dtype=dt, device=feats[0].device)
    if n_out == 0 or C == 0:
        return out
    _lib.check(_lib.load().spx_union_add_fwd(_lib.ptrs([f.data_ptr() for f in feats]),
                                             _lib.ints([f.shape[0] for f in feats]), len(feats), src.data_ptr(), n_out, C,
                                             _DTYPES[dt], out.data_ptr(), _ptr(n_live), _stream(out)))
    return out


def add_bwd(dout: torch.Tensor, rows: Sequence[torch.Tensor], need: Sequence[bool]) -> List[Optional[torch.Tensor]]:
    """din_t[i] = dout[rows_t[i]] or zeros, for the operands that need a gradient (spx_union_add_bwd: one launch)."""
    dout = dout.contiguous()
    C = int(dout.shape[1])
    picked = [t for t, w in enumerate(need) if w]
    dins = [torch.empty((rows[t].shape[0], C), dtype=dout.dtype, device=dout.device) for t in picked]
    if picked and C > 0 and any(d.shape[0] for d in dins):
        _lib.check(_lib.load().spx_union_add_bwd(dout.data_ptr(), dout.shape[0], _lib.ptrs([d.data_ptr() for d in dins]),
                                                 _lib.ptrs([rows[t].data_ptr() for t in picked]),
                                                 _lib.ints([d.shape[0] for d in dins]), len(picked), C,
                                                 dout.element_size(), _stream(dout)))
    out: List[Optional[torch.Tensor]] = [None] * len(need)
    for t, d in zip(picked, dins):
        out[t] = d
    return out
