"""The boundary between sparse and dense tensors on the HIP kernels of csrc/dense.hip.

``SparseConvTensor.dense()`` / ``ToDense`` / ``static.dense_static`` and ``SparseConvTensor.from_dense`` of CUDA
tensors (reference ``spconv/pytorch/core.py`` ``scatter_nd`` / ``dense`` / ``from_dense``).  Everything goes through
the cell map of ``include/spconv_amd.h``: ``map[cell]`` = the row that owns the cell.

  * rows whose batch index or coordinates lie outside the grid, and rows >= ``n_live`` of a static-shape tensor, are
    ignored; of several rows with one coordinate the highest row number wins (on every call)
  * the kernels move bytes: any dtype of 1, 2, 4 or 8 bytes per element; ``qint8`` features give a per-tensor
    quantised dense tensor whose empty cells hold the zero point
  * no read-back and no host-side state except in ``from_dense`` (the number of active cells is its result's shape),
    scratch from the caching allocator: ``to_dense`` can sit inside a captured graph
"""
from __future__ import annotations

import ctypes
from typing import Optional, Sequence

import torch

from spconv_amd import _lib
from spconv_amd.pytorch._rulebook import _ptr, _stream


def supported(t: torch.Tensor) -> bool:
    """A CUDA tensor of a dtype the byte-moving kernels cover (everything but complex128 and the sub-byte types)."""
    return (isinstance(t, torch.Tensor) and t.is_cuda and not t.dtype.is_complex
            and (t.dtype == torch.qint8 or (not t.is_quantized and t.element_size() in (1, 2, 4, 8))))


def _check_geometry(batch_size: int, spatial: Sequence[int]):
    spatial = [int(v) for v in spatial]
    if not 1 <= len(spatial) <= 4:
        raise ValueError(f"1 to 4 spatial dimensions, got {len(spatial)}")
    return int(batch_size), spatial


def cell_map(indices: torch.Tensor, batch_size: int, spatial: Sequence[int],
             n_live: Optional[torch.Tensor] = None) -> torch.Tensor:
    """int32 [batch * prod(spatial)]: the row that owns each cell, -1 = none (spx_dense_map)."""
    B, spatial = _check_geometry(batch_size, spatial)
    assert indices.dtype == torch.int32 and indices.dim() == 2 and indices.shape[1] == len(spatial) + 1
    indices = indices.contiguous()
    L = _lib.load()
    sp = _lib.ints(spatial)
    cells = B
    for v in spatial:
        cells *= v
    if cells > 0x7fffffff:
        raise ValueError(f"dense grid of {cells} cells: more than 2^31 - 1")
    m = torch.empty((cells,), dtype=torch.int32, device=indices.device)
    with torch.cuda.device(indices.device):
        _lib.check(L.spx_dense_map(indices.data_ptr(), indices.shape[0], _ptr(n_live), len(spatial), B, sp,
                                   m.data_ptr(), _stream(indices)))
    return m


def _scatter(rows: torch.Tensor, cmap: torch.Tensor, batch_size: int, spatial, channels_first: bool,
             fill_bits: int = 0) -> torch.Tensor:
    """rows [n, C] (unit stride along C, any row stride) -> [B, C, *spatial] or [B, *spatial, C] (spx_to_dense)."""
    B, spatial = _check_geometry(batch_size, spatial)
    if rows.dim() != 2:
        raise ValueError("features must be [n, C]")
    if rows.shape[0] > 0 and rows.shape[1] > 0 and (rows.stride(1) != 1 or rows.stride(0) < rows.shape[1]):
        rows = rows.contiguous()
    C = rows.shape[1]
    ld = rows.stride(0) if rows.shape[0] > 1 else C
    shape = [B, C] + spatial if channels_first else [B] + spatial + [C]
    out = torch.empty(shape, dtype=rows.dtype, device=rows.device)
    with torch.cuda.device(rows.device):
        _lib.check(_lib.load().spx_to_dense(rows.data_ptr(), rows.shape[0], max(int(ld), C), cmap.data_ptr(), out.data_ptr(), C,
                                            rows.element_size(), int(channels_first), int(fill_bits), len(spatial), B,
                                            _lib.ints(spatial), _stream(rows)))
    return out


def _gather(dense: torch.Tensor, cmap: torch.Tensor, n: int, batch_size: int, spatial,
            channels_first: bool) -> torch.Tensor:
    """[B, C, *spatial] or [B, *spatial, C] -> rows [n, C]; rows that own no cell are zero (spx_dense_gather)."""
    B, spatial = _check_geometry(batch_size, spatial)
    dense = dense.contiguous()
    C = dense.shape[1] if channels_first else dense.shape[-1]
    rows = torch.empty((n, C), dtype=dense.dtype, device=dense.device)
    with torch.cuda.device(dense.device):
        _lib.check(_lib.load().spx_dense_gather(dense.data_ptr(), cmap.data_ptr(), rows.data_ptr(), n, C,
                                                dense.element_size(), int(channels_first), len(spatial), B,
                                                _lib.ints(spatial), _stream(dense)))
    return rows


class _ToDense(torch.autograd.Function):
    """Cell map + scatter; the map is saved, the backward is the gather of the incoming gradient."""

    @staticmethod
    def forward(ctx, features, indices, batch_size, spatial, channels_first, n_live):
        cmap = cell_map(indices, batch_size, spatial, n_live)
        ctx.save_for_backward(cmap)
        ctx.geom = (features.shape[0], int(batch_size), list(spatial), bool(channels_first))
        return _scatter(features, cmap, batch_size, spatial, channels_first)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        (cmap,) = ctx.saved_tensors
        n, B, spatial, channels_first = ctx.geom
        return _gather(g, cmap, n, B, spatial, channels_first), None, None, None, None, None


def to_dense(features: torch.Tensor, indices: torch.Tensor, batch_size: int, spatial: Sequence[int],
             channels_first: bool = True, n_live: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Dense tensor of a sparse one ([B, C, *spatial], or [B, *spatial, C] with channels_first=False); differentiable
    in `features`.  n_live: device int32 [1] of a static-shape tensor, rows >= it are ignored."""
    if not supported(features):
        raise NotImplementedError(f"to_dense: no kernel for {features.dtype} features on {features.device}")
    indices = indices.to(features.device)
    if features.dtype == torch.qint8:
        if features.qscheme() != torch.per_tensor_affine:
            raise NotImplementedError("to_dense: per-tensor affine quantisation only")
        zero = int(features.q_zero_point())
        cmap = cell_map(indices, batch_size, spatial, n_live)
        out = _scatter(features.int_repr(), cmap, batch_size, spatial, channels_first, fill_bits=zero & 0xff)
        return torch._make_per_tensor_quantized_tensor(out, float(features.q_scale()), zero)
    return _ToDense.apply(features, indices, batch_size, spatial, channels_first, n_live)


class _FromDense(torch.autograd.Function):
    """Compaction of a channels-last dense tensor: (features, indices).  The backward is the channels-last scatter
    of the feature gradient through the cell map the compaction leaves behind, zeros elsewhere."""

    @staticmethod
    def forward(ctx, x):
        L = _lib.load()
        x = x.contiguous()
        B, spatial, C = int(x.shape[0]), [int(v) for v in x.shape[1:-1]], int(x.shape[-1])
        nd, sp, dev = len(spatial), _lib.ints(spatial), x.device
        cells = B
        for v in spatial:
            cells *= v
        if cells > 0x7fffffff:
            raise ValueError(f"dense grid of {cells} cells: more than 2^31 - 1")
        ws = torch.empty((max(L.spx_from_dense_ws_bytes(nd, B, sp), 16),), dtype=torch.uint8, device=dev)
        cmap = torch.empty((cells,), dtype=torch.int32, device=dev)
        count = ctypes.c_int(0)
        with torch.cuda.device(dev):
            _lib.check(L.spx_from_dense_count(x.data_ptr(), C, x.element_size(), int(x.is_floating_point()), nd, B, sp,
                                              ws.data_ptr(), ws.numel(), ctypes.byref(count), _stream(x)))
            n = int(count.value)
            feats = torch.empty((n, C), dtype=x.dtype, device=dev)
            indices = torch.empty((n, nd + 1), dtype=torch.int32, device=dev)
            _lib.check(L.spx_from_dense_fill(x.data_ptr(), C, x.element_size(), nd, B, sp, ws.data_ptr(), ws.numel(),
                                             indices.data_ptr(), feats.data_ptr(), cmap.data_ptr(), _stream(x)))
        ctx.save_for_backward(cmap)
        ctx.geom = (B, spatial)
        ctx.mark_non_differentiable(indices)
        return feats, indices

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g, _):
        (cmap,) = ctx.saved_tensors
        B, spatial = ctx.geom
        return _scatter(g, cmap, B, spatial, channels_first=False)


def from_dense(x: torch.Tensor):
    """(features [n, C], indices int32 [n, ndim + 1]) of a channels-last dense CUDA tensor [N, *spatial, C]: the cells
    with a non-zero channel, in ascending cell order -- what ``x.to_sparse(x.ndim - 1)`` holds."""
    if not supported(x) or x.is_quantized:
        raise NotImplementedError(f"from_dense: no kernel for {x.dtype} on {x.device}")
    if not 3 <= x.dim() <= 6:
        raise ValueError(f"from_dense: [N, *spatial, C] with 1 to 4 spatial dimensions, got {list(x.shape)}")
    return _FromDense.apply(x)
