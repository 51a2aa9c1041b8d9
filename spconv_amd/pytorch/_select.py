"""Voxel pruning on the HIP kernels of csrc/select.hip: keep the most important rows of a sparse tensor and drop, or
process separately, the rest (``functional.sparse_prune`` / ``sparse_select`` / ``spatial.SparsePrune``).  Not part of
the reference, whose users write the step with ``abs().mean(1)``, ``topk`` and boolean indexing.

  * ``row_score``     one fp32 score per row (``spx_row_score``): mean or maximum of |features|, -inf for dead rows
  * ``topk_flags``    uint8 flags of exactly k live rows (``spx_topk_flags``): radix select on the score's key, ties to
                      the lowest row index, k from a count or a ratio computed on the device; nothing read back
  * ``select_build``  the stable compaction of the selected rows (include/spconv_amd.h, voxel pruning):

      - eager form: count (the call's one D->H read: selected rows, live rows) + fill
      - static form (the input carries ``n_live`` or a ``static_num_out`` is given): room for ``static_num_out`` rows,
        nothing read back -- the call can sit inside a captured graph; ``n_out_dev`` = {found, 0, live rows}
      - ``rank_map=True`` (the caller's rows are in ascending, unique key order): a subset of them is too, and
        ``out_indices`` leaves with the level's rank map attached -- the SubM layers behind take
        ``spx_subm_rulebook_ranked``

  * ``fwd`` / ``bwd`` move the feature rows with kernels the library already has: ``spx_voxel_to_point`` with a zero
    fill, ``spx_union_add_bwd`` with one operand.  There is no composite to fall back to.
"""
from __future__ import annotations

import ctypes
from typing import NamedTuple, Optional, Sequence, Tuple

import torch

from spconv_amd import _lib
from spconv_amd.pytorch._rulebook import _check_count, _float_code, _ptr, _require_gpu, _stream, _tag_rank_map, _ws

OPS = {"absmean": _lib.SCORE_ABSMEAN, "absmax": _lib.SCORE_ABSMAX}


class Select(NamedTuple):
    """What a selection build leaves: out_indices [n_out, ndim + 1] (ascending input row; rank map attached when asked
    for), rows int32 [n] (output row of each input row, -1: not selected or cut), src int32 [n_out] (input row of each
    output row, -1 past the live rows), n_out_dev (static form: device {found, 0, live rows}), live_rows (eager form:
    live input rows)."""
    out_indices: torch.Tensor
    rows: torch.Tensor
    src: torch.Tensor
    n_out: int
    n_out_dev: Optional[torch.Tensor]
    live_rows: Optional[int]


def _check_indices(indices: torch.Tensor, ndim: int, what: str) -> None:
    _require_gpu(indices, "indices")
    if indices.dtype != torch.int32:
        raise NotImplementedError(f"{what}: indices must be int32, got {indices.dtype}")
    if indices.dim() != 2 or indices.shape[1] != ndim + 1:
        raise ValueError(f"{what}: indices is a CUDA int32 tensor [n, ndim + 1]")


def row_score(features: torch.Tensor, op: str = "absmean", n_live: Optional[torch.Tensor] = None) -> torch.Tensor:
    """score[i] = mean ("absmean") or maximum ("absmax") of |features[i, :]| as fp32, -inf for rows at or beyond
    *n_live (spx_row_score: one launch, a summation order that depends on C and the dtype only)."""
    _require_gpu(features, "features")
    dt = _float_code(features, "row_score")
    if op not in OPS:
        raise ValueError(f"row_score: op must be 'absmean' or 'absmax', got {op!r}")
    if features.dim() != 2 or features.shape[1] < 1:
        raise ValueError("row_score: features is [n, C] with C >= 1")
    _check_count(n_live, "row_score: n_live")
    feat = features.detach().contiguous()
    n, C = int(feat.shape[0]), int(feat.shape[1])
    with torch.cuda.device(feat.device):
        score = torch.empty((n,), dtype=torch.float32, device=feat.device)
        if n > 0:
            _lib.check(_lib.load().spx_row_score(feat.data_ptr(), n, C, dt, OPS[op], _ptr(n_live), score.data_ptr(),
                                                 _stream(feat)))
    return score


def check_count(k, ratio, what: str) -> Tuple[int, float]:
    """(k_abs, ratio) of spx_topk_flags from exactly one of a count and a ratio."""
    if (k is None) == (ratio is None):
        raise ValueError(f"{what}: give exactly one of k and ratio")
    if k is not None:
        if int(k) != k or k < 0:
            raise ValueError(f"{what}: k must be an integer >= 0, got {k!r}")
        return int(k), 0.0
    ratio = float(ratio)
    if not 0.0 <= ratio <= 1.0:
        raise ValueError(f"{what}: ratio must be in [0, 1], got {ratio!r}")
    return -1, ratio


def topk_flags(score: torch.Tensor, k=None, ratio=None, indices: Optional[torch.Tensor] = None,
               batch_size: Optional[int] = None, n_live: Optional[torch.Tensor] = None
               ) -> Tuple[torch.Tensor, torch.Tensor]:
    """(keep uint8 [n], sel_dev int32 [4] = {live, k, threshold key, ties taken}) of spx_topk_flags."""
    k_abs, ratio = check_count(k, ratio, "topk_mask")
    _require_gpu(score, "score")
    if score.dim() != 1:
        raise ValueError("topk_mask: score holds one value per row")
    score = score.detach().to(torch.float32).contiguous()
    n = int(score.shape[0])
    ndim, B = 0, 0
    if indices is not None:
        if batch_size is None:
            raise ValueError("topk_mask: indices need a batch_size")
        ndim, B = int(indices.shape[1]) - 1 if indices.dim() == 2 else -1, int(batch_size)
        _check_indices(indices, ndim, "topk_mask")
        if indices.shape[0] != n or not 1 <= ndim <= 4 or B < 1:
            raise ValueError("topk_mask: indices is [n, ndim + 1] with ndim in [1, 4], batch_size >= 1")
        indices = indices.contiguous()
    _check_count(n_live, "topk_mask: n_live")
    L = _lib.load()
    with torch.cuda.device(score.device):
        keep = torch.empty((n,), dtype=torch.uint8, device=score.device)
        sel = torch.empty((4,), dtype=torch.int32, device=score.device)
        ws = _ws(int(L.spx_topk_ws_bytes(n)), score.device)
        _lib.check(L.spx_topk_flags(score.data_ptr(), _ptr(indices), n, _ptr(n_live), ndim, B, k_abs, ratio,
                                    keep.data_ptr(), sel.data_ptr(), ws.data_ptr(), ws.numel(), _stream(score)))
    return keep, sel


def select_build(indices: torch.Tensor, batch_size: int, spatial_shape: Sequence[int], keep: torch.Tensor,
                 invert: bool = False, n_live: Optional[torch.Tensor] = None, static_num_out: Optional[int] = None,
                 rank_map: bool = False, violation: Optional[torch.Tensor] = None) -> Select:
    """Compacts the live rows of `indices` (int32 [n, ndim + 1], batch index first) with (keep[i] != 0) != invert, in
    ascending input row.  Static form when `static_num_out` is given or `n_live` is a tensor.  rank_map=True: the
    caller vouches that the live rows are in ascending, unique key order; the result leaves tagged with its map."""
    spatial_shape = [int(v) for v in spatial_shape]
    ndim = len(spatial_shape)
    if not 1 <= ndim <= 4:
        raise ValueError(f"sparse_select: ndim must be in [1, 4], got {ndim}")
    _check_indices(indices, ndim, "sparse_select")
    _require_gpu(keep, "keep")
    if keep.dim() != 1 or keep.shape[0] != indices.shape[0]:
        raise ValueError("sparse_select: keep holds one flag per row")
    if keep.dtype == torch.bool:
        keep = keep.view(torch.uint8)
    elif keep.dtype != torch.uint8:
        raise ValueError(f"sparse_select: keep must be bool or uint8, got {keep.dtype}")
    _check_count(n_live, "sparse_select: n_live")
    with torch.cuda.device(indices.device):         # (kernels, fills and scratch belong to the device of the data)
        return _build(indices.contiguous(), int(batch_size), spatial_shape, keep.contiguous(), bool(invert), n_live,
                      static_num_out, rank_map, violation)


def _build(indices, B, spatial_shape, keep, invert, n_live, static_num_out, rank_map, violation) -> Select:
    L = _lib.load()
    ndim, n, dev = len(spatial_shape), int(indices.shape[0]), indices.device
    sp = _lib.ints(spatial_shape)
    i32 = dict(dtype=torch.int32, device=dev)
    cells, nbytes = None, 0
    if rank_map:
        nbytes = int(L.spx_rankmap_bytes(ndim, B, sp))
        if nbytes > 0:
            cells = torch.empty((nbytes // 4,), **i32)
    ws = _ws(int(L.spx_select_ws_bytes(ndim, n)), dev)
    rows = torch.empty((n,), **i32)
    head = (indices.data_ptr(), n, _ptr(n_live), ndim, B, sp, keep.data_ptr(), int(invert))
    tail = (_ptr(cells), nbytes, _ptr(violation), ws.data_ptr(), ws.numel())
    stream = _stream(indices)
    if static_num_out is not None or n_live is not None:
        cap = int(static_num_out) if static_num_out else max(n, 1)
        out_indices = torch.empty((cap, ndim + 1), **i32)
        src = torch.empty((cap,), **i32)
        n_out_dev = torch.empty((3,), **i32)
        _lib.check(L.spx_select_static(*head, cap, out_indices.data_ptr(), rows.data_ptr(), src.data_ptr(),
                                       n_out_dev.data_ptr(), *tail, stream))
        if cells is not None:
            _tag_rank_map(out_indices, cells, B, spatial_shape, cap)
        return Select(out_indices, rows, src, cap, n_out_dev, None)
    result = (ctypes.c_int * 2)()
    _lib.check(L.spx_select_count(*head, ws.data_ptr(), ws.numel(), result, stream))
    n_out, live_rows = int(result[0]), int(result[1])
    out_indices = torch.empty((n_out, ndim + 1), **i32)
    src = torch.empty((n_out,), **i32)
    _lib.check(L.spx_select_fill(*head, n_out, out_indices.data_ptr(), rows.data_ptr(), src.data_ptr(), *tail, stream))
    if cells is not None and n_out > 0:
        _tag_rank_map(out_indices, cells, B, spatial_shape, n_out)
    return Select(out_indices, rows, src, n_out, None, live_rows)


def fwd(feat: torch.Tensor, s: Select) -> torch.Tensor:
    """out[r] = feat[src[r]], zeros where src[r] < 0 (spx_voxel_to_point with a zero fill): a row keeps its bits."""
    _require_gpu(feat, "features")
    _float_code(feat, "sparse_select")
    feat = feat.contiguous()
    C = int(feat.shape[1])
    if s.n_out == 0 or C == 0:
        return torch.empty((s.n_out, C), dtype=feat.dtype, device=feat.device)
    if feat.shape[0] == 0:
        return torch.zeros((s.n_out, C), dtype=feat.dtype, device=feat.device)
    from spconv_amd.pytorch import _pointvoxel
    return _pointvoxel.gather_rows(feat, s.src, 0)


def bwd(dout: torch.Tensor, s: Select) -> torch.Tensor:
    """din[i] = dout[rows[i]], zeros where rows[i] < 0 (spx_union_add_bwd with one operand)."""
    from spconv_amd.pytorch import _union
    return _union.add_bwd(dout, [s.rows], [True])[0]
