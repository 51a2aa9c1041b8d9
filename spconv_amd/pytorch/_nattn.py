"""Neighbour attention and neighbour aggregation on the HIP kernels of csrc/nattn.hip (``functional.neighbor_attention``
/ ``neighbor_aggregate``, ``spatial.NeighborAttention``): attention of every query over its own neighbours, read through
the ``VoxelNeighbors`` table of ``voxel_query`` / ``ball_query`` / ``knn_query``.  Not part of the reference; the code
bases users port call them as Voxel Transformer's local / dilated attention, the ``attention_step1`` /
``attention_step2`` pair of Stratified Transformer and Swin3D and the ``aggregation`` of ``pointops``.

  * forward   one launch (``spx_neighbor_attn_fwd``): no grouped [M, S, C] row is written; with a gradient ahead the
              probabilities are kept as fp32 [M, S, H]
  * backward  two launches (``spx_neighbor_attn_bwd``): the query side (dS = dbias, dq), the key side over the
              transposed list (dk, dv); no atomics, identical run to run

The ``_into`` forms take buffers the caller owns, allocate nothing and read nothing back: they can sit inside a captured
graph behind ``voxel_query_into`` / ``knn_query_into`` and the groups.  There is no composite to fall back to.

Not built: dropout, gradients in coordinates, float64, a fused weight MLP for vector attention, head sizes outside
8, 16, 32, 64, 128.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from spconv_amd import _lib
from spconv_amd.pytorch._level import groups_missing
from spconv_amd.pytorch._query import MAX_NSAMPLE, VoxelNeighbors
from spconv_amd.pytorch._rulebook import _ptr, _require_gpu, _stream

HEAD_SIZES = (8, 16, 32, 64, 128)
MAX_CHANNELS = 512
_CODES = {torch.float16: _lib.DTYPE_F16, torch.bfloat16: _lib.DTYPE_BF16, torch.float32: _lib.DTYPE_F32}
_ATTENTION, _AGGREGATE = 0, 1


def _check_table(op: str, nb: VoxelNeighbors, n_rows: int, dev) -> Tuple[int, int]:
    rows = nb.rows
    if rows.dim() != 2 or rows.dtype != torch.int32 or not rows.is_contiguous():
        raise ValueError(f"{op}: nb.rows is a contiguous int32 tensor [M, nsample], got {tuple(rows.shape)} {rows.dtype}")
    M, S = (int(v) for v in rows.shape)
    if not 1 <= S <= MAX_NSAMPLE:
        raise ValueError(f"{op}: nsample must be in 1 .. {MAX_NSAMPLE}, got {S}")
    if n_rows != nb.num_voxels:
        raise ValueError(f"{op}: k and v hold one row per voxel or point of the table ({nb.num_voxels}), got {n_rows}")
    if rows.device != dev:
        raise ValueError(f"{op}: the table is on {rows.device}, the rows on {dev}")
    return M, S


def _check_rows(op: str, name: str, t: torch.Tensor, dtype, C: int) -> None:
    if t.dim() != 2 or int(t.shape[1]) != C or t.dtype != dtype:
        raise ValueError(f"{op}: {name} is [rows, {C}] of {dtype} (nothing is cast), got {tuple(t.shape)} {t.dtype}")
    _require_gpu(t, name)


def _dtype(op: str, t: torch.Tensor) -> int:
    if t.dtype not in _CODES:
        raise NotImplementedError(f"{op}: rows must be float16, bfloat16 or float32 (nothing is cast), got {t.dtype}")
    return _CODES[t.dtype]


def _heads(op: str, C: int, heads: int, what: str) -> Tuple[int, int]:
    H = int(heads)
    if H != heads or H < 1 or C < 1 or C % H != 0:
        raise ValueError(f"{op}: {what} must be an integer >= 1 that divides C = {C}, got {heads!r}")
    if C // H not in HEAD_SIZES:
        raise NotImplementedError(f"{op}: C / {what} must be one of {list(HEAD_SIZES)}, got {C // H}")
    if C > MAX_CHANNELS:
        raise NotImplementedError(f"{op}: C must be <= {MAX_CHANNELS}, got {C}")
    return H, C // H


def strided_rows(t: torch.Tensor) -> torch.Tensor:
    """t itself when the kernels can read it in place (last dimension contiguous, 16-byte aligned rows: the halves of a
    Linear(C, 2C) output), a contiguous copy otherwise"""
    if t.shape[0] <= 1:
        return t.contiguous()
    ok = (t.stride(1) == 1 and t.stride(0) >= t.shape[1] and t.data_ptr() % 16 == 0
          and (t.stride(0) * t.element_size()) % 16 == 0)
    return t if ok else t.contiguous()


def _ld(t: torch.Tensor) -> int:
    return int(t.stride(0)) if t.shape[0] > 1 else int(t.shape[1])


def check_attention(q, k, v, nb: VoxelNeighbors, num_heads, scale, bias) -> Tuple[int, int, int, int, float]:
    """(M, S, H, D, scale) of a neighbor_attention call; everything that can be refused is refused before a kernel runs"""
    op = "neighbor_attention"
    _dtype(op, q)
    if q.dim() != 2:
        raise ValueError(f"{op}: q is [M, C], got {tuple(q.shape)}")
    C = int(q.shape[1])
    H, D = _heads(op, C, num_heads, "num_heads")
    _check_rows(op, "q", q, q.dtype, C)
    _check_rows(op, "k", k, q.dtype, C)
    _check_rows(op, "v", v, q.dtype, C)
    if k.shape[0] != v.shape[0]:
        raise ValueError(f"{op}: k and v hold the same rows, got {tuple(k.shape)} and {tuple(v.shape)}")
    M, S = _check_table(op, nb, int(k.shape[0]), q.device)
    if int(q.shape[0]) != M:
        raise ValueError(f"{op}: one query row per row of the table ({M}), got {tuple(q.shape)}")
    if bias is not None and (bias.dtype != torch.float32 or tuple(bias.shape) != (M, S, H) or bias.device != q.device):
        raise ValueError(f"{op}: bias is float32 [M, nsample, H] = [{M}, {S}, {H}] on the rows' device (nothing is cast), "
                         f"got {bias.dtype} {tuple(bias.shape)}")
    return M, S, H, D, float(D ** -0.5 if scale is None else scale)


def check_aggregate(w, v, nb: VoxelNeighbors) -> Tuple[int, int, int, int]:
    """(M, S, G, D) of a neighbor_aggregate call"""
    op = "neighbor_aggregate"
    _dtype(op, v)
    if v.dim() != 2 or w.dim() != 3:
        raise ValueError(f"{op}: v is [rows, C] and w [M, nsample, G], got {tuple(v.shape)} and {tuple(w.shape)}")
    C = int(v.shape[1])
    G, D = _heads(op, C, int(w.shape[2]), "the group count")
    _check_rows(op, "v", v, v.dtype, C)
    M, S = _check_table(op, nb, int(v.shape[0]), v.device)
    if w.dtype not in (v.dtype, torch.float32) or tuple(w.shape) != (M, S, G) or w.device != v.device:
        raise ValueError(f"{op}: w is [M, nsample, G] = [{M}, {S}, {G}] in v's dtype or float32 on v's device (nothing is "
                         f"cast), got {w.dtype} {tuple(w.shape)}")
    return M, S, G, D


def probabilities_bytes(M: int, S: int, H: int) -> int:
    """bytes of the fp32 [M, S, H] table the forward leaves for the backward"""
    return int(_lib.load().spx_neighbor_attn_ws_bytes(int(M), int(S), int(H)))


def neighbor_attention_into(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, nb: VoxelNeighbors, H: int, scale: float,
                            bias: Optional[torch.Tensor], out: torch.Tensor, P: Optional[torch.Tensor]) -> None:
    """The one C call into buffers the caller owns (no allocation: capturable).  q, out [M, C] contiguous; k, v as
    ``strided_rows`` leaves them; bias fp32 [M, S, H] contiguous or None; P fp32 [M, S, H] (the workspace a backward
    reads, ``probabilities_bytes``) or None."""
    M, S = (int(s) for s in nb.rows.shape)
    C = int(q.shape[1])
    _lib.check(_lib.load().spx_neighbor_attn_fwd(
        q.data_ptr(), k.data_ptr(), v.data_ptr(), _ld(k), _ld(v), nb.rows.data_ptr(), _ptr(bias), None, _CODES[q.dtype], M,
        S, int(nb.num_voxels), _ptr(nb.n_live), int(H), C // int(H), _CODES[q.dtype], _ATTENTION, float(scale),
        out.data_ptr(), _ptr(P), _stream(q)))


def neighbor_attention_bwd_into(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, nb: VoxelNeighbors, H: int,
                                scale: float, P: torch.Tensor, d_out: torch.Tensor, dq: torch.Tensor,
                                dk: Optional[torch.Tensor], dv: Optional[torch.Tensor], dbias: torch.Tensor) -> None:
    """The backward's one C call.  P as the forward left it; d_out, dq [M, C]; dbias fp32 [M, S, H], always written
    (it is dS); dk, dv [n, C] contiguous, or both None: then the key side is not run and nb.groups is not needed."""
    M, S = (int(s) for s in nb.rows.shape)
    C, g = int(q.shape[1]), nb.groups
    if dk is not None and (g is None or g.offsets is None):
        raise groups_missing("neighbor_attention", "neighbour", "the query")
    _lib.check(_lib.load().spx_neighbor_attn_bwd(
        q.data_ptr(), k.data_ptr(), v.data_ptr(), _ld(k), _ld(v), nb.rows.data_ptr(), P.data_ptr(), _lib.DTYPE_F32,
        d_out.data_ptr(), None if dk is None else g.offsets.data_ptr(), None if dk is None else g.list.data_ptr(), M, S,
        int(nb.num_voxels), _ptr(nb.n_live), int(H), C // int(H), _CODES[q.dtype], _ATTENTION, float(scale), dq.data_ptr(),
        _ptr(dk), _ptr(dv), dbias.data_ptr(), _stream(q)))


def neighbor_aggregate_into(w: torch.Tensor, v: torch.Tensor, nb: VoxelNeighbors, out: torch.Tensor) -> None:
    """out[m, g] = sum over the key slots of w[m, s, g] * v[rows[m, s], g] into a buffer the caller owns"""
    M, S, G = (int(s) for s in w.shape)
    C = int(v.shape[1])
    _lib.check(_lib.load().spx_neighbor_attn_fwd(
        None, None, v.data_ptr(), C, _ld(v), nb.rows.data_ptr(), None, w.data_ptr(), _CODES[w.dtype], M, S,
        int(nb.num_voxels), _ptr(nb.n_live), G, C // G, _CODES[v.dtype], _AGGREGATE, 1.0, out.data_ptr(), None, _stream(v)))


def neighbor_aggregate_bwd_into(w: torch.Tensor, v: torch.Tensor, nb: VoxelNeighbors, d_out: torch.Tensor,
                                dw: Optional[torch.Tensor], dv: Optional[torch.Tensor]) -> None:
    """dw [M, S, G] in w's dtype and / or dv [n, C] (which needs nb.groups) into buffers the caller owns"""
    M, S, G = (int(s) for s in w.shape)
    C, g = int(v.shape[1]), nb.groups
    if dv is not None and (g is None or g.offsets is None):
        raise groups_missing("neighbor_aggregate", "neighbour", "the query")
    _lib.check(_lib.load().spx_neighbor_attn_bwd(
        None, None, v.data_ptr(), C, _ld(v), nb.rows.data_ptr(), w.data_ptr(), _CODES[w.dtype], d_out.data_ptr(),
        None if dv is None else g.offsets.data_ptr(), None if dv is None else g.list.data_ptr(), M, S, int(nb.num_voxels),
        _ptr(nb.n_live), G, C // G, _CODES[v.dtype], _AGGREGATE, 1.0, None, None, _ptr(dv), _ptr(dw), _stream(v)))


def _row_grad(like: torch.Tensor, nb: VoxelNeighbors) -> Tuple[torch.Tensor, bool]:
    """(the [n, C] gradient buffer, whether a kernel has to fill it): zeros when no entry or no row exists"""
    n, C = int(like.shape[0]), int(like.shape[1])
    if n == 0 or nb.rows.numel() == 0:
        return torch.zeros((n, C), dtype=like.dtype, device=like.device), False
    return torch.empty((n, C), dtype=like.dtype, device=like.device), True


def _grad_out(op: str, g: torch.Tensor, like: torch.Tensor) -> torch.Tensor:
    if g.dtype != like.dtype:
        raise NotImplementedError(f"{op}: the gradient arrives as {g.dtype}, the rows are {like.dtype}")
    return g.contiguous()


class NeighborAttentionFunction(Function):
    """spx_neighbor_attn_fwd / _bwd: gradients to q, k, v and bias, none to the table.  Casts nothing under autocast."""

    @staticmethod
    def forward(ctx, q, k, v, bias, nb, H, scale):
        q, k, v = q.detach().contiguous(), strided_rows(k.detach()), strided_rows(v.detach())
        bias = None if bias is None else bias.detach().contiguous()
        M, S = nb.rows.shape
        out = torch.empty_like(q)
        P = torch.empty((M, S, H), dtype=torch.float32, device=q.device)
        if M > 0:
            neighbor_attention_into(q, k, v, nb, H, scale, bias, out, P)
        ctx.save_for_backward(q, k, v, P)
        ctx.nb, ctx.geom = nb, (H, scale)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_output):
        q, k, v, P = ctx.saved_tensors
        nb, (H, scale) = ctx.nb, ctx.geom
        d_out = _grad_out("neighbor_attention", grad_output, q)
        with torch.cuda.device(q.device):
            dq, dbias = torch.empty_like(q), torch.empty_like(P)
            dk = dv = None
            fill = False
            if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
                (dk, fill), (dv, _) = _row_grad(k, nb), _row_grad(v, nb)
            if q.shape[0] > 0:
                neighbor_attention_bwd_into(q, k, v, nb, H, scale, P, d_out, dq, dk if fill else None,
                                            dv if fill else None, dbias)
        return dq, dk, dv, (dbias if ctx.needs_input_grad[3] else None), None, None, None


class NeighborAggregateFunction(Function):
    """spx_neighbor_attn_fwd / _bwd in their aggregate mode: gradients to w and v."""

    @staticmethod
    def forward(ctx, w, v, nb):
        w, v = w.detach().contiguous(), strided_rows(v.detach())
        out = torch.empty((int(w.shape[0]), int(v.shape[1])), dtype=v.dtype, device=v.device)
        if w.shape[0] > 0:
            neighbor_aggregate_into(w, v, nb, out)
        ctx.save_for_backward(w, v)
        ctx.nb = nb
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_output):
        w, v = ctx.saved_tensors
        nb = ctx.nb
        d_out = _grad_out("neighbor_aggregate", grad_output, v)
        with torch.cuda.device(v.device):
            dw = torch.empty_like(w) if ctx.needs_input_grad[0] else None
            dv, fill = _row_grad(v, nb) if ctx.needs_input_grad[1] else (None, False)
            if w.shape[0] > 0 and (dw is not None or fill):
                neighbor_aggregate_bwd_into(w, v, nb, d_out, dw, dv if fill else None)
        return dw, dv, None


def _needs_groups(op: str, rows_need_grad: bool, nb: VoxelNeighbors) -> None:
    if rows_need_grad and nb.groups is None and nb.rows.numel() > 0 and nb.num_voxels > 0:
        raise groups_missing(op, "neighbour", "the query")


def neighbor_attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, nb: VoxelNeighbors, num_heads: int,
                       scale: Optional[float] = None, bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Multi-head attention of every query over its own neighbours, on the kernels of csrc/nattn.hip.  q [M, C]: the
    queries' features; k, v [nb.num_voxels, C]: rows of the level (``voxel_query``) or of the point set (``ball_query``,
    ``PointKNN.neighbors()``), which may be row-strided views with a contiguous last dimension (the halves of one
    Linear(C, 2C) output are read in place); nb: the ``VoxelNeighbors`` table, rows [M, S]; H = num_heads, D = C / H in
    {8, 16, 32, 64, 128}, C <= 512; float16, bfloat16 or float32 -- float64 is refused, nothing is cast, not under
    autocast either.  Slot (m, s) is a key iff ``0 <= rows[m, s] < live`` (live = min(*nb.n_live, num_voxels)): the rule
    of ``group_voxels``.  It looks at the value in the slot only, so duplicates count: a ``pad="first"`` table counts
    slot 0 once more per padded slot -- query with ``pad="none"``.  Per head, ``x[m, s] = scale * q[m, h] . k[rows[m, s],
    h] + bias[m, s, h]`` (scale defaults to D ** -0.5; bias: optional float32 [M, S, H], the place of contextual and
    relative position terms), P = softmax of x over the key slots in fp32, ``out[m, h] = sum_s P[m, s] v[rows[m, s],
    h]``.  Returns out [M, C], written whole; a query without a key gets +0.  Differentiable in q, k, v and bias (the
    gradient of bias is dS, float32, +0 at slots that are no keys); k and v take theirs over ``nb.groups`` -- build the
    table with with_groups=True -- in ascending entry without atomics: identical run to run.  No gradient to
    coordinates.  Nothing is read back.

    Not built: dropout, float64, head sizes outside the list."""
    M, S, H, D, scale = check_attention(q, k, v, nb, num_heads, scale, bias)
    grad = torch.is_grad_enabled()
    _needs_groups("neighbor_attention", grad and (k.requires_grad or v.requires_grad), nb)
    with torch.cuda.device(q.device):
        if grad and (q.requires_grad or k.requires_grad or v.requires_grad or (bias is not None and bias.requires_grad)):
            return NeighborAttentionFunction.apply(q, k, v, bias, nb, H, scale)
        q, out = q.detach().contiguous(), torch.empty((M, H * D), dtype=q.dtype, device=q.device)
        if M > 0:
            neighbor_attention_into(q, strided_rows(k.detach()), strided_rows(v.detach()), nb, H, scale,
                                    None if bias is None else bias.detach().contiguous(), out, None)
        return out


def neighbor_aggregate(w: torch.Tensor, v: torch.Tensor, nb: VoxelNeighbors) -> torch.Tensor:
    """``out[m, g] = sum over the key slots of w[m, s, g] * v[rows[m, s], g]``: the ``aggregation`` of pointops, the last
    step of Point Transformer v1 / v2's grouped vector attention (its softmax and weight MLP stay with the caller).
    w [M, S, G] in v's dtype or float32, v [nb.num_voxels, C] (row-strided views are read in place), C % G == 0 and
    C / G in {8, 16, 32, 64, 128}, C <= 512; float16, bfloat16 or float32.  Key slots are those of
    ``neighbor_attention``; fp32 accumulation in ascending slot, one rounding; a query without a key gets +0.
    Differentiable in w (``dw[m, s, g] = d_out[m, g] . v[rows[m, s], g]``, +0 at slots that are no keys) and in v (over
    ``nb.groups``, no atomics: identical run to run)."""
    M, S, G, D = check_aggregate(w, v, nb)
    grad = torch.is_grad_enabled()
    _needs_groups("neighbor_aggregate", grad and v.requires_grad, nb)
    with torch.cuda.device(v.device):
        if grad and (w.requires_grad or v.requires_grad):
            return NeighborAggregateFunction.apply(w, v, nb)
        out = torch.empty((M, G * D), dtype=v.dtype, device=v.device)
        if M > 0:
            neighbor_aggregate_into(w.detach().contiguous(), strided_rows(v.detach()), nb, out)
        return out
