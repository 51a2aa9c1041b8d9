"""Serialised patch attention on the MFMA kernels of csrc/attn.hip (``functional.patch_attention``): the attention of
Point Transformer V3, OctFormer and FlatFormer-style blocks over the patches of a ``PatchPlan``, read through the plan
from the row-ordered ``qkv`` of a ``Linear(C, 3C)`` -- what PTv3 hands to ``flash_attn_varlen_qkvpacked_func``.  Not part
of the reference.  There is no composite to fall back to.

  * ``fwd``  two launches (``spx_patch_attn_fwd``): out [n, H * D] in row order, and the log-sum-exp of every query slot
  * ``bwd``  four launches (``spx_patch_attn_bwd``): delta, dQ, dK / dV per slot in fp32, the rows; no atomics

With ``rel_bias`` (Point Transformer V3's relative position encoding) the calls go to ``spx_patch_attn_bias_fwd`` /
``_bwd``: the BIAS instances of the kernels; in the backward a first walk of the dQ kernel takes delta = sum P dP in
place of the delta launch, and a fifth launch adds the workgroups' partial tables to the table's gradient.

Not built: dropout, cross-attention, fp32 / fp64 kernels, a returned log-sum-exp, bias tables in 16 bits.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from spconv_amd import _lib
from spconv_amd.pytorch._rulebook import _require_gpu, _stream, _ws
from spconv_amd.pytorch._serialize import PatchPlan, check_plan

HEAD_SIZES = (16, 32, 64)
_CODES = {torch.float16: _lib.DTYPE_F16, torch.bfloat16: _lib.DTYPE_BF16}


def check(qkv: torch.Tensor, plan: PatchPlan, num_heads: int, scale: Optional[float]) -> Tuple[int, int, float]:
    """(H, D, scale) of a patch_attention call; everything that can be refused is refused before a kernel runs."""
    op = "patch_attention"
    H = int(num_heads)
    if H != num_heads or H < 1:
        raise ValueError(f"{op}: num_heads must be an integer >= 1, got {num_heads!r}")
    if qkv.dim() == 2 and qkv.shape[1] % (3 * H) == 0 and qkv.shape[1] > 0:
        D = int(qkv.shape[1]) // (3 * H)
    elif qkv.dim() == 4 and qkv.shape[1] == 3 and qkv.shape[2] == H:
        D = int(qkv.shape[3])
    else:
        raise ValueError(f"{op}: qkv is [n, 3 * H * D] or [n, 3, H, D] with H = {H}, got {tuple(qkv.shape)}")
    if D not in HEAD_SIZES:
        raise NotImplementedError(f"{op}: the head size must be one of {list(HEAD_SIZES)}, got {D}")
    if int(plan.patch_size) % 32 != 0 or int(plan.patch_size) < 32:
        raise ValueError(f"{op}: patch_size must be a multiple of 32, got {plan.patch_size}")
    if qkv.dtype not in _CODES:
        raise NotImplementedError(f"{op}: qkv must be float16 or bfloat16 (nothing is cast), got {qkv.dtype}")
    check_plan(plan, qkv, op)
    if tuple(plan.patch_rows.shape)[1:] != (int(plan.patch_size),):
        raise ValueError(f"{op}: the plan's patch_rows is [P_cap, {plan.patch_size}], got {tuple(plan.patch_rows.shape)}")
    if plan.n_patches_dev.dtype != torch.int32 or plan.n_patches_dev.numel() < 1 or plan.n_patches_dev.device != qkv.device:
        raise ValueError(f"{op}: the plan's n_patches_dev is an int32 tensor of one element on the rows' device")
    n = int(plan.row_slot.shape[0])
    if int(qkv.shape[0]) != n:
        raise ValueError(f"{op}: one row per voxel ({n}), got {tuple(qkv.shape)}")
    if not qkv.is_contiguous():
        raise ValueError(f"{op}: qkv must be contiguous")
    _require_gpu(qkv, "qkv")
    return H, D, float(D ** -0.5 if scale is None else scale)


def default_pos_bnd(patch_size: int) -> int:
    """Point Transformer V3's bound of the relative position, computed exactly as its RPE computes it"""
    return int((4 * patch_size) ** (1 / 3) * 2)


def check_bias(qkv: torch.Tensor, plan: PatchPlan, H: int, rel_bias, coords, pos_bnd) -> int:
    """pos_bnd of a biased call; the table and the coordinates are refused, never cast."""
    op = "patch_attention"
    if rel_bias is None or coords is None:
        raise ValueError(f"{op}: rel_bias and coords come together (coords is normally x.indices[:, 1:])")
    pb = default_pos_bnd(int(plan.patch_size)) if pos_bnd is None else pos_bnd
    if not isinstance(pb, int) or isinstance(pb, bool) or not 1 <= pb <= 63:
        raise ValueError(f"{op}: pos_bnd must be an integer in 1 .. 63, got {pb!r}")
    n = int(qkv.shape[0])
    if rel_bias.dtype != torch.float32 or tuple(rel_bias.shape) != (3 * (2 * pb + 1), H):
        raise ValueError(f"{op}: rel_bias must be float32 [3 * (2 * pos_bnd + 1), H] = [{3 * (2 * pb + 1)}, {H}] (nothing "
                         f"is cast), got {rel_bias.dtype} {tuple(rel_bias.shape)}")
    if coords.dtype != torch.int32 or tuple(coords.shape) != (n, 3) or coords.device != qkv.device:
        raise ValueError(f"{op}: coords must be int32 [n, 3] = [{n}, 3] on the rows' device (nothing is cast), got "
                         f"{coords.dtype} {tuple(coords.shape)} on {coords.device}")
    if rel_bias.device != qkv.device:
        raise ValueError(f"{op}: rel_bias must be on the rows' device, got {rel_bias.device}")
    if coords.requires_grad:
        raise ValueError(f"{op}: coords takes no gradient")
    return pb


def _tables(plan: PatchPlan):
    return (plan.patch_rows.data_ptr(), plan.patch_rows_canon.data_ptr(), plan.row_slot.data_ptr())


def fwd(qkv: torch.Tensor, plan: PatchPlan, H: int, D: int, scale: float):
    """(out [n, H * D], lse fp32 [P_cap * K, H])"""
    P_cap, K = (int(v) for v in plan.patch_rows.shape)
    n, dev = int(qkv.shape[0]), qkv.device
    with torch.cuda.device(dev):
        out = torch.empty((n, H * D), dtype=qkv.dtype, device=dev)
        lse = torch.empty((P_cap * K, H), dtype=torch.float32, device=dev)
        if n > 0:
            _lib.check(_lib.load().spx_patch_attn_fwd(qkv.data_ptr(), *_tables(plan), plan.n_patches_dev.data_ptr(), n,
                                                      P_cap, K, H, D, _CODES[qkv.dtype], scale, out.data_ptr(),
                                                      lse.data_ptr(), _stream(qkv)))
    return out, lse


def bwd(qkv: torch.Tensor, out: torch.Tensor, lse: torch.Tensor, d_out: torch.Tensor, plan: PatchPlan, H: int, D: int,
        scale: float) -> torch.Tensor:
    """dqkv in qkv's shape and dtype, zeros for dead rows"""
    P_cap, K = (int(v) for v in plan.patch_rows.shape)
    n, dev = int(qkv.shape[0]), qkv.device
    if d_out.dtype != qkv.dtype:
        raise NotImplementedError(f"patch_attention: the gradient arrives as {d_out.dtype}, the rows are {qkv.dtype}")
    d_out = d_out.contiguous()
    L = _lib.load()
    with torch.cuda.device(dev):
        dqkv = torch.empty_like(qkv)
        if n > 0:
            ws = _ws(int(L.spx_patch_attn_ws_bytes(n, P_cap, K, H, D)), dev)
            _lib.check(L.spx_patch_attn_bwd(qkv.data_ptr(), out.data_ptr(), lse.data_ptr(), d_out.data_ptr(), *_tables(plan),
                                            plan.row_slot2.data_ptr(), plan.n_patches_dev.data_ptr(), n, P_cap, K, H, D,
                                            _CODES[qkv.dtype], scale, dqkv.data_ptr(), ws.data_ptr(), ws.numel(),
                                            _stream(qkv)))
    return dqkv


def fwd_bias(qkv: torch.Tensor, plan: PatchPlan, H: int, D: int, scale: float, rel_bias: torch.Tensor, coords: torch.Tensor,
             pos_bnd: int):
    """(out, lse) of the biased forward; rel_bias and coords contiguous"""
    P_cap, K = (int(v) for v in plan.patch_rows.shape)
    n, dev = int(qkv.shape[0]), qkv.device
    with torch.cuda.device(dev):
        out = torch.empty((n, H * D), dtype=qkv.dtype, device=dev)
        lse = torch.empty((P_cap * K, H), dtype=torch.float32, device=dev)
        if n > 0:
            _lib.check(_lib.load().spx_patch_attn_bias_fwd(
                qkv.data_ptr(), *_tables(plan), plan.n_patches_dev.data_ptr(), rel_bias.data_ptr(), coords.data_ptr(), n,
                P_cap, K, H, D, _CODES[qkv.dtype], scale, pos_bnd, out.data_ptr(), lse.data_ptr(), _stream(qkv)))
    return out, lse


def bwd_bias(qkv: torch.Tensor, out: torch.Tensor, lse: torch.Tensor, d_out: torch.Tensor, plan: PatchPlan, H: int, D: int,
             scale: float, rel_bias: torch.Tensor, coords: torch.Tensor, pos_bnd: int):
    """(dqkv, d_rel_bias fp32 in the table's shape, written whole)"""
    P_cap, K = (int(v) for v in plan.patch_rows.shape)
    n, dev = int(qkv.shape[0]), qkv.device
    if d_out.dtype != qkv.dtype:
        raise NotImplementedError(f"patch_attention: the gradient arrives as {d_out.dtype}, the rows are {qkv.dtype}")
    d_out = d_out.contiguous()
    L = _lib.load()
    with torch.cuda.device(dev):
        dqkv = torch.empty_like(qkv)
        if n == 0:
            return dqkv, torch.zeros_like(rel_bias)
        d_table = torch.empty_like(rel_bias)
        ws = _ws(int(L.spx_patch_attn_ws_bytes(n, P_cap, K, H, D)), dev)
        part = _ws(int(L.spx_patch_attn_bias_ws_bytes(P_cap, K, H, D, pos_bnd)), dev)
        _lib.check(L.spx_patch_attn_bias_bwd(
            qkv.data_ptr(), out.data_ptr(), lse.data_ptr(), d_out.data_ptr(), *_tables(plan), plan.row_slot2.data_ptr(),
            plan.n_patches_dev.data_ptr(), rel_bias.data_ptr(), coords.data_ptr(), n, P_cap, K, H, D, _CODES[qkv.dtype],
            scale, pos_bnd, dqkv.data_ptr(), d_table.data_ptr(), ws.data_ptr(), ws.numel(), part.data_ptr(), part.numel(),
            _stream(qkv)))
    return dqkv, d_table
