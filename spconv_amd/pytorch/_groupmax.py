"""Fused set abstraction on the MFMA kernels of csrc/groupmax.hip (``functional.group_linear_max``,
``spatial.GroupLinearMax``): gather through a ``VoxelNeighbors`` table, add a position term, ReLU, one linear layer and
the max over the samples -- the body of PointNet++'s SA layer, pointnet2_stack's ``StackSAModuleMSG`` and Voxel R-CNN's
grouped MLP, without the grouped [M, S, Cin] tensor.  Not part of the reference.

  * forward   two launches (``spx_group_linear_max_fwd``: the weight into fragment order, the op).  With a gradient
              ahead it keeps ``arg`` (uint8 [M, Cout], the slot of every maximum) and nothing else
  * backward  the query side (``spx_group_linear_max_bwd``, one launch: dG [M, S, Cin], the one grouped tensor, and the
              fp32 partials of dpos_weight / din_bias) and ``spx_group_bwd`` for dfeats; the weight side (fp32 partials
              per chunk of queries); one launch adds both kinds of partials in a fixed order.  x is recomputed from the
              table.  No atomics, identical run to run

The ``_into`` forms take buffers the caller owns, allocate nothing and read nothing back: they can sit inside a captured
graph behind the query and its groups.  There is no composite to fall back to.

Not built: a training-mode BatchNorm over the grouped pre-activations, more than one linear layer, the weight-less form,
mean / sum pooling, float32 / float64, gradients in offsets or coordinates.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from spconv_amd import _lib
from spconv_amd.pytorch._level import groups_missing
from spconv_amd.pytorch._query import MAX_NSAMPLE, VoxelNeighbors
from spconv_amd.pytorch._rulebook import _ptr, _require_gpu, _stream, _ws

MAX_CHANNELS = 256
_CODES = {torch.float16: _lib.DTYPE_F16, torch.bfloat16: _lib.DTYPE_BF16}
_FWD_ROWS = torch.amp.custom_fwd(device_type="cuda")        # casts nothing: the rows keep their dtype under autocast
_BWD = torch.amp.custom_bwd(device_type="cuda")


def _channels(name: str, C: int) -> None:
    if not (16 <= C <= MAX_CHANNELS and C % 16 == 0):
        raise NotImplementedError(f"group_linear_max: {name} must be a multiple of 16 in 16 .. {MAX_CHANNELS}, got {C}")


def check(feats: torch.Tensor, nb: VoxelNeighbors, weight: torch.Tensor, pos_weight: Optional[torch.Tensor],
          in_bias: Optional[torch.Tensor]) -> Tuple[int, int, int, int]:
    """(M, S, Cin, Cout) of a group_linear_max call; everything that can be refused is refused before a kernel runs, and
    before the refusal of CPU tensors (``check_devices``)"""
    if feats.dtype not in _CODES:
        raise NotImplementedError(f"group_linear_max: feats must be float16 or bfloat16 (nothing is cast), got {feats.dtype}")
    if feats.dim() != 2 or int(feats.shape[0]) != nb.num_voxels:
        raise ValueError(f"group_linear_max: feats holds one row per voxel or point of the table ([{nb.num_voxels}, Cin]), "
                         f"got {tuple(feats.shape)}")
    Cin = int(feats.shape[1])
    _channels("Cin (feats)", Cin)
    if weight.dim() != 2 or int(weight.shape[0]) != Cin or weight.dtype != feats.dtype:
        raise ValueError(f"group_linear_max: weight is [Cin, Cout] = [{Cin}, Cout] of {feats.dtype} (nothing is cast), got "
                         f"{tuple(weight.shape)} {weight.dtype}")
    Cout = int(weight.shape[1])
    _channels("Cout (weight)", Cout)
    rows, offsets = nb.rows, nb.offsets
    if rows.dim() != 2 or rows.dtype != torch.int32 or not rows.is_contiguous():
        raise ValueError(f"group_linear_max: nb.rows is a contiguous int32 tensor [M, nsample], got {tuple(rows.shape)} "
                         f"{rows.dtype}")
    M, S = (int(v) for v in rows.shape)
    if not 1 <= S <= MAX_NSAMPLE:
        raise ValueError(f"group_linear_max: nsample (nb.rows) must be in 1 .. {MAX_NSAMPLE}, got {S}")
    if pos_weight is not None:
        if pos_weight.dtype != torch.float32 or tuple(pos_weight.shape) != (3, Cin):
            raise ValueError(f"group_linear_max: pos_weight is float32 [3, Cin] = [3, {Cin}], got {pos_weight.dtype} "
                             f"{tuple(pos_weight.shape)}")
        if offsets is None:
            raise ValueError("group_linear_max: pos_weight needs nb.offsets; build the table with with_offsets=True")
        if offsets.dtype != torch.float32 or tuple(offsets.shape) != (M, S, 3) or not offsets.is_contiguous():
            raise ValueError(f"group_linear_max: nb.offsets is a contiguous float32 tensor [M, nsample, 3] = [{M}, {S}, 3], "
                             f"got {offsets.dtype} {tuple(offsets.shape)}")
    if in_bias is not None and (in_bias.dtype != torch.float32 or tuple(in_bias.shape) != (Cin,)):
        raise ValueError(f"group_linear_max: in_bias is float32 [Cin] = [{Cin}], got {in_bias.dtype} {tuple(in_bias.shape)}")
    return M, S, Cin, Cout


def check_devices(feats, nb: VoxelNeighbors, weight, pos_weight, in_bias) -> None:
    for name, t in (("feats", feats), ("weight", weight), ("pos_weight", pos_weight), ("in_bias", in_bias),
                    ("nb.rows", nb.rows), ("nb.offsets", nb.offsets if pos_weight is not None else None)):
        if t is None:
            continue
        _require_gpu(t, name)
        if t.device != feats.device:
            raise ValueError(f"group_linear_max: {name} is on {t.device}, feats on {feats.device}")


def group_linear_max_ws_bytes(M: int, S: int, Cin: int, Cout: int, backward: bool = False) -> int:
    """bytes of the workspace of ``group_linear_max_into`` (the weight in fragment order) or, with backward, of
    ``group_linear_max_bwd_into`` with a dweight, dpos_weight or din_bias (the fp32 partials)"""
    return int(_lib.load().spx_group_linear_max_ws_bytes(int(M), int(S), int(Cin), int(Cout), int(bool(backward))))


def group_linear_max_into(feats: torch.Tensor, nb: VoxelNeighbors, weight: torch.Tensor, pos_weight: Optional[torch.Tensor],
                          in_bias: Optional[torch.Tensor], relu_in: bool, out: torch.Tensor, arg: Optional[torch.Tensor],
                          ws: torch.Tensor) -> None:
    """The forward's one C call into buffers the caller owns (no allocation: capturable).  feats [n, Cin], weight [Cin,
    Cout], out [M, Cout] contiguous; arg uint8 [M, Cout] (what ``group_linear_max_bwd_into`` reads; None when no gradient
    follows); ws: uint8, ``group_linear_max_ws_bytes(M, S, Cin, Cout)``."""
    (M, S), (Cin, Cout) = nb.rows.shape, weight.shape
    _lib.check(_lib.load().spx_group_linear_max_fwd(
        feats.data_ptr(), nb.rows.data_ptr(), _ptr(nb.offsets if pos_weight is not None else None), weight.data_ptr(),
        _ptr(pos_weight), _ptr(in_bias), int(M), int(S), int(nb.num_voxels), _ptr(nb.n_queries), _ptr(nb.n_live), int(Cin),
        int(Cout), _CODES[feats.dtype], int(bool(relu_in)), out.data_ptr(), _ptr(arg), ws.data_ptr(), ws.numel(),
        _stream(feats)))


def group_linear_max_bwd_into(feats: torch.Tensor, nb: VoxelNeighbors, weight: torch.Tensor,
                              pos_weight: Optional[torch.Tensor], in_bias: Optional[torch.Tensor], relu_in: bool,
                              arg: torch.Tensor, d_out: torch.Tensor, dg: Optional[torch.Tensor],
                              dfeats: Optional[torch.Tensor], dweight: Optional[torch.Tensor],
                              dpos_weight: Optional[torch.Tensor], din_bias: Optional[torch.Tensor],
                              ws: Optional[torch.Tensor]) -> None:
    """The backward into buffers the caller owns.  arg as the forward left it.  dg [M, S, Cin] and dfeats [n, Cin] come
    together (or both None): the query side writes dg, ``spx_group_bwd`` sums it over ``nb.groups`` into dfeats.  dweight
    [Cin, Cout] in the rows' dtype, dpos_weight float32 [3, Cin], din_bias float32 [Cin]: each or None; any of them needs
    ws of ``group_linear_max_ws_bytes(.., backward=True)``."""
    (M, S), (Cin, Cout) = nb.rows.shape, weight.shape
    g = nb.groups
    if dfeats is not None and (dg is None or g is None or g.offsets is None):
        raise groups_missing("group_linear_max", "neighbour", "the query")
    lib = _lib.load()
    _lib.check(lib.spx_group_linear_max_bwd(
        feats.data_ptr(), nb.rows.data_ptr(), _ptr(nb.offsets if pos_weight is not None else None), weight.data_ptr(),
        _ptr(pos_weight), _ptr(in_bias), arg.data_ptr(), d_out.data_ptr(), int(M), int(S), int(nb.num_voxels),
        _ptr(nb.n_queries), _ptr(nb.n_live), int(Cin), int(Cout), _CODES[weight.dtype], int(bool(relu_in)),
        _ptr(dg if dfeats is not None else None), _ptr(dweight), _ptr(dpos_weight), _ptr(din_bias), _ptr(ws),
        0 if ws is None else ws.numel(), _stream(d_out)))
    if dfeats is not None:
        _lib.check(lib.spx_group_bwd(dg.data_ptr(), int(M), int(S), g.offsets.data_ptr(), g.list.data_ptr(),
                                     int(nb.num_voxels), _ptr(nb.n_live), int(Cin), _CODES[weight.dtype], dfeats.data_ptr(),
                                     _stream(d_out)))


class GroupLinearMaxFunction(Function):
    """spx_group_linear_max_fwd / _bwd: gradients to feats, weight, pos_weight and in_bias, none to the offsets or the
    table.  Casts nothing under autocast."""

    @staticmethod
    @_FWD_ROWS
    def forward(ctx, feats, weight, pos_weight, in_bias, nb, relu_in):
        feats, weight = feats.detach().contiguous(), weight.detach().contiguous()
        pos_weight = None if pos_weight is None else pos_weight.detach().contiguous()
        in_bias = None if in_bias is None else in_bias.detach().contiguous()
        (M, S), (Cin, Cout), dev = nb.rows.shape, weight.shape, feats.device
        out = torch.empty((M, Cout), dtype=feats.dtype, device=dev)
        arg = torch.empty((M, Cout), dtype=torch.uint8, device=dev)
        if M > 0:
            group_linear_max_into(feats, nb, weight, pos_weight, in_bias, relu_in, out, arg,
                                  _ws(group_linear_max_ws_bytes(M, S, Cin, Cout), dev))
        ctx.save_for_backward(feats, weight, pos_weight, in_bias, arg)
        ctx.nb, ctx.relu_in = nb, relu_in
        return out

    @staticmethod
    @once_differentiable
    @_BWD
    def backward(ctx, grad_output):
        feats, weight, pos_weight, in_bias, arg = ctx.saved_tensors
        nb, relu_in = ctx.nb, ctx.relu_in
        if grad_output.dtype != weight.dtype:
            raise NotImplementedError(f"group_linear_max: the gradient arrives as {grad_output.dtype}, the rows are "
                                      f"{weight.dtype}")
        d_out = grad_output.contiguous()
        (M, S), (Cin, Cout), n, dev = nb.rows.shape, weight.shape, nb.num_voxels, d_out.device
        need = ctx.needs_input_grad
        with torch.cuda.device(dev):
            dfeats = dweight = dpos = dbias = dg = ws = None
            new = torch.empty if M > 0 else torch.zeros
            if need[0]:
                fill = M > 0 and n > 0
                dfeats = (torch.empty if fill else torch.zeros)((n, Cin), dtype=weight.dtype, device=dev)
                dg = torch.empty((M, S, Cin), dtype=weight.dtype, device=dev) if fill else None
            if need[1]:
                dweight = new((Cin, Cout), dtype=weight.dtype, device=dev)
            if need[2] and pos_weight is not None:
                dpos = new((3, Cin), dtype=torch.float32, device=dev)
            if need[3] and in_bias is not None:
                dbias = new((Cin,), dtype=torch.float32, device=dev)
            if dweight is not None or dpos is not None or dbias is not None:
                ws = _ws(group_linear_max_ws_bytes(M, S, Cin, Cout, True), dev)
            if M > 0:
                group_linear_max_bwd_into(feats, nb, weight, pos_weight, in_bias, relu_in, arg, d_out, dg,
                                          dfeats if dg is not None else None, dweight, dpos, dbias, ws)
        return dfeats, dweight, dpos, dbias, None, None


def group_linear_max(feats: torch.Tensor, nb: VoxelNeighbors, weight: torch.Tensor,
                     pos_weight: Optional[torch.Tensor] = None, in_bias: Optional[torch.Tensor] = None,
                     relu_in: bool = True) -> torch.Tensor:
    """Gather, position term, ReLU, linear layer and max over the samples in one op, on the MFMA kernels of
    csrc/groupmax.hip.  feats [nb.num_voxels, Cin]: rows of the level or of the point set, float16 or bfloat16 -- float32
    / float64 are refused, nothing is cast, not under autocast either; nb: a ``VoxelNeighbors`` table, S = nsample in 1 ..
    128; weight [Cin, Cout] in feats' dtype, Cin and Cout multiples of 16 in 16 .. 256; pos_weight float32 [3, Cin] or
    None (needs nb.offsets, float32 [M, S, 3]: ``with_offsets=True``); in_bias float32 [Cin] or None.  Slot (m, s) is
    valid iff ``0 <= rows[m, s] < live`` and ``m < *nb.n_queries``: the rule of ``group_voxels``, so ``pad="first"``
    duplicates count.

    ``x[m, s, c] = feats[rows[m, s], c] + sum_d offsets[m, s, d] pos_weight[d, c] + in_bias[c]`` in fp32, with relu_in
    ``max(x, 0)``, rounded to the dtype once; ``y[m, s] = x[m, s] @ weight`` summed in fp32; ``out[m, co]`` the maximum
    of y over the valid slots, rounded once.  Returns out [M, Cout], written whole: a query without a valid slot, or at or
    beyond *nb.n_queries, gets +0.  No [M, S, Cin] tensor exists in the forward.  The first layer of a shared MLP
    commutes with the gather and belongs on the n rows in front of this op; an eval-mode BatchNorm behind the linear layer
    folds in (its scale into the columns of weight, its shift and a ReLU behind the max on [M, Cout]).  A training-mode
    BatchNorm over the grouped pre-activations y is NOT served: its statistics and gradient span all M x S entries; such
    a model keeps the composite for that layer or normalises after the pool.

    Differentiable in feats (over ``nb.groups`` -- build the table with with_groups=True -- through one grouped tensor,
    dG [M, S, Cin] in the rows' dtype), weight, pos_weight and in_bias; the gradient goes to the lowest slot that attains
    the fp32 maximum.  The forward keeps M x Cout bytes for it.  No atomics: identical run to run.  No gradient to the
    offsets.  Nothing is read back."""
    M, S, Cin, Cout = check(feats, nb, weight, pos_weight, in_bias)
    grad = torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (feats, weight, pos_weight, in_bias))
    if grad and feats.requires_grad and nb.groups is None and nb.rows.numel() > 0 and nb.num_voxels > 0:
        raise groups_missing("group_linear_max", "neighbour", "the query")
    check_devices(feats, nb, weight, pos_weight, in_bias)
    with torch.cuda.device(feats.device):
        if grad:
            return GroupLinearMaxFunction.apply(feats, weight, pos_weight, in_bias, nb, bool(relu_in))
        out = torch.empty((M, Cout), dtype=feats.dtype, device=feats.device)
        if M > 0:
            group_linear_max_into(feats.detach().contiguous(), nb, weight.detach().contiguous(),
                                  None if pos_weight is None else pos_weight.detach().contiguous(),
                                  None if in_bias is None else in_bias.detach().contiguous(), bool(relu_in), out, None,
                                  _ws(group_linear_max_ws_bytes(M, S, Cin, Cout), feats.device))
        return out
