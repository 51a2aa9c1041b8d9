"""autograd glue (reference: spconv/pytorch/functional.py:59-429).

``SparseConvFunction`` / ``SparseInverseConvFunction`` / ``SubMConvFunction`` /
``SparseImplicitGemmFunction`` keep the reference's argument lists so user code
calling ``Fsp.indice_subm_conv(...)`` etc. keeps working; all of them save
(features, filters, rulebook tensors) and return ``(din, dW, None...)``.
AMP: inputs are cast to fp16 under autocast like the reference
(functional.py:44-56).
"""
from __future__ import annotations

import sys
from typing import List, Optional

import numpy as np
import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from spconv_amd.pytorch import ops

import torch.amp as _amp

_FWD = _amp.custom_fwd(device_type="cuda", cast_inputs=torch.float16)
_BWD = _amp.custom_bwd(device_type="cuda")


def _report(tag: str, **shapes) -> None:
    msg = f"[Exception|{tag}]" + ",".join(f"{k}={v}" for k, v in shapes.items())
    print(msg, file=sys.stderr)


class _NativeConvBase(Function):
    """Shared body of the three ConvAlgo.Native functions."""
    _inverse = False
    _subm = False

    @classmethod
    def _forward(cls, ctx, features, filters, indice_pairs, indice_pair_num, num_activate_out,
                 algo, timer, bias, act_alpha, act_beta, act_type):
        ctx.save_for_backward(indice_pairs, indice_pair_num, features, filters)
        ctx.algo = algo
        # tensors lose python attributes through save_for_backward; keep the rulebook here
        ctx.rulebook = ops.rulebook_of(indice_pairs)
        try:
            return ops.indice_conv(features, filters, indice_pairs, indice_pair_num,
                                   num_activate_out, cls._inverse, cls._subm, algo=algo,
                                   timer=timer, bias=bias, act_alpha=act_alpha,
                                   act_beta=act_beta, act_type=act_type)
        except Exception:
            _report("indice_conv", feat=features.shape, w=filters.shape, pair=indice_pairs.shape,
                    act=num_activate_out, algo=algo)
            raise

    @classmethod
    def _backward(cls, ctx, grad_output):
        indice_pairs, indice_pair_num, features, filters = ctx.saved_tensors
        if ctx.rulebook is not None:
            ops.attach_rulebook(indice_pairs, ctx.rulebook)
        try:
            din, dw = ops.indice_conv_backward(features, filters, grad_output, indice_pairs,
                                               indice_pair_num, cls._inverse, cls._subm,
                                               algo=ctx.algo, need_din=ctx.needs_input_grad[0])
        except Exception:
            _report("indice_conv_backward", feat=features.shape, w=filters.shape,
                    pair=indice_pairs.shape, do=grad_output.shape)
            raise
        return (din, dw) + (None,) * 9


class SparseConvFunction(_NativeConvBase):
    @staticmethod
    @_FWD
    def forward(ctx, features, filters, indice_pairs, indice_pair_num, num_activate_out, algo,
                timer=None, bias: Optional[torch.Tensor] = None, act_alpha: float = 0.0,
                act_beta: float = 0.0, act_type=ops.Activation.None_):
        return SparseConvFunction._forward(ctx, features, filters, indice_pairs, indice_pair_num,
                                           num_activate_out, algo, timer, bias, act_alpha,
                                           act_beta, act_type)

    @staticmethod
    @once_differentiable
    @_BWD
    def backward(ctx, grad_output):
        return SparseConvFunction._backward(ctx, grad_output)


class SparseInverseConvFunction(_NativeConvBase):
    _inverse = True

    @staticmethod
    @_FWD
    def forward(ctx, features, filters, indice_pairs, indice_pair_num, num_activate_out, algo,
                timer=None, bias: Optional[torch.Tensor] = None, act_alpha: float = 0.0,
                act_beta: float = 0.0, act_type=ops.Activation.None_):
        return SparseInverseConvFunction._forward(ctx, features, filters, indice_pairs,
                                                  indice_pair_num, num_activate_out, algo, timer,
                                                  bias, act_alpha, act_beta, act_type)

    @staticmethod
    @once_differentiable
    @_BWD
    def backward(ctx, grad_output):
        return SparseInverseConvFunction._backward(ctx, grad_output)


class SubMConvFunction(_NativeConvBase):
    _subm = True

    @staticmethod
    @_FWD
    def forward(ctx, features, filters, indice_pairs, indice_pair_num, num_activate_out, algo,
                timer=None, bias: Optional[torch.Tensor] = None, act_alpha: float = 0.0,
                act_beta: float = 0.0, act_type=ops.Activation.None_):
        return SubMConvFunction._forward(ctx, features, filters, indice_pairs, indice_pair_num,
                                         num_activate_out, algo, timer, bias, act_alpha, act_beta,
                                         act_type)

    @staticmethod
    @once_differentiable
    @_BWD
    def backward(ctx, grad_output):
        return SubMConvFunction._backward(ctx, grad_output)


class SparseImplicitGemmFunction(Function):
    @staticmethod
    @_FWD
    def forward(ctx, features: torch.Tensor, filters: torch.Tensor, pair_fwd: torch.Tensor,
                pair_bwd: torch.Tensor, pair_mask_fwd_splits: List[torch.Tensor],
                pair_mask_bwd_splits: List[torch.Tensor],
                mask_argsort_fwd_splits: List[torch.Tensor],
                mask_argsort_bwd_splits: List[torch.Tensor], num_activate_out: int,
                masks: List[np.ndarray], is_train: bool, is_subm: bool, timer=None,
                fp32_accum: Optional[bool] = None, bias: Optional[torch.Tensor] = None,
                act_alpha: float = 0.0, act_beta: float = 0.0,
                act_type=ops.Activation.None_):
        try:
            out, mask_out, mask_width = ops.implicit_gemm(
                features, filters, pair_fwd, pair_mask_fwd_splits, mask_argsort_fwd_splits,
                num_activate_out, masks, is_train, is_subm, timer, fp32_accum, bias, act_alpha,
                act_beta, act_type)
        except Exception:
            _report("implicit_gemm", feat=features.shape, w=filters.shape, pair=pair_fwd.shape,
                    act=num_activate_out, issubm=is_subm, istrain=is_train)
            raise
        ctx.save_for_backward(features, filters, pair_fwd, pair_bwd)
        ctx.rulebook = ops.rulebook_of(pair_fwd)
        ctx.mask_width = mask_width
        ctx.mask_out = mask_out
        ctx.pair_mask_fwd_splits = pair_mask_fwd_splits
        ctx.mask_argsort_fwd_splits = mask_argsort_fwd_splits
        ctx.pair_mask_bwd_splits = pair_mask_bwd_splits
        ctx.mask_argsort_bwd_splits = mask_argsort_bwd_splits
        ctx.masks = masks
        ctx.is_subm = is_subm
        ctx.fp32_accum = fp32_accum
        return out

    @staticmethod
    @once_differentiable
    @_BWD
    def backward(ctx, grad_output):
        features, filters, pair_fwd, pair_bwd = ctx.saved_tensors
        if ctx.rulebook is not None:
            ops.attach_rulebook(pair_fwd, ctx.rulebook)
        try:
            din, dw = ops.implicit_gemm_backward(
                features, filters, grad_output, pair_fwd, pair_bwd, ctx.pair_mask_fwd_splits,
                ctx.pair_mask_bwd_splits, ctx.mask_argsort_fwd_splits,
                ctx.mask_argsort_bwd_splits, mask_output_fwd=ctx.mask_out, masks=ctx.masks,
                mask_width=ctx.mask_width, is_subm=ctx.is_subm, fp32_accum=ctx.fp32_accum,
                need_din=ctx.needs_input_grad[0])
        except Exception:
            _report("implicit_gemm_backward", feat=features.shape, w=filters.shape,
                    pair=pair_fwd.shape, issubm=ctx.is_subm, do=grad_output.shape)
            raise
        return (din, dw) + (None,) * 16


class SparseMaxPoolFunction(Function):
    """ConvAlgo.Native max pool (reference functional.py:360-377)."""
    @staticmethod
    @_FWD
    def forward(ctx, features, indice_pairs, indice_pair_num, num_activate_out):
        out = ops.indice_maxpool(features, indice_pairs, indice_pair_num, num_activate_out)
        ctx.save_for_backward(indice_pairs, indice_pair_num, features, out)
        ctx.rulebook = ops.rulebook_of(indice_pairs)
        return out

    @staticmethod
    @once_differentiable
    @_BWD
    def backward(ctx, grad_output):
        indice_pairs, indice_pair_num, features, out = ctx.saved_tensors
        if ctx.rulebook is not None:
            ops.attach_rulebook(indice_pairs, ctx.rulebook)
        input_bp = ops.indice_maxpool_backward(features, out, grad_output, indice_pairs, indice_pair_num)
        return input_bp, None, None, None


class SparseMaxPoolImplicitGemmFunction(Function):
    """reference functional.py:380-397"""
    @staticmethod
    @_FWD
    def forward(ctx, features: torch.Tensor, indice_pairs_fwd: torch.Tensor,
                indice_pairs_bwd: torch.Tensor, num_activate_out: int):
        out = ops.indice_maxpool_implicit_gemm(features, indice_pairs_fwd, num_activate_out)
        ctx.save_for_backward(indice_pairs_bwd, features, out)
        ctx.rulebook = ops.rulebook_of(indice_pairs_fwd)
        return out

    @staticmethod
    @once_differentiable
    @_BWD
    def backward(ctx, grad_output):
        indice_pairs_bwd, features, out = ctx.saved_tensors
        if ctx.rulebook is not None:
            ops.attach_rulebook(indice_pairs_bwd, ctx.rulebook)
        input_bp = ops.indice_maxpool_implicit_gemm_backward(features, out, grad_output, indice_pairs_bwd)
        return input_bp, None, None, None


class SparseAvgPoolImplicitGemmFunction(Function):
    """reference functional.py:400-420"""
    @staticmethod
    @_FWD
    def forward(ctx, features: torch.Tensor, indice_pairs_fwd: torch.Tensor,
                indice_pairs_bwd: torch.Tensor, num_activate_out: int, calc_count):
        out, count = ops.indice_avgpool_implicit_gemm(features, indice_pairs_fwd, num_activate_out,
                                                      calc_count)
        ctx.save_for_backward(indice_pairs_bwd, features, out, count)
        ctx.rulebook = ops.rulebook_of(indice_pairs_fwd)
        return out

    @staticmethod
    @once_differentiable
    @_BWD
    def backward(ctx, grad_output):
        indice_pairs_bwd, features, out, count = ctx.saved_tensors
        if ctx.rulebook is not None:
            ops.attach_rulebook(indice_pairs_bwd, ctx.rulebook)
        input_bp = ops.indice_avgpool_implicit_gemm_backward(grad_output, indice_pairs_bwd, count)
        return input_bp, None, None, None, None


indice_conv = SparseConvFunction.apply
implicit_gemm = SparseImplicitGemmFunction.apply
indice_inverse_conv = SparseInverseConvFunction.apply
indice_subm_conv = SubMConvFunction.apply
indice_maxpool = SparseMaxPoolFunction.apply
indice_maxpool_implicit_gemm = SparseMaxPoolImplicitGemmFunction.apply
indice_avgpool_implicit_gemm = SparseAvgPoolImplicitGemmFunction.apply


# ------------------------------------------------------------------ sparse add
_MAX_INT32 = 2147483647


def _indice_to_scalar(indices: torch.Tensor, shape: List[int]) -> torch.Tensor:
    """Row-major linear index of (batch, *coords) rows (reference functional.py:430-436)."""
    assert indices.shape[1] == len(shape)
    out = torch.zeros_like(indices[:, 0])
    for d, extent in enumerate(shape):
        out = out * extent + indices[:, d]
    return out.contiguous()


def _like_first(first, features, indices, indice_dict=None):
    from spconv_amd.pytorch.core import SparseConvTensor
    res = SparseConvTensor(features, indices, first.spatial_shape, first.batch_size,
                           benchmark=first.benchmark)
    if indice_dict is not None:
        res.indice_dict = indice_dict
    res.benchmark_record = first.benchmark_record
    res._timer = first._timer
    res.thrust_allocator = first.thrust_allocator
    return res


class SparseUnionAddFunction(Function):
    """Row merge of a misaligned add over the kernels of csrc/union.hip: out[r] = sum of feats[t][src[t, r]] over the
    operands present at r, in operand order, fp32 (fp64) accumulation, one rounding, one launch; rows_t is saved and
    the backward is one gather launch, din_t[i] = dout[rows_t[i]] (zeros for dead and dropped rows)."""

    @staticmethod
    def forward(ctx, src, rows, n_out, n_live, *feats):
        from spconv_amd.pytorch import _union
        ctx.rows = tuple(rows)
        return _union.add_fwd([f.detach() for f in feats], src, int(n_out), n_live)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_output):
        from spconv_amd.pytorch import _union
        return (None, None, None, None) + tuple(_union.add_bwd(grad_output, ctx.rows, ctx.needs_input_grad[4:]))


_UNION_DTYPES = (torch.float16, torch.bfloat16, torch.float32, torch.float64)


def sparse_add_native(tens, static_num_out=None, owner=None):
    """The misaligned add on the union kernels (spconv_amd/pytorch/_union.py), or None when they do not apply: more
    than eight operands, features that are not CUDA floating point of one dtype (quantised ones included), indices
    that are not int32, a key space beyond the rank-map gate, or -- eager form -- a coordinate that occurs twice within
    one operand (the composite sums such rows).  Static form when an operand carries n_live_dev: key order, room for
    `static_num_out` rows (default: the rows of all operands), nothing read back; `owner` (the calling module) keeps
    the device-side counters of its last call in `_static_n_out_dev`."""
    from spconv_amd.pytorch import _union
    first = tens[0]
    feats = [t.features for t in tens]
    dt = feats[0].dtype
    if not 1 <= len(tens) <= _union.MAX_OPERANDS or dt not in _UNION_DTYPES:
        return None
    for t in tens:
        f = t.features
        if not (isinstance(f, torch.Tensor) and f.is_cuda and f.dtype == dt and not f.is_quantized and f.dim() == 2
                and f.shape[1] >= 1 and t.indices.is_cuda and t.indices.dtype == torch.int32):
            return None
    lives = [getattr(t, "n_live_dev", None) for t in tens]
    static = any(v is not None for v in lives)
    u = _union.sparse_union([t.indices for t in tens], first.batch_size, first.spatial_shape,
                            n_live=lives if static else None,
                            static_num_out=(static_num_out or sum(f.shape[0] for f in feats) or 1) if static else None)
    if u is None:
        return None
    n_live = u.n_out_dev[2:3] if static else None
    out_features = SparseUnionAddFunction.apply(u.src, u.rows, u.n_out, n_live, *feats)
    if u.base >= 0:
        # one operand holds every coordinate: the result lives on ITS rows, its cached rulebooks stay valid
        res = _like_first(first, out_features, tens[u.base].indices, tens[u.base].indice_dict)
        res.n_live_dev = tens[u.base].n_live_dev
    else:
        res = _like_first(first, out_features, u.out_indices)
        res.n_live_dev = n_live
    if static and owner is not None:
        owner._static_n_out_dev = u.n_out_dev
    return res


def misaligned_add(tens, composite, static_num_out=None, owner=None):
    """The one body of sparse_add_hash_based, sparse_add and tables.AddTableMisaligned: the union kernels where they
    apply (sparse_add_native), else `composite`."""
    first = tens[0]
    for ten in tens:
        assert ten.spatial_shape == first.spatial_shape
        assert ten.batch_size == first.batch_size
        assert ten.features.shape[1] == first.features.shape[1]
    res = sparse_add_native(tens, static_num_out, owner)
    return res if res is not None else composite(*tens)


class SparseCollapseFunction(Function):
    """Reduction of an axis collapse over the kernels of csrc/collapse.hip: out[r] = sum / mean / max of the rows of
    group r in ascending input row, fp32 (fp64) accumulation, one rounding, one launch, no atomics.  The backward is one
    launch as well: a gather for sum (spx_union_add_bwd), spx_collapse_bwd for mean and max; dead and dropped rows
    receive zeros."""

    @staticmethod
    def forward(ctx, feat, build, reduce, n_live):
        from spconv_amd.pytorch import _collapse
        out = _collapse.fwd(feat.detach(), build, reduce, n_live)
        ctx.build, ctx.reduce = build, reduce
        if reduce == "max":
            ctx.save_for_backward(feat, out)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_output):
        from spconv_amd.pytorch import _collapse
        feat, out = ctx.saved_tensors if ctx.reduce == "max" else (None, None)
        return _collapse.bwd(grad_output, ctx.build, ctx.reduce, feat, out), None, None, None


def sparse_collapse(x, axes, reduce="sum", static_num_out=None, owner=None):
    """Drops the spatial axes `axes` of x (0 = the first: z of a zyx tensor) and merges the rows that land on one
    (batch, kept axes) cell by `reduce` = "sum" | "mean" | "max" -- the height compression of the fully sparse
    detectors, on the kernels of csrc/collapse.hip.  `axes = ()` merges duplicate coordinates.  The result is a fresh
    SparseConvTensor over the kept extents: rows in ascending key order with the level's rank map attached (the SubM
    layers behind build their rulebooks from it), an empty indice_dict, no grid.  Static form when x carries
    n_live_dev or `static_num_out` is given: room for `static_num_out` rows (default: x's rows, which always
    suffices), nothing read back, n_live_dev = the live rows found; `owner` (the calling module) keeps the
    device-side counters {found, 0, live} of its last call in `_static_n_out_dev`."""
    from spconv_amd.pytorch import _collapse
    from spconv_amd.pytorch._rulebook import _float_code, _require_gpu
    from spconv_amd.pytorch.core import SparseConvTensor
    feat = x.features
    _require_gpu(feat, "features")
    _float_code(feat, "sparse_collapse")
    if reduce not in _collapse.OPS:
        raise ValueError(f"sparse_collapse: reduce must be 'sum', 'mean' or 'max', got {reduce!r}")
    n_live_in = getattr(x, "n_live_dev", None)
    static = n_live_in is not None or static_num_out is not None
    build = _collapse.sparse_collapse_build(x.indices, x.batch_size, x.spatial_shape, axes, n_live=n_live_in,
                                            static_num_out=(static_num_out or feat.shape[0] or 1) if static else None)
    n_live = build.n_out_dev[2:3] if static else None
    out_features = SparseCollapseFunction.apply(feat, build, reduce, n_live)
    res = SparseConvTensor(out_features, build.out_indices, build.spatial_shape, x.batch_size, benchmark=x.benchmark)
    res.benchmark_record = x.benchmark_record
    res._timer = x._timer
    res.thrust_allocator = x.thrust_allocator
    res.force_algo = x.force_algo
    res.n_live_dev = n_live
    if static and owner is not None:
        owner._static_n_out_dev = build.n_out_dev
    return res


# ------------------------------------------------------------------ voxel pruning
def row_score(features, op="absmean", n_live=None):
    """One fp32 score per row on the kernel of csrc/select.hip: the mean ("absmean") or the maximum ("absmax") of
    |features[i, :]|, -inf for rows at or beyond *n_live.  The order of the mean's sum depends on the channel count
    and the dtype only (include/spconv_amd.h, voxel pruning): identical run to run and for any number of rows."""
    from spconv_amd.pytorch import _select
    return _select.row_score(features, op, n_live)


def topk_mask(score, k=None, ratio=None, indices=None, batch_size=None, n_live=None):
    """uint8 flags [n] of exactly k live rows: the rows with the largest scores, of equal scores those with the lowest
    row index.  Exactly one of `k` (a count, capped at the live rows) and `ratio` (in [0, 1]: k = int(ratio * live),
    computed on the device) is given.  A row is live below *n_live and, with `indices` and `batch_size`, when its
    batch index is inside [0, batch_size).  Nothing is read back (spx_topk_flags)."""
    from spconv_amd.pytorch import _select
    return _select.topk_flags(score, k, ratio, indices, batch_size, n_live)[0]


class SparseSelectFunction(Function):
    """Feature rows of a row selection: out[r] = feat[src[r]] (zeros past the live rows), one gather launch; the
    backward is one gather launch as well, din[i] = dout[rows[i]] (zeros for rows that were not selected or were cut).
    Bytes move, nothing is added: a row keeps its bits."""

    @staticmethod
    def forward(ctx, feat, build):
        from spconv_amd.pytorch import _select
        ctx.build = build
        return _select.fwd(feat.detach(), build)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_output):
        from spconv_amd.pytorch import _select
        return _select.bwd(grad_output, ctx.build), None


def _select_checks(x, what):
    from spconv_amd.pytorch._rulebook import _float_code, _require_gpu
    feat = x.features
    _require_gpu(feat, "features")
    _float_code(feat, what)
    _require_gpu(x.indices, "indices")
    if x.indices.dtype != torch.int32:
        raise NotImplementedError(f"{what}: indices must be int32, got {x.indices.dtype}")
    return feat


def sparse_select(x, keep, invert=False, static_num_out=None, owner=None):
    """The live rows of x whose flag `keep[i]` (bool or uint8 [n]) is set -- `invert`: is not set -- as a fresh
    SparseConvTensor, rows in x's order, on the kernels of csrc/select.hip.  Spatial shape and batch size are x's; the
    indice_dict is empty (the coordinate set is new) and there is no grid.  When x's index tensor carries the level's
    rank map (its rows are in key order) the result's map is built and attached: the SubM layers behind build their
    rulebooks from it.  Static form when x carries n_live_dev or `static_num_out` is given: room for `static_num_out`
    rows (default: x's rows, which always suffices), nothing read back, n_live_dev = the live rows found; `owner` (the
    calling module) keeps the device-side counters {found, 0, live} of its last call in `_static_n_out_dev`.  Only the
    features carry a gradient."""
    from spconv_amd.pytorch import _select, ops
    from spconv_amd.pytorch.core import SparseConvTensor
    feat = _select_checks(x, "sparse_select")
    n = int(feat.shape[0])
    n_live_in = getattr(x, "n_live_dev", None)
    static = n_live_in is not None or static_num_out is not None
    ranked = ops._rankmap_of(x.indices, x.batch_size, x.spatial_shape, n, 27) is not None
    build = _select.select_build(x.indices, x.batch_size, x.spatial_shape, keep, invert, n_live=n_live_in,
                                 static_num_out=(static_num_out or n or 1) if static else None, rank_map=ranked)
    out_features = SparseSelectFunction.apply(feat, build)
    res = SparseConvTensor(out_features, build.out_indices, x.spatial_shape, x.batch_size, benchmark=x.benchmark)
    res.benchmark_record = x.benchmark_record
    res._timer = x._timer
    res.thrust_allocator = x.thrust_allocator
    res.force_algo = x.force_algo
    res.n_live_dev = build.n_out_dev[2:3] if static else None
    if static and owner is not None:
        owner._static_n_out_dev = build.n_out_dev
    return res


def sparse_prune(x, ratio=None, k=None, score="absmean", return_dropped=False, static_num_out=None, owner=None):
    """Spatial voxel pruning: keeps the k live rows of x with the largest score -- `k` rows, or int(ratio * live rows)
    -- and returns them as a fresh SparseConvTensor (sparse_select); of equal scores the lowest rows stay, so the
    selection is identical run to run.  `score`: "absmean" | "absmax" of the row's features (row_score), or a tensor
    of one value per row (the predicted importance of a small head: detached and cast to fp32).  return_dropped=True
    returns (kept, dropped) from the same flags.  Dead rows (at or beyond n_live_dev, batch index -1) never compete.
    Static form as sparse_select; the kept side's default bound is max(1, int(ratio * rows)) or min(k, rows), which
    always suffices, the dropped side's is x's rows; an explicit `static_num_out` bounds the kept side and is reported
    through `owner._static_n_out_dev`."""
    from spconv_amd.pytorch import _select
    k_abs, r = _select.check_count(k, ratio, "sparse_prune")
    feat = _select_checks(x, "sparse_prune")
    n = int(feat.shape[0])
    n_live_in = getattr(x, "n_live_dev", None)
    if isinstance(score, torch.Tensor):
        if score.numel() != n:
            raise ValueError(f"sparse_prune: score holds {score.numel()} values for {n} rows")
        s = score.detach().reshape(n).to(torch.float32)
    elif score in _select.OPS:
        s = _select.row_score(feat, score, n_live_in)
    else:
        raise ValueError(f"sparse_prune: score must be 'absmean', 'absmax' or a tensor, got {score!r}")
    keep, _ = _select.topk_flags(s, k, ratio, x.indices, x.batch_size, n_live_in)
    static = n_live_in is not None or static_num_out is not None
    bound = None
    if static:
        bound = static_num_out or max(1, int(r * n) if k is None else min(k_abs, n))
    kept = sparse_select(x, keep, False, bound, owner)
    if not return_dropped:
        return kept
    return kept, sparse_select(x, keep, True, (n or 1) if static else None, None)


def sparse_add_hash_based(*tens):
    """Sum of sparse tensors with different coordinate sets (reference functional.py:439-499).  On the union kernels
    where they apply (sparse_add_native): rows in ascending key order with the level's rank map attached, or -- when
    one operand already holds every output coordinate -- in that operand's own numbering, with its index tensor and
    indice_dict.  Otherwise through the hash-table composite below."""
    return misaligned_add(tens, _sparse_add_hash_composite)


def _sparse_add_hash_composite(*tens):
    """The union of the coordinates numbered through a hash table (torch composite).  indice_dict is dropped unless
    one operand already holds every output coordinate."""
    from spconv_amd.pytorch.hash import HashTable
    first = tens[0]
    sizes = [t.features.shape[0] for t in tens]
    biggest = max(range(len(tens)), key=lambda i: sizes[i])
    shape = [first.batch_size, *first.spatial_shape]
    big = int(np.prod(shape)) >= _MAX_INT32
    k_type = torch.int64 if big else torch.int32
    table = HashTable(first.features.device, k_type, torch.int32, max(2 * sum(sizes), 2))
    scalars = []
    for ten in tens:
        scalar = _indice_to_scalar(ten.indices.long() if big else ten.indices, shape)
        scalars.append(scalar)
        table.insert(scalar)
    count_val = int(table.assign_arange_().item())
    feat = first.features
    out_features = torch.zeros([count_val, feat.shape[1]], dtype=feat.dtype, device=feat.device)
    out_indices = torch.zeros([count_val, first.indices.shape[1]], dtype=first.indices.dtype,
                              device=first.indices.device)
    for ten, scalar in zip(tens, scalars):
        rows = table.query(scalar)[0].long()
        out_features.index_add_(0, rows, ten.features)
        out_indices[rows] = ten.indices
    keep = tens[biggest].indice_dict if count_val == sizes[biggest] else None
    return _like_first(first, out_features, out_indices, keep)


def sparse_add(*tens):
    """Same sum (reference functional.py:502-545 goes through torch.sparse).  On the union kernels where they apply
    (as sparse_add_hash_based); otherwise through the sort + unique composite below."""
    return misaligned_add(tens, _sparse_add_sorted_composite)


def _sparse_add_sorted_composite(*tens):
    """Sort + unique of the linear keys (torch composite): output rows are ordered by coordinate."""
    first = tens[0]
    sizes = [t.features.shape[0] for t in tens]
    biggest = max(range(len(tens)), key=lambda i: sizes[i])
    shape = [first.batch_size, *first.spatial_shape]
    scalars = torch.cat([_indice_to_scalar(t.indices.long(), shape) for t in tens])
    uniq, inverse = torch.unique(scalars, sorted=True, return_inverse=True)
    feats = torch.cat([t.features for t in tens])
    out_features = torch.zeros([uniq.shape[0], feats.shape[1]], dtype=feats.dtype, device=feats.device)
    out_features.index_add_(0, inverse, feats)
    cols = []
    rest = uniq
    for extent in reversed(shape):
        cols.append(rest % extent)
        rest = rest // extent
    out_indices = torch.stack(cols[::-1], dim=1).to(first.indices.dtype).contiguous()
    keep = tens[biggest].indice_dict if uniq.shape[0] == sizes[biggest] else None
    return _like_first(first, out_features, out_indices, keep)


# point <-> voxel features (csrc/pointvoxel.hip; not part of the reference): the groups of a point cloud, the reductions
# over them and the way back, for learned voxel feature encoders (vfe.DynamicVFE)
from spconv_amd.pytorch._pointvoxel import (PointGroups, decorate_points, point_groups,  # noqa: E402,F401
                                            points_to_voxels, voxels_to_points)

# trilinear devoxelisation (csrc/interp.hip; not part of the reference): the corner table of a point cloud over a sparse
# level and the interpolation of its rows to the points
from spconv_amd.pytorch._interp import (PointCorners, point_corners, point_corners_into,  # noqa: E402,F401
                                        voxels_to_points_trilinear)

# voxel query and neighbour grouping (csrc/query.hip; not part of the reference): the first nsample voxels of a level
# around each query point, and their rows gathered
from spconv_amd.pytorch._query import (VoxelNeighbors, group_voxels, voxel_query,  # noqa: E402,F401
                                       voxel_query_into)

# farthest-point sampling and ball query over raw points (csrc/sample.hip; not part of the reference): keypoints of a
# cloud, and the first nsample raw points around each query as the neighbour table group_voxels gathers
from spconv_amd.pytorch._sample import (PointSamples, ball_query, ball_query_into,  # noqa: E402,F401
                                        farthest_point_sample, fps_into, gather_samples, scene_groups)

# sectorised keypoint sampling (csrc/sample.hip; not part of the reference): segment ids by scene, RoI filter and azimuth
# sector, a quota per segment and farthest-point sampling with K read per segment -- PV-RCNN++'s
# sectorized_proposal_centric_sampling, pointnet2_stack's stack_farthest_point_sample
from spconv_amd.pytorch._sample import (SectorBuffers, farthest_point_sample_segments,  # noqa: E402,F401
                                        fps_quota_into, fps_segments_into, sector_buffers, sector_fps,
                                        sector_fps_into, sector_ids, sector_ids_into, sector_table)

# k-nearest-neighbour query and inverse-distance interpolation over raw points (csrc/knn.hip; not part of the reference):
# the k points that come first under (squared distance, point index), as the tables group_voxels gathers and
# voxels_to_points_trilinear blends
from spconv_amd.pytorch._knn import (PointKNN, knn_interpolate, knn_query, knn_query_into,  # noqa: E402,F401
                                     three_nn)

# rotated boxes (csrc/box.hip; not part of the reference): corners, pairwise overlap / IoU in the plane and in space, and
# a non-maximum suppression that stays on the device -- the iou3d_nms extension of OpenPCDet / mmdet3d
from spconv_amd.pytorch._box import (BoxCorners, BoxNMS, boxes_iou3d, boxes_iou3d_aligned,  # noqa: E402,F401
                                     boxes_iou_bev, boxes_overlap_bev, boxes_to_corners, nms_rotated,
                                     nms_rotated_into, nms_ws_bytes)

# differentiable rotated IoU (csrc/boxgrad.hip; not part of the reference): the IoU of aligned pairs in the plane and in
# space, with or without the DIoU penalty, and its gradient -- mmcv's diff_iou_rotated_3d
from spconv_amd.pytorch._boxgrad import (boxes_iou3d_diff, boxes_iou_aligned_grad_into,  # noqa: E402,F401
                                         boxes_iou_bev_diff, boxes_to_corners_bwd_into)

# points in rotated boxes (csrc/roi.hip; not part of the reference): the frames of boxes, the box of every point, the
# points of every box, and RoI point / RoI-aware pooling composed from them with group_voxels, point_groups and
# points_to_voxels -- the roiaware_pool3d / roipoint_pool3d extensions of OpenPCDet / mmdet3d
from spconv_amd.pytorch._roi import (BoxFrames, BoxPoints, box_query, box_query_into,  # noqa: E402,F401
                                     boxes_to_frames, points_in_boxes, roi_aware_pool, roi_point_pool)

# centre-head targets (csrc/center.hip; not part of the reference): the records of the ground-truth boxes, the dense
# Gaussian heatmaps and the heat of the rows of a sparse 2-D level -- CenterHead.assign_target_of_single_head of
# OpenPCDet and VoxelNeXt's sparse twin, without their Python loop
from spconv_amd.pytorch._center import (BoxCenters, CenterParams, SparseCenters, box_centers,  # noqa: E402,F401
                                        box_centers_into, center_buffers, center_groups_ws, center_heatmap,
                                        center_heatmap_into, center_heatmap_sparse, center_heatmap_sparse_into,
                                        center_nearest_into, center_tile)

# voxel serialisation (csrc/serialize.hip; not part of the reference): rows ordered along Z-order / Hilbert curves and
# cut into fixed-size patches, for the serialised point / voxel transformers
from spconv_amd.pytorch import _serialize  # noqa: E402
from spconv_amd.pytorch._serialize import PatchPlan, Serialization  # noqa: E402,F401


def serialize(x_or_indices, spatial_shape=None, batch_size=None, orders=("z", "z-trans", "hilbert", "hilbert-trans"),
              depth=None, axes=None, n_live=None):
    """The rows of a level in the order of space-filling curves, on the kernels of csrc/serialize.hip.  x_or_indices: a
    SparseConvTensor (which supplies indices, spatial shape, batch size and its n_live_dev) or int32 indices [n, ndim +
    1] with `batch_size` and a `spatial_shape` or `depth`.  orders: up to 8 of "z", "z-trans", "hilbert",
    "hilbert-trans".  A curve takes the spatial index columns through `axes`, the first entry the most significant:
    by default the columns reversed -- (x, y, z) for [batch, z, y, x] --, the -trans orders with the first two entries
    swapped.  depth (bits per axis, 1 .. 16; default: the bit length of max(spatial_shape) - 1) is known on the host,
    and ndim * depth + bit_length(batch_size) may not exceed 63.  Returns a Serialization: code int64 [K, n] = (batch <<
    (ndim * depth)) | curve code, order / inverse int32 [K, n], offsets int32 [batch_size + 1], depth, orders.  A row
    is dead when its batch index is outside [0, batch_size), a coordinate is outside [0, 2^depth) or it lies at or beyond
    *n_live: its code is -1 and it follows every live row, in ascending row.  The sort is stable.  Nothing is read
    back: the call can sit inside a captured graph.  No gradients: every output is an integer."""
    if hasattr(x_or_indices, "indices") and hasattr(x_or_indices, "spatial_shape"):
        x = x_or_indices
        indices = x.indices
        spatial_shape = list(x.spatial_shape) if spatial_shape is None else spatial_shape
        batch_size = x.batch_size if batch_size is None else batch_size
        n_live = getattr(x, "n_live_dev", None) if n_live is None else n_live
    else:
        indices = x_or_indices
        if batch_size is None:
            raise ValueError("serialize: indices need a batch_size")
    return _serialize.serialize(indices, int(batch_size), spatial_shape, orders, depth, axes, n_live)


def patch_plan(ser, patch_size, which=0, pad="borrow"):
    """The fixed-shape patch layout of order `which` of a Serialization (spx_patch_plan): P_cap = n // patch_size +
    batch_size patches of patch_size slots, a host-known bound.  Every scene starts on a patch boundary; the tail slots
    of a scene's last patch hold -1 (pad="mask") or the row held patch_size slots earlier (pad="borrow", as Point
    Transformer V3 pads; scenes shorter than one patch: -1) -- borrowed duplicates serve as attention keys, never as
    results.  Returns a PatchPlan; nothing is read back (n_patches_dev stays on the device)."""
    return _serialize.patch_plan(ser, patch_size, which, pad)


# A row move casts nothing: under autocast the rows keep their dtype and their bits (custom_fwd without cast_inputs; the
# convolutions' _FWD would turn every floating argument into float16 and rebuild the plan tuple on the way).
_FWD_ROWS = _amp.custom_fwd(device_type="cuda")


class RowsToPatchesFunction(Function):
    """[n, C] -> [P_cap, K, C] over patch_rows (one gather launch); the backward adds a row's canonical and borrowed
    slot in fp32 (fp64), rounded once (spx_patch_rows_bwd: one launch, no atomics)."""

    @staticmethod
    @_FWD_ROWS
    def forward(ctx, features, plan):
        ctx.plan = plan
        return _serialize.rows_fwd(features.detach(), plan)

    @staticmethod
    @once_differentiable
    @_BWD
    def backward(ctx, grad_output):
        return _serialize.rows_bwd(grad_output, ctx.plan), None


class PatchesToRowsFunction(Function):
    """[P_cap, K, C] -> [n, C] over row_slot; the backward is the gather over patch_rows_canon.  Bytes move, nothing is
    added: a row keeps its bits."""

    @staticmethod
    @_FWD_ROWS
    def forward(ctx, patches, plan):
        ctx.plan = plan
        return _serialize.patches_fwd(patches.detach(), plan)

    @staticmethod
    @once_differentiable
    @_BWD
    def backward(ctx, grad_output):
        return _serialize.patches_bwd(grad_output, ctx.plan), None


def rows_to_patches(features, plan):
    """Feature rows [n, C] into the patches of a PatchPlan: [P_cap, patch_size, C], zeros in the -1 slots.
    Differentiable in the features over the four floating dtypes; a borrowed slot's gradient is added to its row's."""
    _serialize.check_rows(features, plan, "rows_to_patches")
    return RowsToPatchesFunction.apply(features, plan)


def patches_to_rows(patches, plan):
    """Patches [P_cap, patch_size, C] back to rows [n, C]: every live row reads its canonical slot, dead rows get zeros.
    Differentiable in the patches; borrowed and empty slots get a zero gradient."""
    _serialize.check_patches(patches, plan, "patches_to_rows")
    return PatchesToRowsFunction.apply(patches, plan)
