"""Op drivers: torch tensors in, C-ABI calls out.

Mirrors the public functions of ``spconv/pytorch/ops.py`` (names, argument
meaning, error behaviour) for the hot path:

* ``get_conv_output_size`` / ``get_deconv_output_size``   (ops.py:73-96)
* ``get_indice_pairs``                                     (ops.py:132-326)
* ``get_indice_pairs_implicit_gemm``                       (ops.py:329-808)
* ``indice_conv`` / ``indice_conv_backward``               (ops.py:811-1095,1103-1447)
* ``implicit_gemm`` / ``implicit_gemm_backward``           (ops.py:1450-1664,1667-1896)

All compute happens in the HIP library behind ``include/spconv_amd.h``; torch is
used for allocation (the reference's TorchAllocator role, cppcore.py:112-223)
and to read the current stream (cppcore.py:98-99).  CPU tensors are rejected:
this implementation has no CPU path.

This module is the facade; the bodies live in ``_rulebook`` and ``_gemm``, whose headers say what state each owns.  Here
stay the reference-shaped API (pooling included: it owns no state) and the two host decisions whose switches tests and
tools set through this module (an assignment would not reach a re-exported name): `build_rulebook`
(_SORTED_MAX_CELLS_PER_ROW, _LAYOUT_SKIP, rows_layout) and `igemm_bwd` (_BWD_ROWS, _igemm_bwd_rows); modules.py reads
BN_EPILOGUE through it.
Which driver sees which row order and table form, and which kernel family results: DESIGN.md section 3.0.
"""
from __future__ import annotations

import ctypes
import os
from typing import List, Optional, Tuple

import numpy as np
import torch

from spconv_amd import _lib
from spconv_amd.constants import SPCONV_DO_SORT
from spconv_amd.pytorch.core import ConvAlgo, Rulebook
from spconv_amd.pytorch._rulebook import (  # noqa: F401  (re-exports: what callers reach through this module)
    _CLS0_ATTR, _DTYPES, _LAYOUT_MIN_ROWS, _MFMA_COUT, _ROWS_LAYOUT, _SORTED_MAX_SCRATCH, Activation, _build_conv,
    _build_subm, _cells, _dtype_code, _int_repr, _kv, _native_from_table, _on_device, _pred_get, _ptr, _rankmap_of,
    _require_gpu, _set_class, _stream, _table_from_native, _with_dense_hint, _with_hints, _with_sparse_hint, _ws,
    attach_rank_map, attach_rulebook,
    get_conv_output_size, get_deconv_output_size, key_argsort, layout_views, mask_argsort, poll_class, rows_layout,
    rulebook_of, sort_rulebook, sparse_neighbourhoods, sparse_rows_hint, split_tile_order, tables_of)
from spconv_amd.pytorch._gemm import (  # noqa: F401
    _STAGE2_JOB_BYTES, _WGRAD_MAX_KV, StatsSink, _check_feat, _defer_lock, _defer_passes, _defer_state, _lane_mult,
    bias_act_inplace, collect_bn_stats, current_stats_sink, deferred_wgrad, igemm_dgrad, igemm_fwd, igemm_fwd_int8,
    igemm_wgrad, output_stays_cached, wgrad_plan)
from spconv_amd.pytorch._union import sparse_union  # noqa: F401  (misaligned add: the union build of csrc/union.hip)

# ---- the switches that tests and tools set through this module -----------------------------------------------------
BN_EPILOGUE = os.environ.get("SPCONV_AMD_BN_EPILOGUE", "1") != "0"      # see _gemm.collect_bn_stats
_LAYOUT_SKIP = os.environ.get("SPCONV_AMD_LAYOUT_SKIP", "1") != "0"     # see build_rulebook
# The rank-map builder's cost grows with the GRID (one byte per cell filled and scanned, cells / 4 bytes of map kept for
# the level's SubM layers), the hash builder's with the INPUT rows (~0.45 us per 1000).  Measured break-even is a few
# hundred cells per input row (config 4: 118 cells per row at level 1 -> 2, 20 at level 2 -> 3; 174 -> 118 us); beyond
# `_SORTED_MAX_CELLS_PER_ROW` cells per row, or 1 GiB of scratch, the first-seen hash build is taken instead (round-5
# ADVICE: a 500^3 x 2 grid with 50 k voxels would fill and scan 250 MB per build).  0 = no gate.
_SORTED_MAX_CELLS_PER_ROW = float(os.environ.get("SPCONV_AMD_SORTED_MAX_CELLS_PER_ROW", "512"))


def _sorted_pays(n_in: int, batch_size: int, out_shape) -> bool:
    cells = _cells(batch_size, out_shape)
    return _SORTED_MAX_CELLS_PER_ROW <= 0 or (cells <= _SORTED_MAX_CELLS_PER_ROW * max(n_in, 1)
                                              and cells * 1.25 <= _SORTED_MAX_SCRATCH)


@_on_device
def build_rulebook(indices: torch.Tensor, batch_size: int, spatial_shape: List[int],
                   ksize: List[int], stride: List[int], padding: List[int],
                   dilation: List[int], out_padding: List[int], subm: bool = False,
                   transpose: bool = False, need_bwd_table: bool = False,
                   do_sort=False, need_native: bool = True,
                   num_out_act_bound: int = -1, static_num_out: int = 0,
                   pred_key=None, out_order: str = "first_seen") -> Tuple[Rulebook, List[int]]:
    """One call builds every artefact (dense tables, masks, Native lists).  need_native=False
    (inference) leaves the ConvAlgo.Native lists out -- three launches and two thirds of the
    fill traffic -- and the Rulebook derives them from the tables if they are asked for later.

    static_num_out > 0 (regular / transposed convolution, inference): the STATIC-SHAPE form -- every
    output tensor has static_num_out rows, nothing is read back from the device (the whole build can
    be captured in a graph), rows past the real output count are dead (out_indices -1, no pairs) and
    `rb.n_out_dev` holds {outputs found, table overflow} on the device.  Input rows with a negative
    batch index are dead rows in every mode.

    do_sort: False = rows stay in input order; "layout" (the modules' default; "auto" is an alias) =
    density-aware rows layout of a SubM rulebook, built on the device (rows_layout); True = the
    reference's explicit mask sort (sort_rulebook).

    out_order (regular convolution): "first_seen" = the CPU reference's numbering of the outputs (indices.py:1742-1771);
    "sorted" = ascending linear coordinate key, the order of the reference's GPU sort + unique path
    (all.py:1533-1552), built through the level's RANK MAP (include/spconv_amd.h, sorted-order levels) where the geometry
    allows it (k3 s2, k2 s2, ...; otherwise first seen).  The map travels with rb.out_indices (`_spx_rankmap`): a SubM
    build over exactly that tensor reads its neighbours from it instead of hashing the coordinates again."""
    _require_gpu(indices, "indices")
    assert indices.dtype == torch.int32 and indices.ndim == 2
    L = _lib.load()
    indices = indices.contiguous()
    n_in, ndim = indices.shape[0], indices.shape[1] - 1
    kv = _kv(ksize)
    words = (kv + 31) // 32
    if subm:
        out_shape = list(spatial_shape)
    elif transpose:
        out_shape = get_deconv_output_size(spatial_shape, ksize, stride, padding, dilation, out_padding)
    else:
        out_shape = get_conv_output_size(spatial_shape, ksize, stride, padding, dilation)
    if any(x <= 0 for x in out_shape):
        raise ValueError(f"your out spatial shape {out_shape} reach zero!!! input shape: {spatial_shape}")
    stream = _stream(indices)
    in_key_order = False
    if subm:
        rb = _build_subm(L, indices, batch_size, spatial_shape, ksize, dilation, need_native, need_bwd_table, stream)
    else:
        if out_order not in ("first_seen", "sorted"):
            raise ValueError(f"out_order must be 'first_seen' or 'sorted', got {out_order!r}")
        in_key_order = bool(out_order == "sorted" and n_in > 0
                            and L.spx_conv_sorted_ok(ndim, batch_size, _lib.ints(spatial_shape), _lib.ints(out_shape),
                                                     _lib.ints(ksize), _lib.ints(stride), _lib.ints(padding),
                                                     _lib.ints(dilation), int(transpose))
                            and _sorted_pays(n_in, batch_size, out_shape))
        rb = _build_conv(L, indices, batch_size, spatial_shape, out_shape, ksize, stride, padding, dilation, transpose,
                         need_native, num_out_act_bound, static_num_out, in_key_order, stream)
    # pred_key: whose rulebook this is, for the density-class prediction (poll_class).  Only a SubM rulebook is ever
    # classified, so that every form records it -- the static first-seen form used not to -- shows nowhere.
    rb.set_geometry(indices, spatial_shape, out_shape, batch_size, pred_key)
    if not subm and static_num_out > 0 and not in_key_order:
        do_sort = False               # the static first-seen form has never looked at do_sort: its rows stay as they are
    elif in_key_order:
        do_sort = do_sort is True     # (of the row orders only SPCONV_DO_SORT=1, "explicit mask sort of every rulebook")
    if do_sort in ("layout", "auto"):
        # the default row order: classified and regrouped on the device inside the build (SubM; nothing
        # read back).  Strided layers keep their row order (dense by construction: every output has
        # several inputs), small rulebooks are launch-bound either way.
        if subm and 1 < kv <= 32 and n_in >= _LAYOUT_MIN_ROWS:
            if (_LAYOUT_SKIP and torch.cuda.is_current_stream_capturing()
                    and bool(getattr(pred_key, _CLS0_ATTR, False))):
                # Inside a capture the class of this module's rulebooks is what the warm-up passes saw.  Class 0 (most
                # rows have a neighbour: every level of a LiDAR backbone) uses nothing of a layout but its class word:
                # the three launches that make it are left out, the gather-GEMMs walk the row-order tables as they do for
                # small rulebooks, with the density hint the prediction gives (a scene of the other class still computes
                # the same values, on the slower walk).
                _set_class(rb)
            else:
                rows_layout(rb)
    elif do_sort and words == 1:
        sort_rulebook(rb)
    return rb, out_shape


def get_indice_pairs(indices: torch.Tensor, batch_size: int, spatial_shape: List[int],
                     algo: ConvAlgo, ksize: List[int], stride: List[int], padding: List[int],
                     dilation: List[int], out_padding: List[int], subm: bool = False,
                     transpose: bool = False, num_out_act_bound: int = -1):
    """Returns (out_inds, pair [2, kv, N_in], indice_num_per_loc [kv]) -- ConvAlgo.Native layout."""
    rb, _ = build_rulebook(indices, batch_size, spatial_shape, ksize, stride, padding, dilation,
                           out_padding, subm, transpose, num_out_act_bound=num_out_act_bound)
    return rb.out_indices, attach_rulebook(rb.pair_native, rb), rb.num_per_loc


def get_indice_pairs_implicit_gemm(indices: torch.Tensor, batch_size: int,
                                   spatial_shape: List[int], algo: ConvAlgo, ksize: List[int],
                                   stride: List[int], padding: List[int], dilation: List[int],
                                   out_padding: List[int], subm: bool = False,
                                   transpose: bool = False, is_train: bool = True, alloc=None,
                                   timer=None, num_out_act_bound: int = -1,
                                   direct_table: bool = True, do_sort: bool = SPCONV_DO_SORT):
    """Returns the reference's 9-tuple (ops.py:347-359):
    (out_inds, num_inds_per_loc, pair_fwd, pair_bwd, pair_mask_fwd_splits, pair_mask_bwd_splits,
     mask_argsort_fwd_splits, mask_argsort_bwd_splits, masks)."""
    if algo not in (ConvAlgo.MaskImplicitGemm, ConvAlgo.MaskSplitImplicitGemm):
        raise ValueError(f"get_indice_pairs_implicit_gemm builds the masked implicit-GEMM tables; algo {algo} "
                         f"(ConvAlgo.Native) goes through get_indice_pairs")
    kv = _kv(ksize)
    rb, _ = build_rulebook(indices, batch_size, spatial_shape, ksize, stride, padding, dilation,
                           out_padding, subm, transpose, need_bwd_table=subm and is_train,
                           do_sort=do_sort if kv <= 32 else False, num_out_act_bound=num_out_act_bound)
    masks = [np.array([0xffffffff], dtype=np.uint32)]
    arg_fwd = rb.argsort_fwd if rb.argsort_fwd is not None else torch.arange(
        rb.n_out, dtype=torch.int32, device=indices.device)
    pair_fwd = attach_rulebook(rb.pair_fwd, rb)
    if subm:
        pair_bwd = rb.pair_bwd if (is_train and rb.pair_bwd is not None) else torch.Tensor()
        return (rb.out_indices, rb.num_per_loc, pair_fwd, pair_bwd, [rb.mask_fwd], [], [arg_fwd],
                [], masks)
    arg_bwd = rb.argsort_bwd if rb.argsort_bwd is not None else torch.arange(
        rb.n_in, dtype=torch.int32, device=indices.device)
    return (rb.out_indices, rb.num_per_loc, pair_fwd, rb.pair_bwd, [rb.mask_fwd], [rb.mask_bwd],
            [arg_fwd], [arg_bwd], masks)


@_on_device
def igemm_bwd(features: torch.Tensor, out_bp: torch.Tensor, filters: torch.Tensor,
              table: torch.Tensor, mask: Optional[torch.Tensor], argsort: Optional[torch.Tensor],
              native: torch.Tensor, num_per_loc: torch.Tensor, subm: bool,
              plan: Optional[torch.Tensor] = None, need_din: bool = True,
              tile_order: int = 0, dense_rows: bool = False, lists=None):
    """(din, dW) of one layer from one launch (+ the wgrad second stage).  need_din=False (the
    input does not require grad: a network's first layer) computes dW only and returns None.
    `table` / `mask` are row-order tables unless tile_order == 1 (see tables_of).  `native` may be None
    when `lists` is given: a callable returning (native, num_per_loc, plan), asked only if the pair-list
    weight gradient runs (the rows walk of narrow layers needs none of the three)."""
    _check_feat(out_bp, filters)
    K0, C0 = filters.shape[0], filters.shape[-1]
    m = _lane_mult(out_bp.dtype)
    kvf = filters.numel() // (K0 * C0)
    if ((_BWD_ROWS is True or (_BWD_ROWS == "auto" and dense_rows))
            and out_bp.dtype in (torch.float16, torch.bfloat16) and K0 in (16, 32) and C0 in (16, 32)
            and kvf <= 27 and table is not None and mask is not None and mask.shape[1] == 1
            and (argsort is None or tile_order == _ROWS_LAYOUT) and tile_order != 1):
        # (the rows walk reads the row-order tables: a rows layout does not concern it)
        return _igemm_bwd_rows(features, out_bp, filters, table, mask, subm, need_din, K0, C0, kvf)
    if native is None:
        native, num_per_loc, plan = lists()
    if (not need_din or K0 % m or C0 not in _MFMA_COUT or kvf > 32      # (kv > 32: dgrad in groups of 32 offsets)
            or out_bp.dtype == torch.float64):                          # (float64: dgrad + wgrad, no fused launch)
        din = igemm_dgrad(out_bp, filters, table, mask, argsort, features.shape[0], subm,
                          tile_order=tile_order) if need_din else None
        return din, igemm_wgrad(features, out_bp, filters.shape, native, num_per_loc, subm, plan)
    L = _lib.load()
    features = features.contiguous()
    out_bp = out_bp.contiguous()
    st = _defer_state(filters)
    filters_leaf = filters
    filters = filters.contiguous()
    K, C = filters.shape[0], filters.shape[-1]
    kv = filters.numel() // (K * C)
    n_in = features.shape[0]
    din = torch.empty((n_in, C), dtype=out_bp.dtype, device=out_bp.device)
    dw = torch.empty_like(filters)
    ws = _ws(L.spx_igemm_wgrad_ws_bytes(native.shape[2], C, K, kv), features.device)
    args = (features.data_ptr(), out_bp.data_ptr(), filters.data_ptr(), din.data_ptr(), dw.data_ptr(), _ptr(table),
            _ptr(mask), _ptr(argsort), _with_sparse_hint(int(tile_order), argsort), native.data_ptr(), num_per_loc.data_ptr(),
            _ptr(plan), n_in,
            out_bp.shape[0], C, K, kv, _dtype_code(out_bp), int(subm), ws.data_ptr(), ws.numel(), _stream(out_bp))
    if st is not None:
        job = ctypes.create_string_buffer(_STAGE2_JOB_BYTES)
        _lib.check(L.spx_igemm_bwd_deferred(*args, job))
        with _defer_lock:       # (ws, plan and the lists live until the batch launch; dw is the engine's from here on)
            st["jobs"].append((job, filters_leaf, (ws, plan, native, num_per_loc)))
        return din, dw
    _lib.check(L.spx_igemm_bwd(*args))
    return din, dw


# Narrow layers (16 / 32 channels): the backward from one gather per pair (csrc/igemm_bwdn.hip).  Its tile
# walk visits every table row of a 128-row tile, so it pays where neighbourhoods are DENSE (level 2 of a LiDAR
# backbone, 15 pairs per voxel: 185 -> 114 us) and loses where they are not (level 1, 5 pairs per voxel: 98 ->
# 108 us; a uniform scene far more).  The pairs-per-voxel count lives on the device; what the host knows without
# a read-back is the OCCUPANCY of the grid the table's rows live in (voxels / cells), which grows with it:
# 0.1 % at level 1, 0.66 % at level 2, 1.8 % at level 3 of the config-4 network.
# SPCONV_AMD_BWD_ROWS: "auto" (default: occupancy >= _BWD_ROWS_OCC), "1" always, "0" never.
_BWD_ROWS = {"0": False, "1": True}.get(os.environ.get("SPCONV_AMD_BWD_ROWS", "auto"), "auto")
_BWD_ROWS_OCC = float(os.environ.get("SPCONV_AMD_BWD_ROWS_OCC", "0.003"))


def rows_backward_expected(dtype: torch.dtype, cin: int, cout: int, kv: int, n_rows: int, batch_size: int,
                           dims) -> bool:
    """Will the backward of a layer with these shapes take the rows walk (igemm_bwdn.hip), which reads the dense
    table and needs neither the Native lists nor the range plan?  The same rule as igemm_bwd / _dense_rows, usable
    BEFORE the rulebook exists: a module asks it to decide whether its build has to produce the lists at all (a
    layer that shares the rulebook and does need them derives them from the table on first use)."""
    if (_BWD_ROWS is False or dtype not in (torch.float16, torch.bfloat16) or cin not in (16, 32) or cout not in (16, 32)
            or kv > 27):
        return False
    return _BWD_ROWS is True or n_rows >= _BWD_ROWS_OCC * _cells(batch_size, dims)


def _dense_rows(rb: Optional[Rulebook], n_rows: int, which: str) -> bool:
    """Occupancy of the grid that the rows of table `which` ("fwd": output rows, "bwd": input rows) live in."""
    dims = None if rb is None else (rb.out_shape if which == "fwd" else rb.in_shape)
    return bool(dims) and n_rows >= _BWD_ROWS_OCC * _cells(rb.batch_size, dims)


@_on_device
def _igemm_bwd_rows(features, out_bp, filters, table, mask, subm, need_din, K, C, kv):
    L = _lib.load()
    features, out_bp = features.contiguous(), out_bp.contiguous()
    n_in = features.shape[0]
    # the weights with the dout channel contiguous ([kv, C, K]: one small copy; SubM's mirrored slice order is the
    # kernel's business)
    wt = filters.reshape(K, kv, C).permute(1, 2, 0).contiguous()
    din = torch.empty((n_in, C), dtype=out_bp.dtype, device=out_bp.device) if need_din else None
    dw = torch.empty_like(filters)
    ws = _ws(L.spx_igemm_bwd_rows_ws_bytes(n_in, C, K, kv), features.device)
    _lib.check(L.spx_igemm_bwd_rows(features.data_ptr(), out_bp.data_ptr(), wt.data_ptr(), _ptr(din), dw.data_ptr(),
                                    table.data_ptr(), mask.data_ptr(), n_in, out_bp.shape[0], C, K, kv, int(subm),
                                    _dtype_code(out_bp), ws.data_ptr(), ws.numel(), _stream(out_bp)))
    return din, dw


def _plan_of(rb: Optional[Rulebook]) -> Optional[torch.Tensor]:
    if rb is None or rb.pair_native is None or rb.kv > _WGRAD_MAX_KV:
        return None
    if rb.wgrad_plan is None:
        rb.wgrad_plan = wgrad_plan(rb.num_per_loc, rb.n_in, rb.kv, rb.subm)
    return rb.wgrad_plan


def record_voxel_count_(buf: torch.Tensor, rb: Rulebook, rows: int) -> None:
    """max_num_voxels_during_training (reference conv.py:44,131-138): the running maximum of a strided layer's
    output count.  A static-shape build has `rows` = the frozen BOUND, not the count -- recording that would
    inflate every bound later derived from the buffer (freeze_bounds: recorded * margin) -- so there the count
    the build found on the device is folded in, without a read-back."""
    if rb.n_out_dev is not None:
        buf.copy_(torch.maximum(buf, rb.n_out_dev[:1].to(buf.dtype).reshape(buf.shape)))
    else:
        buf.clamp_(min=int(rows))


def maximum_value_int_(ten: torch.Tensor, value: int) -> torch.Tensor:
    """In-place ``ten = max(ten, value)`` for integer tensors (reference ops.py:2099-2105; used by the
    voxeliser to clamp counts)."""
    return ten.clamp_(min=int(value))


def fused_indice_conv(features, filters, bias, indice_pairs, indice_pair_num, num_activate_out,
                      inverse, subm):
    """Present in the reference's namespace and unimplemented there as well (ops.py:1098-1100)."""
    raise NotImplementedError


# ------------------------------------------- reference-shaped public op API
def indice_conv(features: torch.Tensor, filters: torch.Tensor, indice_pairs: torch.Tensor,
                indice_pair_num: torch.Tensor, num_activate_out: int, inverse: bool = False,
                subm: bool = False, algo: ConvAlgo = ConvAlgo.Native, timer=None,
                bias: Optional[torch.Tensor] = None, act_alpha: float = 0.0,
                act_beta: float = 0.0, act_type: int = Activation.None_) -> torch.Tensor:
    """ConvAlgo.Native forward (ops.py:811-1095) on the Native lists [2, kv, N_in]."""
    _check_feat(features, filters)
    rb: Optional[Rulebook] = rulebook_of(indice_pairs)
    kv = indice_pairs.shape[1]
    argsort, tile_order = None, 0
    if rb is not None and not inverse:
        table, mask, argsort, tile_order = tables_of(rb, "fwd", filters.shape[0])
    elif rb is not None and inverse and rb.pair_bwd is not None:
        table, mask, argsort, tile_order = tables_of(rb, "bwd", filters.shape[0])
    else:
        table, mask = _table_from_native(indice_pairs, indice_pair_num, num_activate_out, subm, inverse)
    return igemm_fwd(features, filters, table, mask, argsort, num_activate_out,
                     kv // 2 if subm else -1, bias, act_type, act_alpha, tile_order=tile_order)


def indice_conv_backward(features: torch.Tensor, filters: torch.Tensor, out_bp: torch.Tensor,
                         indice_pairs: torch.Tensor, indice_pair_num: torch.Tensor,
                         inverse: bool = False, subm: bool = False,
                         algo: ConvAlgo = ConvAlgo.Native, timer=None, need_din: bool = True):
    """ConvAlgo.Native backward (ops.py:1103-1447): returns (din, dfilters)."""
    _check_feat(features, filters)
    rb: Optional[Rulebook] = rulebook_of(indice_pairs)
    n_in = features.shape[0]
    argsort, tile_order, which = None, 0, None
    if rb is not None:
        # dgrad gathers dout rows for every input row: SubM reads the forward table (mirrored
        # weights), a regular conv the table indexed by its input rows, an inverse conv the forward one
        which = "fwd" if (subm or inverse) else "bwd"
        table, mask, argsort, tile_order = tables_of(rb, which, filters.shape[-1])
    else:
        table, mask = _table_from_native(indice_pairs, indice_pair_num, n_in, subm, (not subm) and (not inverse))
    if rb is not None and not inverse and not rb.has_native:
        # the build left the lists out (conv.py: _needs_native_lists): they -- and the range plan -- are derived
        # only if the launch below turns out to need them
        return igemm_bwd(features, out_bp, filters, table, mask, argsort, None, None, subm, None, need_din,
                         tile_order=tile_order, dense_rows=_dense_rows(rb, n_in, which),
                         lists=lambda: (rb.pair_native, rb.num_per_loc, _plan_of(rb)))
    native = indice_pairs if (rb is None or indice_pairs.shape[2] > 0 or rb.n_in == 0) else rb.pair_native
    if rb is not None and indice_pair_num.numel() != rb.kv:
        indice_pair_num = rb.num_per_loc
    if inverse:
        native = rb.native_swapped() if rb is not None else torch.stack(
            [indice_pairs[1], indice_pairs[0]]).contiguous()
    plan = _plan_of(rb)
    if native.shape[2] == n_in or not need_din:
        return igemm_bwd(features, out_bp, filters, table, mask, argsort, native, indice_pair_num,
                         subm, plan, need_din, tile_order=tile_order,
                         dense_rows=_dense_rows(rb, n_in, which) if rb is not None else False)
    return (igemm_dgrad(out_bp, filters, table, mask, argsort, n_in, subm, tile_order=tile_order),
            igemm_wgrad(features, out_bp, filters.shape, native, indice_pair_num, subm, plan))


def implicit_gemm(features: torch.Tensor, filters: torch.Tensor, pair_fwd: torch.Tensor,
                  pair_mask_fwd_splits: List[torch.Tensor],
                  mask_argsort_fwd_splits: List[torch.Tensor], num_activate_out: int,
                  masks: List[np.ndarray], is_train: bool, is_subm: bool, timer=None,
                  fp32_accum: Optional[bool] = None, bias: Optional[torch.Tensor] = None,
                  act_alpha: float = 0.0, act_beta: float = 0.0,
                  act_type: int = Activation.None_, output_scale: float = 1.0,
                  scale: Optional[torch.Tensor] = None, output_add: Optional[torch.Tensor] = None,
                  output_add_scale: float = 0.0, output_dtype: Optional[torch.dtype] = None):
    """Masked implicit GEMM forward (ops.py:1450-1664).  Returns (out, mask_out, mask_width);
    the last two exist for signature parity (this wgrad does not consume tile masks)."""
    mask = pair_mask_fwd_splits[0] if pair_mask_fwd_splits else None
    rb: Optional[Rulebook] = rulebook_of(pair_fwd)
    argsort, tile_order = (rb.argsort_fwd if rb is not None else None), 0
    kv = pair_fwd.shape[0]
    if rb is not None and pair_fwd is rb.pair_fwd:
        pair_fwd, mask, argsort, tile_order = tables_of(rb, "fwd", filters.shape[0])
    if features.dtype in (torch.int8, torch.qint8):
        # int8 inference (ops.py:1540-1553,1631-1662): scale = per-channel multiplier, bias is
        # fp32 in output-quantised units, the residual input is scaled by add_scale / out_scale
        assert not is_train, "int8 is inference only"
        out_dt = torch.int8 if output_dtype in (None, torch.int8, torch.qint8) else output_dtype
        beta = output_add_scale / output_scale if output_add is not None else 0.0
        out = igemm_fwd_int8(features, filters, pair_fwd, mask, argsort, num_activate_out,
                             kv // 2 if is_subm else -1, scale, bias, output_add, beta, out_dt,
                             act_type, act_alpha, tile_order=tile_order,
                             sparse_hint=rb is not None and rb.sparse_class is True,
                             hint_rows=rb.heavy_rows if rb is not None else 0)
        if out_dt == torch.int8 and features.is_quantized:
            out = torch._make_per_tensor_quantized_tensor(out, float(output_scale), 0)
        return out, None, -1
    if scale is not None or output_add is not None:
        raise NotImplementedError("scale / output_add belong to the int8 path")
    out = igemm_fwd(features, filters, pair_fwd, mask, argsort, num_activate_out,
                    kv // 2 if is_subm else -1, bias, act_type, act_alpha, tile_order=tile_order)
    return out, None, -1


def implicit_gemm_backward(features: torch.Tensor, filters: torch.Tensor, out_bp: torch.Tensor,
                           pair_fwd: torch.Tensor, pair_bwd: torch.Tensor,
                           pair_mask_fwd_splits: List[torch.Tensor],
                           pair_mask_bwd_splits: List[torch.Tensor],
                           mask_argsort_fwd_splits: List[torch.Tensor],
                           mask_argsort_bwd_splits: List[torch.Tensor],
                           mask_output_fwd: Optional[torch.Tensor], masks: List[np.ndarray],
                           mask_width: int, is_subm: bool, timer=None,
                           fp32_accum: Optional[bool] = None, need_din: bool = True):
    """Masked implicit GEMM backward (ops.py:1667-1896): returns (din, dfilters)."""
    rb: Optional[Rulebook] = rulebook_of(pair_fwd)
    n_in = features.shape[0]
    if rb is not None and rb.pair_native is not None:
        native, num = rb.pair_native, rb.num_per_loc
    else:
        native, num = _native_from_table(pair_fwd if is_subm else pair_bwd, is_subm)
    plan = _plan_of(rb)
    tile_order = 0
    if is_subm:
        table, mask = pair_fwd, pair_mask_fwd_splits[0]
        argsort = rb.argsort_fwd if rb is not None else None
        if rb is not None and pair_fwd is rb.pair_fwd:
            table, mask, argsort, tile_order = tables_of(rb, "fwd", filters.shape[-1])
    else:
        table, mask = pair_bwd, pair_mask_bwd_splits[0]
        argsort = rb.argsort_bwd if rb is not None else None
        if rb is not None and pair_bwd is rb.pair_bwd:
            table, mask, argsort, tile_order = tables_of(rb, "bwd", filters.shape[-1])
    if native.shape[2] == n_in or not need_din:
        return igemm_bwd(features, out_bp, filters, table, mask, argsort, native, num, is_subm, plan,
                         need_din, tile_order=tile_order,
                         dense_rows=_dense_rows(rb, n_in, "fwd" if is_subm else "bwd"))
    return (igemm_dgrad(out_bp, filters, table, mask, argsort, n_in, is_subm, tile_order=tile_order),
            igemm_wgrad(features, out_bp, filters.shape, native, num, is_subm, plan))


# ------------------------------------------------------------------ pooling
_POOL_CODES = dict(_DTYPES)
_POOL_CODES[torch.int8] = _lib.DTYPE_I8


def _pool_code(t: torch.Tensor) -> int:
    return _dtype_code(t, _POOL_CODES, "pooling")


def _mask_of(pair: torch.Tensor, fwd: bool) -> Optional[torch.Tensor]:
    rb = rulebook_of(pair)
    if rb is None:
        return None
    if fwd:
        return rb.mask_fwd
    # a SubM rulebook keeps ONE mask (bits of pair_fwd); its pair_bwd is the mirrored table, whose
    # bit positions differ -> walk every offset instead
    return None if rb.subm else rb.mask_bwd


@_on_device
def indice_maxpool_implicit_gemm(features: torch.Tensor, indice_pairs: torch.Tensor,
                                 num_activate_out: int, init_zero: bool = False) -> torch.Tensor:
    """out[o] = max over the valid pairs of column o of pair_fwd [kv, n_out] (ops.py:1976-1997)."""
    _require_gpu(features, "features")
    L = _lib.load()
    q = features.is_quantized
    feats = _int_repr(features).contiguous()
    out = torch.empty((num_activate_out, feats.shape[1]), dtype=feats.dtype, device=feats.device)
    _lib.check(L.spx_maxpool_fwd(feats.data_ptr(), out.data_ptr(), indice_pairs.data_ptr(),
                                 _ptr(_mask_of(indice_pairs, True)), num_activate_out, feats.shape[1],
                                 indice_pairs.shape[0], _pool_code(feats), int(init_zero), _stream(feats)))
    if q:
        out = torch._make_per_tensor_quantized_tensor(out, features.q_scale(), features.q_zero_point())
    return out


@_on_device
def indice_maxpool_implicit_gemm_backward(features: torch.Tensor, out_features: torch.Tensor,
                                          out_bp: torch.Tensor, indice_pairs: torch.Tensor) -> torch.Tensor:
    """din from pair_bwd [kv, n_in] (ops.py:2000-2023)."""
    L = _lib.load()
    features, out_features, out_bp = features.contiguous(), out_features.contiguous(), out_bp.contiguous()
    din = torch.empty_like(features)
    _lib.check(L.spx_maxpool_bwd(features.data_ptr(), out_features.data_ptr(), out_bp.data_ptr(),
                                 din.data_ptr(), indice_pairs.data_ptr(),
                                 _ptr(_mask_of(indice_pairs, False)), features.shape[0],
                                 features.shape[1], indice_pairs.shape[0], _pool_code(features),
                                 _stream(features)))
    return din


@_on_device
def indice_avgpool_implicit_gemm(features: torch.Tensor, indice_pairs: torch.Tensor,
                                 num_activate_out: int, calc_count: bool):
    """(mean over the valid pairs, count [n_out] or empty) -- ops.py:2026-2056."""
    _require_gpu(features, "features")
    L = _lib.load()
    features = features.contiguous()
    out = torch.empty((num_activate_out, features.shape[1]), dtype=features.dtype, device=features.device)
    count = (torch.empty((num_activate_out,), dtype=torch.int32, device=features.device)
             if calc_count else None)
    _lib.check(L.spx_avgpool_fwd(features.data_ptr(), out.data_ptr(), _ptr(count), indice_pairs.data_ptr(),
                                 _ptr(_mask_of(indice_pairs, True)), num_activate_out, features.shape[1],
                                 indice_pairs.shape[0], _pool_code(features), _stream(features)))
    return out, (count if count is not None else torch.Tensor())


@_on_device
def indice_avgpool_implicit_gemm_backward(out_bp: torch.Tensor, indice_pairs: torch.Tensor,
                                          count_out: torch.Tensor) -> torch.Tensor:
    """din[i] = sum_o dout[o] / count[o] over pair_bwd [kv, n_in] (cf. ops.py:2059-2084).  With
    SPCONV_AMD_REFERENCE_QUIRKS=1 the reference's own arithmetic (it MULTIPLIES by the count, maxpool.py:262-300): the
    Python constant is the single source of truth and is handed to the library with every call (round-4 ADVICE: the
    native side used to re-read the environment by itself)."""
    from spconv_amd import constants
    L = _lib.load()
    _lib.check(L.spx_set_option(b"SPCONV_AMD_REFERENCE_QUIRKS", int(bool(constants.REFERENCE_QUIRKS))))
    out_bp = out_bp.contiguous()
    n_in = indice_pairs.shape[1]
    din = torch.empty((n_in, out_bp.shape[1]), dtype=out_bp.dtype, device=out_bp.device)
    _lib.check(L.spx_avgpool_bwd(out_bp.data_ptr(), din.data_ptr(), count_out.data_ptr(),
                                 indice_pairs.data_ptr(), _ptr(_mask_of(indice_pairs, False)), n_in,
                                 out_bp.shape[1], indice_pairs.shape[0], _pool_code(out_bp),
                                 _stream(out_bp)))
    return din


def indice_maxpool(features: torch.Tensor, indice_pairs: torch.Tensor, indice_pair_num: torch.Tensor,
                   num_activate_out: int) -> torch.Tensor:
    """ConvAlgo.Native max pool on the lists [2, kv, N_in] (ops.py:1899-1935).  Its output starts
    as zeros in the reference, so the result is max(0, max over the pairs); kept."""
    rb = rulebook_of(indice_pairs)
    table = rb.pair_fwd if rb is not None else _table_from_native(
        indice_pairs, indice_pair_num, num_activate_out, False, False)[0]
    if rb is not None:
        attach_rulebook(table, rb)
    return indice_maxpool_implicit_gemm(features, table, num_activate_out, init_zero=True)


def indice_maxpool_backward(features, out_features, out_bp, indice_pairs, indice_pair_num):
    """ConvAlgo.Native max pool backward (ops.py:1938-1973)."""
    rb = rulebook_of(indice_pairs)
    n_in = features.shape[0]
    table = rb.pair_bwd if rb is not None and rb.pair_bwd is not None else _table_from_native(
        indice_pairs, indice_pair_num, n_in, False, True)[0]
    if rb is not None:
        attach_rulebook(table, rb)
    return indice_maxpool_implicit_gemm_backward(features, out_features, out_bp, table)


def global_pool_rearrange(indices: torch.Tensor, batch_size: int):
    """Row ids of every batch item, padded to [batch, N], and the counts (ops.py:2087-2100).  One
    stable sort by batch id + a scatter: no per-scene loop, no read-back."""
    n = indices.shape[0]
    dev = indices.device
    out = torch.zeros((batch_size, n), dtype=torch.int32, device=dev)
    if n == 0:
        return out, torch.zeros((batch_size,), dtype=torch.int32, device=dev)
    b = indices[:, 0].long()
    key = torch.where((b >= 0) & (b < batch_size), b, torch.full_like(b, batch_size))
    order = torch.argsort(key, stable=True)
    skey = key[order]
    counts = torch.bincount(key, minlength=batch_size + 1)
    starts = torch.cumsum(counts, 0) - counts
    col = torch.arange(n, device=dev) - starts[skey]
    keep = skey < batch_size
    out[skey[keep], col[keep]] = order[keep].int()
    return out, counts[:batch_size].int()
