"""The gather-GEMM drivers: forward (float and int8), dgrad, wgrad, and the deferred second stage of the weight gradient.

Owns: the per-thread output policy and BatchNorm-statistics sink of the forward, the pending jobs of the deferred stage,
and THE padding rule (`_padded_ck`).  The backward's choice of kernel family is made in ops.igemm_bwd; which row orders
and table forms reach which kernel is tabulated in DESIGN.md section 3.0.
"""
from __future__ import annotations

import contextlib
import ctypes
import functools
import os
import threading
from typing import Optional

import numpy as np
import torch

from spconv_amd import _lib
from spconv_amd.pytorch._rulebook import (_MFMA_COUT, _ROWS_LAYOUT, Activation, _dtype_code, _int_repr, _on_device, _ptr,
                                          _require_gpu, _stream, _with_hints, _ws)

# SPX_OUT_CACHED (include/spconv_amd.h): inside this context igemm_fwd asks for result rows that stay in
# the caches -- SparseSequential opens it around a convolution whose output a BatchNorm reads next
_OUT_CACHED = 0x100
_TILE_ORDER = 0x200           # SPX_TILE_ORDER: tables of the int8 forward are stored in tile order
_ROWS_LAYOUT_ACT = 0x400      # SPX_ROWS_LAYOUT_ACT: `argsort` of the int8 forward is a rows layout blob
_SPARSE_HINT = 0x800          # SPX_SPARSE_HINT: the host has seen class word 1 (launch-shape hint)
_out_policy = threading.local()


@contextlib.contextmanager
def output_stays_cached():
    prev = getattr(_out_policy, "cached", False)
    _out_policy.cached = True
    try:
        yield
    finally:
        _out_policy.cached = prev


# BatchNorm statistics out of the convolution's epilogue (include/spconv_amd.h: spx_igemm_fwd_stats).  SparseSequential
# opens `collect_bn_stats()` around a training-mode convolution that a plain BatchNorm1d follows; the first plain
# igemm_fwd inside it (no bias, no activation, kernel volume <= 32, MFMA shapes) leaves the per-workgroup {rows, mean, M2}
# records in the sink, and norm.batch_norm starts at its merge step.  Anything else leaves the sink empty and the
# normalisation layer runs its own statistics pass.  SPCONV_AMD_BN_EPILOGUE=0 switches it off (ops.BN_EPILOGUE).
_stats_req = threading.local()


class StatsSink:
    __slots__ = ("n_live", "records", "count", "rows", "channels")

    def __init__(self):
        self.n_live, self.records, self.count, self.rows, self.channels = None, None, 0, 0, 0


@contextlib.contextmanager
def collect_bn_stats():
    sink = StatsSink()
    prev = getattr(_stats_req, "sink", None)
    _stats_req.sink = sink
    try:
        yield sink
    finally:
        _stats_req.sink = prev


def current_stats_sink() -> Optional[StatsSink]:
    return getattr(_stats_req, "sink", None)


def _check_feat(features: torch.Tensor, filters: torch.Tensor):
    _require_gpu(features, "features")
    if features.dtype != filters.dtype:
        raise TypeError(f"features ({features.dtype}) and filters ({filters.dtype}) must share a dtype")
    if features.dtype in (torch.int8, torch.qint8):
        raise NotImplementedError("int8 tensors go through implicit_gemm / igemm_fwd_int8 "
                                  "(inference only, like the reference)")


_OUT_CODES = {torch.int8: _lib.DTYPE_I8, torch.float16: _lib.DTYPE_F16,
              torch.bfloat16: _lib.DTYPE_BF16, torch.float32: _lib.DTYPE_F32}


@_on_device
def igemm_fwd_int8(features: torch.Tensor, filters: torch.Tensor, pair: torch.Tensor,
                   mask: Optional[torch.Tensor], argsort: Optional[torch.Tensor], n_out: int,
                   identity_k: int = -1, scale: Optional[torch.Tensor] = None,
                   bias: Optional[torch.Tensor] = None, add: Optional[torch.Tensor] = None,
                   add_scale: float = 0.0, out_dtype: torch.dtype = torch.int8,
                   act_type: int = Activation.None_, act_alpha: float = 0.0,
                   tile_order: int = 0, sparse_hint: bool = False, hint_rows: int = 0) -> torch.Tensor:
    """int8 inference forward (i32 accumulate on v_mfma_i32_16x16x64_i8):
    ``v = acc * scale[k] + bias[k] + add * add_scale; v = act(v)``; int8 output =
    ``clip(round_half_even(v), -128, 127)`` (reference numerics test/test_all_algo.py:272-287)."""
    _require_gpu(features, "features")
    L = _lib.load()
    features = _int_repr(features).contiguous()
    filters = _int_repr(filters).contiguous()
    if features.dtype != torch.int8 or filters.dtype != torch.int8:
        raise TypeError("igemm_fwd_int8 needs int8 features and filters")
    K0, C0 = filters.shape[0], filters.shape[-1]
    kv = filters.numel() // (K0 * C0)
    assert features.shape[1] == C0, "channel size mismatch"
    C, K = _padded_ck(torch.int8, "fwd", C0, K0, kv)
    features, filters = _pad_last(features, C), _pad_first(_pad_last(filters, C), K)
    out = torch.empty((n_out, K), dtype=out_dtype, device=features.device)
    f32 = lambda t: None if t is None else t.to(device=features.device, dtype=torch.float32).contiguous()
    scale, bias = f32(scale), f32(bias)
    if K != K0:
        scale = None if scale is None else torch.nn.functional.pad(scale.reshape(-1), (0, K - K0), value=1.0)
        bias = None if bias is None else torch.nn.functional.pad(bias.reshape(-1), (0, K - K0))
    if add is not None:
        add = _int_repr(add).contiguous()
        assert add.dtype == torch.int8 and tuple(add.shape) == (n_out, K0)
        add = _pad_last(add, K)
    if sparse_hint and int(tile_order) == _ROWS_LAYOUT:
        # The hint sizes the appendix part of the grid: rows past it would never be computed (round-4 ADVICE).  It is
        # therefore taken from what has been READ from this very blob (poll_class / sparse_neighbourhoods leave it on the
        # tensor), never from a caller's number alone: unknown -> no hint (the launch reserves n / 4 rows' worth).
        known = getattr(argsort, "_spx_heavy", None)
        if known is None:
            sparse_hint, hint_rows = False, 0
        else:
            hint_rows = max(int(hint_rows), int(known))
    _lib.check(L.spx_igemm_fwd_int8(features.data_ptr(), filters.data_ptr(), out.data_ptr(), _ptr(pair),
                                    _ptr(mask), _ptr(argsort), features.shape[0], n_out, C, K, kv,
                                    identity_k, _ptr(scale), _ptr(bias), _ptr(add), float(add_scale),
                                    _OUT_CODES[out_dtype],
                                    int(act_type) | (0 if argsort is None else
                                                     {0: 0, 1: _TILE_ORDER, 2: _ROWS_LAYOUT_ACT}[int(tile_order)])
                                    | ((_SPARSE_HINT | (min(65535, -(-int(hint_rows) // 64)) << 16)) if sparse_hint else 0),
                                    float(act_alpha), _stream(features)))
    return out if K == K0 else out[:, :K0].contiguous()


def _lane_mult(dtype: torch.dtype) -> int:
    """Channels per 16-byte MFMA lane piece: reduction lengths must be a multiple of this."""
    return 4 if dtype == torch.float32 else 16 if dtype == torch.int8 else 8


_WIDE_TILE = 128        # column block of the wide launches (csrc/igemm_wide.hip: kWideNT)


def _round_cout(c: int) -> int:
    """Smallest output width the MFMA kernels run: an instantiated width up to 256, the next multiple of the column
    block beyond (csrc/igemm_wide.hip: one column-blocked launch, at most 127 zero columns)."""
    for v in _MFMA_COUT:
        if c <= v:
            return v
    return -(-c // _WIDE_TILE) * _WIDE_TILE


def _pad_last(t: torch.Tensor, to: int) -> torch.Tensor:
    """Last dimension zero-padded to `to` entries: one launch of spx_pad_rows for contiguous CUDA tensors of 2- / 4-byte
    elements outside autograd (torch's pad is a fill + a copy: 4 of the ~190 launches of a backbone step went there)."""
    if t.shape[-1] == to:
        return t
    if (t.is_cuda and t.is_contiguous() and t.element_size() in (2, 4) and t.numel() > 0
            and not (torch.is_grad_enabled() and t.requires_grad)
            and not t.is_quantized):
        out = torch.empty(t.shape[:-1] + (to,), dtype=t.dtype, device=t.device)
        es = t.element_size()
        with torch.cuda.device(t.device):
            _lib.check(_lib.load().spx_pad_rows(t.data_ptr(), out.data_ptr(), t.numel() // t.shape[-1],
                                                t.shape[-1] * es, to * es, _stream(t)))
        return out
    return torch.nn.functional.pad(t, (0, to - t.shape[-1]))


def _pad_first(t: torch.Tensor, to: int) -> torch.Tensor:
    if t.shape[0] == to:
        return t
    pad = [0, 0] * (t.ndim - 1) + [0, to - t.shape[0]]
    return torch.nn.functional.pad(t, pad)


@functools.lru_cache(maxsize=None)       # (a pure function of five small values, asked for every launch)
def _padded_ck(dtype: torch.dtype, role: str, C0: int, K0: int, kv: int):
    """THE padding rule: the (C, K) a driver runs filters [K0, kv, C0] in.  The MFMA kernels take reduction lengths in
    whole 16-byte lane pieces and the output widths of _MFMA_COUT; beyond 256 columns the column-blocked launch takes
    every multiple of 128 (float and int8 alike).  Shapes they are not instantiated for (a backbone's first layer has
    3-5 input channels; widths like 48, 96 or 320) are zero-padded to the next supported shape instead of falling to the
    one-thread-per-output generic kernel: the extra columns cost a few bytes per row and contribute exact zeros; the
    driver slices them off its result.  Only kernel volumes beyond 128 keep the generic kernel, and their shape.  role
    "fwd" reduces over C into K columns, "dgrad" over K into C columns; "wgrad" has both as lane dimensions."""
    if dtype == torch.float64:                  # csrc/igemm_f64.hip runs every width as it is
        return C0, K0
    lane = _lane_mult(dtype)
    if role == "wgrad":
        return -(-C0 // lane) * lane, -(-K0 // lane) * lane
    red, out = (C0, K0) if role == "fwd" else (K0, C0)
    width = _round_cout(out) if (kv <= 128 or dtype == torch.int8) else out     # (kv > 128: the grouped kernel, any width)
    red = -(-red // lane) * lane
    return (red, width) if role == "fwd" else (width, red)


@_on_device
def igemm_fwd(features: torch.Tensor, filters: torch.Tensor, pair: torch.Tensor,
              mask: Optional[torch.Tensor], argsort: Optional[torch.Tensor], n_out: int,
              identity_k: int = -1, bias: Optional[torch.Tensor] = None,
              act_type: int = Activation.None_, act_alpha: float = 0.0,
              tile_order: int = 0) -> torch.Tensor:
    """out[o] = act(bias + sum_k feat[pair[k][o]] @ W[:, k, :].T); filters KRSC.  tile_order: see tables_of."""
    _check_feat(features, filters)
    L = _lib.load()
    K0, C0 = filters.shape[0], filters.shape[-1]
    assert features.shape[1] == C0, "channel size mismatch"
    kv = filters.numel() // (K0 * C0)
    C, K = _padded_ck(features.dtype, "fwd", C0, K0, kv)
    if C != C0 or K != K0:        # (the usual shapes skip even the calls: this runs for every launch)
        features, filters = _pad_last(features, C), _pad_first(_pad_last(filters, C), K)
        bias = None if bias is None else _pad_last(bias, K)
    features, filters = features.contiguous(), filters.contiguous()
    out = torch.empty((n_out, K), dtype=features.dtype, device=features.device)
    if bias is not None:
        bias = bias.to(features.dtype).contiguous()
    f64 = features.dtype == torch.float64
    # every entry point shares its arguments up to the bias pointer
    head = (features.data_ptr(), filters.data_ptr(), out.data_ptr(), _ptr(pair), _ptr(mask), _ptr(argsort),
            int(tile_order) if f64 else _with_hints(int(tile_order), argsort, mask), features.shape[0], n_out, C, K,
            kv, _dtype_code(features), identity_k)
    if f64:
        # csrc/igemm_f64.hip: every width and kernel volume as it is -- no hint, no scratch, no BatchNorm statistics out
        # of the epilogue (a sink stays empty and the normalisation layer runs its own pass)
        _lib.check(L.spx_igemm_fwd(*head, _ptr(bias), int(act_type), float(act_alpha), None, 0, _stream(features)))
        return out
    ws = _ws(L.spx_igemm_acc_bytes(n_out, K, kv), features.device) if kv > 32 else None   # fp32 partial sums
    act = int(act_type) | (_OUT_CACHED if getattr(_out_policy, "cached", False) else 0)
    sink = getattr(_stats_req, "sink", None)
    if (sink is not None and sink.records is None and bias is None and int(act_type) == Activation.None_
            and K == K0 and K <= _MFMA_COUT[-1] and kv <= 32 and n_out > 0):    # (wide layers leave no statistics)
        slots = int(L.spx_igemm_fwd_stats_slots(n_out))
        # [field][channel][workgroup] over the `used` workgroups of the launch (igemm_defs.h bn_record_store): a flat buffer
        records = torch.empty((3 * K * slots,), dtype=torch.float32, device=features.device)
        used = ctypes.c_int(0)
        _lib.check(L.spx_igemm_fwd_stats(*head, None, act, float(act_alpha), None, 0, records.data_ptr(), slots,
                                         _ptr(sink.n_live), ctypes.byref(used), _stream(features)))
        if used.value > 0:
            sink.records, sink.count, sink.rows, sink.channels = records, int(used.value), n_out, K
        return out
    _lib.check(L.spx_igemm_fwd(*head, _ptr(bias), act, float(act_alpha), _ptr(ws), 0 if ws is None else ws.numel(),
                               _stream(features)))
    return out if K == K0 else out[:, :K0].contiguous()


@_on_device
def igemm_dgrad(out_bp: torch.Tensor, filters: torch.Tensor, pair: torch.Tensor,
                mask: Optional[torch.Tensor], argsort: Optional[torch.Tensor], n_in: int,
                subm: bool, tile_order: int = 0) -> torch.Tensor:
    """din[i] = sum_k dout[pair[k][i]] @ W[:, k, :] (SubM: pass the forward table, subm=True)."""
    _check_feat(out_bp, filters)
    L = _lib.load()
    K0, C0 = filters.shape[0], filters.shape[-1]
    kv = filters.numel() // (K0 * C0)
    C, K = _padded_ck(out_bp.dtype, "dgrad", C0, K0, kv)
    if C != C0 or K != K0:
        out_bp, filters = _pad_last(out_bp, K), _pad_first(_pad_last(filters, C), K)
    out_bp, filters = out_bp.contiguous(), filters.contiguous()
    din = torch.empty((n_in, C), dtype=out_bp.dtype, device=out_bp.device)
    code = _dtype_code(out_bp)
    # (float64 needs no scratch: the fp32 partial sums of the grouped kernel volumes > 32 belong to the MFMA kernels)
    ws = None if code == _lib.DTYPE_F64 else _ws(max(L.spx_igemm_dgrad_ws_bytes(C, K, kv, code),
                                                     L.spx_igemm_acc_bytes(n_in, C, kv)), out_bp.device)
    _lib.check(L.spx_igemm_dgrad(out_bp.data_ptr(), filters.data_ptr(), din.data_ptr(), _ptr(pair),
                                 _ptr(mask), _ptr(argsort), _with_hints(int(tile_order), argsort, mask), out_bp.shape[0],
                                 n_in, C, K, kv, code,
                                 int(subm), _ptr(ws), 0 if ws is None else ws.numel(), _stream(out_bp)))
    return din if C == C0 else din[:, :C0].contiguous()


@_on_device
def wgrad_plan(num_per_loc: torch.Tensor, n_in: int, kv: int, subm: bool) -> torch.Tensor:
    """Work plan of wgrad for one rulebook (built once, reused by every backward)."""
    L = _lib.load()
    plan = torch.empty((L.spx_wgrad_plan_bytes(n_in, kv) // 4,), dtype=torch.int32,
                       device=num_per_loc.device)
    _lib.check(L.spx_wgrad_plan(num_per_loc.data_ptr(), n_in, kv, int(subm), plan.data_ptr(),
                                _stream(num_per_loc)))
    return plan


_WGRAD_MAX_KV = 128     # offsets one spx_igemm_wgrad call / one plan covers


def _wgrad_in_groups(features, out_bp, filters_shape, native, num_per_loc, subm: bool, kv: int):
    """Kernel volumes beyond 128 (6x6x6, 7x7x7: the reference's Native path trains any volume,
    ops.py:962-1015): the offsets go through spx_igemm_wgrad 128 at a time, each group with its own
    slice of the lists and explicit per-list counts (SubM: the mirror rule of ops.py:962-968 resolved
    here, on the device)."""
    K0, C0 = filters_shape[0], filters_shape[-1]
    n_in = native.shape[2]
    counts = num_per_loc.to(torch.int32).clone()
    if subm:
        centre = kv // 2
        counts[centre] = n_in
        counts[centre + 1:] = num_per_loc[:kv - centre - 1].flip(0)
    dw = torch.empty((K0, kv, C0), dtype=features.dtype, device=features.device)
    for kbase in range(0, kv, _WGRAD_MAX_KV):
        g = min(_WGRAD_MAX_KV, kv - kbase)
        part = igemm_wgrad(features, out_bp, (K0, g, C0), native[:, kbase:kbase + g].contiguous(),
                           counts[kbase:kbase + g].contiguous(), False, None)
        dw[:, kbase:kbase + g] = part
    return dw.view(tuple(filters_shape))


@_on_device
def igemm_wgrad(features: torch.Tensor, out_bp: torch.Tensor, filters_shape, native: torch.Tensor,
                num_per_loc: torch.Tensor, subm: bool,
                plan: Optional[torch.Tensor] = None) -> torch.Tensor:
    """dW[:, k, :] = sum_j dout[native[1][k][j]].T (x) feat[native[0][k][j]]."""
    _require_gpu(features, "features")
    L = _lib.load()
    K0, C0 = filters_shape[0], filters_shape[-1]
    kv = int(np.prod(filters_shape)) // (K0 * C0)
    if kv > _WGRAD_MAX_KV:
        return _wgrad_in_groups(features, out_bp, filters_shape, native, num_per_loc, subm, kv)
    C, K = _padded_ck(features.dtype, "wgrad", C0, K0, kv)
    f64 = features.dtype == torch.float64
    features = _pad_last(features, C).contiguous()
    out_bp = _pad_last(out_bp, K).contiguous()
    n_in = native.shape[2]
    shape = (K,) + tuple(filters_shape[1:-1]) + (C,)
    dw = torch.empty(shape, dtype=features.dtype, device=features.device)
    ws = _ws(L.spx_igemm_wgrad_ws_bytes_dtype(n_in, C, K, kv, _lib.DTYPE_F64) if f64
             else L.spx_igemm_wgrad_ws_bytes(n_in, C, K, kv), features.device)
    _lib.check(L.spx_igemm_wgrad(features.data_ptr(), out_bp.data_ptr(), dw.data_ptr(),
                                 native.data_ptr(), num_per_loc.data_ptr(), _ptr(plan), n_in,
                                 out_bp.shape[0], C, K, kv, _dtype_code(features), int(subm),
                                 ws.data_ptr(), ws.numel(), _stream(features)))
    return dw if (C == C0 and K == K0) else dw[:K0, ..., :C0].contiguous()


# The weight gradient's second stage, deferred to the END of a backward pass (include/spconv_amd.h: spx_igemm_bwd_deferred
# / spx_wgrad_stage2_batch).  Nothing inside a pass waits for a layer's dW when the weight is a leaf whose .grad is empty
# (AccumulateGrad then just keeps the tensor it is handed): the reductions of the partial tiles -- a dependent 4-9 us
# launch per layer -- leave the chain and run as ONE launch per sixteen layers from the autograd engine's final callback.
# Only inside `deferred_wgrad()` -- the static training runner opens it around its backward call; eager passes never
# defer -- and not for weights that are not leaves (a cast in front: its backward READS dW), that already hold a gradient
# (accumulation reads it), that carry hooks, or whose shapes take a path without a second stage.  A weight that shows up a
# second time in a pass flushes what is pending first (the engine adds the two gradients).
# SPCONV_AMD_WGRAD_DEFER=0 turns it off.
_WGRAD_DEFER = os.environ.get("SPCONV_AMD_WGRAD_DEFER", "1") != "0"
_STAGE2_JOB_BYTES = 64     # SPX_STAGE2_JOB_BYTES
_defer_depth = [0]
_defer_passes = {}         # autograd graph-task id -> {"jobs": [...], "seen": {weight address}}
_defer_lock = threading.Lock()


class deferred_wgrad:
    """Context of a backward pass whose caller reads no weight gradient before the pass has ended."""

    def __enter__(self):
        _defer_depth[0] += 1
        return self

    def __exit__(self, *exc):
        _defer_depth[0] -= 1
        if _defer_depth[0] == 0 and _defer_passes:
            # (a pass that ended in an exception never reached its final callback: what it left pending is dropped)
            with _defer_lock:
                _defer_passes.clear()
        return False


def _flush_deferred(task_id: int) -> None:
    with _defer_lock:
        st = _defer_passes.pop(task_id, None)
    if not st or not st["jobs"]:
        return
    L = _lib.load()
    by_dev = {}
    for job, param, _keep in st["jobs"]:
        g = param.grad
        if g is not None:                   # (the engine kept the tensor it was handed, or made one of its own)
            if not (g.is_contiguous() and g.shape == param.shape and g.dtype == param.dtype):
                raise RuntimeError("deferred weight gradient: .grad of a weight has another layout than the weight")
            L.spx_stage2_job_retarget(job, g.data_ptr())
        by_dev.setdefault(param.device, []).append(job)
    for dev, jobs in by_dev.items():
        blob = b"".join(j.raw for j in jobs)
        with torch.cuda.device(dev):
            _lib.check(L.spx_wgrad_stage2_batch(blob, len(jobs), torch._C._cuda_getCurrentRawStream(dev.index)))


def _defer_state(filters: torch.Tensor):
    """The pending list of the backward pass this call belongs to, or None (see above)."""
    if not (_WGRAD_DEFER and _defer_depth[0] > 0 and filters.is_cuda):
        return None
    if not (filters.is_leaf and filters.requires_grad and filters.grad is None and filters.is_contiguous()):
        return None
    if filters._backward_hooks or getattr(filters, "_post_accumulate_grad_hooks", None):
        return None
    task = torch._C._current_graph_task_id()
    if task < 0:
        return None
    with _defer_lock:
        st = _defer_passes.get(task)
        if st is None:
            try:
                torch.autograd.Variable._execution_engine.queue_callback(lambda t=task: _flush_deferred(t))
            except RuntimeError:            # not inside a backward pass
                return None
            st = _defer_passes[task] = {"jobs": [], "seen": set()}
        key = filters.data_ptr()
        again = key in st["seen"]
        st["seen"].add(key)
    if again:
        # a second use of this weight in the pass: every pending gradient is completed before the engine adds the two
        _flush_deferred(task)
        return None
    return st


@_on_device
def bias_act_inplace(out: torch.Tensor, bias: Optional[torch.Tensor], act_type: int,
                     act_alpha: float = 0.0) -> torch.Tensor:
    """InferenceOps.bias_add_act_inplace & friends (csrc/sparse/inference.py:26-146)."""
    L = _lib.load()
    if bias is not None:
        bias = bias.to(out.dtype).contiguous()
    _lib.check(L.spx_bias_act_inplace(out.data_ptr(), _ptr(bias), out.shape[0], out.shape[1],
                                      _dtype_code(out), int(act_type), float(act_alpha),
                                      _stream(out)))
    return out
