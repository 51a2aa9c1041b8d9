"""Rulebook builds and the row orders on top of them (rank maps, rows layout, explicit mask sort), and the plumbing
every driver shares (device guard, stream, scratch, dtype codes).

Owns all host state of a `Rulebook`: its tables and row-order fields; `RankMap`, the one association a tensor carries
for its own sake; and the density class -- sparse_class and heavy_rows and the hint on the tensor a driver is handed
(`_spx_dense` / `_spx_heavy`), written by `_set_class` alone, the pending read _class_req, the two prediction attributes
on the owning module and the ring of pinned host slots the class words are copied to.  Which build and row order a call
gets is decided in ops.build_rulebook.
"""
from __future__ import annotations

import collections
import ctypes
import functools
import math
import os
import weakref
from typing import NamedTuple, Optional

import torch

from spconv_amd import _lib
from spconv_amd.pytorch.core import Rulebook

_DTYPES = {torch.float32: _lib.DTYPE_F32, torch.float16: _lib.DTYPE_F16,
           torch.bfloat16: _lib.DTYPE_BF16, torch.float64: _lib.DTYPE_F64}


class Activation:
    """tv.gemm.Activation values used by the reference's conv modules."""
    None_ = _lib.ACT_NONE
    ReLU = _lib.ACT_RELU
    Sigmoid = _lib.ACT_SIGMOID
    LeakyReLU = _lib.ACT_LEAKY_RELU


# ---------------------------------------------------------------- plumbing
def _require_gpu(t: torch.Tensor, what: str) -> None:
    if not t.is_cuda:
        raise NotImplementedError(
            f"spconv_amd runs on MI355X only: {what} is on {t.device}. There is no CPU path "
            f"(move the SparseConvTensor to 'cuda').")


def _stream(t: torch.Tensor) -> int:
    """Raw hipStream_t of torch's current stream on t's device (the C call, not the Stream object:
    this runs for every kernel launch)."""
    return torch._C._cuda_getCurrentRawStream(t.device.index)


def _on_device(fn):
    """Runs a driver with the first tensor argument's device current (torch's DeviceGuard convention):
    kernels, fills and scratch allocations of a call all belong to the device the data lives on, also
    when the caller never called torch.cuda.set_device (model on cuda:1)."""
    @functools.wraps(fn)
    def guarded(*args, **kwargs):
        t = next((a for a in args if isinstance(a, torch.Tensor)), None)
        if t is not None and t.is_cuda and t.device.index != torch.cuda.current_device():
            with torch.cuda.device(t.device):
                return fn(*args, **kwargs)
        return fn(*args, **kwargs)
    return guarded


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


def _ws(nbytes: int, device) -> torch.Tensor:
    return torch.empty((max(int(nbytes), 16),), dtype=torch.uint8, device=device)


def _dtype_code(t: torch.Tensor, codes=_DTYPES, what: str = "feature") -> int:
    try:
        return codes[t.dtype]
    except KeyError:
        raise NotImplementedError(f"unsupported {what} dtype {t.dtype}") from None


def _float_code(t: torch.Tensor, what: str) -> int:
    """dtype code of the feature rows a row op takes (the union, collapse, select, interp and point-voxel wrappers):
    the four floating dtypes, nothing quantized."""
    if t.is_quantized or t.dtype not in _DTYPES:
        raise NotImplementedError(f"{what}: features must be float16, bfloat16, float32 or float64, got {t.dtype}")
    return _DTYPES[t.dtype]


def _check_count(t: Optional[torch.Tensor], what: str) -> None:
    """A device-side count (n_live, n_points) is None or a CUDA int32 tensor whose first element is read."""
    if t is not None and not (t.is_cuda and t.dtype == torch.int32 and t.numel() >= 1):
        raise ValueError(f"{what} is a CUDA int32 tensor of one element")


def _kv(ksize) -> int:
    return int(functools.reduce(lambda a, b: a * b, ksize, 1))


def _cells(batch_size: int, dims) -> int:
    return int(batch_size) * math.prod(map(int, dims))


def _int_repr(t: torch.Tensor) -> torch.Tensor:
    return t.int_repr() if t.is_quantized else t


_MFMA_COUT = (16, 32, 64, 128, 256)      # output widths the MFMA gather-GEMM kernels are instantiated for

_POINT_VANISH_MSG = """Your points vanished here, this usually because you provide
conv params that may ignore some input points. Example:
    spatial_shape=[8, 200, 200]
    ksize=3
    stride=2
    padding=[0, 1, 1]
    dilation=1
    Coordinates=[[0, 7, 153, 142]]
these params will cause ALL points in z == 7 dropped because of padding_z=0.
enlarge your spatial shape or change your conv param to make sure
every input point has a corresponding output point.
Your Conv Params:
    spatial_shape={}
    ksize={}
    stride={}
    padding={}
    dilation={}"""


def get_conv_output_size(input_size, kernel_size, stride, padding, dilation):
    return [1 if kernel_size[i] == -1 else
            (input_size[i] + 2 * padding[i] - dilation[i] * (kernel_size[i] - 1) - 1) // stride[i] + 1
            for i in range(len(input_size))]


def get_deconv_output_size(input_size, kernel_size, stride, padding, dilation, output_padding):
    output_size = []
    for i in range(len(input_size)):
        if kernel_size[i] == -1:
            raise ValueError("deconv don't support kernel_size < 0")
        output_size.append((input_size[i] - 1) * stride[i] - 2 * padding[i] + kernel_size[i]
                           + output_padding[i])
    return output_size


def _build_subm(L, indices, batch_size, spatial_shape, ksize, dilation, need_native, need_bwd_table, stream) -> Rulebook:
    """SubM rulebook: over the level's rank map when the index tensor carries one, else through the hash table."""
    dev = indices.device
    n_in, ndim = indices.shape[0], indices.shape[1] - 1
    kv = _kv(ksize)
    i32 = dict(dtype=torch.int32, device=dev)
    # the -1 filled tables live in ONE buffer, so that the library needs a single fill
    tb = kv * n_in
    nat = 2 if need_native else 0
    buf = torch.empty(((1 + nat + (1 if need_bwd_table else 0)) * tb,), **i32)
    pair_fwd = buf[:tb].view(kv, n_in)
    native = buf[tb:3 * tb].view(2, kv, n_in) if need_native else None
    pair_bwd = buf[(1 + nat) * tb:].view(kv, n_in) if need_bwd_table else None
    mask = torch.empty((n_in, (kv + 31) // 32), **i32)
    num = torch.empty((kv,), **i32) if need_native else None
    head = (indices.data_ptr(), n_in, ndim, batch_size, _lib.ints(spatial_shape), _lib.ints(ksize), _lib.ints(dilation),
            pair_fwd.data_ptr(), _ptr(pair_bwd), mask.data_ptr(), _ptr(native), _ptr(num))
    rm = _rankmap_of(indices, batch_size, spatial_shape, n_in, kv)
    if rm is not None:
        # rows in key order with their level's rank map (a sorted-order strided layer built them): no table
        ws = _ws(L.spx_subm_rulebook_ranked_ws_bytes(n_in, kv), dev)
        _lib.check(L.spx_subm_rulebook_ranked(*head, rm.data_ptr(), rm.numel() * 4, ws.data_ptr(), ws.numel(), stream))
    else:
        ws = _ws(L.spx_subm_rulebook_ws_bytes(n_in, kv), dev)
        _lib.check(L.spx_subm_rulebook(*head, ws.data_ptr(), ws.numel(), stream))
    return Rulebook(indices, pair_fwd, pair_bwd, mask, mask, native, num, n_in, n_in, kv, True)


def _build_conv(L, indices, batch_size, spatial_shape, out_shape, ksize, stride, padding, dilation, transpose,
                need_native, num_out_act_bound, static_num_out, in_key_order: bool, stream) -> Rulebook:
    """Regular / transposed convolution rulebook in one of four forms.  in_key_order=False: outputs in first-seen order
    through the hash table (spx_conv_rulebook_count / _fill / _static); True: in key order through the output level's
    rank map (spx_conv_rulebook_*_sorted), which then travels with out_indices.  static_num_out > 0 is the static-shape
    form of either: no count, nothing read back, the counters on the device."""
    dev = indices.device
    n_in, ndim = indices.shape[0], indices.shape[1] - 1
    kv = _kv(ksize)
    i32 = dict(dtype=torch.int32, device=dev)
    static = static_num_out > 0
    head = (indices.data_ptr(), n_in, ndim, batch_size, _lib.ints(spatial_shape), _lib.ints(out_shape), _lib.ints(ksize),
            _lib.ints(stride), _lib.ints(padding), _lib.ints(dilation))
    n_out_dev = None
    if in_key_order:
        count, fill, fill_static = (L.spx_conv_rulebook_count_sorted, L.spx_conv_rulebook_fill_sorted,
                                    L.spx_conv_rulebook_static_sorted)
        cells = torch.empty((L.spx_rankmap_bytes(ndim, batch_size, _lib.ints(out_shape)) // 4,), **i32)
        ws = _ws(L.spx_conv_rulebook_sorted_ws_bytes(n_in, ndim, batch_size, _lib.ints(out_shape), _lib.ints(ksize)), dev)
        tail = (cells.data_ptr(), cells.numel() * 4, ws.data_ptr(), ws.numel())
        if static:
            n_out_dev = torch.empty((4,), **i32)      # {found, 0, live rows = min(found, bound), -}
    else:
        count, fill, fill_static = L.spx_conv_rulebook_count, L.spx_conv_rulebook_fill, L.spx_conv_rulebook_static
        head += (int(transpose),)
        ws = _ws(L.spx_conv_rulebook_ws_bytes(n_in, ndim, _lib.ints(ksize), _lib.ints(stride), _lib.ints(dilation),
                                              int(transpose)), dev)
        tail = (ws.data_ptr(), ws.numel())
    if static:
        n_out = int(static_num_out)
    else:
        n_out_c = ctypes.c_int(0)
        _lib.check(count(*head, *tail, ctypes.byref(n_out_c), stream))
        n_out = int(n_out_c.value)
        if n_out == 0:
            raise ValueError(_POINT_VANISH_MSG.format(spatial_shape, ksize, stride, padding, dilation))
        if 0 < num_out_act_bound < n_out:
            # the reference's bounded mode (ops.py:263-266, indices.py:460-499): at most `bound` outputs exist; here the
            # FIRST `bound` in the build's own order (first seen, or smallest keys) survive, pairs into the rest are dropped
            n_out = int(num_out_act_bound)
    words = (kv + 31) // 32
    out_indices = torch.empty((n_out, ndim + 1), **i32)
    pair_fwd = torch.empty((kv, n_out), **i32)
    pair_bwd = torch.empty((kv, n_in), **i32)
    mask_fwd = torch.empty((n_out, words), **i32)
    mask_bwd = torch.empty((n_in, words), **i32)
    if static and not in_key_order:
        # (between the masks and the lists, where this form has always had it: a captured build's pool layout)
        n_out_dev = torch.empty((2,), **i32)
    native = torch.empty((2, kv, n_in), **i32) if need_native else None
    num = torch.empty((kv,), **i32) if need_native else None
    outs = (out_indices, pair_fwd, pair_bwd, mask_fwd, mask_bwd, native, num)
    out_ptrs = tuple(_ptr(t) for t in outs)
    if static:
        _lib.check(fill_static(*head, n_out, *out_ptrs, n_out_dev.data_ptr(), *tail, stream))
    else:
        _lib.check(fill(*head, n_out, *out_ptrs, *tail, stream))
    rb = Rulebook(*outs, n_in, n_out, kv, False)
    rb.n_out_dev = n_out_dev
    if static and in_key_order:         # (the live-row count is written by the build itself: no clamp launch behind it)
        rb.n_out_dev, rb.out_n_live_dev = n_out_dev[:2], n_out_dev[2:3]
    if in_key_order:
        rb.rankmap = cells
        _tag_rank_map(outs[0], cells, batch_size, out_shape, n_out)
    return rb


class RankMap(NamedTuple):
    """The rank map of one level (include/spconv_amd.h, sorted-order levels), what it describes, and the version counter
    and address of the index tensor it was built from.  Attached to that tensor as `_spx_rankmap`: the one tensor attribute
    that is an association in its own right -- index tensors travel through user code from the strided layer that made
    them to the SubM layers behind it.  Readers index it; a bare 4-tuple (no version, no address) is never invalidated."""
    cells: torch.Tensor
    batch_size: int
    shape: tuple
    rows: int
    version: Optional[int] = None
    ptr: Optional[int] = None


def _tag_rank_map(indices: torch.Tensor, cells: torch.Tensor, batch_size: int, shape, rows: int) -> None:
    indices._spx_rankmap = RankMap(cells, batch_size, tuple(int(v) for v in shape), rows,
                                   indices._version, indices.data_ptr())


def _rankmap_of(indices: torch.Tensor, batch_size: int, spatial_shape, n: int, kv: int):
    """The rank map a sorted-order build attached to exactly this index tensor, if it describes this level -- and if
    the tensor has not been written since (its version counter and storage are the ones recorded with the map: an
    in-place edit of `out.indices` between the strided layer and the SubM layer behind it drops the map, round-5
    ADVICE)."""
    rm = getattr(indices, "_spx_rankmap", None)
    if rm is None or not (1 < kv <= 128) or n > (4 << 20):
        return None
    cells, bs, shape, rows = rm[:4]
    if bs != batch_size or shape != tuple(int(v) for v in spatial_shape) or rows != n or cells.device != indices.device:
        return None
    if len(rm) >= 6 and (rm[4] != indices._version or rm[5] != indices.data_ptr()):
        indices._spx_rankmap = None
        return None
    return cells


# Level 1 in key order.  The levels behind a strided layer are numbered by THIS library (ascending key: _build_conv);
# the level a caller hands in is in the caller's order, and its SubM rulebook pays hash insert + probe (the largest
# rulebook build of a backbone: 160 us at 4 x 100 k voxels).  When the caller's rows ARE in ascending, unique key order
# (spconv_amd.pytorch.utils.sort_voxels_by_coordinate; a voxeliser that emits key order), `attach_rank_map` builds the
# level's rank map from them directly (row = rank: a fill + one pass, spx_rankmap_from_sorted) and leaves it on the index
# tensor exactly as a sorted-order strided build does: SubM layers over the tensor then take spx_subm_rulebook_ranked.
# The map costs grid cells / 4 bytes of fill: taken up to `_RANKMAP_MAX_CELLS_PER_ROW` cells per row and 1 GiB.
_RANKMAP_MAX_CELLS_PER_ROW = float(os.environ.get("SPCONV_AMD_RANKMAP_MAX_CELLS_PER_ROW", "4096"))
_SORTED_MAX_SCRATCH = 1 << 30


def _rankmap_fits(nbytes: int, cells: int, n: int) -> bool:
    """The size gates of a rank map built from the rows themselves (attach_rank_map, key_argsort)."""
    return (0 < nbytes <= _SORTED_MAX_SCRATCH and n > 0
            and not (_RANKMAP_MAX_CELLS_PER_ROW > 0 and cells > _RANKMAP_MAX_CELLS_PER_ROW * n))


@_on_device
def attach_rank_map(indices: torch.Tensor, batch_size: int, spatial_shape, check: bool = True,
                    violation: Optional[torch.Tensor] = None) -> bool:
    """Declares `indices` [n, ndim + 1] (int32, batch index first) to be in ascending, unique coordinate-key order
    (batch-major, last axis fastest; rows with batch index -1 -- static shapes -- trail) and attaches the level's rank
    map to the tensor.  check=True reads the device-side verdict back (ONE synchronisation; a data loader's place): a
    tensor that breaks the contract is left untouched and False is returned.  check=False (inside a stream capture;
    the caller vouches for the order) never synchronises; `violation` (int32 [1] on the device) then receives the
    verdict for whoever wants to read it later (1 = the rows break the contract).  Returns whether a map was attached."""
    _require_gpu(indices, "indices")
    assert indices.dtype == torch.int32 and indices.ndim == 2 and indices.is_contiguous()
    L = _lib.load()
    n, ndim = indices.shape[0], indices.shape[1] - 1
    nbytes = int(L.spx_rankmap_bytes(ndim, batch_size, _lib.ints(spatial_shape)))
    if not _rankmap_fits(nbytes, _cells(batch_size, spatial_shape), n):
        return False
    i32 = dict(dtype=torch.int32, device=indices.device)
    cells_t = torch.empty((nbytes // 4,), **i32)
    bad = torch.empty((1,), **i32) if check else violation
    _lib.check(L.spx_rankmap_from_sorted(indices.data_ptr(), n, ndim, batch_size, _lib.ints(spatial_shape),
                                         cells_t.data_ptr(), nbytes, _ptr(bad), _stream(indices)))
    if check and int(bad.item()) != 0:
        return False
    _tag_rank_map(indices, cells_t, batch_size, spatial_shape, n)
    return True


@_on_device
def key_argsort(indices: torch.Tensor, batch_size: int, spatial_shape, want_indices: bool = True,
                rank_map: bool = False, violation: Optional[torch.Tensor] = None, rows: Optional[torch.Tensor] = None):
    """(order, indices[order]) with order[t] = the row of the t-th smallest coordinate key (batch-major, last axis
    fastest); dead rows (batch index -1) trail in their own order and come out as -1 in every column.  One C-ABI call
    (spx_key_argsort: four launches -- one stable radix pass on the upper key bits, then workgroups per bucket rank
    their rows through an occupancy map in LDS; the keys of a level are unique), nothing read back, so it can sit inside
    a stream capture -- the static runners sort their scene at the entry with it (static.py entry_sort).
    rank_map=True: the sorted index tensor leaves with the level's rank map attached, written by the same bucket pass
    (what attach_rank_map would build from it; same size gates -- beyond them the tensor stays untagged); `violation`
    (int32 [1] on the device) is raised when a coordinate occurs twice.  `rows` ([n, ...] contiguous, row size a
    multiple of 4 bytes: the level's features): a third result, rows[order], written by the same bucket pass.  Returns
    None when the key space of batch x grid does not fit 32 bits."""
    _require_gpu(indices, "indices")
    assert indices.dtype == torch.int32 and indices.ndim == 2 and indices.is_contiguous()
    cells = _cells(batch_size, spatial_shape)
    if cells > 0xffe00000:
        return None
    L = _lib.load()
    n, ndim = indices.shape[0], indices.shape[1] - 1
    order = torch.empty((n,), dtype=torch.int32, device=indices.device)
    out = torch.empty_like(indices) if (want_indices or rank_map) else None
    cells_t = None
    if rank_map:
        nbytes = int(L.spx_rankmap_bytes(ndim, batch_size, _lib.ints(spatial_shape)))
        if _rankmap_fits(nbytes, cells, n):
            cells_t = torch.empty((nbytes // 4,), dtype=torch.int32, device=indices.device)
    ws = _ws(L.spx_key_argsort_ws_bytes(n), indices.device)
    rows_sorted, row_bytes = None, 0
    if rows is not None:
        assert rows.is_cuda and rows.is_contiguous() and rows.shape[0] == n
        row_bytes = (rows.numel() // max(n, 1)) * rows.element_size()
        assert row_bytes % 4 == 0, "rows carried by the sort: row size must be a multiple of 4 bytes"
        rows_sorted = torch.empty_like(rows)
    _lib.check(L.spx_key_argsort(indices.data_ptr(), n, ndim, int(batch_size), _lib.ints(spatial_shape),
                                 order.data_ptr(), _ptr(out), _ptr(cells_t), 0 if cells_t is None else cells_t.numel() * 4,
                                 _ptr(violation), _ptr(rows), _ptr(rows_sorted), row_bytes,
                                 ws.data_ptr(), ws.numel(), _stream(indices)))
    if cells_t is not None:
        _tag_rank_map(out, cells_t, batch_size, spatial_shape, n)
    return (order, out) if rows is None else (order, out, rows_sorted)


# ---- the density class on the HOST, without a synchronisation ------------------------------------------------------
# A launch SHAPE cannot be picked on the device: the weight-stationary gather-GEMM of dense C = K = 64 layers
# (csrc/igemm_ws.hip, 512-row workgroups) and the int8 tile height are host choices.  The class word of a rows layout
# is therefore copied to pinned host memory asynchronously when the layout is built and looked at (never waited for)
# when a launch is prepared: until it has arrived -- the host usually runs ahead of the device on the first layer that
# uses a new rulebook -- the launch goes by what the same layer's previous rulebook turned out to be (an attribute of
# the owning module, `_pred_get`), and inside a stream capture, where nothing can be polled, by that prediction alone.
# Both kernels give bit-identical results, so neither a late answer nor a wrong prediction shows in an output.
# (values and bits of a gather-GEMM call's `tile_order`; the bits of its `act` argument are in _gemm)
_ROWS_LAYOUT = 2              # SPX_ROWS_LAYOUT: `argsort` of a gather-GEMM call is a layout blob
_DENSE_HINT = 0x100           # SPX_DENSE_HINT (include/spconv_amd.h)
_SPARSE_ROWS_HINT = 0x200     # SPX_SPARSE_ROWS_HINT: class word 1 and M of this blob have been READ; M rides in the bits above
_SPARSE_ROWS_SHIFT = 12       # SPX_SPARSE_ROWS_SHIFT
_SPARSE_ROWS_MAX = 0x7ffff    # SPX_SPARSE_ROWS_MAX: an M beyond it travels as no hint
_WS_MIN_ROWS = 98304          # one 512-row workgroup per CU: below ~3/4 of 256 x 512 rows the 128-row tiles fill the chip better
_CLASS_SLOTS = 1024
_class_ring = {}              # device index -> [pinned int32 [_CLASS_SLOTS, 2], next slot, owner tokens]
_PRED_ATTR = "_spx_dense_pred"     # on the owning module (rb.pred_key): the rulebook built for it last time was dense
_CLS0_ATTR = "_spx_class0_pred"    # ... and its rows layout was of class 0 (no appendix)
_LAYOUT_MIN_ROWS = 32768      # smaller SubM rulebooks get no rows layout and no class: launch-bound either way


def _pred_get(key) -> bool:
    """The prediction lives ON the module that owns the rulebooks (round-5 ADVICE: a dict keyed by id(module) outlives
    the module and can be answered by another object that reuses the id)."""
    return bool(getattr(key, _PRED_ATTR, False)) if key is not None else False


def _dense_rule(cls, heavy: int, n: int) -> bool:
    """The dense hint of a measured rulebook: class 0, rows for one 512-row workgroup per CU, three rows in four heavy."""
    return (not cls) and n >= _WS_MIN_ROWS and 4 * heavy >= 3 * n


def _predict(key, cls, heavy: int, n: int) -> None:
    """Leaves on the owning module what its rulebook turned out to be: what its next one is taken for until measured."""
    if key is None:
        return
    try:
        object.__setattr__(key, _PRED_ATTR, _dense_rule(cls, heavy, n))
        if heavy > 0:      # (no row with a neighbour -- the empty scene a runner warms up on -- says nothing)
            object.__setattr__(key, _CLS0_ATTR, (not cls) and 4 * heavy >= n)
    except (AttributeError, TypeError):       # (a key that cannot carry attributes: no prediction)
        pass


def _set_class(rb: Rulebook, cls=None, heavy: int = 0, predict: bool = True) -> None:
    """The ONE writer of a rulebook's class knowledge.  (rb): nothing measured, the hint is the owning module's
    prediction.  (rb, cls, heavy): the two leading words of rb.layout have been read; the module's prediction follows
    unless predict=False.  The drivers take bare tensors: the hint reaches them as an attribute of the layout blob, or
    of mask_fwd when the layout was left out (ops.build_rulebook), set here only.  (The one exception: the estimate
    sparse_neighbourhoods makes from the masks of a rulebook without a layout is a host-side view, sparse_class alone.)"""
    rb.sparse_class, rb.heavy_rows = (None if cls is None else bool(cls)), heavy
    carrier = rb.layout if rb.layout is not None else rb.mask_fwd
    if cls is None:
        carrier._spx_dense = _pred_get(rb.pred_key)
        return
    carrier._spx_dense, carrier._spx_heavy = _dense_rule(cls, heavy, rb.n_out), heavy
    carrier._spx_class = int(bool(cls))
    if predict:
        _predict(rb.pred_key, cls, heavy, rb.n_out)


class _ClassRequest:
    """One asynchronous read of a rows layout's class word (see above)."""
    __slots__ = ("ring", "slot", "token", "event", "key", "n", "rb", "done")

    def resolve(self) -> bool:
        """Non-blocking; True once the request is settled (answer taken, or lost to a wrapped ring)."""
        if self.done or self.ring[2][self.slot] is not self.token:
            self.done = True              # (or the ring wrapped before anybody looked: stay with the prediction)
            return True
        if not self.event.query():
            return False
        cls, heavy = (int(v) for v in self.ring[0][self.slot])
        self.done = True
        rb = self.rb()
        if rb is not None and rb.layout is not None:
            _set_class(rb, cls, heavy)
        else:                                             # (the rulebook is gone: its module still learns from it)
            _predict(self.key, cls, heavy, self.n)
        return True


_class_pending = collections.deque()


def _request_class(rb: Rulebook) -> None:
    """A new rows layout on rb: the hint starts as the prediction, the read of its class word is queued (no capture)."""
    blob = rb.layout
    rb._class_req = None
    if blob is None:
        return
    capturing = torch.cuda.is_current_stream_capturing()
    if not capturing:
        # answers to earlier requests (a layer that uses every rulebook once, right behind its build, never comes back
        # to ask: the next build does it for it)
        while _class_pending and _class_pending[0].resolve():
            _class_pending.popleft()
        if len(_class_pending) > 64:
            _class_pending.popleft()
    _set_class(rb)
    if capturing:
        return
    ring = _class_ring.get(blob.device.index)
    if ring is None:
        ring = [torch.zeros((_CLASS_SLOTS, 2), dtype=torch.int32).pin_memory(), 0, [None] * _CLASS_SLOTS]
        _class_ring[blob.device.index] = ring
    host, slot = ring[0], ring[1]
    ring[1] = (slot + 1) % _CLASS_SLOTS
    req = _ClassRequest()
    req.ring, req.slot, req.token, req.done = ring, slot, object(), False
    req.key, req.n, req.rb = rb.pred_key, rb.n_out, weakref.ref(rb)
    ring[2][slot] = req.token
    host[slot].copy_(blob[:2], non_blocking=True)
    req.event = torch.cuda.Event()
    req.event.record()
    rb._class_req = req
    _class_pending.append(req)


def poll_class(rb: Optional[Rulebook]) -> None:
    """Non-blocking: takes the class word of rb's rows layout if its copy has arrived (see above)."""
    if rb is None or rb.layout is None or rb.sparse_class is not None:
        return
    req = rb._class_req
    if req is not None and not torch.cuda.is_current_stream_capturing() and req.resolve():
        rb._class_req = None


def sparse_rows_hint(tile_order: int, rows) -> int:
    """`tile_order` with the sparse-class hint for an appendix of exactly `rows` rows (None, negative or beyond the bits
    of the word: no hint).  The encoding only -- whether a hint may be given is _with_sparse_hint's business."""
    if tile_order != _ROWS_LAYOUT or rows is None or not 0 <= int(rows) <= _SPARSE_ROWS_MAX:
        return tile_order
    return tile_order | _SPARSE_ROWS_HINT | (int(rows) << _SPARSE_ROWS_SHIFT)


def split_tile_order(word: int):
    """(table form, dense hint, M of the sparse hint or None) of a `tile_order` word as the drivers pass it."""
    rows = (word >> _SPARSE_ROWS_SHIFT) & _SPARSE_ROWS_MAX if word & _SPARSE_ROWS_HINT else None
    return word & 0xff, bool(word & _DENSE_HINT), rows


def _with_sparse_hint(tile_order: int, argsort) -> int:
    """The hint sizes the appendix part of the grid from the EXACT row count: it is given when, and only when, class
    word 1 and M have been READ from this very blob (_set_class leaves both on the tensor; _gemm.igemm_fwd_int8 spells
    out the discipline) -- never from a prediction or a caller's number.  Inside a capture nothing is polled: what was
    read before it shapes the captured launch, and a blob built inside it carries nothing."""
    if tile_order != _ROWS_LAYOUT or getattr(argsort, "_spx_class", None) != 1:
        return tile_order
    return sparse_rows_hint(tile_order, getattr(argsort, "_spx_heavy", None))


def _with_dense_hint(tile_order: int, argsort, mask=None) -> int:
    if tile_order == _ROWS_LAYOUT and getattr(argsort, "_spx_dense", False):
        return tile_order | _DENSE_HINT
    if tile_order == 0 and argsort is None and getattr(mask, "_spx_dense", False):
        return _DENSE_HINT               # (a rulebook whose layout was left out: ops.build_rulebook)
    return tile_order


def _with_hints(tile_order: int, argsort, mask=None) -> int:
    """What the 16-bit forward and dgrad drivers pass as `tile_order`: the dense hint, or else the sparse one (a blob is
    of one class).  Runs for every launch: one pass over the attributes."""
    if tile_order == _ROWS_LAYOUT:
        if getattr(argsort, "_spx_dense", False):
            return tile_order | _DENSE_HINT
        if getattr(argsort, "_spx_class", None) == 1:
            return sparse_rows_hint(tile_order, getattr(argsort, "_spx_heavy", None))
        return tile_order
    return _with_dense_hint(tile_order, argsort, mask)


def sparse_neighbourhoods(rb: Rulebook) -> bool:
    """True for a rulebook whose rows were regrouped (one device -> host read of the class word; cached
    on the rulebook).  A HOST-side view for tools and for choices that change a launch's shape (the
    int8 tile height); the kernels themselves read the class on the device."""
    if rb.sparse_class is not None:
        return rb.sparse_class
    if rb.layout is not None:
        head = rb.layout[:2].tolist()
        _set_class(rb, head[0], int(head[1]), predict=False)   # (the module learns from the queued read, as ever)
        rb._class_req = None
    elif rb.subm and 1 < rb.kv <= 32 and rb.n_out >= _LAYOUT_MIN_ROWS and rb.mask_fwd is not None:
        centre = 1 << (rb.kv // 2)
        rb.sparse_class = float((rb.mask_fwd.view(-1) != centre).float().mean().item()) < 0.25
    else:
        rb.sparse_class = False
    return rb.sparse_class


# Density-aware row order = the DEFAULT of the layer modules (the reference sorts every rulebook by mask:
# SPCONV_DO_SORT = "1", constants.py:121, ops.py:346,550,763-785).  spx_subm_layout classifies the finished
# masks on the device and, for a SPARSE rulebook (fewer than a quarter of the rows have any neighbour),
# moves the rows with a neighbour into a compact appendix grouped by offset (a stable counting partition),
# which turns "every 128-row tile walks ~4 extra offsets" into "97 % of the rows run as a plain streaming
# GEMM on their centre pair -- no row order, no pair word to fetch -- and ~25 appendix tiles walk 2-3
# offsets each"; a dense (LiDAR) rulebook keeps everything in the row-order walk (regrouping loses 19 %
# there).  No sort, no read-back: class and count are words in the blob that the appendix workgroups of
# the gather-GEMM launch read, so the same launch serves both classes and the whole thing sits in a hipGraph.


@_on_device
def rows_layout(rb: Rulebook) -> None:
    """Builds rb.layout (int32 blob, include/spconv_amd.h: spx_subm_layout) for a SubM rulebook."""
    L = _lib.load()
    n, kv = rb.n_out, rb.kv
    dev = rb.pair_fwd.device
    blob = torch.empty((L.spx_subm_layout_bytes(n, kv) // 4,), dtype=torch.int32, device=dev)
    ws = _ws(L.spx_subm_layout_ws_bytes(n), dev)
    _lib.check(L.spx_subm_layout(rb.pair_fwd.data_ptr(), rb.mask_fwd.data_ptr(), n, kv, blob.data_ptr(),
                                 ws.data_ptr(), ws.numel(), _stream(rb.pair_fwd)))
    rb.layout = blob
    _request_class(rb)            # (what was known of the class belonged to the blob this one replaces)


def layout_views(rb: Rulebook):
    """(header [5]: class, M, n, kv, mcap; main mask words [n]; appendix row list [mcap]; appendix mask words [mcap];
    appendix pair table [kv, mcap]) of rb.layout -- views for tests and tools; only the first M appendix entries are
    defined, and only for a class-1 rulebook."""
    n, kv, blob = rb.n_out, rb.kv, rb.layout
    npad = (n + 63) // 64 * 64
    mcap = int(_lib.load().spx_subm_layout_mcap(n))
    o = 64 + npad
    return (blob[:5], blob[64:64 + n], blob[o:o + mcap], blob[o + mcap:o + 2 * mcap],
            blob[o + 2 * mcap:o + (2 + kv) * mcap].view(kv, mcap))


def sort_rulebook(rb: Rulebook) -> None:
    """The reference's explicit mask sort (SPCONV_DO_SORT=1): argsort of the mask words + copies of the
    tables in that order (both directions of a regular-conv rulebook).  The gather-GEMM then reads
    pair / mask by tile position."""
    L = _lib.load()
    for which in (("fwd",) if rb.subm else ("fwd", "bwd")):
        pair, mask = (rb.pair_fwd, rb.mask_fwd) if which == "fwd" else (rb.pair_bwd, rb.mask_bwd)
        if pair is None or mask is None or mask.shape[1] != 1 or pair.shape[1] == 0:
            continue
        order = mask_argsort(mask, rb.kv)
        pair_t, mask_t = torch.empty_like(pair), torch.empty_like(mask)
        with torch.cuda.device(pair.device):           # launches belong to the device the tables live on
            _lib.check(L.spx_permute_tables(pair.data_ptr(), mask.data_ptr(), order.data_ptr(), pair.shape[0],
                                            pair.shape[1], mask.shape[1], pair_t.data_ptr(), mask_t.data_ptr(),
                                            _stream(pair)))
        if which == "fwd":
            rb.argsort_fwd = order
        else:
            rb.argsort_bwd = order
        rb.sorted_tables[which] = (pair_t, mask_t)


def tables_of(rb: Rulebook, which: str, cout: int = 64):
    """(pair, mask, argsort, tile_order) the gather-GEMM should read for `which` ("fwd": pair_fwd
    over the output rows, "bwd": pair_bwd over the input rows).  tile_order 0: tables by row (argsort,
    if any, permutes the rows); 1: copies in tile order (explicit mask sort); 2: `argsort` is the rows
    layout blob and pair / mask the row-order tables (the device picks).  `cout`: output width of the
    GEMM (every width reaches a kernel that takes all three forms; kernel volumes beyond 32 read the tables by row)."""
    pair, mask, order = ((rb.pair_fwd, rb.mask_fwd, rb.argsort_fwd) if which == "fwd"
                         else (rb.pair_bwd, rb.mask_bwd, rb.argsort_bwd))
    if rb.kv > 32:
        return pair, mask, None, 0
    st = rb.sorted_tables.get(which)
    if order is not None and st is not None:
        return st[0], st[1], order, 1
    if order is None and which == "fwd" and rb.subm and rb.layout is not None:
        poll_class(rb)
        return pair, mask, rb.layout, _ROWS_LAYOUT
    return pair, mask, order, 0


@_on_device
def mask_argsort(mask: torch.Tensor, kv: int = 0) -> torch.Tensor:
    """SpconvOps.sort_1d_by_key_allocator (all.py:935-991): stable argsort of the mask words.  kv (1..32): the kernel
    volume the words belong to -- only their low kv bits can be set, the sort runs fewer digit passes."""
    L = _lib.load()
    n, words = mask.shape
    out = torch.empty((n,), dtype=torch.int32, device=mask.device)
    ws = _ws(L.spx_mask_argsort_ws_bytes(n), mask.device)
    if 1 <= int(kv) <= 32 and words == 1:
        _lib.check(L.spx_mask_argsort_kv(mask.data_ptr(), n, int(kv), out.data_ptr(), ws.data_ptr(), ws.numel(),
                                         _stream(mask)))
    else:
        _lib.check(L.spx_mask_argsort(mask.data_ptr(), n, words, out.data_ptr(), ws.data_ptr(),
                                      ws.numel(), _stream(mask)))
    return out


def attach_rulebook(t: torch.Tensor, rb: Rulebook) -> torch.Tensor:
    """Side channel for the reference-shaped op signatures below: a bare pair tensor
    remembers (weakly, to avoid a tensor<->rulebook cycle) the rulebook it belongs to."""
    t._spx_rulebook = weakref.ref(rb)
    return t


def rulebook_of(t: torch.Tensor) -> Optional[Rulebook]:
    ref = getattr(t, "_spx_rulebook", None)
    return ref() if ref is not None else None


# ----------------------------------------- layout conversion for bare tensors
def _table_from_native(indice_pairs: torch.Tensor, indice_pair_num: torch.Tensor, n_dst: int,
                       subm: bool, inverse: bool):
    L = _lib.load()
    kv, n_in = indice_pairs.shape[1], indice_pairs.shape[2]
    table = torch.empty((kv, n_dst), dtype=torch.int32, device=indice_pairs.device)
    mask = torch.empty((n_dst, (kv + 31) // 32), dtype=torch.int32, device=indice_pairs.device)
    _lib.check(L.spx_native_to_table(indice_pairs.data_ptr(), indice_pair_num.data_ptr(), n_in,
                                     n_dst, kv, int(subm), int(inverse), table.data_ptr(),
                                     mask.data_ptr(), _stream(indice_pairs)))
    return table, mask


def _native_from_table(table: torch.Tensor, subm: bool):
    L = _lib.load()
    kv, n = table.shape
    native = torch.empty((2, kv, n), dtype=torch.int32, device=table.device)
    num = torch.empty((kv,), dtype=torch.int32, device=table.device)
    ws = _ws(L.spx_table_to_native_ws_bytes(n, kv), table.device)
    _lib.check(L.spx_table_to_native(table.data_ptr(), int(subm), kv, n, native.data_ptr(),
                                     num.data_ptr(), ws.data_ptr(), ws.numel(), _stream(table)))
    return native, num
