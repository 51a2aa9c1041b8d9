"""Kernel point convolution on the MFMA kernels of csrc/kpconv.hip (``functional.kpconv``, ``spatial.KPConv``): rigid
KPConv with the linear influence and sum aggregation, read through the ``VoxelNeighbors`` table of ``ball_query`` /
``knn_query`` / ``voxel_query`` and its fp32 offsets.  Not part of the reference; the code bases users port call it as
the ``KPConv`` layer of KPConv-PyTorch (KPFCNN, Predator, D3Feat, GeoTransformer).

  * forward   two launches (``spx_kpconv_fwd``: the weight into fragment order, the convolution): no grouped [M, S, Cin]
              row and no [M, S, K] influence is written; with a gradient ahead the weighted features WF are kept as
              [M, K, Cin] in the rows' dtype, 2 * K * Cin bytes per query
  * backward  the query side (``spx_kpconv_bwd``, one launch: dG [M, S, Cin], the one grouped tensor, in the rows'
              dtype) and ``spx_group_bwd`` for dfeats; the weight side, two launches (fp32 partials per chunk of
              queries, added in a fixed order); no atomics, identical run to run

The ``_into`` forms take buffers the caller owns, allocate nothing and read nothing back: they can sit inside a captured
graph behind ``knn_query_into`` / ``ball_query_cells_into`` and the groups.  There is no composite to fall back to.

Not built: deformable KPConv, gradients in kernel points or offsets, Gaussian or constant influence, "closest"
aggregation, float32 / float64, KPConv's feature-sum neighbour count (``normalize`` divides by the valid slots).
"""
from __future__ import annotations

import math
from typing import Optional, Tuple

import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from spconv_amd import _lib
from spconv_amd.pytorch._level import groups_missing
from spconv_amd.pytorch._query import MAX_NSAMPLE, VoxelNeighbors
from spconv_amd.pytorch._rulebook import _ptr, _require_gpu, _stream

MAX_POINTS, MAX_CHANNELS = 16, 256
_CODES = {torch.float16: _lib.DTYPE_F16, torch.bfloat16: _lib.DTYPE_BF16}
_FWD_ROWS = torch.amp.custom_fwd(device_type="cuda")        # casts nothing: the rows keep their dtype under autocast
_BWD = torch.amp.custom_bwd(device_type="cuda")


def _channels(name: str, C: int) -> None:
    if not (16 <= C <= MAX_CHANNELS and C % 16 == 0):
        raise NotImplementedError(f"kpconv: {name} must be a multiple of 16 in 16 .. {MAX_CHANNELS}, got {C}")


def check(feats: torch.Tensor, nb: VoxelNeighbors, kernel_points: torch.Tensor, weight: torch.Tensor,
          sigma: float) -> Tuple[int, int, int, int, int]:
    """(M, S, K, Cin, Cout) of a kpconv call; everything that can be refused is refused before a kernel runs, and before
    the refusal of CPU tensors (``check_devices``)"""
    if feats.dtype not in _CODES:
        raise NotImplementedError(f"kpconv: feats must be float16 or bfloat16 (nothing is cast), got {feats.dtype}")
    if feats.dim() != 2 or int(feats.shape[0]) != nb.num_voxels:
        raise ValueError(f"kpconv: feats holds one row per voxel or point of the table ([{nb.num_voxels}, Cin]), got "
                         f"{tuple(feats.shape)}")
    Cin = int(feats.shape[1])
    _channels("Cin (feats)", Cin)
    if weight.dim() != 3 or int(weight.shape[1]) != Cin or weight.dtype != feats.dtype:
        raise ValueError(f"kpconv: weight is [K, Cin, Cout] = [K, {Cin}, Cout] of {feats.dtype} (nothing is cast), got "
                         f"{tuple(weight.shape)} {weight.dtype}")
    K, Cout = int(weight.shape[0]), int(weight.shape[2])
    if not 1 <= K <= MAX_POINTS:
        raise NotImplementedError(f"kpconv: K (weight, kernel_points) must be in 1 .. {MAX_POINTS}, got {K}")
    _channels("Cout (weight)", Cout)
    if kernel_points.dtype != torch.float32 or tuple(kernel_points.shape) != (K, 3):
        raise ValueError(f"kpconv: kernel_points is float32 [K, 3] = [{K}, 3], got {kernel_points.dtype} "
                         f"{tuple(kernel_points.shape)}")
    rows, offsets = nb.rows, nb.offsets
    if rows.dim() != 2 or rows.dtype != torch.int32 or not rows.is_contiguous():
        raise ValueError(f"kpconv: nb.rows is a contiguous int32 tensor [M, nsample], got {tuple(rows.shape)} {rows.dtype}")
    M, S = (int(v) for v in rows.shape)
    if not 1 <= S <= MAX_NSAMPLE:
        raise ValueError(f"kpconv: nsample (nb.rows) must be in 1 .. {MAX_NSAMPLE}, got {S}")
    if offsets is None:
        raise ValueError("kpconv: nb.offsets is missing; build the table with with_offsets=True")
    if offsets.dtype != torch.float32 or tuple(offsets.shape) != (M, S, 3) or not offsets.is_contiguous():
        raise ValueError(f"kpconv: nb.offsets is a contiguous float32 tensor [M, nsample, 3] = [{M}, {S}, 3] (ndim is 3), "
                         f"got {offsets.dtype} {tuple(offsets.shape)}")
    if not float(sigma) > 0:
        raise ValueError(f"kpconv: sigma must be > 0, got {sigma}")
    return M, S, K, Cin, Cout


def check_devices(feats, nb: VoxelNeighbors, kernel_points, weight) -> None:
    for name, t in (("feats", feats), ("weight", weight), ("kernel_points", kernel_points), ("nb.rows", nb.rows),
                    ("nb.offsets", nb.offsets)):
        _require_gpu(t, name)
        if t.device != feats.device:
            raise ValueError(f"kpconv: {name} is on {t.device}, feats on {feats.device}")


def kpconv_ws_bytes(M: int, K: int, Cin: int, Cout: int, backward: bool = False) -> int:
    """bytes of the workspace of ``kpconv_into`` (the weight in fragment order) or, with backward, of
    ``kpconv_bwd_into`` with a dweight (d_out * norm and the fp32 partials)"""
    return int(_lib.load().spx_kpconv_ws_bytes(int(M), int(K), int(Cin), int(Cout), int(bool(backward))))


def _ws(nbytes: int, dev) -> torch.Tensor:
    return torch.empty((max(nbytes, 16),), dtype=torch.uint8, device=dev)


def kpconv_into(feats: torch.Tensor, nb: VoxelNeighbors, kernel_points: torch.Tensor, weight: torch.Tensor, sigma: float,
                normalize: bool, out: torch.Tensor, wf: Optional[torch.Tensor], ws: torch.Tensor) -> None:
    """The forward's one C call into buffers the caller owns (no allocation: capturable).  feats [n, Cin], weight [K,
    Cin, Cout], out [M, Cout] contiguous; wf [M, K, Cin] in the rows' dtype (what ``kpconv_bwd_into`` reads for dweight,
    2 * K * Cin bytes per query) or None; ws: uint8, ``kpconv_ws_bytes(M, K, Cin, Cout)``."""
    (M, S), (K, Cin, Cout) = nb.rows.shape, weight.shape
    _lib.check(_lib.load().spx_kpconv_fwd(
        feats.data_ptr(), nb.rows.data_ptr(), nb.offsets.data_ptr(), kernel_points.data_ptr(), weight.data_ptr(), int(M),
        int(S), int(nb.num_voxels), _ptr(nb.n_queries), _ptr(nb.n_live), int(K), int(Cin), int(Cout), _CODES[feats.dtype],
        float(sigma), int(bool(normalize)), out.data_ptr(), _ptr(wf), ws.data_ptr(), ws.numel(), _stream(feats)))


def kpconv_bwd_into(wf: Optional[torch.Tensor], nb: VoxelNeighbors, kernel_points: torch.Tensor, weight: torch.Tensor,
                    sigma: float, normalize: bool, d_out: torch.Tensor, dg: Optional[torch.Tensor],
                    dfeats: Optional[torch.Tensor], dweight: Optional[torch.Tensor], ws: Optional[torch.Tensor]) -> None:
    """The backward into buffers the caller owns.  dg [M, S, Cin] and dfeats [n, Cin] come together (or both None):
    the query side writes dg, ``spx_group_bwd`` sums it over ``nb.groups`` into dfeats.  dweight [K, Cin, Cout] (or
    None) needs wf as the forward left it and ws of ``kpconv_ws_bytes(.., backward=True)``."""
    (M, S), (K, Cin, Cout) = nb.rows.shape, weight.shape
    g = nb.groups
    if dfeats is not None and (dg is None or g is None or g.offsets is None):
        raise groups_missing("kpconv", "neighbour", "the query")
    lib = _lib.load()
    _lib.check(lib.spx_kpconv_bwd(
        _ptr(wf), nb.rows.data_ptr(), nb.offsets.data_ptr(), kernel_points.data_ptr(), weight.data_ptr(), d_out.data_ptr(),
        int(M), int(S), int(nb.num_voxels), _ptr(nb.n_queries), _ptr(nb.n_live), int(K), int(Cin), int(Cout),
        _CODES[weight.dtype], float(sigma), int(bool(normalize)), _ptr(dg if dfeats is not None else None), _ptr(dweight),
        _ptr(ws), 0 if ws is None else ws.numel(), _stream(d_out)))
    if dfeats is not None:
        _lib.check(lib.spx_group_bwd(dg.data_ptr(), int(M), int(S), g.offsets.data_ptr(), g.list.data_ptr(),
                                     int(nb.num_voxels), _ptr(nb.n_live), int(Cin), _CODES[weight.dtype], dfeats.data_ptr(),
                                     _stream(d_out)))


class KPConvFunction(Function):
    """spx_kpconv_fwd / _bwd: gradients to feats and weight, none to the kernel points, sigma or the table.  Casts
    nothing under autocast."""

    @staticmethod
    @_FWD_ROWS
    def forward(ctx, feats, weight, nb, kernel_points, sigma, normalize):
        feats, weight = feats.detach().contiguous(), weight.detach().contiguous()
        (M, _), (K, Cin, Cout), dev = nb.rows.shape, weight.shape, feats.device
        out = torch.empty((M, Cout), dtype=feats.dtype, device=dev)
        wf = torch.empty((M, K, Cin), dtype=feats.dtype, device=dev) if ctx.needs_input_grad[1] else None
        if M > 0:
            kpconv_into(feats, nb, kernel_points, weight, sigma, normalize, out, wf, _ws(kpconv_ws_bytes(M, K, Cin, Cout), dev))
        ctx.save_for_backward(weight, kernel_points, wf)
        ctx.nb, ctx.geom = nb, (sigma, normalize)
        return out

    @staticmethod
    @once_differentiable
    @_BWD
    def backward(ctx, grad_output):
        weight, kernel_points, wf = ctx.saved_tensors
        nb, (sigma, normalize) = ctx.nb, ctx.geom
        if grad_output.dtype != weight.dtype:
            raise NotImplementedError(f"kpconv: the gradient arrives as {grad_output.dtype}, the rows are {weight.dtype}")
        d_out = grad_output.contiguous()
        (M, S), (K, Cin, Cout), n, dev = nb.rows.shape, weight.shape, nb.num_voxels, d_out.device
        with torch.cuda.device(dev):
            dfeats = dweight = dg = ws = None
            if ctx.needs_input_grad[0]:
                fill = M > 0 and n > 0
                dfeats = (torch.empty if fill else torch.zeros)((n, Cin), dtype=weight.dtype, device=dev)
                dg = torch.empty((M, S, Cin), dtype=weight.dtype, device=dev) if fill else None
            if ctx.needs_input_grad[1]:
                dweight = (torch.empty if M > 0 else torch.zeros)((K, Cin, Cout), dtype=weight.dtype, device=dev)
                ws = _ws(kpconv_ws_bytes(M, K, Cin, Cout, True), dev)
            if M > 0:
                kpconv_bwd_into(wf, nb, kernel_points, weight, sigma, normalize, d_out, dg, dfeats if dg is not None else None,
                                dweight, ws)
        return dfeats, dweight, None, None, None, None


def kpconv(feats: torch.Tensor, nb: VoxelNeighbors, kernel_points: torch.Tensor, weight: torch.Tensor, sigma: float,
           normalize: bool = False) -> torch.Tensor:
    """Rigid KPConv (linear influence, sum aggregation) of every query over its own neighbours, on the MFMA kernels of
    csrc/kpconv.hip.  feats [nb.num_voxels, Cin]: rows of the level or of the point set; nb: the ``VoxelNeighbors``
    table with its fp32 offsets [M, S, 3] = neighbour - query (``with_offsets=True``; S in 1 .. 128); kernel_points
    float32 [K, 3], K in 1 .. 16; weight [K, Cin, Cout] in feats' dtype (KPConv-PyTorch's shape); Cin and Cout multiples
    of 16 in 16 .. 256; float16 or bfloat16 -- float32 / float64 are refused, nothing is cast, not under autocast either.
    Slot (m, s) is valid iff ``0 <= rows[m, s] < live`` (live = min(*nb.n_live, num_voxels)): the rule of
    ``group_voxels``, so ``pad="first"`` duplicates count.  ``h[m, s, k] = max(0, 1 - |offsets[m, s] - kernel_points[k]|
    / sigma)`` in fp32 for a valid slot, 0 otherwise; ``WF[m, k] = sum_s h[m, s, k] feats[rows[m, s]]``; ``out[m] =
    sum_k WF[m, k] @ weight[k]``, with normalize divided by max(1, valid slots of m).  h and WF are rounded to the rows'
    dtype once, sums are fp32.  Returns out [M, Cout], written whole: a query at or beyond *nb.n_queries gets zeros, a
    query without a valid slot +0.  No [M, S, Cin] and no [M, S, K] tensor exists in memory.

    Differentiable in feats (over ``nb.groups`` -- build the table with with_groups=True -- through one grouped tensor,
    dG [M, S, Cin] in the rows' dtype) and in weight; with a weight gradient ahead the forward keeps WF as [M, K, Cin]
    in the rows' dtype, 2 * K * Cin bytes per query.  No atomics: identical run to run.  No gradient to kernel_points,
    sigma or the offsets.  Nothing is read back."""
    M, S, K, Cin, Cout = check(feats, nb, kernel_points, weight, sigma)
    grad = torch.is_grad_enabled() and (feats.requires_grad or weight.requires_grad)
    if grad and feats.requires_grad and nb.groups is None and nb.rows.numel() > 0 and nb.num_voxels > 0:
        raise groups_missing("kpconv", "neighbour", "the query")
    check_devices(feats, nb, kernel_points, weight)
    kernel_points = kernel_points.detach().contiguous()
    with torch.cuda.device(feats.device):
        if grad:
            return KPConvFunction.apply(feats, weight, nb, kernel_points, float(sigma), bool(normalize))
        out = torch.empty((M, Cout), dtype=feats.dtype, device=feats.device)
        if M > 0:
            kpconv_into(feats.detach().contiguous(), nb, kernel_points, weight.detach().contiguous(), float(sigma),
                        bool(normalize), out, None, _ws(kpconv_ws_bytes(M, K, Cin, Cout), feats.device))
        return out


def default_kernel_points(kp_radius: float) -> torch.Tensor:
    """The fixed 15-point layout: the centre, the six axis points and the eight cube diagonals, all at distance
    kp_radius from the centre.  float32 [15, 3]; deterministic, no optimisation and no files."""
    r, d = float(kp_radius), float(kp_radius) / math.sqrt(3.0)
    pts = [(0.0, 0.0, 0.0)]
    for axis in range(3):
        for sign in (r, -r):
            pts.append(tuple(sign if a == axis else 0.0 for a in range(3)))
    pts += [(sx * d, sy * d, sz * d) for sx in (1, -1) for sy in (1, -1) for sz in (1, -1)]
    return torch.tensor(pts, dtype=torch.float32)
