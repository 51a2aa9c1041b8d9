"""Selective scan and causal convolution over serialised rows on the HIP kernels of csrc/scan.hip
(``functional.scan_sequences`` / ``selective_scan`` / ``causal_conv1d_rows``, ``SerializedMamba``): the state-space step
of the Mamba backbones that serialise voxels along a curve (Voxel Mamba, LION, PointMamba, Mamba3D).  Not part of the
reference; the code bases users port call ``selective_scan_fn`` of ``mamba_ssm`` behind ``causal_conv1d_fn``, both on a
padded channel-first [B, Dm, L] layout.  Here the rows stay in row order, channel-last, and are read through the
serialisation's order: ragged sequences, no padding, no read-back.

  * ``scan_sequences``      the sequences of a ``Serialization`` (or of plain offsets): views, no launch
  * ``selective_scan``      forward five launches, backward five to seven (``spx_selective_scan_fwd`` / ``_bwd``); the
                            workspace the forward leaves (chunk table, entry states) is what the backward reads
  * ``causal_conv1d_rows``  forward one launch, backward four (``spx_causal_conv_rows_fwd`` / ``_bwd``)

The ``_into`` forms take buffers the caller owns, allocate nothing and read nothing back: serialize -> convolution ->
scan -> both backwards can sit in one captured graph.  There is no composite to fall back to.

Not built: Mamba-2 / SSD, d_state other than 16, complex A, a returned last state or an initial state, dt clamping other
than the softplus threshold, a gradient with respect to the order, float64.
"""
from __future__ import annotations

import math
from typing import NamedTuple, Optional, Tuple

import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from spconv_amd import _lib
from spconv_amd.pytorch._rulebook import _ptr, _require_gpu, _stream, _ws

CHUNK = 64                  # SPX_SCAN_CHUNK: positions of a chunk
STATES = 16                 # SPX_SCAN_STATES
CHANNEL_BLOCK, MAX_CHANNELS = 64, 2048
WIDTHS = (2, 3, 4)
_CODES = {torch.float16: _lib.DTYPE_F16, torch.bfloat16: _lib.DTYPE_BF16, torch.float32: _lib.DTYPE_F32}
_ACTS = {None: 0, "silu": 1}


class ScanSequences(NamedTuple):
    """order int32 [n] or None (identity), offsets int32 [S + 1], num_sequences = S, n: sequence s is the positions p in
    [offsets[s], offsets[s + 1]), its row order[p]; positions at or beyond offsets[S] belong to no sequence."""
    order: Optional[torch.Tensor]
    offsets: torch.Tensor
    num_sequences: int
    n: int


def scan_sequences(ser=None, which: int = 0, *, offsets: Optional[torch.Tensor] = None,
                   order: Optional[torch.Tensor] = None, n: Optional[int] = None) -> ScanSequences:
    """The sequences of a ``Serialization`` (one per scene, along order ``which``) or of plain ``offsets`` (int32
    [S + 1]) with an optional ``order`` (int32 [n]; None: identity, then give ``n``).  No launch: the tuple holds views."""
    if ser is not None:
        if offsets is not None or order is not None:
            raise ValueError("scan_sequences: give a Serialization or offsets / order, not both")
        if ser.order.dim() != 2 or not 0 <= int(which) < int(ser.order.shape[0]):
            raise ValueError(f"scan_sequences: which must name one of the {tuple(ser.order.shape)[:1]} orders, got {which}")
        order, offsets = ser.order[int(which)], ser.offsets
    if offsets is None:
        raise ValueError("scan_sequences: give a Serialization or offsets")
    if offsets.dtype != torch.int32 or offsets.dim() != 1 or offsets.shape[0] < 2 or not offsets.is_contiguous():
        raise ValueError(f"scan_sequences: offsets is a contiguous int32 tensor [S + 1], S >= 1, got {offsets.dtype} "
                         f"{tuple(offsets.shape)}")
    if order is not None:
        if order.dtype != torch.int32 or order.dim() != 1 or not order.is_contiguous():
            raise ValueError(f"scan_sequences: order is a contiguous int32 tensor [n], got {order.dtype} {tuple(order.shape)}")
        if order.device != offsets.device:
            raise ValueError(f"scan_sequences: order is on {order.device}, offsets on {offsets.device}")
        if n is not None and int(n) != int(order.shape[0]):
            raise ValueError(f"scan_sequences: order names {int(order.shape[0])} positions, n is {n}")
        n = int(order.shape[0])
    if n is None or int(n) < 0:
        raise ValueError("scan_sequences: without an order, give n >= 0 (the number of rows)")
    return ScanSequences(order, offsets, int(offsets.shape[0]) - 1, int(n))


def _check_rows(op: str, name: str, t: torch.Tensor, n: int, Dm: int, dtype) -> None:
    if t.dim() != 2 or tuple(t.shape) != (n, Dm) or t.dtype != dtype:
        raise ValueError(f"{op}: {name} is [{n}, {Dm}] of {dtype} (nothing is cast), got {tuple(t.shape)} {t.dtype}")


def _check_vec(op: str, name: str, t: Optional[torch.Tensor], shape) -> None:
    if t is not None and (t.dtype != torch.float32 or tuple(t.shape) != tuple(shape)):
        raise ValueError(f"{op}: {name} is float32 {list(shape)}, got {t.dtype} {tuple(t.shape)}")


def _check_channels(op: str, Dm: int) -> None:
    if Dm < CHANNEL_BLOCK or Dm % CHANNEL_BLOCK != 0 or Dm > MAX_CHANNELS:
        raise NotImplementedError(f"{op}: Dm must be a multiple of {CHANNEL_BLOCK}, at most {MAX_CHANNELS}, got {Dm}")


def _check_seq(op: str, seq, x: torch.Tensor) -> None:
    if not isinstance(seq, ScanSequences):
        raise ValueError(f"{op}: seq is what scan_sequences returns, got {type(seq).__name__}")
    if seq.n != int(x.shape[0]):
        raise ValueError(f"{op}: the sequences name {seq.n} rows, the tensors hold {int(x.shape[0])}")
    _require_gpu(x, "the rows")
    if seq.offsets.device != x.device:
        raise ValueError(f"{op}: the sequences are on {seq.offsets.device}, the rows on {x.device}")


def check_scan(u, delta, A, B, C, D, z, delta_bias, seq) -> Tuple[int, int, int]:
    """(n, Dm, G) of a selective_scan call; every limit is refused before the library is called"""
    op = "selective_scan"
    if u.dtype not in _CODES:
        raise NotImplementedError(f"{op}: rows must be float16, bfloat16 or float32 (nothing is cast), got {u.dtype}")
    if u.dim() != 2 or B.dim() != 3:
        raise ValueError(f"{op}: u is [n, Dm] and B [n, G, N], got {tuple(u.shape)} and {tuple(B.shape)}")
    n, Dm = (int(v) for v in u.shape)
    G, N = int(B.shape[1]), int(B.shape[2])
    if N != STATES:
        raise NotImplementedError(f"{op}: d_state must be {STATES}, got {N}")
    _check_channels(op, Dm)
    if G < 1 or Dm % G != 0 or (Dm // G) % CHANNEL_BLOCK != 0:
        raise NotImplementedError(f"{op}: G must divide Dm into multiples of {CHANNEL_BLOCK} channels, got G = {G}, Dm = {Dm}")
    _check_rows(op, "delta", delta, n, Dm, u.dtype)
    if z is not None:
        _check_rows(op, "z", z, n, Dm, u.dtype)
    for name, t in (("B", B), ("C", C)):
        if tuple(t.shape) != (n, G, N) or t.dtype != u.dtype:
            raise ValueError(f"{op}: {name} is [{n}, {G}, {N}] of {u.dtype} (nothing is cast), got {tuple(t.shape)} {t.dtype}")
    if A.is_complex():
        raise NotImplementedError(f"{op}: complex A is not built")
    _check_vec(op, "A", A, (Dm, N))
    _check_vec(op, "D", D, (Dm,))
    _check_vec(op, "delta_bias", delta_bias, (Dm,))
    _check_seq(op, seq, u)
    return n, Dm, G


def scan_ws_bytes(n: int, S: int, Dm: int, G: int) -> int:
    """bytes of the workspace of selective_scan_into / _bwd_into, from host-known numbers alone"""
    return int(_lib.load().spx_selective_scan_ws_bytes(int(n), int(S), int(Dm), int(G)))


def _step(reverse: bool) -> int:
    return -1 if reverse else 1


def selective_scan_into(u, delta, A, B, C, D, z, delta_bias, delta_softplus: bool, seq: ScanSequences, reverse: bool,
                        y: torch.Tensor, ws: torch.Tensor) -> None:
    """The forward's one C call into buffers the caller owns (no allocation: capturable).  Contiguous tensors as
    ``selective_scan`` documents them; y [n, Dm]; ws uint8 of ``scan_ws_bytes`` -- the backward reads what this leaves."""
    n, Dm = (int(v) for v in u.shape)
    _lib.check(_lib.load().spx_selective_scan_fwd(
        u.data_ptr(), delta.data_ptr(), A.data_ptr(), B.data_ptr(), C.data_ptr(), _ptr(D), _ptr(z), _ptr(delta_bias),
        _ptr(seq.order), seq.offsets.data_ptr(), n, seq.num_sequences, Dm, int(B.shape[1]), _CODES[u.dtype],
        int(bool(delta_softplus)), _step(reverse), y.data_ptr(), ws.data_ptr(), ws.numel(), _stream(u)))


def selective_scan_bwd_into(u, delta, A, B, C, D, z, delta_bias, delta_softplus: bool, seq: ScanSequences, reverse: bool,
                            d_out, du, ddelta, dA, dB, dC, dD, dz, ddelta_bias, ws: torch.Tensor) -> None:
    """The backward's one C call.  ws as ``selective_scan_into`` left it for the same arguments; du, ddelta, dz [n, Dm]
    and dB, dC [n, G, 16] in the rows' dtype, dA [Dm, 16], dD, ddelta_bias [Dm] float32; dz / dD / ddelta_bias are None
    exactly when z / D / delta_bias are.  Every buffer is written whole."""
    n, Dm = (int(v) for v in u.shape)
    _lib.check(_lib.load().spx_selective_scan_bwd(
        u.data_ptr(), delta.data_ptr(), A.data_ptr(), B.data_ptr(), C.data_ptr(), _ptr(D), _ptr(z), _ptr(delta_bias),
        d_out.data_ptr(), _ptr(seq.order), seq.offsets.data_ptr(), n, seq.num_sequences, Dm, int(B.shape[1]),
        _CODES[u.dtype], int(bool(delta_softplus)), _step(reverse), du.data_ptr(), ddelta.data_ptr(), dA.data_ptr(),
        dB.data_ptr(), dC.data_ptr(), _ptr(dD), _ptr(dz), _ptr(ddelta_bias), ws.data_ptr(), ws.numel(), _stream(u)))


def _opt(t):
    return None if t is None else t.detach().contiguous()


class SelectiveScanFunction(Function):
    """spx_selective_scan_fwd / _bwd: gradients to u, delta, A, B, C, D, z and delta_bias, none to the sequences."""

    @staticmethod
    def forward(ctx, u, delta, A, B, C, D, z, delta_bias, softplus, seq, reverse):
        u, delta, A, B, C = (t.detach().contiguous() for t in (u, delta, A, B, C))
        D, z, delta_bias = _opt(D), _opt(z), _opt(delta_bias)
        n, Dm = u.shape
        y = torch.empty_like(u)
        ws = _ws(scan_ws_bytes(n, seq.num_sequences, Dm, B.shape[1]), u.device)
        if n > 0:
            selective_scan_into(u, delta, A, B, C, D, z, delta_bias, softplus, seq, reverse, y, ws)
        ctx.save_for_backward(u, delta, A, B, C, D, z, delta_bias, ws)
        ctx.seq, ctx.flags = seq, (softplus, reverse)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_output):
        u, delta, A, B, C, D, z, delta_bias, ws = ctx.saved_tensors
        if grad_output.dtype != u.dtype:
            raise NotImplementedError(f"selective_scan: the gradient arrives as {grad_output.dtype}, the rows are {u.dtype}")
        with torch.cuda.device(u.device):
            f32 = dict(dtype=torch.float32, device=u.device)
            du, ddelta, dB, dC = torch.empty_like(u), torch.empty_like(u), torch.empty_like(B), torch.empty_like(C)
            dz = None if z is None else torch.empty_like(u)
            dA = torch.zeros(A.shape, **f32) if u.shape[0] == 0 else torch.empty(A.shape, **f32)
            dD = None if D is None else torch.zeros(D.shape, **f32)
            db = None if delta_bias is None else torch.zeros(delta_bias.shape, **f32)
            if u.shape[0] > 0:
                selective_scan_bwd_into(u, delta, A, B, C, D, z, delta_bias, ctx.flags[0], ctx.seq, ctx.flags[1],
                                        grad_output.contiguous(), du, ddelta, dA, dB, dC, dD, dz, db, ws)
        return du, ddelta, dA, dB, dC, dD, dz, db, None, None, None


def selective_scan(u: torch.Tensor, delta: torch.Tensor, A: torch.Tensor, B: torch.Tensor, C: torch.Tensor,
                   D: Optional[torch.Tensor] = None, z: Optional[torch.Tensor] = None,
                   delta_bias: Optional[torch.Tensor] = None, delta_softplus: bool = False, *, seq: ScanSequences,
                   reverse: bool = False) -> torch.Tensor:
    """Mamba's selective scan (``selective_scan_fn``) over the ragged sequences ``seq`` (``scan_sequences``), on the
    kernels of csrc/scan.hip.  u, delta, z [n, Dm] in ROW order, channel-last; B, C [n, G, 16]; A float32 [Dm, 16]; D,
    delta_bias float32 [Dm]; the row tensors share one dtype out of float16, bfloat16, float32 -- nothing is cast, not
    under autocast either.  Dm a multiple of 64, at most 2048; G divides Dm with Dm / G a multiple of 64.  Per sequence
    and channel d of group g, fp32 state h[0 .. 16) from +0, positions ascending (descending for ``reverse``), r the row
    of the position::

        dt   = delta[r, d] (+ delta_bias[d]);  dt = dt <= 20 ? log1p(exp(dt)) : dt   when delta_softplus
        h[k] = exp(dt * A[d, k]) * h[k] + dt * B[r, g, k] * u[r, d]
        y    = sum_k C[r, g, k] * h[k] (+ D[d] * u[r, d]);  y *= z * sigmoid(z)   when z is given

    Returns y [n, Dm], rounded once, written whole: rows of no sequence get +0.  State never crosses a sequence.
    Differentiable in everything but the sequences; the row gradients come in the rows' dtype (+0 for rows of no
    sequence), dA, dD and ddelta_bias in float32; no atomics: identical run to run.  Nothing is read back.

    Not built: Mamba-2 / SSD, d_state other than 16, complex A, a returned last state or an initial state, float64."""
    n, Dm, G = check_scan(u, delta, A, B, C, D, z, delta_bias, seq)
    with torch.cuda.device(u.device):
        tensors = (u, delta, A, B, C, D, z, delta_bias)
        if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors):
            return SelectiveScanFunction.apply(*tensors, bool(delta_softplus), seq, bool(reverse))
        y = torch.empty((n, Dm), dtype=u.dtype, device=u.device)
        if n > 0:
            selective_scan_into(u.detach().contiguous(), delta.detach().contiguous(), A.detach().contiguous(),
                                B.detach().contiguous(), C.detach().contiguous(), _opt(D), _opt(z), _opt(delta_bias),
                                delta_softplus, seq, reverse, y, _ws(scan_ws_bytes(n, seq.num_sequences, Dm, G), u.device))
        return y


# ---------------------------------------------------------------------------------------------- convolution

def check_conv(x, weight, bias, seq, activation) -> Tuple[int, int, int]:
    """(n, Dm, W) of a causal_conv1d_rows call"""
    op = "causal_conv1d_rows"
    if x.dtype not in _CODES:
        raise NotImplementedError(f"{op}: rows must be float16, bfloat16 or float32 (nothing is cast), got {x.dtype}")
    if x.dim() != 2 or weight.dim() != 2:
        raise ValueError(f"{op}: x is [n, Dm] and weight [Dm, W], got {tuple(x.shape)} and {tuple(weight.shape)}")
    n, Dm = (int(v) for v in x.shape)
    W = int(weight.shape[1])
    if W not in WIDTHS:
        raise NotImplementedError(f"{op}: the width must be in {WIDTHS[0]} .. {WIDTHS[-1]}, got {W}")
    _check_channels(op, Dm)
    if activation not in _ACTS:
        raise NotImplementedError(f"{op}: activation is None or 'silu', got {activation!r}")
    for name, t, shape in (("weight", weight, (Dm, W)), ("bias", bias, (Dm,))):
        if t is not None and (tuple(t.shape) != shape or t.dtype not in (x.dtype, torch.float32)):
            raise ValueError(f"{op}: {name} is {list(shape)} of {x.dtype} or float32, got {tuple(t.shape)} {t.dtype}")
    _check_seq(op, seq, x)
    return n, Dm, W


def conv_ws_bytes(n: int, Dm: int, W: int) -> int:
    """bytes of the workspace of causal_conv1d_rows_bwd_into"""
    return int(_lib.load().spx_causal_conv_rows_ws_bytes(int(n), int(Dm), int(W)))


def causal_conv1d_rows_into(x, weight, bias, seq: ScanSequences, reverse: bool, activation, out: torch.Tensor) -> None:
    """out[r(p)] = act(bias + sum_j weight[:, j] * x[r(p - (W - 1) + j)]) into a buffer the caller owns: one launch"""
    n, Dm = (int(v) for v in x.shape)
    _lib.check(_lib.load().spx_causal_conv_rows_fwd(
        x.data_ptr(), weight.data_ptr(), _CODES[weight.dtype], _ptr(bias), _CODES[(weight if bias is None else bias).dtype],
        _ptr(seq.order), seq.offsets.data_ptr(), n, seq.num_sequences, Dm, int(weight.shape[1]), _CODES[x.dtype],
        _ACTS[activation], _step(reverse), out.data_ptr(), _stream(x)))


def causal_conv1d_rows_bwd_into(x, weight, bias, seq: ScanSequences, reverse: bool, activation, d_out, dx, dweight,
                                dbias, ws: torch.Tensor) -> None:
    """dx [n, Dm] in the rows' dtype, dweight [Dm, W] and dbias [Dm] (or None) float32, ws uint8 of ``conv_ws_bytes``"""
    n, Dm = (int(v) for v in x.shape)
    _lib.check(_lib.load().spx_causal_conv_rows_bwd(
        x.data_ptr(), weight.data_ptr(), _CODES[weight.dtype], _ptr(bias), _CODES[(weight if bias is None else bias).dtype],
        d_out.data_ptr(), _ptr(seq.order), seq.offsets.data_ptr(), n, seq.num_sequences, Dm, int(weight.shape[1]),
        _CODES[x.dtype], _ACTS[activation], _step(reverse), dx.data_ptr(), dweight.data_ptr(), _ptr(dbias), ws.data_ptr(),
        ws.numel(), _stream(x)))


class CausalConvRowsFunction(Function):
    """spx_causal_conv_rows_fwd / _bwd: gradients to x, weight and bias"""

    @staticmethod
    def forward(ctx, x, weight, bias, seq, reverse, activation):
        x, weight, bias = x.detach().contiguous(), weight.detach().contiguous(), _opt(bias)
        out = torch.empty_like(x)
        if x.shape[0] > 0:
            causal_conv1d_rows_into(x, weight, bias, seq, reverse, activation, out)
        ctx.save_for_backward(x, weight, bias)
        ctx.seq, ctx.flags = seq, (reverse, activation)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_output):
        x, weight, bias = ctx.saved_tensors
        if grad_output.dtype != x.dtype:
            raise NotImplementedError(f"causal_conv1d_rows: the gradient arrives as {grad_output.dtype}, the rows are {x.dtype}")
        with torch.cuda.device(x.device):
            dx = torch.empty_like(x)
            dw = torch.zeros(weight.shape, dtype=torch.float32, device=x.device)
            db = None if bias is None else torch.zeros(bias.shape, dtype=torch.float32, device=x.device)
            if x.shape[0] > 0:
                ws = _ws(conv_ws_bytes(x.shape[0], x.shape[1], weight.shape[1]), x.device)
                causal_conv1d_rows_bwd_into(x, weight, bias, ctx.seq, ctx.flags[0], ctx.flags[1], grad_output.contiguous(),
                                            dx, dw, db, ws)
        return dx, dw.to(weight.dtype), None if db is None else db.to(bias.dtype), None, None, None


def causal_conv1d_rows(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor] = None, *, seq: ScanSequences,
                       reverse: bool = False, activation: Optional[str] = None) -> torch.Tensor:
    """Causal depthwise convolution along the sequences ``seq`` (``causal_conv1d_fn`` without its padded layout), on the
    kernels of csrc/scan.hip.  x [n, Dm] in row order (float16, bfloat16 or float32; Dm a multiple of 64, at most 2048),
    weight [Dm, W] with W in 2 .. 4 and bias [Dm] in x's dtype or float32, activation None or "silu"::

        out[r(p), d] = act(bias[d] + sum_j weight[d, j] * x[r(p - (W - 1) + j), d])

    with taps before the sequence's first position zero; for ``reverse`` the taps reach the other way, so the
    convolution is causal in the walk direction.  fp32 accumulation in ascending j, one rounding; rows of no sequence get
    +0 (``seq.order`` is a permutation of the rows, as ``serialize`` leaves it).  Differentiable in x, weight and bias
    without atomics: identical run to run."""
    n, Dm, W = check_conv(x, weight, bias, seq, activation)
    with torch.cuda.device(x.device):
        if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (x, weight, bias)):
            return CausalConvRowsFunction.apply(x, weight, bias, seq, bool(reverse), activation)
        out = torch.empty_like(x, memory_format=torch.contiguous_format)
        if n > 0:
            causal_conv1d_rows_into(x.detach().contiguous(), weight.detach().contiguous(), _opt(bias), seq, reverse,
                                    activation, out)
        return out


# ---------------------------------------------------------------------------------------------- module

class SerializedMamba(torch.nn.Module):
    """A Mamba block over the serialised rows of a sparse level: ``mamba_ssm.Mamba`` with its parameter names, shapes and
    initialisation (``in_proj``, ``conv1d.weight`` [Dm, 1, W], ``conv1d.bias``, ``x_proj``, ``dt_proj``, ``A_log``, ``D``,
    ``out_proj``: those state dicts load), its convolution and scan on the kernels of csrc/scan.hip.  Not part of the
    reference.  ``bidirectional=True`` adds a second set of convolution and SSM parameters under a ``_b`` suffix
    (``conv1d_b``, ``x_proj_b``, ``dt_proj_b``, ``A_log_b``, ``D_b``) that walks every sequence backwards; the two outputs
    are summed ahead of ``out_proj`` (Voxel Mamba's form).  ``forward(x, ser, which=0)`` takes a ``SparseConvTensor`` and
    the ``Serialization`` of its indices and returns the tensor with new features; ``forward(feats, seq)`` takes plain
    rows [n, d_model] and ``scan_sequences``' tuple.  d_state is 16; expand * d_model a multiple of 64, at most 2048.  The
    linears stay torch; nothing is read back."""

    def __init__(self, d_model: int, d_state: int = 16, d_conv: int = 4, expand: int = 2, dt_rank="auto",
                 bidirectional: bool = False, dt_min: float = 0.001, dt_max: float = 0.1, dt_init_floor: float = 1e-4):
        super().__init__()
        self.d_model, self.d_state, self.d_conv = int(d_model), int(d_state), int(d_conv)
        self.d_inner = int(expand * self.d_model)
        self.dt_rank = math.ceil(self.d_model / 16) if dt_rank == "auto" else int(dt_rank)
        self.bidirectional = bool(bidirectional)
        if self.d_state != STATES:
            raise NotImplementedError(f"SerializedMamba: d_state must be {STATES}, got {d_state}")
        if self.d_conv not in WIDTHS:
            raise NotImplementedError(f"SerializedMamba: d_conv must be in {WIDTHS[0]} .. {WIDTHS[-1]}, got {d_conv}")
        _check_channels("SerializedMamba", self.d_inner)
        self.in_proj = torch.nn.Linear(self.d_model, 2 * self.d_inner, bias=False)
        self.out_proj = torch.nn.Linear(self.d_inner, self.d_model, bias=False)
        for sfx in ("", "_b")[:1 + self.bidirectional]:
            conv = torch.nn.Conv1d(self.d_inner, self.d_inner, self.d_conv, groups=self.d_inner, padding=self.d_conv - 1)
            x_proj = torch.nn.Linear(self.d_inner, self.dt_rank + 2 * self.d_state, bias=False)
            dt_proj = torch.nn.Linear(self.dt_rank, self.d_inner, bias=True)
            std = self.dt_rank ** -0.5
            torch.nn.init.uniform_(dt_proj.weight, -std, std)
            dt = torch.exp(torch.rand(self.d_inner) * (math.log(dt_max) - math.log(dt_min)) + math.log(dt_min))
            dt = dt.clamp(min=dt_init_floor)
            with torch.no_grad():
                dt_proj.bias.copy_(dt + torch.log(-torch.expm1(-dt)))      # (softplus of the bias gives dt back)
            A = torch.arange(1, self.d_state + 1, dtype=torch.float32).repeat(self.d_inner, 1)
            self.add_module("conv1d" + sfx, conv)
            self.add_module("x_proj" + sfx, x_proj)
            self.add_module("dt_proj" + sfx, dt_proj)
            self.register_parameter("A_log" + sfx, torch.nn.Parameter(torch.log(A)))
            self.register_parameter("D" + sfx, torch.nn.Parameter(torch.ones(self.d_inner)))

    def _ssm(self, x, z, seq, sfx: str, reverse: bool):
        conv, x_proj, dt_proj = (getattr(self, name + sfx) for name in ("conv1d", "x_proj", "dt_proj"))
        R, N = self.dt_rank, self.d_state
        x = causal_conv1d_rows(x, conv.weight.squeeze(1), conv.bias, seq=seq, reverse=reverse, activation="silu")
        dbl = x_proj(x)
        delta = torch.nn.functional.linear(dbl[:, :R], dt_proj.weight)
        B, C = dbl[:, R:R + N].contiguous().unsqueeze(1), dbl[:, R + N:].contiguous().unsqueeze(1)
        A = -torch.exp(getattr(self, "A_log" + sfx).float())
        return selective_scan(x, delta, A, B, C, getattr(self, "D" + sfx).float(), z, dt_proj.bias.float(), True, seq=seq,
                              reverse=reverse)

    def forward(self, x, ser, which: int = 0):
        from spconv_amd.pytorch.core import SparseConvTensor
        sparse = isinstance(x, SparseConvTensor)
        feats = x.features if sparse else x
        seq = ser if isinstance(ser, ScanSequences) else scan_sequences(ser, which)
        w = self.in_proj.weight                  # (two products: x and z leave contiguous, no strided halves to copy)
        xi = torch.nn.functional.linear(feats, w[:self.d_inner])
        z = torch.nn.functional.linear(feats, w[self.d_inner:])
        y = self._ssm(xi, z, seq, "", False)
        if self.bidirectional:
            y = y + self._ssm(xi, z, seq, "_b", True)
        out = self.out_proj(y)
        return x.replace_feature(out) if sparse else out

    def extra_repr(self) -> str:
        return (f"d_model={self.d_model}, d_state={self.d_state}, d_conv={self.d_conv}, d_inner={self.d_inner}, "
                f"dt_rank={self.dt_rank}, bidirectional={self.bidirectional}")
