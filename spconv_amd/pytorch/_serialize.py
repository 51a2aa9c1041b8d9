"""Voxel serialisation on the HIP kernels of csrc/serialize.hip: the rows of a sparse level ordered along Z-order and
Hilbert curves and cut into fixed-size patches (``functional.serialize`` / ``patch_plan`` / ``rows_to_patches`` /
``patches_to_rows``).  Not part of the reference; the serialised point / voxel transformers (Point Transformer V3,
OctFormer, FlatFormer-style blocks) write the step as a Python loop over bits and axes, ``argsort`` on int64, a scatter,
``bincount`` + ``cumsum`` and padding arithmetic with read-backs.

  * ``serialize``        per requested order the 64-bit key of every row (``spx_curve_keys``: one launch), the rows in
                         key order, the inverse permutation and the scenes' offsets (``spx_serialize``: a stable radix
                         sort over exactly the key bits in use); dead rows behind every live one; nothing read back
  * ``patch_plan``       scenes laid out on patch boundaries in a host-known number of patches (``spx_patch_plan``)
  * ``rows_fwd`` / ``rows_bwd`` / ``patches_fwd`` / ``patches_bwd`` move the feature rows: three of them are
    ``spx_voxel_to_point`` with a zero fill, the gradient of the way into the patches adds a row's canonical and
    borrowed slot (``spx_patch_rows_bwd``: no atomics).  There is no composite to fall back to.

``depth`` is known on the host (from the spatial shape), which is what lets the whole step sit inside a captured graph.
"""
from __future__ import annotations

from typing import NamedTuple, Optional, Sequence, Tuple

import torch

from spconv_amd import _lib
from spconv_amd.pytorch._rulebook import _check_count, _float_code, _ptr, _require_gpu, _stream, _ws

ORDERS = {"z": 0, "z-trans": 1, "hilbert": 2, "hilbert-trans": 3}     # SPX_ORDER_*
PADS = {"mask": 0, "borrow": 1}                                        # SPX_PAD_*
DEFAULT_ORDERS = ("z", "z-trans", "hilbert", "hilbert-trans")
MAX_ORDERS, MAX_DEPTH, MAX_KEY_BITS = 8, 16, 63


class Serialization(NamedTuple):
    """code int64 [K, n] ((batch << (ndim * depth)) | curve code, -1 for a dead row), order / inverse int32 [K, n]
    (order[k, t] = the row with the t-th smallest key, dead rows last in ascending row; inverse[k, order[k, t]] = t),
    offsets int32 [batch_size + 1] (live rows of a smaller batch index; shared by all orders), depth (bits per axis),
    orders (the names asked for)."""
    code: torch.Tensor
    order: torch.Tensor
    inverse: torch.Tensor
    offsets: torch.Tensor
    depth: int
    orders: Tuple[str, ...]


class PatchPlan(NamedTuple):
    """patch_rows / patch_rows_canon int32 [P_cap, K] (row of each slot, -1: none; canon: borrowed slots as -1),
    row_slot / row_slot2 int32 [n] (canonical / borrowed slot of a row, -1: none), patch_scene int32 [P_cap] (batch
    index, -1: patch not in use), n_patches_dev int32 [1] (patches in use), patch_size, pad."""
    patch_rows: torch.Tensor
    patch_rows_canon: torch.Tensor
    row_slot: torch.Tensor
    row_slot2: torch.Tensor
    patch_scene: torch.Tensor
    n_patches_dev: torch.Tensor
    patch_size: int
    pad: str


def default_depth(spatial_shape: Sequence[int]) -> int:
    """Bits that hold every coordinate of the grid: the bit length of its largest extent - 1, at least 1."""
    return max(1, (max(int(v) for v in spatial_shape) - 1).bit_length())


def key_bits(ndim: int, depth: int, batch_size: int) -> int:
    """Key bits in use: the curve code and a batch field wide enough for the dead key to sort behind batch_size - 1."""
    return int(ndim) * int(depth) + int(batch_size).bit_length()


def serialize_ws_bytes(n: int, n_orders: int, bits: int) -> int:
    return int(_lib.load().spx_serialize_ws_bytes(int(n), int(n_orders), int(bits)))


def check_geometry(ndim: int, batch_size: int, spatial_shape, orders, depth, axes):
    """(order codes, depth, axes) of a serialize call, from host-known arguments alone."""
    if not 1 <= ndim <= 4:
        raise ValueError(f"serialize: ndim must be in [1, 4], got {ndim}")
    if int(batch_size) < 1:
        raise ValueError(f"serialize: batch_size must be >= 1, got {batch_size}")
    orders = (orders,) if isinstance(orders, str) else tuple(orders)
    if not 1 <= len(orders) <= MAX_ORDERS:
        raise ValueError(f"serialize: 1 to {MAX_ORDERS} orders per call, got {len(orders)}")
    for o in orders:
        if o not in ORDERS:
            raise ValueError(f"serialize: unknown order {o!r}; known: {sorted(ORDERS)}")
    if axes is None:
        axes = tuple(range(ndim - 1, -1, -1))
    else:
        axes = tuple(int(a) for a in axes)
        if sorted(axes) != list(range(ndim)):
            raise ValueError(f"serialize: axes must be a permutation of 0 .. {ndim - 1}, got {axes}")
    if depth is None:
        if spatial_shape is None:
            raise ValueError("serialize: give a spatial_shape or a depth")
        depth = default_depth(spatial_shape)
    depth = int(depth)
    if not 1 <= depth <= MAX_DEPTH:
        raise ValueError(f"serialize: depth must be in [1, {MAX_DEPTH}], got {depth}")
    bits = key_bits(ndim, depth, batch_size)
    if bits > MAX_KEY_BITS:
        raise ValueError(f"serialize: {ndim} axes x {depth} bits and {int(batch_size).bit_length()} batch bits make a "
                         f"key of {bits} bits; at most {MAX_KEY_BITS}")
    return orders, depth, axes


def serialize(indices: torch.Tensor, batch_size: int, spatial_shape=None, orders=DEFAULT_ORDERS, depth=None, axes=None,
              n_live: Optional[torch.Tensor] = None) -> Serialization:
    if indices.dim() != 2:
        raise ValueError(f"serialize: indices is [n, ndim + 1], got {tuple(indices.shape)}")
    ndim, n = int(indices.shape[1]) - 1, int(indices.shape[0])
    if spatial_shape is not None and len(spatial_shape) != ndim:
        raise ValueError(f"serialize: indices have {ndim} spatial columns, spatial_shape {len(spatial_shape)}")
    orders, depth, axes = check_geometry(ndim, batch_size, spatial_shape, orders, depth, axes)
    if indices.dtype != torch.int32:
        raise NotImplementedError(f"serialize: indices must be int32, got {indices.dtype}")
    _require_gpu(indices, "indices")
    _check_count(n_live, "serialize: n_live")
    if n_live is not None and n_live.device != indices.device:
        raise ValueError(f"serialize: indices are on {indices.device}, n_live on {n_live.device}")
    B, K, dev = int(batch_size), len(orders), indices.device
    bits = key_bits(ndim, depth, B)
    L = _lib.load()
    with torch.cuda.device(dev), torch.no_grad():
        indices = indices.contiguous()
        code = torch.empty((K, n), dtype=torch.int64, device=dev)
        order = torch.empty((K, n), dtype=torch.int32, device=dev)
        inverse = torch.empty((K, n), dtype=torch.int32, device=dev)
        offsets = torch.empty((B + 1,), dtype=torch.int32, device=dev)
        ws = _ws(serialize_ws_bytes(n, K, bits), dev)
        stream = _stream(indices)
        _lib.check(L.spx_curve_keys(indices.data_ptr(), n, _ptr(n_live), ndim, B, depth, K,
                                    _lib.ints([ORDERS[o] for o in orders]), _lib.ints(axes), code.data_ptr(), stream))
        _lib.check(L.spx_serialize(code.data_ptr(), n, K, bits, B, ndim * depth, order.data_ptr(), inverse.data_ptr(),
                                   offsets.data_ptr(), ws.data_ptr(), ws.numel(), stream))
    return Serialization(code, order, inverse, offsets, depth, orders)


def patch_plan(ser: Serialization, patch_size: int, which: int = 0, pad: str = "borrow") -> PatchPlan:
    if int(patch_size) != patch_size or patch_size < 1:
        raise ValueError(f"patch_plan: patch_size must be an integer >= 1, got {patch_size!r}")
    if pad not in PADS:
        raise ValueError(f"patch_plan: pad must be 'mask' or 'borrow', got {pad!r}")
    if ser.order.dim() != 2:
        raise ValueError(f"patch_plan: order is int32 [K, n], got {tuple(ser.order.shape)}")
    K_orders, n = (int(v) for v in ser.order.shape)
    if not 0 <= int(which) < K_orders:
        raise ValueError(f"patch_plan: which must be in [0, {K_orders}), got {which}")
    if ser.order.dtype != torch.int32 or ser.offsets.dtype != torch.int32 or ser.offsets.dim() != 1 or ser.offsets.shape[0] < 2:
        raise ValueError("patch_plan: order is int32 [K, n] and offsets int32 [batch_size + 1]")
    if ser.offsets.device != ser.order.device:
        raise ValueError(f"patch_plan: order is on {ser.order.device}, offsets on {ser.offsets.device}")
    _require_gpu(ser.order, "order")
    K, B, dev = int(patch_size), int(ser.offsets.shape[0]) - 1, ser.order.device
    P_cap = n // K + B
    if P_cap * K >= 1 << 31:
        raise ValueError(f"patch_plan: {P_cap} patches x {K} slots do not fit 32-bit slot numbers")
    L = _lib.load()
    i32 = dict(dtype=torch.int32, device=dev)
    with torch.cuda.device(dev), torch.no_grad():
        order, offsets = ser.order[int(which)].contiguous(), ser.offsets.contiguous()
        patch_rows = torch.empty((P_cap, K), **i32)
        canon = torch.empty((P_cap, K), **i32)
        row_slot = torch.empty((n,), **i32)
        row_slot2 = torch.empty((n,), **i32)
        scene = torch.empty((P_cap,), **i32)
        n_patches = torch.empty((1,), **i32)
        ws = _ws(int(L.spx_patch_plan_ws_bytes(n, B, K)), dev)
        _lib.check(L.spx_patch_plan(order.data_ptr(), offsets.data_ptr(), n, B, K, PADS[pad], patch_rows.data_ptr(),
                                    canon.data_ptr(), row_slot.data_ptr(), row_slot2.data_ptr(), scene.data_ptr(),
                                    n_patches.data_ptr(), ws.data_ptr(), ws.numel(), _stream(order)))
    return PatchPlan(patch_rows, canon, row_slot, row_slot2, scene, n_patches, K, pad)


def _gather(feat: torch.Tensor, rows: torch.Tensor) -> torch.Tensor:
    from spconv_amd.pytorch import _pointvoxel
    with torch.cuda.device(feat.device):
        return _pointvoxel.gather_rows(feat, rows.reshape(-1), 0)


def rows_fwd(feat: torch.Tensor, plan: PatchPlan) -> torch.Tensor:
    """[n, C] -> [P_cap, K, C]: slot s holds feat[patch_rows[s]], zeros where it is -1 (spx_voxel_to_point)."""
    P_cap, K = (int(v) for v in plan.patch_rows.shape)
    return _gather(feat, plan.patch_rows).reshape(P_cap, K, int(feat.shape[1]))


def rows_bwd(g: torch.Tensor, plan: PatchPlan) -> torch.Tensor:
    """[P_cap, K, C] -> [n, C]: g[row_slot[r]] + g[row_slot2[r]], canonical term first, rounded once
    (spx_patch_rows_bwd: one launch, no atomics); zeros for dead rows."""
    dt = _float_code(g, "rows_to_patches")
    P_cap, K = (int(v) for v in plan.patch_rows.shape)
    n, C = int(plan.row_slot.shape[0]), int(g.shape[-1])
    g = g.contiguous()
    with torch.cuda.device(g.device):
        out = torch.empty((n, C), dtype=g.dtype, device=g.device)
        if n > 0 and C > 0:
            _lib.check(_lib.load().spx_patch_rows_bwd(g.data_ptr(), P_cap * K, plan.row_slot.data_ptr(),
                                                      plan.row_slot2.data_ptr(), n, C, dt, out.data_ptr(), _stream(g)))
    return out


def patches_fwd(patches: torch.Tensor, plan: PatchPlan) -> torch.Tensor:
    """[P_cap, K, C] -> [n, C]: row r is its canonical slot, zeros for a dead row (spx_voxel_to_point)."""
    P_cap, K = (int(v) for v in plan.patch_rows.shape)
    return _gather(patches.reshape(P_cap * K, int(patches.shape[-1])), plan.row_slot)


def patches_bwd(g: torch.Tensor, plan: PatchPlan) -> torch.Tensor:
    """[n, C] -> [P_cap, K, C]: slot s takes g[patch_rows_canon[s]], zeros for borrowed and empty slots."""
    P_cap, K = (int(v) for v in plan.patch_rows.shape)
    return _gather(g, plan.patch_rows_canon).reshape(P_cap, K, int(g.shape[1]))


def check_plan(plan: PatchPlan, t: torch.Tensor, what: str) -> None:
    """The kernels read the plan's tables through raw pointers: contiguous int32 tensors on the rows' device, shaped as
    patch_plan leaves them."""
    P_cap, K = (int(v) for v in plan.patch_rows.shape) if plan.patch_rows.dim() == 2 else (-1, -1)
    n = int(plan.row_slot.shape[0]) if plan.row_slot.dim() == 1 else -1
    shapes = {"patch_rows": (P_cap, K), "patch_rows_canon": (P_cap, K), "row_slot": (n,), "row_slot2": (n,)}
    for name, shape in shapes.items():
        v = getattr(plan, name)
        if v.dtype != torch.int32 or tuple(v.shape) != shape or min(shape) < 0 or not v.is_contiguous():
            raise ValueError(f"{what}: the plan's {name} is a contiguous int32 tensor {list(shapes[name])}, got "
                             f"{v.dtype} {tuple(v.shape)}")
        if v.device != t.device:
            raise ValueError(f"{what}: the plan's {name} is on {v.device}, the rows on {t.device}")


def check_rows(feat: torch.Tensor, plan: PatchPlan, what: str) -> None:
    _require_gpu(feat, "features")
    _float_code(feat, what)
    check_plan(plan, feat, what)
    n = int(plan.row_slot.shape[0])
    if feat.dim() != 2 or feat.shape[0] != n:
        raise ValueError(f"{what}: one row per voxel ([{n}, C]), got {tuple(feat.shape)}")


def check_patches(patches: torch.Tensor, plan: PatchPlan, what: str) -> None:
    _require_gpu(patches, "patches")
    _float_code(patches, what)
    check_plan(plan, patches, what)
    P_cap, K = (int(v) for v in plan.patch_rows.shape)
    if patches.dim() != 3 or tuple(patches.shape[:2]) != (P_cap, K):
        raise ValueError(f"{what}: patches is [{P_cap}, {K}, C], got {tuple(patches.shape)}")
