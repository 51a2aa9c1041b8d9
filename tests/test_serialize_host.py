"""CPU: the host side of voxel serialisation (csrc/serialize.hip, pytorch/_serialize.py) -- workspace queries, the
63-bit rule and every refusal, all of which come before any launch (nothing here touches a GPU)."""
import pytest
import torch

from spconv_amd import _lib
from spconv_amd.pytorch import _serialize
from spconv_amd.pytorch import functional as F


@pytest.fixture(scope="module")
def lib():
    if not __import__("os").path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


def test_workspace_queries_are_monotone_in_n(lib):
    for fn, rest in ((lib.spx_serialize_ws_bytes, (4, 36)), (lib.spx_serialize_ws_bytes, (1, 14)),
                     (lib.spx_serialize_ws_bytes, (8, 63)), (lib.spx_patch_plan_ws_bytes, (4, 48))):
        sizes = [int(fn(n, *rest)) for n in (0, 1, 511, 512, 513, 5000, 100_000, 400_000)]
        assert sizes[0] > 0 and sizes == sorted(sizes), (rest, sizes)
    # 64-bit keys and their buffers cost more than the narrowed 32-bit ones
    assert lib.spx_serialize_ws_bytes(100_000, 1, 33) > lib.spx_serialize_ws_bytes(100_000, 1, 32)


def test_workspace_queries_refuse_with_zero(lib):
    for args in ((-1, 4, 36), (100, 0, 36), (100, 9, 36), (100, 4, 0), (100, 4, 64)):
        assert lib.spx_serialize_ws_bytes(*args) == 0, args
    for args in ((-1, 2, 4), (100, 0, 4), (100, 2, 0), (100, 2, -3), (2**31 - 1, 2**20, 2**12)):
        assert lib.spx_patch_plan_ws_bytes(*args) == 0, args


def test_c_calls_refuse_before_any_pointer(lib):
    """Every argument check that needs no pointer comes first: NULL everywhere, the geometry is what is refused."""
    I = _lib.ints
    keys = lambda **kw: lib.spx_curve_keys(None, kw.get("n", 8), None, kw.get("ndim", 3), kw.get("batch", 2),
                                           kw.get("depth", 4), kw.get("k", 1), I(kw.get("orders", [0])),
                                           I(kw.get("axes", [2, 1, 0])), None, None)
    for kw, word in ((dict(ndim=5), "ndim"), (dict(depth=17), "depth"), (dict(depth=0), "depth"), (dict(batch=0), "batch"),
                     (dict(k=0), "orders"), (dict(k=9, orders=[0] * 9), "orders"), (dict(depth=16, batch=65536), "63"),
                     (dict(orders=[4]), "order"), (dict(axes=[0, 0, 1]), "permutation"), (dict(n=-1), "row count")):
        assert keys(**kw) != 0 and word.encode() in lib.spx_last_error(), kw
    assert keys(n=0) == 0                                        # nothing to do: no pointer is needed
    assert keys(depth=16, batch=32767, n=0) == 0                 # exactly 63 bits
    assert lib.spx_serialize(None, 8, 1, 64, 2, 12, None, None, None, None, 0, None) != 0
    assert lib.spx_serialize(None, 8, 1, 13, 2, 12, None, None, None, None, 0, None) != 0      # no room for batch 2
    assert b"geometry" in lib.spx_last_error()
    assert lib.spx_patch_plan(None, None, 8, 2, 0, 1, None, None, None, None, None, None, None, 0, None) != 0
    assert b"patch_size" in lib.spx_last_error()
    assert lib.spx_patch_plan(None, None, 8, 2, 4, 2, None, None, None, None, None, None, None, 0, None) != 0
    assert b"pad" in lib.spx_last_error()
    assert lib.spx_patch_rows_bwd(None, 8, None, None, 8, 0, _lib.DTYPE_F32, None, None) != 0
    assert lib.spx_patch_rows_bwd(None, 8, None, None, 8, 4, _lib.DTYPE_I8, None, None) != 0


def test_the_63_bit_rule():
    assert _serialize.key_bits(3, 11, 4) == 36 and _serialize.default_depth([41, 1600, 1408]) == 11
    assert _serialize.key_bits(3, 16, 32767) == 63 and _serialize.key_bits(3, 16, 32768) == 64
    _serialize.check_geometry(3, 32767, None, ("z",), 16, None)
    _serialize.check_geometry(4, 7, None, ("hilbert",), 15, None)
    for ndim, batch, depth in ((3, 32768, 16), (4, 1, 16), (4, 16, 15)):
        with pytest.raises(ValueError, match="at most 63"):
            _serialize.check_geometry(ndim, batch, None, ("z",), depth, None)
    assert _serialize.check_geometry(3, 2, [1, 1, 1], "z", None, None) == (("z",), 1, (2, 1, 0))
    assert _serialize.check_geometry(2, 2, [5, 70000], ("z",), 3, (0, 1))[1:] == (3, (0, 1))
    with pytest.raises(ValueError, match="depth"):
        _serialize.check_geometry(2, 2, [5, 70000], ("z",), None, None)          # 17 bits per axis


def _ser(n=6, batch=2, device="cpu"):
    i32 = dict(dtype=torch.int32, device=device)
    return F.Serialization(torch.zeros((1, n), dtype=torch.int64, device=device), torch.zeros((1, n), **i32),
                           torch.zeros((1, n), **i32), torch.zeros((batch + 1,), **i32), 4, ("z",))


def test_every_refusal_is_raised_before_any_launch():
    idx = torch.zeros((6, 4), dtype=torch.int32)
    with pytest.raises(NotImplementedError, match="MI355X"):
        F.serialize(idx, [8, 8, 8], 2)                                              # CPU tensors
    with pytest.raises(NotImplementedError, match="int32"):
        F.serialize(idx.long(), [8, 8, 8], 2)
    with pytest.raises(ValueError, match="unknown order"):
        F.serialize(idx, [8, 8, 8], 2, orders=("z", "morton"))
    for axes in ((0, 1), (0, 1, 1), (1, 2, 3)):
        with pytest.raises(ValueError, match="permutation"):
            F.serialize(idx, [8, 8, 8], 2, axes=axes)
    with pytest.raises(ValueError, match="at most 63"):
        F.serialize(idx, None, 32768, depth=16)
    with pytest.raises(ValueError, match="depth"):
        F.serialize(idx, None, 2, depth=17)
    with pytest.raises(ValueError, match="batch_size"):
        F.serialize(idx, [8, 8, 8])
    with pytest.raises(ValueError, match="orders"):
        F.serialize(idx, [8, 8, 8], 2, orders=())
    for size in (0, -4, 2.5):
        with pytest.raises(ValueError, match="patch_size"):
            F.patch_plan(_ser(), size)
    with pytest.raises(ValueError, match="pad"):
        F.patch_plan(_ser(), 4, pad="wrap")
    with pytest.raises(ValueError, match="which"):
        F.patch_plan(_ser(), 4, which=1)
    with pytest.raises(NotImplementedError, match="MI355X"):
        F.patch_plan(_ser(), 4)


def test_hand_built_serializations_and_plans_are_checked():
    """The kernels read these tables through raw pointers: dtype, shape and device are checked on the host."""
    ser = _ser()
    for bad in (ser._replace(order=ser.order.long()), ser._replace(offsets=ser.offsets.long()),
                ser._replace(offsets=ser.offsets[:1]), ser._replace(order=ser.order[0])):
        with pytest.raises(ValueError, match="int32"):
            F.patch_plan(bad, 4)
    with pytest.raises(ValueError, match="offsets on meta"):
        F.patch_plan(ser._replace(offsets=ser.offsets.to("meta")), 4)
    i32 = dict(dtype=torch.int32)
    plan = F.PatchPlan(torch.zeros((3, 4), **i32), torch.zeros((3, 4), **i32), torch.zeros((6,), **i32),
                       torch.zeros((6,), **i32), torch.zeros((3,), **i32), torch.zeros((1,), **i32), 4, "borrow")
    feat = torch.zeros((6, 8))
    _serialize.check_plan(plan, feat, "rows_to_patches")
    for bad in (plan._replace(row_slot=plan.row_slot.long()), plan._replace(row_slot2=plan.row_slot2[:5]),
                plan._replace(patch_rows_canon=plan.patch_rows_canon.t()), plan._replace(patch_rows=plan.patch_rows[:, ::2])):
        with pytest.raises(ValueError, match="contiguous int32"):
            _serialize.check_plan(bad, feat, "rows_to_patches")
    with pytest.raises(ValueError, match="row_slot is on meta"):
        _serialize.check_plan(plan._replace(row_slot=plan.row_slot.to("meta")), feat, "rows_to_patches")
