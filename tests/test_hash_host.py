"""CPU: the user hash table before any kernel (csrc/hash.hip: spx_hash_*; spconv_amd/pytorch/hash.py).  The unit is linked,
the workspace size is positive and monotone, every refusal of the hash section of include/spconv_amd.h comes back as a
status with its message before a pointer is looked at (no kernel is launched in this file: the pointers that are not NULL
are host addresses that a launch would fault on), and hash.check_operand refuses what no kernel may be handed.

The device and dtype refusals live HERE and not in the GPU suite: without them such an operand reaches a kernel as a
foreign pointer, and no GPU test may be able to cause that."""
import ctypes

import pytest
import torch

from capi import exported, fails as _fails
from spconv_amd import _lib

ENTRIES = ("spx_hash_ws_bytes", "spx_hash_clear", "spx_hash_insert", "spx_hash_query", "spx_hash_insert_exist",
           "spx_hash_assign_arange", "spx_hash_items")
CAPS = (1, 2048, 2049, 524_289, 16_779_265)


def test_the_hash_unit_is_linked():
    assert "hash.o" in [o.rsplit("/", 1)[-1] for o in _lib.linked_objects()]
    assert set(ENTRIES) <= exported()
    L = _lib.load()
    for name in ENTRIES:
        assert getattr(L, name).argtypes is not None, name


def test_ws_bytes_is_positive_and_monotone():
    L = _lib.load()
    sizes = [int(L.spx_hash_ws_bytes(c)) for c in CAPS]
    assert all(s > 0 for s in sizes) and sizes == sorted(sizes), sizes
    # two int32 per block of 2048 slots (count, offset) and the total
    assert all(s >= 2 * 4 * -(-c // 2048) + 4 for s, c in zip(sizes, CAPS)), sizes
    assert int(L.spx_hash_ws_bytes(0)) > 0 and int(L.spx_hash_ws_bytes(-5)) > 0


def test_every_refusal_comes_before_the_device():
    L = _lib.load()
    host = (ctypes.c_longlong * 64)()                       # stands for "not NULL": never dereferenced by a refusal
    P = ctypes.cast(host, ctypes.c_void_p)
    ws_ok = int(L.spx_hash_ws_bytes(64))

    def insert(tk=P, tv=P, cap=64, kb=8, vb=8, keys=P, values=P, n=4):
        return L.spx_hash_insert(tk, tv, cap, kb, vb, keys, values, n, None)

    def query(tk=P, tv=P, cap=64, kb=8, vb=8, keys=P, out=P, flags=P, n=4):
        return L.spx_hash_query(tk, tv, cap, kb, vb, keys, out, flags, n, None)

    def exist(tk=P, tv=P, cap=64, kb=8, vb=8, keys=P, values=P, flags=P, n=4):
        return L.spx_hash_insert_exist(tk, tv, cap, kb, vb, keys, values, flags, n, None)

    def arange(tk=P, tv=P, cap=64, kb=8, vb=8, count=P, ws=P, ws_bytes=ws_ok):
        return L.spx_hash_assign_arange(tk, tv, cap, kb, vb, count, ws, ws_bytes, None)

    def items(tk=P, tv=P, cap=64, kb=8, vb=8, ko=P, vo=P, max_out=64, count=P, ws=P, ws_bytes=ws_ok):
        return L.spx_hash_items(tk, tv, cap, kb, vb, ko, vo, max_out, count, ws, ws_bytes, None)

    for call in (insert, query, exist, arange, items):
        for bad in (0, 2, 3, 16, -4):                        # bad widths
            _fails(call(kb=bad), "4 or 8 bytes")
            _fails(call(vb=bad), "4 or 8 bytes")
        _fails(call(tk=None), "storage required")            # null table
        _fails(call(tv=None), "storage required")
        _fails(call(cap=0), "storage required")              # capacity 0
        _fails(call(cap=-1), "storage required")
    for call in (insert, query, exist):
        _fails(call(keys=None), "keys is NULL")              # null keys with n > 0
        _fails(call(n=-1), "negative")
        assert call(keys=None, n=0) == 0                     # n = 0: nothing to read, nothing launched
    _fails(query(out=None), "values_out is NULL")
    _fails(exist(values=None), "values is NULL")
    assert query(keys=None, out=None, flags=None, n=0) == 0 and exist(keys=None, values=None, flags=None, n=0) == 0
    assert insert(keys=None, values=None, n=0) == 0
    for call in (arange, items):
        _fails(call(ws=None), "workspace too small")
        _fails(call(ws_bytes=ws_ok - 1), "workspace too small")
        _fails(call(ws_bytes=0), "workspace too small")
        _fails(call(cap=16_779_265, ws_bytes=int(L.spx_hash_ws_bytes(524_289))), "workspace too small")
    _fails(items(ko=None), "keys_out / vals_out is NULL")    # null outputs with max_out > 0
    _fails(items(vo=None), "keys_out / vals_out is NULL")
    _fails(items(ko=None, vo=None, max_out=1), "keys_out / vals_out is NULL")
    _fails(items(max_out=-1), "max_out")                     # negative max_out
    _fails(items(ko=None, vo=None, max_out=-1), "max_out")
    _fails(L.spx_hash_clear(None, 64, 8, None), "bad hash table")
    _fails(L.spx_hash_clear(P, 0, 8, None), "bad hash table")
    _fails(L.spx_hash_clear(P, 64, 5, None), "bad hash table")


def test_check_operand_refuses_what_no_kernel_may_see():
    from spconv_amd.pytorch.hash import check_operand
    cpu, gpu = torch.device("cpu"), torch.device("cuda:0")
    k = torch.arange(8, dtype=torch.int64)
    assert check_operand("keys", k, torch.int64, cpu) is k
    assert check_operand("values", k, torch.int64, cpu, 8, in_place=True) is k
    for wrong in (torch.int32, torch.float64, torch.float32):           # wrong dtype (a 4-byte buffer for an 8-byte table)
        with pytest.raises(ValueError, match=r"^keys must have dtype torch\.int64"):
            check_operand("keys", k.to(wrong), torch.int64, cpu)
    with pytest.raises(ValueError, match="^values must have dtype torch.float64"):
        check_operand("values", torch.zeros(8, dtype=torch.float32), torch.float64, cpu, 8, in_place=True)
    with pytest.raises(ValueError, match="^keys must be 1-d"):          # 2-d, 0-d
        check_operand("keys", k.reshape(2, 4), torch.int64, cpu)
    with pytest.raises(ValueError, match="^keys must be 1-d"):
        check_operand("keys", k[0], torch.int64, cpu)
    for n in (7, 9, 0):                                                 # wrong length
        with pytest.raises(ValueError, match=f"^values must have length {n}, got 8"):
            check_operand("values", k, torch.int64, cpu, n)
    with pytest.raises(ValueError, match="^keys must be on the table's device cuda:0, got cpu"):      # wrong device
        check_operand("keys", k, torch.int64, gpu)
    with pytest.raises(ValueError, match="^values must be on the table's device cuda:0, got cpu"):
        check_operand("values", k, torch.int64, gpu, 8, in_place=True)
    with pytest.raises(ValueError, match="^keys must be on the table's device cuda:1"):
        check_operand("keys", torch.empty(8, dtype=torch.int64, device="meta"), torch.int64, torch.device("cuda:1"))
    with pytest.raises(ValueError, match="^keys must be a tensor"):
        check_operand("keys", [1, 2, 3], torch.int64, cpu)
    # a strided view: an input is made contiguous, a buffer the kernel fills for the caller is refused (never copied)
    wide = torch.arange(16, dtype=torch.int64)
    view = wide[::2]
    made = check_operand("keys", view, torch.int64, cpu, 8)
    assert made.is_contiguous() and torch.equal(made, view) and made.data_ptr() != view.data_ptr()
    with pytest.raises(ValueError, match="^values must be contiguous"):
        check_operand("values", view, torch.int64, cpu, 8, in_place=True)
    same = wide[4:12]                                                    # a contiguous view stays the caller's memory
    assert check_operand("values", same, torch.int64, cpu, 8, in_place=True).data_ptr() == same.data_ptr()


def test_every_method_checks_its_operands():
    """insert, query and insert_exist_keys refuse a bad keys or values operand before anything native is touched: a
    table whose storage is on the meta device has no library handle and no memory a kernel could be given"""
    from spconv_amd.pytorch.hash import HashTable

    class Table(HashTable):
        def __init__(self):
            self.key_dtype, self.value_dtype = torch.int64, torch.float64
            self.keys_data = torch.empty(16, dtype=torch.int64, device="meta")
            self.values_data = torch.empty(16, dtype=torch.float64, device="meta")

    t = Table()
    k = torch.empty(3, dtype=torch.int64, device="meta")
    v = torch.empty(3, dtype=torch.float64, device="meta")
    for method in (t.insert, t.query, t.insert_exist_keys):
        with pytest.raises(ValueError, match="^keys must be on the table's device meta, got cpu"):
            method(torch.zeros(3, dtype=torch.int64), v)
        with pytest.raises(ValueError, match="^keys must have dtype torch.int64"):
            method(k.to(torch.int32), v)
        with pytest.raises(ValueError, match="^keys must be 1-d"):
            method(k.reshape(3, 1), v)
        with pytest.raises(ValueError, match="^values must have dtype torch.float64"):       # the narrow buffer
            method(k, v.to(torch.float32))
        with pytest.raises(ValueError, match="^values must have length 3, got 4"):
            method(k, torch.empty(4, dtype=torch.float64, device="meta"))
        with pytest.raises(ValueError, match="^values must be on the table's device meta, got cpu"):
            method(k, torch.zeros(3, dtype=torch.float64))
    with pytest.raises(ValueError, match="^values must be contiguous"):                      # query fills it in place
        t.query(k, torch.empty(6, dtype=torch.float64, device="meta")[::2])
    with pytest.raises(ValueError, match="max_size"):
        t.items(max_size=-2)
    with pytest.raises(NotImplementedError, match="MI355X"):
        HashTable(torch.device("cpu"), torch.int64, torch.float64, 16)
