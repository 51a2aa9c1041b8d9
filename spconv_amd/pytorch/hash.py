"""Fixed-size GPU hash table for 32 / 64 bit keys and values (reference:
``spconv/pytorch/hash.py:29-170``).  Same constructor and methods; storage is two torch tensors
owned by this object, the operations run in ``spx_hash_*``.

The contract is the hash section of ``include/spconv_amd.h``.  In short: the all-ones key (-1) marks an empty slot and
is never a member -- ``insert`` ignores it, ``query`` / ``insert_exist_keys`` report it absent; a key that finds no free
slot is dropped and later reported absent; ``query`` writes a value only where the key is present; ``assign_arange_`` /
``items`` enumerate the occupied slots in ascending slot index -- two calls on an unchanged table agree bit for bit, and
the numbering depends on the slot contents, hence on insertion and arrival order.  Every ``keys`` / ``values`` operand
goes through ``check_operand`` before a kernel sees its pointer."""
from __future__ import annotations

from typing import Optional

import contextlib
import functools

import torch

from spconv_amd import _lib


def _on_table_device(method):
    """Runs a method with the table's device current (torch's DeviceGuard convention): the native calls
    and their scratch allocations belong to the device the table lives on, also when the caller never
    called torch.cuda.set_device."""
    @functools.wraps(method)
    def guarded(self, *args, **kwargs):
        dev = self.keys_data.device
        ctx = (torch.cuda.device(dev) if dev.type == "cuda" and dev.index != torch.cuda.current_device()
               else contextlib.nullcontext())
        with ctx:
            return method(self, *args, **kwargs)
    return guarded

_ITEMSIZE = {torch.int32: 4, torch.int64: 8, torch.float32: 4, torch.float64: 8}


def check_operand(name: str, t, dtype: torch.dtype, device: torch.device, length: Optional[int] = None,
                  in_place: bool = False) -> torch.Tensor:
    """The operand a kernel may be handed: a 1-d tensor of `dtype` on `device` (the table's) with `length` elements
    (None: any), contiguous.  ValueError naming the operand otherwise.  A strided operand is made contiguous, except
    one the kernel writes for the caller (in_place): that one is refused, a copy would be filled in its stead.
    Pure: looks at the tensor's metadata only, needs no GPU."""
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{name} must be a tensor, got {type(t).__name__}")
    if t.dtype != dtype:
        raise ValueError(f"{name} must have dtype {dtype} (the table's), got {t.dtype}")
    if t.ndim != 1:
        raise ValueError(f"{name} must be 1-d, got shape {tuple(t.shape)}")
    if length is not None and t.shape[0] != length:
        raise ValueError(f"{name} must have length {length}, got {t.shape[0]}")
    if t.device != torch.device(device):
        raise ValueError(f"{name} must be on the table's device {device}, got {t.device}")
    if not t.is_contiguous():
        if in_place:
            raise ValueError(f"{name} must be contiguous (it is written in place), got stride {tuple(t.stride())}")
        t = t.contiguous()
    return t


class HashTable:
    def __init__(self, device: torch.device, key_dtype: torch.dtype, value_dtype: torch.dtype,
                 max_size: int = -1) -> None:
        device = torch.device(device)
        if device.type != "cuda":
            raise NotImplementedError("spconv_amd runs on MI355X only: HashTable needs a cuda device")
        assert key_dtype in (torch.int32, torch.int64), "key must be int32/int64"
        assert value_dtype in _ITEMSIZE, "value must be a 32 or 64 bit type"
        assert max_size > 0, ("you must provide max_size for fixed-size cuda hash table, usually *2 "
                              "of num of keys")
        self.is_cpu = False
        self.key_dtype = key_dtype
        self.value_dtype = value_dtype
        self.key_itemsize = _ITEMSIZE[key_dtype]
        self.value_itemsize = _ITEMSIZE[value_dtype]
        self.keys_data = torch.empty([max_size], dtype=key_dtype, device=device)
        self.values_data = torch.empty([max_size], dtype=value_dtype, device=device)
        self._L = _lib.load()
        with torch.cuda.device(device):
            _lib.check(self._L.spx_hash_clear(self.keys_data.data_ptr(), max_size, self.key_itemsize,
                                              self._stream()))

    def _stream(self):
        return torch.cuda.current_stream(self.keys_data.device).cuda_stream

    def _args(self):
        return (self.keys_data.data_ptr(), self.values_data.data_ptr(), self.keys_data.shape[0],
                self.key_itemsize, self.value_itemsize)

    def _keys(self, keys: torch.Tensor) -> torch.Tensor:
        return check_operand("keys", keys, self.key_dtype, self.keys_data.device)

    def _values(self, values: torch.Tensor, n: int, in_place: bool = False) -> torch.Tensor:
        return check_operand("values", values, self.value_dtype, self.keys_data.device, n, in_place)

    @_on_table_device
    def insert(self, keys: torch.Tensor, values: Optional[torch.Tensor] = None):
        """insert keys (and values; without values the value storage is not written).  -1 is ignored; a key that finds
        no free slot is dropped"""
        keys = self._keys(keys)
        if values is not None:
            values = self._values(values, keys.shape[0])
        _lib.check(self._L.spx_hash_insert(*self._args(), keys.data_ptr(),
                                           None if values is None else values.data_ptr(),
                                           keys.shape[0], self._stream()))

    @_on_table_device
    def query(self, keys: torch.Tensor, values: Optional[torch.Tensor] = None):
        """-> (values, bool tensor that is True where the key was NOT found).  A row of `values` is written only where
        the key was found: with a caller's `values` (filled in place, never replaced by a copy) the other rows keep
        their content, without one they are uninitialised"""
        keys = self._keys(keys)
        if values is None:
            values = torch.empty([keys.shape[0]], dtype=self.value_dtype, device=keys.device)
        else:
            values = self._values(values, keys.shape[0], in_place=True)
        is_empty = torch.empty([keys.shape[0]], dtype=torch.uint8, device=keys.device)
        _lib.check(self._L.spx_hash_query(*self._args(), keys.data_ptr(), values.data_ptr(),
                                          is_empty.data_ptr(), keys.shape[0], self._stream()))
        return values, is_empty > 0

    @_on_table_device
    def insert_exist_keys(self, keys: torch.Tensor, values: torch.Tensor):
        """overwrite the values of keys that exist; -> uint8 tensor, 1 where the key was missing"""
        keys = self._keys(keys)
        values = self._values(values, keys.shape[0])
        is_empty = torch.empty([keys.shape[0]], dtype=torch.uint8, device=keys.device)
        _lib.check(self._L.spx_hash_insert_exist(*self._args(), keys.data_ptr(),
                                                 values.data_ptr(), is_empty.data_ptr(),
                                                 keys.shape[0], self._stream()))
        return is_empty

    def _ws(self):
        return torch.empty((int(self._L.spx_hash_ws_bytes(self.keys_data.shape[0])),), dtype=torch.uint8,
                           device=self.keys_data.device)

    @_on_table_device
    def assign_arange_(self):
        """every key gets its rank among the occupied slots, in ascending slot index, as value; -> count (1-element
        tensor of the key dtype)"""
        assert self.value_dtype in (torch.int32, torch.int64)
        count = torch.zeros([1], dtype=self.key_dtype, device=self.keys_data.device)
        ws = self._ws()
        _lib.check(self._L.spx_hash_assign_arange(*self._args(), count.data_ptr(), ws.data_ptr(),
                                                  ws.numel(), self._stream()))
        return count

    @_on_table_device
    def items(self, max_size: int = -1):
        """-> (keys, values, count): the first min(count, max_size) entries are the table's content in ascending slot
        index (the order of assign_arange_), the rest is uninitialised; count is the number of keys also when max_size
        is smaller"""
        if max_size == -1:
            max_size = self.values_data.shape[0]
        if max_size < 0:
            raise ValueError(f"max_size must be -1 (the capacity) or >= 0, got {max_size}")
        dev = self.keys_data.device
        keys = torch.empty([max_size], dtype=self.key_dtype, device=dev)
        values = torch.empty([max_size], dtype=self.value_dtype, device=dev)
        count = torch.zeros([1], dtype=self.key_dtype, device=dev)
        ws = self._ws()
        _lib.check(self._L.spx_hash_items(*self._args(), keys.data_ptr(), values.data_ptr(), max_size,
                                          count.data_ptr(), ws.data_ptr(), ws.numel(), self._stream()))
        return keys, values, count
