"""The user hash table (csrc/hash.hip: spx_hash_*; spconv_amd/pytorch/hash.py) against the dictionary model of
tests/refhash.py, at every key / value width and at the capacities, loads and keys where an open-addressing table goes
wrong.  The contract is the hash section of include/spconv_amd.h.  Every comparison is bit for bit.

Every case goes through the public HashTable (the C entries directly only in the dirty-workspace case).  The value
storage of a table, every buffer a method allocates (outputs, flags, the workspace of assign_arange_ / items: the table's
module sees a torch whose `empty` hands out 0xA5 bytes) and every buffer the case passes in start as a byte pattern, so a
row that must not be written is seen to keep it.  After every mutation refhash.check_storage reads the RAW arrays:
exactly the model's keys, each once; no key behind a hole of its probe path; the model's value bits; empty slots still at
their prefill.

Nothing here hands a kernel a foreign pointer: the refusals of wrong devices and dtypes are host tests
(tests/test_hash_host.py), and the narrow buffer of test_a_narrow_buffer_is_refused lies inside an allocation that the
8-byte result would fit twice."""
import numpy as np
import pytest
import torch

import refhash as rh

pytestmark = pytest.mark.gpu

FILL = 0xA5
PREFILL = {4: 0xA5A5A5A5, 8: 0xA5A5A5A5A5A5A5A5}
SINT = {4: torch.int32, 8: torch.int64}
UINT = {4: np.uint32, 8: np.uint64}
I32, I64, F32, F64 = torch.int32, torch.int64, torch.float32, torch.float64
INT_PAIRS = [(I32, I32), (I32, I64), (I64, I32), (I64, I64)]          # the four (key, value) width pairs
FLOAT_PAIRS = [(I64, F32), (I32, F64)]                                # values that are NaN payloads and -0.0
KEY_BITS = {I32: 32, I64: 64}


def ids(pairs):
    return [f"{str(k)[6:]}-{str(v)[6:]}" for k, v in pairs]


@pytest.fixture(autouse=True)
def _end_the_run_at_a_gpu_fault(request):
    """A mismatch is one failed test.  A faulted device fails every later launch as well: the run ends at the first."""
    yield
    if torch.cuda.is_available():
        try:
            torch.cuda.synchronize()
        except RuntimeError as e:
            pytest.exit(f"the GPU faulted in {request.node.nodeid}: {e}", returncode=3)


def filled(shape, dtype, device, byte=FILL):
    """a buffer whose every byte is `byte`"""
    n = int(np.prod(shape))
    raw = torch.full((n * torch.empty((), dtype=dtype).element_size(),), byte, dtype=torch.uint8, device=device)
    return raw.view(dtype).reshape(shape)


class _PrefilledTorch:
    """torch as spconv_amd.pytorch.hash sees it in this file: `empty` hands out 0xA5 bytes, the rest is torch's"""

    def __getattr__(self, name):
        return getattr(torch, name)

    @staticmethod
    def empty(shape, dtype, device):
        return filled(shape, dtype, device)


@pytest.fixture(autouse=True)
def _prefilled_allocations(monkeypatch):
    from spconv_amd.pytorch import hash as H
    monkeypatch.setattr(H, "torch", _PrefilledTorch())


def bits(t):
    """the bit patterns of a tensor of 4- or 8-byte items, as unsigned numpy integers"""
    w = t.element_size()
    return t.detach().contiguous().view(SINT[w]).cpu().numpy().view(UINT[w])


def signed(t):
    return t.detach().cpu().numpy().astype(np.int64)


class Harness:
    """A table and its model side by side: every method runs the operation on both and holds the table to the model."""

    def __init__(self, dev, kdt, vdt, cap):
        from spconv_amd.pytorch.hash import HashTable
        self.dev, self.kdt, self.vdt, self.cap, self.key_bits = dev, kdt, vdt, cap, KEY_BITS[kdt]
        self.vw = torch.empty((), dtype=vdt).element_size()
        self.table = HashTable(dev, kdt, vdt, max_size=cap)
        self.table.values_data.view(torch.uint8).fill_(FILL)
        self.model = rh.Model()
        assert self.table.keys_data.shape == (cap,) and bool((self.table.keys_data == -1).all())

    def keys(self, k):
        return torch.from_numpy(np.asarray(k, dtype=np.int64)).to(self.kdt).to(self.dev)

    def vals(self, v):
        v = np.ascontiguousarray(np.asarray(v).astype(UINT[self.vw]))
        return torch.from_numpy(v.view(np.int32 if self.vw == 4 else np.int64)).to(self.dev).view(self.vdt)

    def storage(self):
        return signed(self.table.keys_data), bits(self.table.values_data)

    def check(self):
        kd, vd = self.storage()
        rh.check_storage(kd, vd, self.cap, self.model, self.key_bits)
        assert (vd[kd == rh.EMPTY] == PREFILL[self.vw]).all(), "the value of an empty slot was written"
        return kd, vd

    def insert(self, k, v=None):
        self.table.insert(self.keys(k), None if v is None else self.vals(v))
        self.model.insert(k, v)
        return self.check()

    def query(self, k, own_buffer=True):
        """with own_buffer the values land in a caller's prefilled tensor: the rows of absent keys must keep it"""
        k = np.asarray(k, dtype=np.int64)
        before = self.storage()
        out = filled((k.size,), self.vdt, self.dev) if own_buffer else None
        got, missing = self.table.query(self.keys(k), out)
        assert got.dtype == self.vdt and got.shape == (k.size,) and missing.dtype == torch.bool
        if own_buffer:
            assert got.data_ptr() == out.data_ptr(), "the caller's buffer was replaced"
        absent, defined = self.model.query(k)
        np.testing.assert_array_equal(missing.cpu().numpy(), absent, err_msg="is_empty differs from the model")
        got = bits(got)
        assert (got[absent] == PREFILL[self.vw]).all(), "the row of an absent key was written"
        for i in np.flatnonzero(~absent):
            assert rh.accepts(defined[i], int(got[i])), (int(k[i]), hex(int(got[i])), defined[i])
        after = self.storage()
        assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1]), "query changed the table"
        return got, absent

    def insert_exist(self, k, v):
        keys_before = signed(self.table.keys_data)
        flags = self.table.insert_exist_keys(self.keys(k), self.vals(v))
        assert flags.dtype == torch.uint8
        want = self.model.insert_exist(k, v)
        np.testing.assert_array_equal(flags.cpu().numpy(), want.astype(np.uint8), err_msg="flags are exactly 0 / 1")
        kd, vd = self.check()
        assert np.array_equal(kd, keys_before), "insert_exist changed the key storage"
        return want

    def items(self, max_size=-1):
        kd, vd = self.storage()
        _, slots = rh.slot_order(kd)
        k, v, count = self.table.items(max_size)
        m = self.cap if max_size == -1 else max_size
        assert k.dtype == self.kdt and v.dtype == self.vdt and k.shape == v.shape == (m,)
        assert count.dtype == self.kdt and count.shape == (1,) and int(count.item()) == slots.size == len(self.model)
        c = min(slots.size, m)
        assert (bits(v)[c:] == PREFILL[self.vw]).all() and (bits(k)[c:] == PREFILL[self.key_bits // 8]).all(), \
            "items wrote at or beyond min(count, max_out)"
        k, v = signed(k), bits(v)
        np.testing.assert_array_equal(k[:c], kd[slots][:c], err_msg="items: keys are not in slot order")
        np.testing.assert_array_equal(v[:c], vd[slots][:c], err_msg="items: values are not in slot order")
        after = self.storage()
        assert np.array_equal(kd, after[0]) and np.array_equal(vd, after[1]), "items changed the table"
        return k[:c], v[:c]

    def arange(self):
        kd, _ = self.storage()
        rank, slots = rh.slot_order(kd)
        count = self.table.assign_arange_()
        assert count.dtype == self.kdt and count.shape == (1,) and int(count.item()) == slots.size == len(self.model)
        first = self.storage()
        assert np.array_equal(first[0], kd), "assign_arange changed the key storage"
        np.testing.assert_array_equal(first[1][slots], rank[slots].astype(UINT[self.vw]),
                                      err_msg="values are not the slot-order ranks")
        assert (first[1][kd == rh.EMPTY] == PREFILL[self.vw]).all(), "the value of an empty slot was written"
        count2 = self.table.assign_arange_()                       # an unchanged table: bit for bit the same
        second = self.storage()
        assert int(count2.item()) == slots.size and np.array_equal(first[0], second[0]) and np.array_equal(first[1], second[1])
        self.model.settle(*first)
        self.check()

    def everything(self, keys, vals, absent, rng):
        """insert, query, insert_exist, items and (integer values) assign_arange over one scene"""
        n, half = keys.size, keys.size // 2
        self.insert(keys[:half], vals[:half])
        self.insert(keys[half:], vals[half:])
        self.insert(keys[:half // 2 + 1], vals[:half // 2 + 1])                 # again: nothing moves
        mixed = rng.permutation(np.concatenate([keys, absent]))
        self.query(mixed)
        self.query(mixed, own_buffer=False)
        some = rng.permutation(np.concatenate([keys[::2], absent]))
        absent_flags = self.insert_exist(some, rh.value_bits(rng, some.size, self.vw))
        assert int((~absent_flags).sum()) == keys[::2].size
        self.query(mixed)
        self.items()
        if not self.vdt.is_floating_point:
            self.arange()
            self.items()
            got, _ = self.query(keys)
            assert sorted(got.tolist()) == list(range(n))


def split_absent(rng, keys, n_absent, key_bits):
    """n_absent keys of the full range that are not in `keys`"""
    extra = rh.full_range_keys(rng, n_absent + 64, key_bits)
    return extra[~np.isin(extra, keys)][:n_absent]


# --------------------------------------------------------------------------------------------------- widths
def _width_scene(name, key_bits, rng):
    if name == "full":
        return rh.full_range_keys(rng, 1500, key_bits)
    if name == "families":
        return rh.low32_families(rng, 24)                                       # 24 x 64 keys equal in the low word
    keys = np.concatenate([rh.extremes(key_bits), rh.full_range_keys(rng, 60, key_bits)])
    return rng.permutation(np.unique(keys))


WIDTH_CASES = [(k, v, s) for k, v in INT_PAIRS + FLOAT_PAIRS for s in ("full", "families", "extremes")
               if not (s == "families" and k is I32)]


@pytest.mark.parametrize("kdt,vdt,scene", WIDTH_CASES, ids=[f"{str(k)[6:]}-{str(v)[6:]}-{s}" for k, v, s in WIDTH_CASES])
def test_widths(cuda, kdt, vdt, scene):
    rng = np.random.default_rng(11)
    key_bits = KEY_BITS[kdt]
    keys = _width_scene(scene, key_bits, rng)
    H = Harness(cuda, kdt, vdt, 2 * keys.size + 1)
    vals = rh.value_bits(rng, keys.size, H.vw, floating=vdt.is_floating_point)
    absent = split_absent(rng, keys, 300, key_bits)
    if scene == "families":                  # absent keys that agree with present ones in their low word
        absent = np.concatenate([absent, (keys[:200] & 0xffffffff) + (np.int64(64 + 7) << 32)])
    H.everything(keys, vals, absent, rng)
    if scene == "extremes":
        got, miss = H.query(rh.extremes(key_bits))
        assert not miss.any()


# --------------------------------------------------------------------------------------------------- capacities
CAPS = (1, 2, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 4097)


@pytest.mark.parametrize("kdt,vdt", [(I32, I64), (I64, I32)], ids=ids([(I32, I64), (I64, I32)]))
@pytest.mark.parametrize("load", [0.5, 1.0])
@pytest.mark.parametrize("cap", CAPS)
def test_capacities(cuda, cap, load, kdt, vdt):
    """block and wave edges of the count / walk passes, half full and completely full; from 64 slots on half the keys
    are homed in one sixteenth of the table (refhash.collision_keys: over a quarter displaced at load 0.5)"""
    rng = np.random.default_rng(cap)
    key_bits = KEY_BITS[kdt]
    n = max(int(cap * load), 1)
    keys = rh.collision_keys(rng, n, cap, key_bits) if cap >= 64 else rh.full_range_keys(rng, n, key_bits)
    H = Harness(cuda, kdt, vdt, cap)
    H.everything(keys, rh.value_bits(rng, n, H.vw), split_absent(rng, keys, 40, key_bits), rng)
    kd, _ = H.storage()
    assert int((kd != rh.EMPTY).sum()) == n
    if cap >= 64:
        _, dist = rh.displacement(kd, key_bits)
        assert (dist > 0).mean() >= 0.25                       # (whatever order the inserts arrived in)


@pytest.mark.parametrize("cap,n,kdt,vdt", [(524_289, 200_000, I64, I64), (16_779_265, 1_000_000, I32, I32)],
                         ids=["257-blocks-one-pass-scan", "8194-blocks-loop-scan"])
def test_large_capacities(cuda, cap, n, kdt, vdt):
    """more count blocks than one scan round (257: two items per thread of the one-pass form; 8194: the loop form of
    scan_kernel).  Storage and numbering are checked with torch ops on the device."""
    rng = np.random.default_rng(cap)
    key_bits, w = KEY_BITS[kdt], torch.empty((), dtype=vdt).element_size()
    every = rh.full_range_keys(rng, n + 1000, key_bits)
    H = Harness(cuda, kdt, vdt, cap)
    keys, absent = H.keys(every[:n]), H.keys(every[n:])
    vals = H.vals(rh.value_bits(rng, n, w))
    t = H.table
    prefill = filled((1,), vdt, cuda)[0]
    t.insert(keys[: n // 2], vals[: n // 2])
    t.insert(keys[n // 2:], vals[n // 2:])
    rh.check_storage_torch(t.keys_data, t.values_data, keys, vals, key_bits)
    occ = t.keys_data != -1
    assert bool((t.values_data[~occ] == prefill).all())
    got, missing = t.query(torch.cat([keys, absent]), filled((n + 1000,), vdt, cuda))
    assert not bool(missing[:n].any()) and bool(missing[n:].all())
    assert torch.equal(got[:n], vals) and bool((got[n:] == prefill).all())
    k, v, count = t.items()
    assert count.dtype == kdt and int(count.item()) == n
    assert torch.equal(k[:n], t.keys_data[occ]) and torch.equal(v[:n], t.values_data[occ])
    assert bool((v[n:] == prefill).all()) and bool((k[n:] == filled((1,), kdt, cuda)[0]).all())
    keys_before = t.keys_data.clone()
    rank = (torch.cumsum(occ.to(torch.int64), 0) - 1).to(vdt)
    for _ in range(2):                                         # the second call agrees bit for bit
        count = t.assign_arange_()
        assert int(count.item()) == n and torch.equal(t.keys_data, keys_before)
        assert torch.equal(t.values_data[occ], rank[occ]) and bool((t.values_data[~occ] == prefill).all())
    k2, v2, _ = t.items()
    assert torch.equal(k2[:n], k[:n]) and torch.equal(v2[:n], torch.arange(n, device=cuda, dtype=vdt))
    rh.check_storage_torch(t.keys_data, t.values_data, keys, t.query(keys)[0], key_bits)


# --------------------------------------------------------------------------------------------------- wrap-around
@pytest.mark.parametrize("kdt,vdt", [(I32, I32), (I64, F64)], ids=ids([(I32, I32), (I64, F64)]))
def test_wrap_around(cuda, kdt, vdt):
    """40 keys homed in the last four of 257 slots: the probe walks leave the end of the table and go on at slot 0"""
    rng = np.random.default_rng(3)
    cap, key_bits = 257, KEY_BITS[kdt]
    keys = rh.wrap_keys(rng, cap, 40, key_bits)
    H = Harness(cuda, kdt, vdt, cap)
    vals = rh.value_bits(rng, 40, H.vw, floating=vdt.is_floating_point)
    kd, _ = H.insert(keys, vals)
    slots, dist = rh.displacement(kd, key_bits)
    assert int((slots < (slots - dist) % cap).sum()) >= 1, "no key wrapped: the case would pass vacuously"
    H.query(np.concatenate([keys, split_absent(rng, keys, 40, key_bits), rh.wrap_keys(rng, cap, 60, key_bits)]))
    H.insert_exist(keys[::3], rh.value_bits(rng, keys[::3].size, H.vw))
    H.items()
    if not vdt.is_floating_point:
        H.arange()


# --------------------------------------------------------------------------------------------------- numbering
@pytest.mark.parametrize("kdt,vdt", [(I64, I32), (I32, I64)], ids=ids([(I64, I32), (I32, I64)]))
def test_numbering(cuda, kdt, vdt):
    """assign_arange_ / items number the occupied slots in ascending slot index; items stops at max_size, count does not"""
    rng = np.random.default_rng(5)
    cap, c, key_bits = 4097, 1500, KEY_BITS[kdt]
    keys = rh.collision_keys(rng, c, cap, key_bits)
    H = Harness(cuda, kdt, vdt, cap)
    H.insert(keys, rh.value_bits(rng, c, H.vw))
    full = H.items()
    for m in (0, 1, c - 1, c, c + 5):
        k, v = H.items(max_size=m)
        assert np.array_equal(k, full[0][:m]) and np.array_equal(v, full[1][:m])
    H.arange()
    k, v = H.items()
    assert np.array_equal(k, full[0]) and v.tolist() == list(range(c))     # items order = assign_arange order
    for m in (0, 1, c - 1, c, c + 5):
        H.items(max_size=m)
    with pytest.raises(ValueError, match="max_size"):
        H.table.items(max_size=-2)


# --------------------------------------------------------------------------------------------------- the empty marker
@pytest.mark.parametrize("kdt,vdt", INT_PAIRS + FLOAT_PAIRS, ids=ids(INT_PAIRS + FLOAT_PAIRS))
def test_the_empty_marker_is_never_a_member(cuda, kdt, vdt):
    """-1 (all ones) marks an empty slot.  On a cleared table the home slot of -1 HOLDS -1: a lookup that compared before
    it tested for the marker reported the key present and copied the slot's value; an insert 'claimed' the slot (the
    compare-and-swap returns the marker, which reads as success) and wrote a value into a slot that stays empty."""
    rng = np.random.default_rng(9)
    key_bits = KEY_BITS[kdt]
    H = Harness(cuda, kdt, vdt, 64)
    clean = H.storage()
    H.query([-1])                                              # absent, its output row untouched
    H.query([-1] * 300 + [5, -1])
    H.insert([-1], rh.value_bits(rng, 1, H.vw))               # both arrays untouched
    H.insert([-1] * 200, rh.value_bits(rng, 200, H.vw))
    H.insert([-1, -1])
    now = H.storage()
    assert np.array_equal(clean[0], now[0]) and np.array_equal(clean[1], now[1]) and len(H.model) == 0
    assert H.insert_exist([-1, -1, 3], rh.value_bits(rng, 3, H.vw)).all()
    H.items()
    # -1 mixed into 4096 real keys
    keys = rh.full_range_keys(rng, 4096, key_bits)
    vals = rh.value_bits(rng, 4096, H.vw, floating=vdt.is_floating_point)
    at = np.sort(rng.choice(4096, 64, replace=False))
    mixed_k, mixed_v = np.insert(keys, at, -1), np.insert(vals, at, rh.value_bits(rng, 64, H.vw))
    H = Harness(cuda, kdt, vdt, 8209)
    H.insert(mixed_k, mixed_v)
    assert len(H.model) == 4096
    H.items()
    _, absent = H.query(mixed_k)
    assert int(absent.sum()) == 64
    flags = H.insert_exist(mixed_k, rh.value_bits(rng, mixed_k.size, H.vw))
    assert int(flags.sum()) == 64 and (mixed_k[flags] == -1).all()
    if not vdt.is_floating_point:
        H.arange()


# --------------------------------------------------------------------------------------------------- absent keys, insert_exist
@pytest.mark.parametrize("kdt,vdt", INT_PAIRS + FLOAT_PAIRS, ids=ids(INT_PAIRS + FLOAT_PAIRS))
def test_absent_rows_keep_the_callers_bytes(cuda, kdt, vdt):
    rng = np.random.default_rng(13)
    key_bits = KEY_BITS[kdt]
    keys = rh.full_range_keys(rng, 700, key_bits)
    H = Harness(cuda, kdt, vdt, 1031)
    H.insert(keys, rh.value_bits(rng, 700, H.vw, floating=vdt.is_floating_point))
    absent = split_absent(rng, keys, 900, key_bits)
    mixed = rng.permutation(np.concatenate([keys, absent]))
    got, miss = H.query(mixed)                                 # (Harness.query: exactly the absent rows are untouched)
    assert int(miss.sum()) == 900 and int((got != PREFILL[H.vw]).sum()) >= 699
    H.query(absent)
    H.query(keys)


@pytest.mark.parametrize("kdt,vdt", INT_PAIRS + FLOAT_PAIRS, ids=ids(INT_PAIRS + FLOAT_PAIRS))
def test_insert_exist_changes_only_present_keys(cuda, kdt, vdt):
    rng = np.random.default_rng(17)
    key_bits = KEY_BITS[kdt]
    keys = rh.full_range_keys(rng, 600, key_bits)
    H = Harness(cuda, kdt, vdt, 1031)
    H.insert(keys[:500], rh.value_bits(rng, 500, H.vw))
    H.insert(keys[500:])                                       # 100 keys without a value
    absent = split_absent(rng, keys, 500, key_bits)
    H.insert_exist(absent, rh.value_bits(rng, 500, H.vw))      # nothing present: nothing changes (Harness.check)
    mixed = rng.permutation(np.concatenate([keys[250:], absent[:200]]))
    flags = H.insert_exist(mixed, rh.value_bits(rng, mixed.size, H.vw, floating=vdt.is_floating_point))
    assert int(flags.sum()) == 200
    H.query(np.concatenate([keys, absent]))
    twice = np.concatenate([keys[:50], keys[:50]])             # copies within one call: either value
    H.insert_exist(twice, rh.value_bits(rng, 100, H.vw))
    H.query(keys)


# --------------------------------------------------------------------------------------------------- duplicates
@pytest.mark.parametrize("kdt,vdt", INT_PAIRS, ids=ids(INT_PAIRS))
def test_duplicates_take_one_slot(cuda, kdt, vdt):
    rng = np.random.default_rng(19)
    key_bits = KEY_BITS[kdt]
    key = int(rh.full_range_keys(rng, 1, key_bits)[0])
    H = Harness(cuda, kdt, vdt, 257)                            # 4096 copies of one key with one value
    kd, _ = H.insert([key] * 4096, [0x1234567] * 4096)
    assert int((kd != rh.EMPTY).sum()) == 1
    H.query([key, key + 1])
    H = Harness(cuda, kdt, vdt, 257)                            # ... with 4096 values: one slot, one of the values
    given = rh.value_bits(rng, 4096, H.vw)
    kd, vd = H.insert([key] * 4096, given)
    assert int((kd != rh.EMPTY).sum()) == 1 and int(vd[kd != rh.EMPTY][0]) in set(given.tolist())
    H.model.settle(kd, vd)
    got, _ = H.query([key] * 100)
    assert len(set(got.tolist())) == 1
    H = Harness(cuda, kdt, vdt, 2049)                           # 512 keys x 8 copies
    keys = rh.full_range_keys(rng, 512, key_bits)
    order = rng.permutation(np.repeat(np.arange(512), 8))
    kd, vd = H.insert(keys[order], rh.value_bits(rng, 4096, H.vw))
    assert int((kd != rh.EMPTY).sum()) == 512
    H.model.settle(kd, vd)
    H.query(keys[order])
    H.items()
    H.arange()


# --------------------------------------------------------------------------------------------------- key-only insert
@pytest.mark.parametrize("kdt,vdt", INT_PAIRS + FLOAT_PAIRS, ids=ids(INT_PAIRS + FLOAT_PAIRS))
def test_a_key_only_insert_writes_no_value(cuda, kdt, vdt):
    rng = np.random.default_rng(23)
    key_bits = KEY_BITS[kdt]
    keys = rh.full_range_keys(rng, 1000, key_bits)
    H = Harness(cuda, kdt, vdt, 2049)
    _, vd = H.insert(keys)
    assert (vd == PREFILL[H.vw]).all(), "insert without values wrote the value storage"
    vals = rh.value_bits(rng, 500, H.vw, floating=vdt.is_floating_point)
    H.insert(keys[:500], vals)
    _, before = H.storage()
    _, vd = H.insert(keys)                                      # present keys again, without values: theirs stay
    assert np.array_equal(vd, before)
    got, miss = H.query(keys)
    assert not miss.any() and np.array_equal(got[:500], vals) and (got[500:] == PREFILL[H.vw]).all()


# --------------------------------------------------------------------------------------------------- overflow
@pytest.mark.parametrize("kdt,vdt", [(I32, I64), (I64, I32)], ids=ids([(I32, I64), (I64, I32)]))
@pytest.mark.parametrize("cap", [64, 257])
def test_a_full_table_drops_keys(cuda, cap, kdt, vdt):
    """cap + 7 distinct keys: exactly cap are kept, all of them from the input, each with its own value; the seven others
    are absent.  (Small capacities: a probe that fails walks the whole table.)"""
    rng = np.random.default_rng(cap)
    key_bits, n = KEY_BITS[kdt], cap + 7
    keys = rh.full_range_keys(rng, n, key_bits)
    H = Harness(cuda, kdt, vdt, cap)
    vals = rh.value_bits(rng, n, H.vw)
    H.table.insert(H.keys(keys), H.vals(vals))
    kd, vd = H.storage()
    assert (kd != rh.EMPTY).all() and len(set(kd.tolist())) == cap and set(kd.tolist()) <= set(keys.tolist())
    kept = np.isin(keys, kd)
    assert int(kept.sum()) == cap
    H.model.insert(keys[kept], vals[kept])                      # the model of what the table kept
    H.check()
    _, absent = H.query(keys)
    assert np.array_equal(absent, ~kept)
    H.table.insert(H.keys(keys[~kept]), H.vals(vals[~kept]))   # the seven again: still no room
    H.check()                                                   # still full, still the same keys and values
    flags = H.insert_exist(keys, rh.value_bits(rng, n, H.vw))
    assert np.array_equal(flags, ~kept)
    H.items()
    if not vdt.is_floating_point:
        H.arange()


# --------------------------------------------------------------------------------------------------- empty call
@pytest.mark.parametrize("kdt,vdt", INT_PAIRS + FLOAT_PAIRS, ids=ids(INT_PAIRS + FLOAT_PAIRS))
def test_empty_calls(cuda, kdt, vdt):
    rng = np.random.default_rng(29)
    key_bits = KEY_BITS[kdt]
    none = np.empty(0, dtype=np.int64)
    for n in (0, 100):                                          # a cleared table, then one with content
        H = Harness(cuda, kdt, vdt, 257)
        if n:
            H.insert(rh.full_range_keys(rng, n, key_bits), rh.value_bits(rng, n, H.vw))
        before = H.storage()
        H.insert(none)
        H.insert(none, none)
        got, absent = H.query(none)
        assert got.shape == (0,) and absent.shape == (0,)
        H.query(none, own_buffer=False)
        assert H.insert_exist(none, none).shape == (0,)
        H.items(max_size=0)
        H.items()
        after = H.storage()
        assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
        if not vdt.is_floating_point:
            H.arange()                                          # n = 0: count 0, no value written
            assert n or np.array_equal(H.storage()[1], before[1])


# --------------------------------------------------------------------------------------------------- dirty workspace
@pytest.mark.parametrize("cap,n", [(257, 200), (4097, 3000), (524_289, 100_000)])
def test_a_dirty_workspace_changes_nothing(cuda, cap, n):
    """spx_hash_assign_arange / spx_hash_items through ctypes with the workspace at 0x00 and at 0xFF: the same bits"""
    from spconv_amd import _lib
    L = _lib.load()
    rng = np.random.default_rng(cap)
    H = Harness(cuda, I64, I32, cap)
    H.table.insert(H.keys(rh.full_range_keys(rng, n, 64)), H.vals(rh.value_bits(rng, n, 4)))
    t = H.table
    stream = torch.cuda.current_stream(cuda).cuda_stream
    ws_bytes = int(L.spx_hash_ws_bytes(cap))
    runs = []
    for byte in (0x00, 0xFF):
        ws = torch.full((ws_bytes,), byte, dtype=torch.uint8, device=cuda)
        tv = t.values_data.clone()
        ko, vo, c1, c2 = filled((cap,), I64, cuda), filled((cap,), I32, cuda), filled((1,), I64, cuda), filled((1,), I64, cuda)
        _lib.check(L.spx_hash_items(t.keys_data.data_ptr(), tv.data_ptr(), cap, 8, 4, ko.data_ptr(), vo.data_ptr(), cap,
                                    c1.data_ptr(), ws.data_ptr(), ws_bytes, stream))
        ws.fill_(byte)
        _lib.check(L.spx_hash_assign_arange(t.keys_data.data_ptr(), tv.data_ptr(), cap, 8, 4, c2.data_ptr(), ws.data_ptr(),
                                            ws_bytes, stream))
        runs.append([x.cpu() for x in (ko, vo, c1, c2, tv)])
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    ko, vo, c1, c2, tv = runs[0]
    assert int(c1.item()) == n == int(c2.item())
    kd = signed(t.keys_data)
    rank, slots = rh.slot_order(kd)
    assert np.array_equal(ko.numpy()[:n], kd[slots]) and np.array_equal(vo.numpy()[:n], t.values_data.cpu().numpy()[slots])
    assert np.array_equal(tv.numpy()[slots], rank[slots]) and (bits(tv)[kd == rh.EMPTY] == PREFILL[4]).all()
    assert (bits(vo)[n:] == PREFILL[4]).all() and (bits(ko)[n:] == PREFILL[8]).all()


# --------------------------------------------------------------------------------------------------- narrow buffer
def test_a_narrow_buffer_is_refused(cuda):
    """query(values=...) with a 4-byte tensor on an 8-byte table raises and launches nothing.  The tensor is a view into
    an allocation four times as large as the 8-byte result needs: no version of the code can write outside it."""
    rng = np.random.default_rng(31)
    n = 256
    for vdt, narrow_dt in ((I64, I32), (F64, F32)):
        H = Harness(cuda, I64, vdt, 1031)
        keys = rh.full_range_keys(rng, n, 64)
        H.insert(keys, rh.value_bits(rng, n, 8))
        before = H.storage()
        room = filled((8 * n,), narrow_dt, cuda)                # 32 n bytes; the result would take 8 n
        wide = room.view(vdt)                                   # the same bytes as 8-byte items [4 n]
        for bad, word in ((room[:n], "values must have dtype"), (wide[:n - 1], "values must have length"),
                          (wide[:n + 1], "values must have length"), (wide[:2 * n:2], "values must be contiguous"),
                          (wide[:n].reshape(n // 2, 2), "values must be 1-d")):
            with pytest.raises(ValueError, match=word):
                H.table.query(H.keys(keys), bad)
        with pytest.raises(ValueError, match="values must have dtype"):
            H.table.insert(H.keys(keys), room[:n])
        with pytest.raises(ValueError, match="values must have dtype"):
            H.table.insert_exist_keys(H.keys(keys), room[:n])
        with pytest.raises(ValueError, match="keys must have dtype"):
            H.table.query(H.keys(keys).to(I32))
        torch.cuda.synchronize()
        assert (bits(room) == PREFILL[4]).all(), "a refused call wrote the buffer"
        after = H.storage()
        assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
        got, missing = H.table.query(H.keys(keys), wide[:n])    # the right view of the same room is filled in place
        assert not bool(missing.any()) and (bits(wide)[n:] == PREFILL[8]).all()
        H.query(keys)


# --------------------------------------------------------------------------------------------------- streams
def test_on_a_side_stream(cuda):
    rng = np.random.default_rng(37)
    side = torch.cuda.Stream(cuda)
    side.wait_stream(torch.cuda.current_stream(cuda))
    with torch.cuda.stream(side):
        keys = rh.collision_keys(rng, 600, 1031, 64)
        H = Harness(cuda, I64, I32, 1031)
        H.everything(keys, rh.value_bits(rng, 600, 4), split_absent(rng, keys, 100, 64), rng)
    side.synchronize()
    torch.cuda.current_stream(cuda).wait_stream(side)
    H.check()


def test_query_in_a_captured_graph(cuda):
    """one single-branch capture of query over a static key buffer, replayed after the keys are changed"""
    rng = np.random.default_rng(41)
    n = 512
    keys = rh.full_range_keys(rng, 2 * n, 64)
    H = Harness(cuda, I64, F64, 2049)
    H.insert(keys, rh.value_bits(rng, 2 * n, 8, floating=True))
    absent = split_absent(rng, keys, n, 64)
    rounds = [rng.permutation(np.concatenate([keys[:n // 2], absent[:n // 2]])),
              rng.permutation(np.concatenate([keys[n:n + 300], absent[n // 2:n // 2 + 211], [-1]])),
              keys[:n], absent]
    static_keys, static_vals = H.keys(rounds[0]), filled((n,), F64, cuda)
    H.table.query(static_keys, static_vals)                     # (first use outside the capture)
    static_vals.view(torch.uint8).fill_(FILL)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got, missing = H.table.query(static_keys, static_vals)
    assert got.data_ptr() == static_vals.data_ptr()
    for k in rounds:
        static_keys.copy_(H.keys(k))
        static_vals.view(torch.uint8).fill_(FILL)
        graph.replay()
        torch.cuda.synchronize()
        absent_want, defined = H.model.query(k)
        np.testing.assert_array_equal(missing.cpu().numpy(), absent_want)
        want = np.array([PREFILL[8] if d is None else d for d in defined], dtype=np.uint64)
        np.testing.assert_array_equal(bits(static_vals), want)
    H.check()
