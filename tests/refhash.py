"""The model the user hash table (csrc/hash.hip, spconv_amd/pytorch/hash.py) is held to: a Python dict with the rules of
the hash section of include/spconv_amd.h, a restatement of the home slot of a key, the invariants that any arrival order
of a linear-probing table leaves in its RAW storage, the slot-order numbering, and the key generators of the scenes.
Shares no code with the library.  tests/test_refhash.py holds it to its own conditions on the CPU.

Keys are signed integers of 32 or 64 bits, -1 (all ones) is the empty marker.  Values travel as BIT PATTERNS: unsigned
numpy integers of the value width (a float table's values are viewed, never converted).

Home slot.  The kernel hashes a 64-bit word with murmur3's fmix64, takes the low 32 bits of the result and reduces them
modulo the capacity.  The word of a 64-bit key is the key; the word of a 32-bit key is its bit pattern ZERO-extended
(the kernel holds 32-bit keys as unsigned words), so the int32 key -2 and the int64 key -2 have different homes.
A wrong restatement cannot hide: invariant (b) of check_storage fails on the device at once."""
import numpy as np

EMPTY = -1
BITS_NP = {4: np.uint32, 8: np.uint64}
INT_MIN = {32: -(1 << 31), 64: -(1 << 63)}
INT_MAX = {32: (1 << 31) - 1, 64: (1 << 63) - 1}


# ------------------------------------------------------------------------------------------------ home slot
def fmix64(x):
    """murmur3's 64-bit finaliser over a uint64 array (arithmetic modulo 2^64)"""
    x = np.array(x, dtype=np.uint64)                     # (a copy: the caller's array stays as it is)
    with np.errstate(over="ignore"):
        x ^= x >> np.uint64(33)
        x *= np.uint64(0xff51afd7ed558ccd)
        x ^= x >> np.uint64(33)
        x *= np.uint64(0xc4ceb9fe1a85ec53)
        x ^= x >> np.uint64(33)
    return x


def key_word(keys, key_bits):
    """the 64-bit word the table hashes for a key of key_bits"""
    k = np.asarray(keys, dtype=np.int64)
    if key_bits == 32:
        assert ((k >= INT_MIN[32]) & (k <= INT_MAX[32])).all()
        return k.astype(np.int32).view(np.uint32).astype(np.uint64)
    assert key_bits == 64
    return k.view(np.uint64)


def home(keys, cap, key_bits):
    """home slot of every key in a table of `cap` slots (int64 array)"""
    return ((fmix64(key_word(keys, key_bits)) & np.uint64(0xffffffff)) % np.uint64(cap)).astype(np.int64)


def home_torch(keys, cap, key_bits):
    """home() in torch ops, on the device of `keys` (an int32 / int64 tensor): the form the large-capacity cases use.
    int64 arithmetic wraps modulo 2^64 as the unsigned does; a logical shift is an arithmetic one with its sign copies
    masked off."""
    import torch

    def lsr33(x):
        return (x >> 33) & ((1 << 31) - 1)
    x = keys.to(torch.int64)
    if key_bits == 32:
        x = x & 0xffffffff
    x = x ^ lsr33(x)
    x = x * torch.tensor(0xff51afd7ed558ccd - (1 << 64), dtype=torch.int64, device=keys.device)
    x = x ^ lsr33(x)
    x = x * torch.tensor(0xc4ceb9fe1a85ec53 - (1 << 64), dtype=torch.int64, device=keys.device)
    x = x ^ lsr33(x)
    return (x & 0xffffffff) % cap


# ------------------------------------------------------------------------------------------------ the model
class Model:
    """The table as a dict: key -> what the header defines of its value.
         int         the value's bit pattern
         frozenset   copies of the key came with these values in ONE call: the stored value is one of them
         None        the key was inserted without a value: the header defines none
       The dict knows no capacity: the overflow case builds its model from what the table kept."""

    def __init__(self):
        self.d = {}

    def __len__(self):
        return len(self.d)

    @staticmethod
    def _given(keys, values):
        given = {}
        for k, v in zip((int(k) for k in keys), (int(v) for v in values)):
            if k != EMPTY:
                given.setdefault(k, set()).add(v)
        return {k: (next(iter(s)) if len(s) == 1 else frozenset(s)) for k, s in given.items()}

    def insert(self, keys, values=None):
        if values is None:
            for k in (int(k) for k in keys):
                if k != EMPTY:
                    self.d.setdefault(k, None)
        else:
            self.d.update(self._given(keys, values))

    def query(self, keys):
        """-> (absent [n] bool, values: list of what the model defines, None for an absent key)"""
        keys = [int(k) for k in keys]
        absent = np.array([k == EMPTY or k not in self.d for k in keys], dtype=bool)
        return absent, [None if a else self.d[k] for k, a in zip(keys, absent)]

    def insert_exist(self, keys, values):
        absent, _ = self.query(keys)
        self.d.update({k: v for k, v in self._given(keys, values).items() if k in self.d})
        return absent

    def settle(self, keys_data, values_data):
        """pins every value the model leaves open (frozenset, None) to the one the storage holds, after check_storage
        has accepted it: from here on the value is defined"""
        for s in np.flatnonzero(np.asarray(keys_data) != EMPTY):
            self.d[int(keys_data[s])] = int(values_data[s])


def accepts(defined, stored):
    """does the model's definition of a value admit the stored bit pattern?"""
    return defined is None or (stored in defined if isinstance(defined, frozenset) else stored == defined)


# ------------------------------------------------------------------------------------------------ raw storage
def displacement(keys_data, key_bits):
    """(occupied slots, cyclic distance of each from the home slot of its key)"""
    keys_data = np.asarray(keys_data).astype(np.int64)
    cap = keys_data.shape[0]
    slots = np.flatnonzero(keys_data != EMPTY)
    return slots, (slots - home(keys_data[slots], cap, key_bits)) % cap


def check_storage(keys_data, values_data, cap, model, key_bits):
    """The raw arrays of a table that holds exactly the model's keys:
       (a) the non-empty slots hold the model's keys, each once;
       (b) for a key at slot s with home h every slot of the cyclic range [h, s) is occupied (true for ANY arrival order
           of a linear-probing table whose slots never empty);
       (c) values_data[s] is, bit for bit, what the model defines for the key at s.
    values_data: the bit patterns (unsigned integers of the value width), or None to leave (c) out."""
    keys_data = np.asarray(keys_data).astype(np.int64)
    assert keys_data.shape == (cap,)
    slots, dist = displacement(keys_data, key_bits)
    stored = keys_data[slots].tolist()
    assert len(stored) <= cap
    assert len(set(stored)) == len(stored), "(a) a key is stored twice"
    assert set(stored) == set(model.d), (f"(a) stored keys differ from the model's: {len(set(stored) - set(model.d))} "
                                         f"foreign, {len(set(model.d) - set(stored))} missing")
    # (b): empties in the cyclic range [h, s) through the prefix count of empty slots
    P = np.concatenate([[0], np.cumsum(keys_data == EMPTY)])
    h = (slots - dist) % cap
    empties = np.where(h <= slots, P[slots] - P[h], P[cap] - P[h] + P[slots])
    bad = np.flatnonzero(empties != 0)
    assert bad.size == 0, (f"(b) {bad.size} keys lie behind an empty slot of their probe path, first: key "
                           f"{stored[bad[0]]} at slot {slots[bad[0]]}, home {h[bad[0]]}")
    if values_data is not None:
        values_data = np.asarray(values_data)
        assert values_data.shape == (cap,) and values_data.dtype.kind == "u"
        for s, k in zip(slots.tolist(), stored):
            assert accepts(model.d[k], int(values_data[s])), \
                f"(c) key {k} at slot {s} holds {int(values_data[s]):#x}, the model {model.d[k]!r}"


def check_storage_torch(keys_data, values_data, keys, values, key_bits):
    """check_storage in torch ops on the device of the table, for capacities at which a host loop takes too long.
    keys: the DISTINCT keys the table must hold (no -1), values: their values or None; values_data / values are
    integer tensors (bit patterns)."""
    import torch
    cap = keys_data.shape[0]
    empty = keys_data == EMPTY
    slots = torch.nonzero(~empty).flatten()
    stored = keys_data[slots]
    s_sorted, s_order = torch.sort(stored)
    k_sorted, k_order = torch.sort(keys)
    assert s_sorted.shape == k_sorted.shape and torch.equal(s_sorted, k_sorted), "(a) stored keys differ from the given"
    assert s_sorted.numel() < 2 or bool((s_sorted[1:] != s_sorted[:-1]).all()), "(a) a key is stored twice"
    P = torch.cat([torch.zeros(1, dtype=torch.int64, device=keys_data.device), torch.cumsum(empty.to(torch.int64), 0)])
    h = home_torch(stored, cap, key_bits)
    empties = torch.where(h <= slots, P[slots] - P[h], P[cap] - P[h] + P[slots])
    assert int((empties != 0).sum()) == 0, "(b) a key lies behind an empty slot of its probe path"
    if values is not None:
        assert torch.equal(values_data[slots][s_order], values[k_order]), "(c) a stored value differs from the given"


def slot_order(keys_data):
    """-> (rank [cap]: the exclusive rank of every occupied slot among the occupied slots, -1 at empty ones;
           slots: the occupied slots in ascending index -- keys_data[slots], values_data[slots] is the items sequence)"""
    keys_data = np.asarray(keys_data)
    occ = keys_data != EMPTY
    rank = np.where(occ, np.cumsum(occ) - 1, -1).astype(np.int64)
    return rank, np.flatnonzero(occ)


def simulate(keys, values, cap, key_bits, keys_data=None, values_data=None, prefill=0):
    """Sequential linear probing, one key after the other: -> (keys_data int64 [cap], values_data uint64 [cap]).
    The last value given for a key stays; a key that finds no free slot is dropped; -1 is ignored."""
    keys_data = np.full(cap, EMPTY, dtype=np.int64) if keys_data is None else keys_data
    values_data = np.full(cap, prefill, dtype=np.uint64) if values_data is None else values_data
    homes = home(keys, cap, key_bits).tolist()
    for i, (k, s) in enumerate(zip((int(k) for k in keys), homes)):
        if k == EMPTY:
            continue
        for _ in range(cap):
            if keys_data[s] == EMPTY or keys_data[s] == k:
                keys_data[s] = k
                if values is not None:
                    values_data[s] = values[i]
                break
            s = s + 1 if s + 1 < cap else 0
    return keys_data, values_data


# ------------------------------------------------------------------------------------------------ key generators
def full_range_keys(rng, n, key_bits):
    """n distinct keys drawn from the whole range of the width, the empty marker excluded"""
    out = np.empty(0, dtype=np.int64)
    while out.size < n:
        k = rng.integers(INT_MIN[key_bits], INT_MAX[key_bits], 2 * n + 16, dtype=np.int64, endpoint=True)
        out = np.unique(np.concatenate([out, k[k != EMPTY]]))
    return rng.permutation(out)[:n]


def low32_families(rng, n_base, members=64):
    """64-bit keys in families that agree in their low 32 bits: k + (j << 32), j = 0 .. members - 1.  A table that
    hashed or compared the low word alone would fold each family into one entry."""
    base = full_range_keys(rng, n_base, 32) & 0xffffffff          # the low word, upper half clear
    base = base[base != 0xffffffff]
    keys = (base[:, None] + (np.arange(members, dtype=np.int64)[None, :] << 32)).reshape(-1)
    return rng.permutation(keys[keys != EMPTY])


def extremes(key_bits):
    return np.array([INT_MIN[key_bits], -2, 0, INT_MAX[key_bits]], dtype=np.int64)


def keys_homed_in(rng, n, cap, key_bits, lo, hi):
    """n distinct keys of the full range whose home slot lies in [lo, hi), found by brute force through home()"""
    assert 0 <= lo < hi <= cap
    out = np.empty(0, dtype=np.int64)
    while out.size < n:
        k = full_range_keys(rng, 1 << 14, key_bits)
        h = home(k, cap, key_bits)
        out = np.unique(np.concatenate([out, k[(h >= lo) & (h < hi)]]))
    return rng.permutation(out)[:n]


def wrap_keys(rng, cap=257, n=40, key_bits=64, last=4):
    """the wrap-around scene: keys whose home is one of the last few slots, more of them than those slots hold"""
    return keys_homed_in(rng, n, cap, key_bits, cap - last, cap)


def collision_keys(rng, n, cap, key_bits):
    """the collision scene: half the keys at home anywhere, half homed in one sixteenth of the table, so that long runs
    form at any load"""
    a = full_range_keys(rng, n - n // 2, key_bits)
    b = keys_homed_in(rng, n // 2 + 8, cap, key_bits, cap // 4, cap // 4 + max(cap // 16, 1))
    b = b[~np.isin(b, a)][:n // 2]
    return rng.permutation(np.concatenate([a, b]))


def value_bits(rng, n, val_bytes, floating=False):
    """n random full-width bit patterns; for a float table the first few are NaN payloads, -0.0, infinities"""
    v = rng.integers(0, 1 << (8 * val_bytes), n, dtype=np.uint64, endpoint=False) if val_bytes == 4 else \
        rng.integers(0, 1 << 63, n, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, n, dtype=np.uint64)
    v = v.astype(BITS_NP[val_bytes])
    if floating:
        special = {4: [0x7fc00001, 0xffc12345, 0x7f800001, 0x80000000, 0x7f800000, 0xff800000, 0x00000001],
                   8: [0x7ff8000000000001, 0xfff8123456789abc, 0x7ff0000000000001, 0x8000000000000000,
                       0x7ff0000000000000, 0xfff0000000000000, 0x0000000000000001]}[val_bytes]
        m = min(n, len(special))
        v[:m] = np.array(special[:m], dtype=BITS_NP[val_bytes])
    return v
