"""CPU: tests/refhash.py held to its own conditions.  The invariants accept what a sequential linear-probing table leaves
and refuse what a broken one would; the scenes of tests/test_gpu_hash_matrix.py are sharp (keys wrap round the end of
the table, a quarter of the collision scene is displaced, the low-32-equal families are large); and the record of why
the "numbering is a function of the key set" claim was withdrawn: forward and reversed insertion of the same keys fill
the slots differently."""
import numpy as np
import pytest
import torch

import refhash as rh

WIDTHS = (32, 64)


def scene(key_bits, cap, n, seed=0, val_bytes=8):
    rng = np.random.default_rng(seed)
    keys = rh.full_range_keys(rng, n, key_bits)
    vals = rh.value_bits(rng, n, val_bytes)
    return keys, vals


def test_fmix64_known_values():
    """murmur3's finaliser: 0 is a fixed point, and the published avalanche of 1"""
    assert int(rh.fmix64(np.array([0], dtype=np.uint64))[0]) == 0
    x = 1
    for mul in (0xff51afd7ed558ccd, 0xc4ceb9fe1a85ec53):      # the same steps in Python integers
        x ^= x >> 33
        x = x * mul & (1 << 64) - 1
    x ^= x >> 33
    assert int(rh.fmix64(np.array([1], dtype=np.uint64))[0]) == x
    keys = np.array([-2, -(1 << 31), 5, (1 << 31) - 1], dtype=np.int64)
    assert rh.key_word(keys, 32).tolist() == [0xfffffffe, 0x80000000, 5, 0x7fffffff]        # zero-extended
    assert rh.key_word(keys, 64).tolist() == [(1 << 64) - 2, (1 << 64) - (1 << 31), 5, 0x7fffffff]


@pytest.mark.parametrize("key_bits", WIDTHS)
def test_home_torch_is_home(key_bits):
    rng = np.random.default_rng(1)
    keys = np.concatenate([rh.full_range_keys(rng, 5000, key_bits), rh.extremes(key_bits)])
    dt = torch.int32 if key_bits == 32 else torch.int64
    for cap in (1, 257, 4097, 16_779_265):
        got = rh.home_torch(torch.from_numpy(keys).to(dt), cap, key_bits).numpy()
        assert np.array_equal(got, rh.home(keys, cap, key_bits)), cap


@pytest.mark.parametrize("key_bits", WIDTHS)
@pytest.mark.parametrize("cap,n", [(1, 1), (2, 2), (65, 32), (257, 257), (2049, 1024), (4097, 4097)])
def test_the_simulator_satisfies_check_storage(key_bits, cap, n):
    keys, vals = scene(key_bits, cap, n, seed=cap)
    model = rh.Model()
    model.insert(keys, vals)
    kd, vd = rh.simulate(keys, vals, cap, key_bits)
    rh.check_storage(kd, vd, cap, model, key_bits)
    assert int((kd != rh.EMPTY).sum()) == n == len(model)
    # the torch form agrees (CPU tensors here, the device's in the large-capacity cases)
    dt = torch.int32 if key_bits == 32 else torch.int64
    rh.check_storage_torch(torch.from_numpy(kd).to(dt), torch.from_numpy(vd.view(np.int64)),
                           torch.from_numpy(keys).to(dt), torch.from_numpy(vals.view(np.int64)), key_bits)


def test_check_storage_refuses_broken_tables():
    key_bits, cap, n = 64, 257, 128
    keys, vals = scene(key_bits, cap, n, seed=7)
    model = rh.Model()
    model.insert(keys, vals)
    kd, vd = rh.simulate(keys, vals, cap, key_bits)
    tk, tv = torch.from_numpy(keys), torch.from_numpy(vals.view(np.int64))

    def refused(kd2, vd2, word):
        with pytest.raises(AssertionError, match=word):
            rh.check_storage(kd2, vd2, cap, model, key_bits)
        with pytest.raises(AssertionError, match=word):
            rh.check_storage_torch(torch.from_numpy(kd2), torch.from_numpy(vd2.view(np.int64)), tk, tv, key_bits)
    slots, dist = rh.displacement(kd, key_bits)
    free = np.flatnonzero(kd == rh.EMPTY)
    # a key stored twice
    kd2, vd2 = kd.copy(), vd.copy()
    kd2[free[0]], vd2[free[0]] = kd[slots[0]], vd[slots[0]]
    refused(kd2, vd2, r"\(a\)")
    # a key lost
    kd2 = kd.copy()
    kd2[slots[0]] = rh.EMPTY
    with pytest.raises(AssertionError, match=r"\(a\)"):
        rh.check_storage(kd2, vd, cap, model, key_bits)
    # a key behind a hole of its probe path: moved from its slot to a free slot that is not reachable without a gap
    s = slots[np.argmin(dist)]
    far = [f for f in free if kd[(f - 1) % cap] == rh.EMPTY and (f - rh.home([kd[s]], cap, key_bits)[0]) % cap > 1][0]
    kd2, vd2 = kd.copy(), vd.copy()
    kd2[far], vd2[far], kd2[s] = kd[s], vd[s], rh.EMPTY
    refused(kd2, vd2, r"\(b\)")
    # a table that hashed the low word alone (home of the key truncated to 32 bits): (b) sees it
    wrong, _ = rh.simulate(keys & 0xffffffff, vals, cap, key_bits)
    wrong[wrong != rh.EMPTY] = [keys[(keys & 0xffffffff) == k][0] for k in wrong[wrong != rh.EMPTY]]
    with pytest.raises(AssertionError, match=r"\(b\)"):
        rh.check_storage(wrong, None, cap, model, key_bits)
    # one value bit flipped
    vd2 = vd.copy()
    vd2[slots[3]] ^= np.uint64(1 << 40)
    refused(kd, vd2, r"\(c\)")


def test_the_model():
    m = rh.Model()
    m.insert([5, -1, 7, 5], [1, 2, 3, 4])
    assert m.d == {5: frozenset({1, 4}), 7: 3}                     # -1 never enters; copies leave either value
    absent, vals = m.query([7, -1, 6, 5])
    assert absent.tolist() == [False, True, True, False] and vals == [3, None, None, frozenset({1, 4})]
    assert rh.accepts(vals[3], 4) and not rh.accepts(vals[3], 2) and rh.accepts(None, 99) and not rh.accepts(3, 4)
    assert m.insert_exist([6, 7, -1], [10, 11, 12]).tolist() == [True, False, True]
    assert m.d == {5: frozenset({1, 4}), 7: 11}
    m.insert([9])
    m.insert([7])
    assert m.d[9] is None and m.d[7] == 11                         # a key-only insert defines and changes no value
    kd, vd = rh.simulate([5, 7, 9], [4, 11, 77], 8, 64)
    rh.check_storage(kd, vd, 8, m, 64)
    m.settle(kd, vd)
    assert m.d == {5: 4, 7: 11, 9: 77}
    rank, slots = rh.slot_order(np.array([-1, 4, -1, -1, 9, 2]))
    assert rank.tolist() == [-1, 0, -1, -1, 1, 2] and slots.tolist() == [1, 4, 5]


@pytest.mark.parametrize("key_bits", WIDTHS)
def test_the_wrap_scene_wraps(key_bits):
    """cap 257, 40 keys homed in the last four slots: at least one is stored BELOW its home slot"""
    cap = 257
    keys = rh.wrap_keys(np.random.default_rng(3), cap, 40, key_bits)
    assert len(set(keys.tolist())) == 40 and (rh.home(keys, cap, key_bits) >= cap - 4).all()
    kd, _ = rh.simulate(keys, None, cap, key_bits)
    slots, dist = rh.displacement(kd, key_bits)
    wrapped = int((slots < (slots - dist) % cap).sum())
    assert wrapped >= 36, wrapped                                  # four slots before the end: the rest wraps
    model = rh.Model()
    model.insert(keys)
    rh.check_storage(kd, None, cap, model, key_bits)


@pytest.mark.parametrize("key_bits", WIDTHS)
@pytest.mark.parametrize("cap", [257, 4097])
def test_the_collision_scene_displaces_a_quarter(key_bits, cap):
    n = cap // 2
    keys = rh.collision_keys(np.random.default_rng(cap), n, cap, key_bits)
    assert len(set(keys.tolist())) == n
    kd, _ = rh.simulate(keys, None, cap, key_bits)
    _, dist = rh.displacement(kd, key_bits)
    share = float((dist > 0).mean())
    print(f"cap {cap}, {key_bits}-bit keys: {share:.3f} of the keys displaced, longest walk {int(dist.max())}")
    assert share >= 0.25


def test_the_families_agree_in_their_low_word():
    keys = rh.low32_families(np.random.default_rng(0), 8)
    assert keys.size == 8 * 64 and len(set(keys.tolist())) == keys.size
    assert len(set((keys & 0xffffffff).tolist())) == 8 and set((keys >> 32).tolist()) == set(range(64))
    assert rh.extremes(32).tolist() == [-(1 << 31), -2, 0, (1 << 31) - 1]
    assert rh.extremes(64).tolist() == [-(1 << 63), -2, 0, (1 << 63) - 1]
    for bits in WIDTHS:
        k = rh.full_range_keys(np.random.default_rng(0), 4096, bits)
        assert len(set(k.tolist())) == 4096 and rh.EMPTY not in k and (k < 0).any() and (abs(k) > 1 << (bits - 3)).any()
    v = rh.value_bits(np.random.default_rng(0), 64, 8, floating=True)
    assert np.isnan(v[:3].view(np.float64)).all() and v[3] == 1 << 63 and (v >> np.uint64(32)).any()


@pytest.mark.parametrize("cap,least", [(10_000, 0.35), (5000, 0.70)])
def test_slot_contents_depend_on_insertion_order(cap, least):
    """Why the header no longer calls the numbering a function of the key set: the 5000 keys of
    test_gpu_hash.py::test_hash_table_contract, inserted one after the other forwards and reversed, end up in different
    slots (2153 of 5000 at capacity 10 000, 4030 of 5000 at capacity 5000), and so does their slot-order numbering.
    Both tables satisfy the same invariants."""
    keys = np.random.default_rng(0).choice(10_000_000, 5000, replace=False).astype(np.int64)
    model = rh.Model()
    model.insert(keys)
    slot_of = []
    for order in (keys, keys[::-1]):
        kd, _ = rh.simulate(order, None, cap, 64)
        rh.check_storage(kd, None, cap, model, 64)
        slots = np.flatnonzero(kd != rh.EMPTY)
        slot_of.append(dict(zip(kd[slots].tolist(), slots.tolist())))
    moved = sum(slot_of[0][k] != slot_of[1][k] for k in keys.tolist())
    print(f"cap {cap}: {moved} of 5000 keys in another slot")
    assert moved >= least * 5000
