"""Misaligned add on the union kernels (csrc/union.hip, spconv_amd/pytorch/_union.py) against numpy.

The expectation is computed here: the union is np.unique of the linear keys, the features are the sequential sum in
operand order over the operands present, in float32 (float64 for f64 inputs), cast once to the row dtype (through
torch's CPU cast).  Only IEEE additions are involved, so every comparison is bit for bit; no tolerance appears."""
import numpy as np
import pytest
import torch

from util import scene

pytestmark = pytest.mark.gpu

GRID_A = (2, [3, 160, 160])            # 153 600 keys: crosses two 65 536-key rank-map blocks
FORCED = [0, 31, 32, 63, 65535, 65536, 131071, 131072, 153599]
SMALL = (2, [12, 14, 16])
KEYS = ("union/mark", "union/prefix", "union/claim", "union/fill", "union/add_fwd", "union/add_bwd")


def counts():
    from spconv_amd import _lib
    return _lib.launch_counts(KEYS)


def bits(t):
    t = t.detach().cpu().contiguous()
    return t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def keys_of(idx, bs, shape):
    """int64 linear key per row (batch-major, last axis fastest), -1 for a row outside the batch or the grid"""
    idx = np.asarray(idx, dtype=np.int64)
    ok = (idx[:, 0] >= 0) & (idx[:, 0] < bs)
    key = idx[:, 0].copy()
    for d, ext in enumerate(shape):
        ok &= (idx[:, 1 + d] >= 0) & (idx[:, 1 + d] < ext)
        key = key * ext + idx[:, 1 + d]
    return np.where(ok, key, -1)


def decode(keys, shape):
    keys = np.asarray(keys, dtype=np.int64)
    cols = []
    for ext in reversed(shape):
        cols.append(keys % ext)
        keys = keys // ext
    return np.stack([keys] + cols[::-1], axis=1).astype(np.int32)


def operand(bs, shape, n, seed, forced=()):
    """n scene rows plus the forced keys, distinct, in shuffled row order"""
    idx = scene(shape, n, bs, seed) if n > 0 else np.zeros((0, len(shape) + 1), np.int32)
    keys = np.unique(np.concatenate([keys_of(idx, bs, shape), np.asarray(forced, dtype=np.int64)]))
    rng = np.random.default_rng(1000 + seed)
    return decode(rng.permutation(keys), shape)


def features(n, C, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn((n, C), generator=g, dtype=torch.float32).to(dtype)


def expect(idxs, feats, bs, shape, n_live=None):
    """(sorted union keys, features [n_out, C] in the row dtype, rows_t per operand)"""
    dtype = feats[0].dtype
    acc_t = torch.float64 if dtype == torch.float64 else torch.float32
    ks = []
    for t, idx in enumerate(idxs):
        k = keys_of(idx, bs, shape)
        if n_live is not None and n_live[t] is not None:
            k[n_live[t]:] = -1
        ks.append(k)
    uniq = np.unique(np.concatenate(ks))
    uniq = uniq[uniq >= 0]
    acc = np.zeros((uniq.shape[0], feats[0].shape[1]), dtype=np.float64 if acc_t == torch.float64 else np.float32)
    present = np.zeros((uniq.shape[0],), dtype=bool)
    rows = []
    for k, f in zip(ks, feats):
        live = k >= 0
        r = np.searchsorted(uniq, k[live])
        assert np.unique(r).shape[0] == r.shape[0], "the expectation assumes distinct coordinates within an operand"
        fl = f.to(acc_t).numpy()[live]
        first = ~present[r]
        acc[r[first]] = fl[first]                       # an absent operand is skipped, not added as zero
        acc[r[~first]] = acc[r[~first]] + fl[~first]
        present[r] = True
        full = np.full(k.shape, -1, dtype=np.int64)
        full[live] = r
        rows.append(full)
    return uniq, torch.from_numpy(acc).to(dtype), rows


def check_tables(u, idxs, rows_ref, n_out):
    """rows_t / src against the expectation and against each other"""
    src = u.src.cpu().numpy()
    assert src.shape == (len(idxs), n_out)
    for t, ref in enumerate(rows_ref):
        rows = u.rows[t].cpu().numpy()
        np.testing.assert_array_equal(rows, ref)
        live = np.nonzero(rows >= 0)[0]
        np.testing.assert_array_equal(src[t][rows[live]], live)
        assert int((src[t] >= 0).sum()) == live.shape[0]
        assert src[t].min(initial=-1) >= -1 and src[t].max(initial=-1) < max(len(rows), 1)


def run_native(idxs, feats, bs, shape, cuda, gate=True):
    from spconv_amd.pytorch import _union, ops
    dev_idx = [torch.from_numpy(np.ascontiguousarray(i)).to(cuda) for i in idxs]
    u = ops.sparse_union(dev_idx, bs, shape, base=-1, gate=gate)
    assert u is not None
    out = _union.add_fwd([f.to(cuda) for f in feats], u.src, u.n_out)
    return u, out


def mix_a(name):
    bs, shape = GRID_A
    if name.startswith("T"):
        T = int(name[1:])
        forced = [[] for _ in range(T)]
        for j, key in enumerate(FORCED):
            if j < 3:
                holders = [j % T]                                   # in one operand
            elif j < 6:
                holders = [t for t in range(T) if t % 2 == 0]       # in several
            else:
                holders = list(range(T))                            # in all
            for t in holders:
                forced[t].append(key)
        return [operand(bs, shape, 100 + 12 * t, 10 + t, forced[t]) for t in range(T)]
    a, b = operand(bs, shape, 150, 1, FORCED), operand(bs, shape, 200, 2, FORCED[::2])
    if name == "one_empty":
        return [a, operand(bs, shape, 0, 0), b]
    if name == "all_empty":
        return [operand(bs, shape, 0, 0), operand(bs, shape, 0, 0)]
    if name == "identical":
        return [a, a.copy()]
    assert name == "disjoint"
    kb = keys_of(b, bs, shape)
    return [a, b[~np.isin(kb, keys_of(a, bs, shape))]]


@pytest.mark.parametrize("mix", ["T1", "T2", "T3", "T8", "one_empty", "all_empty", "identical", "disjoint"])
def test_grid_a(cuda, mix):
    bs, shape = GRID_A
    idxs = mix_a(mix)
    feats = [features(i.shape[0], 8, torch.float16, 7 + t) for t, i in enumerate(idxs)]
    uniq, want, rows_ref = expect(idxs, feats, bs, shape)
    u, out = run_native(idxs, feats, bs, shape, cuda, gate=mix != "all_empty")
    assert u.n_out == uniq.shape[0]
    np.testing.assert_array_equal(u.out_indices.cpu().numpy(), decode(uniq, shape))      # exactly the sorted union
    check_tables(u, idxs, rows_ref, uniq.shape[0])
    assert torch.equal(bits(out), bits(want))


@pytest.mark.parametrize("C", [1, 3, 8, 20, 64, 260])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, torch.float32, torch.float64])
def test_dtype_width(cuda, dtype, C):
    import spconv_amd.pytorch as spconv
    from spconv_amd.pytorch import functional as Fsp
    bs, shape = SMALL
    idxs = [operand(bs, shape, 300 + 40 * t, 20 + t) for t in range(3)]
    feats = [features(i.shape[0], C, dtype, 30 + t) for t, i in enumerate(idxs)]
    uniq, want, _ = expect(idxs, feats, bs, shape)
    tens = [spconv.SparseConvTensor(f.to(cuda), torch.from_numpy(i).to(cuda), shape, bs) for f, i in zip(feats, idxs)]
    before = counts()
    out = Fsp.sparse_add_hash_based(*tens)
    assert counts()["union/add_fwd"] == before["union/add_fwd"] + 1
    np.testing.assert_array_equal(out.indices.cpu().numpy(), decode(uniq, shape))
    assert out.features.dtype == dtype and torch.equal(bits(out.features), bits(want))


@pytest.mark.parametrize("bs,shape", [(3, [97]), (2, [33, 70]), (1, [5, 6, 7, 9])])
def test_ndim(cuda, bs, shape):
    idxs = [operand(bs, shape, 60 + 10 * t, 40 + t, [0, bs * int(np.prod(shape)) - 1] if t else []) for t in range(3)]
    feats = [features(i.shape[0], 5, torch.float32, 50 + t) for t, i in enumerate(idxs)]
    uniq, want, rows_ref = expect(idxs, feats, bs, shape)
    u, out = run_native(idxs, feats, bs, shape, cuda)
    np.testing.assert_array_equal(u.out_indices.cpu().numpy(), decode(uniq, shape))
    check_tables(u, idxs, rows_ref, uniq.shape[0])
    assert torch.equal(bits(out), bits(want))


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, torch.float32, torch.float64])
def test_negative_zero_of_a_single_operand_keeps_its_bits(cuda, dtype):
    bs, shape = SMALL
    idxs = [decode([5, 9, 700], shape), decode([9, 11], shape)]
    feats = [torch.full((3, 4), -0.0, dtype=dtype), torch.full((2, 4), -0.0, dtype=dtype)]
    feats[1][1, 2] = 1.5
    _, want, _ = expect(idxs, feats, bs, shape)
    _, out = run_native(idxs, feats, bs, shape, cuda, gate=False)
    out = out.cpu()
    assert torch.equal(bits(out), bits(want))
    sign = torch.signbit(out)
    assert bool(sign[0].all()) and bool(sign[3].all())          # keys 5 and 700: one operand, -0.0 as it came
    assert bool(sign[1].all())                                  # key 9: (-0.0) + (-0.0) = -0.0
    assert bool(sign[2, :2].all()) and float(out[2, 2]) == 1.5  # key 11: one operand


def test_dead_rows_contribute_nothing(cuda):
    import spconv_amd.pytorch as spconv
    from spconv_amd.pytorch import functional as Fsp
    from spconv_amd.pytorch import ops
    bs, shape = SMALL
    a = operand(bs, shape, 120, 60)
    dead = np.array([[-1, 1, 1, 1], [bs, 2, 2, 2], [0, 12, 0, 0], [1, 3, -1, 5], [0, 1, 14, 2], [1, 0, 0, 16]], np.int32)
    a = np.concatenate([a[:50], dead[:3], a[50:], dead[3:]])
    b = operand(bs, shape, 150, 61)
    live_b = 100                                                # in-range rows behind n_live
    idxs, lives = [a, b], [None, live_b]
    feats = [features(i.shape[0], 6, torch.float32, 62 + t) for t, i in enumerate(idxs)]
    uniq, want, rows_ref = expect(idxs, feats, bs, shape, lives)
    dev_idx = [torch.from_numpy(i).to(cuda) for i in idxs]
    n_live_b = torch.tensor([live_b], dtype=torch.int32, device=cuda)
    u = ops.sparse_union(dev_idx, bs, shape, n_live=[None, n_live_b])      # (static form: key order)
    found, dup, live = u.n_out_dev.cpu().tolist()
    assert (found, dup, live) == (uniq.shape[0], 0, uniq.shape[0])
    for t in range(2):
        np.testing.assert_array_equal(u.rows[t].cpu().numpy(), rows_ref[t])
    assert int((u.rows[0].cpu() < 0).sum()) == 6 and int((u.rows[1].cpu() < 0).sum()) == b.shape[0] - live_b
    # through the public function, with gradients
    tens = []
    for f, i, nl in zip(feats, dev_idx, [None, n_live_b]):
        t = spconv.SparseConvTensor(f.to(cuda).requires_grad_(True), i, shape, bs)
        t.n_live_dev = nl
        tens.append(t)
    out = Fsp.sparse_add_hash_based(*tens)
    n = uniq.shape[0]
    np.testing.assert_array_equal(out.indices[:n].cpu().numpy(), decode(uniq, shape))
    assert bool((out.indices[n:] == -1).all()) and int(out.n_live_dev.item()) == n
    assert torch.equal(bits(out.features[:n]), bits(want)) and not bool(out.features[n:].any())
    g = torch.randn(out.features.shape, generator=torch.Generator().manual_seed(3)).to(cuda)
    out.features.backward(g)
    for t, ref in enumerate(rows_ref):
        grad = tens[t].features.grad.cpu()
        dead_rows = torch.from_numpy(ref < 0)
        assert not bool(grad[dead_rows].any())                  # a dead row receives a zero gradient
        assert torch.equal(bits(grad[~dead_rows]), bits(g.cpu()[torch.from_numpy(ref[ref >= 0])]))


def test_covering_operand_keeps_its_numbering_and_rulebooks(cuda):
    import spconv_amd.pytorch as spconv
    from spconv_amd.pytorch import functional as Fsp
    from spconv_amd.pytorch import ops
    bs, shape = SMALL
    ia = operand(bs, shape, 300, 70)
    rng = np.random.default_rng(5)
    ib = ia[rng.permutation(ia.shape[0])[:120]]                 # a strict subset, shuffled
    fa, fb = features(ia.shape[0], 8, torch.float16, 71), features(ib.shape[0], 8, torch.float16, 72)
    a = spconv.SparseConvTensor(fa.to(cuda), torch.from_numpy(ia).to(cuda), shape, bs)
    b = spconv.SparseConvTensor(fb.to(cuda), torch.from_numpy(ib).to(cuda), shape, bs)
    a.indice_dict["k"] = marker = object()
    # the expectation in a's numbering: a's row + b's row where b holds the coordinate
    pos = {int(k): r for r, k in enumerate(keys_of(ia, bs, shape))}
    acc = fa.float().numpy().copy()
    rb = np.array([pos[int(k)] for k in keys_of(ib, bs, shape)])
    acc[rb] = acc[rb] + fb.float().numpy()
    want = torch.from_numpy(acc).to(torch.float16)
    for operands in ((a, b), (b, a)):
        for fn in (Fsp.sparse_add_hash_based, Fsp.sparse_add, lambda *t: spconv.AddTableMisaligned()(list(t))):
            out = fn(*operands)
            assert out.indices is a.indices
            assert out.indice_dict.get("k") is marker
            assert torch.equal(bits(out.features), bits(want))
    # no operand covers: a fresh coordinate set in key order with its rank map, no rulebooks
    ic = operand(bs, shape, 119, 73)
    c = spconv.SparseConvTensor(features(ic.shape[0], 8, torch.float16, 74).to(cuda), torch.from_numpy(ic).to(cuda), shape, bs)
    c.indice_dict["k"] = marker
    out = Fsp.sparse_add_hash_based(a, c)
    assert out.indice_dict == {} and out.indices is not a.indices
    assert ops._rankmap_of(out.indices, bs, shape, out.indices.shape[0], 27) is not None


def test_subm_over_the_result_matches_the_untagged_build(cuda):
    import spconv_amd.pytorch as spconv
    from spconv_amd.pytorch import functional as Fsp
    from spconv_amd.pytorch import ops
    bs, shape = SMALL
    tens = []
    for t in range(2):
        i = operand(bs, shape, 300, 80 + t)
        tens.append(spconv.SparseConvTensor(features(i.shape[0], 16, torch.float16, 82 + t).to(cuda),
                                            torch.from_numpy(i).to(cuda), shape, bs))
    out = Fsp.sparse_add_hash_based(*tens)
    torch.manual_seed(0)
    conv = spconv.SubMConv3d(16, 16, 3, bias=False).to(cuda).half().eval()
    plain = spconv.SparseConvTensor(out.features, out.indices.clone(), shape, bs)
    assert ops._rankmap_of(out.indices, bs, shape, out.indices.shape[0], 27) is not None
    assert ops._rankmap_of(plain.indices, bs, shape, plain.indices.shape[0], 27) is None      # the hash build
    with torch.no_grad():
        got, ref = conv(out), conv(plain)
    assert torch.equal(bits(got.features), bits(ref.features))


def test_duplicates_take_the_composite(cuda):
    import spconv_amd.pytorch as spconv
    from spconv_amd.pytorch import functional as Fsp
    bs, shape = SMALL
    ia, ib = operand(bs, shape, 200, 90), operand(bs, shape, 220, 91)
    ib = ib[keys_of(ib, bs, shape) != keys_of(ia[17:18], bs, shape)[0]]
    ia = np.concatenate([ia, ia[17:18]])                        # one coordinate twice, in this operand only
    fa, fb = features(ia.shape[0], 4, torch.float32, 92), features(ib.shape[0], 4, torch.float32, 93)
    fa[-1] = fa[17]
    # at most two terms per coordinate (the repeated one: x + x): one IEEE addition, whatever the order
    dense = torch.zeros((bs, *shape, 4), dtype=torch.float32)
    for i, f in ((ia, fa), (ib, fb)):
        for r in range(i.shape[0]):
            dense[tuple(int(v) for v in i[r])] += f[r]
    tens = [spconv.SparseConvTensor(f.to(cuda), torch.from_numpy(i).to(cuda), shape, bs) for f, i in ((fa, ia), (fb, ib))]
    before = counts()
    out = Fsp.sparse_add_hash_based(*tens)
    after = counts()
    assert after["union/claim"] == before["union/claim"] + 1            # the count ran and saw the flag
    assert after["union/add_fwd"] == before["union/add_fwd"] and after["union/fill"] == before["union/fill"]
    oi = out.indices.cpu().long()
    uniq = np.unique(np.concatenate([keys_of(ia, bs, shape), keys_of(ib, bs, shape)]))
    assert oi.shape[0] == uniq.shape[0] and np.array_equal(np.sort(keys_of(oi.numpy(), bs, shape)), uniq)
    assert torch.equal(bits(out.features), bits(dense[oi[:, 0], oi[:, 1], oi[:, 2], oi[:, 3]]))
    row = int(np.nonzero(keys_of(oi.numpy(), bs, shape) == keys_of(ia[17:18], bs, shape)[0])[0][0])
    assert torch.equal(out.features[row].cpu(), fa[17] + fa[17])         # the two rows summed


def test_key_space_beyond_the_gate_keeps_the_hash_path(cuda):
    import spconv_amd.pytorch as spconv
    from spconv_amd.pytorch import functional as Fsp
    bs, shape = 1, [4096, 4096, 4096]
    rng = np.random.default_rng(9)
    idxs = [np.concatenate([np.zeros((50, 1), np.int64), rng.integers(0, 4096, (50, 3))], 1).astype(np.int32)
            for _ in range(2)]
    idxs[1][:10] = idxs[0][:10]
    feats = [features(50, 4, torch.float32, 95 + t) for t in range(2)]
    tens = [spconv.SparseConvTensor(f.to(cuda), torch.from_numpy(i).to(cuda), shape, bs) for f, i in zip(feats, idxs)]
    before = counts()
    out = Fsp.sparse_add_hash_based(*tens)
    assert counts() == before
    got = {tuple(r): out.features[j].cpu() for j, r in enumerate(out.indices.cpu().tolist())}
    want = {}
    for i, f in zip(idxs, feats):
        for r in range(50):
            k = tuple(int(v) for v in i[r])
            want[k] = want[k] + f[r] if k in want else f[r]
    assert set(got) == set(want)
    assert all(torch.equal(got[k], want[k]) for k in want)     # (at most two terms: one IEEE addition, commutative)


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
def test_launches_and_backward_bits(cuda, dtype):
    import spconv_amd.pytorch as spconv
    from spconv_amd.pytorch import functional as Fsp
    bs, shape = SMALL
    idxs = [operand(bs, shape, 250 + 30 * t, 100 + t) for t in range(3)]
    feats = [features(i.shape[0], 12, dtype, 103 + t) for t, i in enumerate(idxs)]
    uniq, want, rows_ref = expect(idxs, feats, bs, shape)
    tens = [spconv.SparseConvTensor(f.to(cuda).requires_grad_(True), torch.from_numpy(i).to(cuda), shape, bs)
            for f, i in zip(feats, idxs)]
    c0 = counts()
    out = Fsp.sparse_add_hash_based(*tens)
    c1 = counts()
    assert c1["union/add_fwd"] == c0["union/add_fwd"] + 1 and c1["union/add_bwd"] == c0["union/add_bwd"]
    assert c1["union/mark"] == c0["union/mark"] + 1 and c1["union/fill"] == c0["union/fill"] + 1
    assert torch.equal(bits(out.features), bits(want))
    g = torch.randn(out.features.shape, generator=torch.Generator().manual_seed(4)).to(dtype)
    out.features.backward(g.to(cuda))
    c2 = counts()
    assert c2["union/add_bwd"] == c1["union/add_bwd"] + 1 and c2["union/add_fwd"] == c1["union/add_fwd"]
    for t, ref in enumerate(rows_ref):
        assert torch.equal(bits(tens[t].features.grad), bits(g[torch.from_numpy(ref)]))


def test_gradcheck_f64(cuda):
    from spconv_amd.pytorch import functional as Fsp
    from spconv_amd.pytorch import ops
    bs, shape = 1, [4, 5, 6]
    idxs = [operand(bs, shape, 40, 110), operand(bs, shape, 50, 111)]
    u = ops.sparse_union([torch.from_numpy(i).to(cuda) for i in idxs], bs, shape, base=-1)
    feats = [features(i.shape[0], 3, torch.float64, 112 + t).to(cuda).requires_grad_(True) for t, i in enumerate(idxs)]
    fn = lambda a, b: Fsp.SparseUnionAddFunction.apply(u.src, u.rows, u.n_out, None, a, b)
    assert torch.autograd.gradcheck(fn, feats, eps=1e-6, atol=1e-9, rtol=1e-7)


def static_inputs(cuda, idxs, feats, pad):
    """operands padded with dead rows (batch -1, zero features) + their device-side live counts"""
    dev_idx, dev_feat, lives = [], [], []
    for i, f in zip(idxs, feats):
        full = np.full((i.shape[0] + pad, i.shape[1]), -1, np.int32)
        full[:i.shape[0]] = i
        ff = torch.zeros((f.shape[0] + pad, f.shape[1]), dtype=f.dtype)
        ff[:f.shape[0]] = f
        dev_idx.append(torch.from_numpy(full).to(cuda))
        dev_feat.append(ff.to(cuda))
        lives.append(torch.tensor([i.shape[0]], dtype=torch.int32, device=cuda))
    return dev_idx, dev_feat, lives


@pytest.mark.parametrize("short", [0, 10])
def test_static_form(cuda, short):
    from spconv_amd.pytorch import _union, ops
    bs, shape = SMALL
    idxs = [operand(bs, shape, 260 + 30 * t, 120 + t) for t in range(3)]
    feats = [features(i.shape[0], 8, torch.float16, 123 + t) for t, i in enumerate(idxs)]
    uniq, want, rows_ref = expect(idxs, feats, bs, shape)
    n = uniq.shape[0]
    dev_idx, dev_feat, lives = static_inputs(cuda, idxs, feats, pad=7)
    cap = n - short if short else None
    u = ops.sparse_union(dev_idx, bs, shape, n_live=lives, static_num_out=cap)
    rows_cap = u.n_out
    assert rows_cap == (cap if short else sum(i.shape[0] for i in dev_idx))
    found, dup, live = u.n_out_dev.cpu().tolist()
    assert (found, dup, live) == (n, 0, min(n, rows_cap))                  # the full size, also beyond the bound
    out = _union.add_fwd(dev_feat, u.src, u.n_out, u.n_out_dev[2:3])
    np.testing.assert_array_equal(u.out_indices[:live].cpu().numpy(), decode(uniq[:live], shape))
    assert bool((u.out_indices[live:] == -1).all()) and not bool(out[live:].any())
    assert torch.equal(bits(out[:live]), bits(want[:live]))                # the first `cap` rows in key order
    src = u.src.cpu().numpy()
    assert bool((src[:, live:] == -1).all())
    for t, ref in enumerate(rows_ref):
        rows = u.rows[t].cpu().numpy()
        full = np.full(rows.shape, -1, np.int64)
        full[:ref.shape[0]] = np.where(ref < live, ref, -1)                # outputs beyond the bound are dropped
        np.testing.assert_array_equal(rows, full)
        held = np.nonzero(rows >= 0)[0]
        np.testing.assert_array_equal(src[t][rows[held]], held)
        assert int((src[t] >= 0).sum()) == held.shape[0]
    if not short:                                                          # the eager key-order result, bit for bit
        e = ops.sparse_union([torch.from_numpy(i).to(cuda) for i in idxs], bs, shape, base=-1)
        eo = _union.add_fwd([f.to(cuda) for f in feats], e.src, e.n_out)
        assert e.n_out == live and torch.equal(e.out_indices, u.out_indices[:live])
        assert torch.equal(bits(eo), bits(out[:live]))


def test_module_is_captured_in_one_graph(cuda):
    import spconv_amd.pytorch as spconv
    bs, shape, C, cap = 2, [12, 14, 16], 8, 400
    scenes = []
    for s in range(2):
        idxs = [operand(bs, shape, 100 + 30 * s + 10 * t, 130 + 2 * s + t) for t in range(2)]
        scenes.append((idxs, [features(i.shape[0], C, torch.float16, 140 + 2 * s + t) for t, i in enumerate(idxs)]))
    idx_buf = [torch.full((cap, 4), -1, dtype=torch.int32, device=cuda) for _ in range(2)]
    feat_buf = [torch.zeros((cap, C), dtype=torch.float16, device=cuda) for _ in range(2)]
    lives = [torch.zeros((1,), dtype=torch.int32, device=cuda) for _ in range(2)]
    add = spconv.AddTableMisaligned()

    def load(idxs, feats):
        for t in range(2):
            n = idxs[t].shape[0]
            idx_buf[t].fill_(-1)
            feat_buf[t].zero_()
            idx_buf[t][:n].copy_(torch.from_numpy(idxs[t]))
            feat_buf[t][:n].copy_(feats[t])
            lives[t].fill_(n)

    def forward():
        tens = []
        for t in range(2):
            x = spconv.SparseConvTensor(feat_buf[t], idx_buf[t], shape, bs)
            x.n_live_dev = lives[t]
            tens.append(x)
        return add(tens)

    load(*scenes[0])
    side = torch.cuda.Stream(device=cuda)
    side.wait_stream(torch.cuda.current_stream(cuda))
    with torch.cuda.stream(side), torch.no_grad():
        forward()
    torch.cuda.current_stream(cuda).wait_stream(side)
    torch.cuda.synchronize(cuda)
    graph = torch.cuda.CUDAGraph()
    with torch.no_grad(), torch.cuda.graph(graph):              # one stream, no forked branches
        out = forward()
    for idxs, feats in scenes[::-1] + scenes:
        uniq, want, _ = expect(idxs, feats, bs, shape)
        load(idxs, feats)
        graph.replay()
        n = int(out.n_live_dev.item())
        assert n == uniq.shape[0] and add._static_n_out_dev.cpu().tolist() == [n, 0, n]
        np.testing.assert_array_equal(out.indices[:n].cpu().numpy(), decode(uniq, shape))
        assert bool((out.indices[n:] == -1).all()) and not bool(out.features[n:].any())
        assert torch.equal(bits(out.features[:n]), bits(want))


class TwoBranch(torch.nn.Module):
    def __init__(self, C, static_num_out=None):
        super().__init__()
        import spconv_amd.pytorch as spconv
        self.conv0 = spconv.SubMConv3d(C, C, 3, bias=False, indice_key="s0")
        self.branch = spconv.SparseConv3d(C, C, 3, stride=1, padding=1, bias=False)
        self.add = spconv.AddTableMisaligned(static_num_out=static_num_out)
        self.conv1 = spconv.SubMConv3d(C, C, 3, bias=False, indice_key="s1")

    def forward(self, x):
        x = self.conv0(x)
        return self.conv1(self.add([self.branch(x), x]))


def by_key(out, bs, shape):
    idx = out.indices.cpu().numpy()
    k = keys_of(idx, bs, shape)
    live = np.nonzero(k >= 0)[0]
    order = live[np.argsort(k[live])]
    return k[order], out.features.detach().cpu()[torch.from_numpy(order)]


def test_two_branch_network_under_static_inference(cuda):
    import spconv_amd.pytorch as spconv
    from spconv_amd.pytorch.static import StaticInference
    bs, shape, C = 2, [12, 14, 16], 16
    torch.manual_seed(1)
    net = TwoBranch(C, static_num_out=6000).to(cuda).half().eval()
    idx = torch.from_numpy(operand(bs, shape, 150, 150)).to(cuda)
    feat = (features(idx.shape[0], C, torch.float16, 151) * 0.25).to(cuda)
    with torch.no_grad():
        eager = net(spconv.SparseConvTensor(feat, idx, shape, bs))
    ek, ef = by_key(eager, bs, shape)
    runner = StaticInference(net, max_voxels=320, in_channels=C, spatial_shape=shape, batch_size=bs,
                             dtype=torch.float16, bounds={"branch": ek.shape[0] + 32})
    try:
        out = runner(feat, idx)
        sk, sf = by_key(out, bs, shape)
        np.testing.assert_array_equal(sk, ek)
        assert torch.equal(bits(sf), bits(ef))                  # per coordinate, bit for bit
        assert runner.overflowed() == {} and set(runner.counts()) == {"branch", "add"}
        first = (out.indices.clone(), out.features.clone())
        out = runner(feat, idx)
        assert torch.equal(out.indices, first[0]) and torch.equal(bits(out.features), bits(first[1]))
    finally:
        runner.release_bounds()
