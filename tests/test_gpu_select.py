"""Voxel pruning on the kernels of csrc/select.hip (spconv_amd/pytorch/_select.py, functional.row_score / topk_mask /
sparse_select / sparse_prune, spatial.SparsePrune) against the numpy reference of tests/refselect.py.

Everything integer -- flags, counters, tables -- and every moved feature row is compared bit for bit.  The absmean
score is compared bit for bit with the reference, which adds in the header's order with the same IEEE float32 (float64)
additions, and independently against an fp64 evaluation inside refselect.score_bound: (C + 2) 2^-24 relative, the bound
of a sum of C non-negative fp32 terms in any order plus one division and one rounding (f64 inputs: half an fp32 ulp).
absmax is exact."""
import numpy as np
import pytest
import torch

import refcollapse as rc
import refselect as rs

pytestmark = pytest.mark.gpu

KEYS = ("select/score", "select/hist", "select/pick", "select/ties", "select/flags", "select/count", "select/scan",
        "select/scatter", "select/map")
DTYPES = [torch.float16, torch.bfloat16, torch.float32, torch.float64]


def counts():
    from spconv_amd import _lib
    return _lib.launch_counts(KEYS)


def delta(before):
    after = counts()
    return {k.split("/")[1]: after[k] - before[k] for k in KEYS if after[k] != before[k]}


def bits(t):
    t = t.detach().cpu().contiguous()
    return t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def i32(cuda, values):
    return torch.tensor(values, dtype=torch.int32, device=cuda)


# ---------------------------------------------------------------------------------------- score
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[1])
@pytest.mark.parametrize("C", [1, 3, 8, 64, 129, 260])
def test_score(cuda, dtype, C):
    import spconv_amd.pytorch as spconv
    F = spconv.functional
    for n in (0, 1, 257, 3000) + ((9000,) if C == 260 and dtype == torch.float16 else ()):     # 9000 x 64 lanes: grid-stride
        feat = rc.features(n, C, dtype, 7 * C + n)
        n_live = n - n // 5
        dev = feat.to(cuda)
        before = counts()
        got = F.row_score(dev, "absmean", i32(cuda, [n_live])).cpu().numpy()
        assert delta(before) == ({"score": 1} if n else {})
        assert got.dtype == np.float32 and got.shape == (n,)
        np.testing.assert_array_equal(got.view(np.uint32), rs.score(feat, "absmean", n_live).view(np.uint32))
        assert bool(np.isneginf(got[n_live:]).all())
        want = rs.score_f64(feat[:n_live], "absmean")
        assert bool((np.abs(got[:n_live].astype(np.float64) - want) <= rs.score_bound(dtype, C, want)).all())
        mx = F.row_score(dev, "absmax").cpu().numpy()
        np.testing.assert_array_equal(mx.view(np.uint32), rs.score_f64(feat, "absmax").astype(np.float32).view(np.uint32))
        if n:       # a tensor that starts off a 16-byte boundary: the same elements in the same order
            buf = torch.zeros((n * C + 1,), dtype=dtype, device=cuda)
            buf[1:] = dev.flatten()
            off = F.row_score(buf[1:].view(n, C), "absmean").cpu().numpy()
            np.testing.assert_array_equal(off.view(np.uint32), rs.score(feat, "absmean").view(np.uint32))


def test_score_refusals(cuda):
    import spconv_amd.pytorch as spconv
    F = spconv.functional
    with pytest.raises(NotImplementedError, match="float16"):
        F.row_score(torch.zeros((4, 4), dtype=torch.int8, device=cuda))
    with pytest.raises(ValueError, match="absmean"):
        F.row_score(torch.zeros((4, 4), device=cuda), "l2")


# ---------------------------------------------------------------------------------------- flags
@pytest.mark.parametrize("kind", rs.SCORE_KINDS)
@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 3000, 20000])
def test_flags(cuda, kind, n):
    from spconv_amd.pytorch import _select
    s = rs.scores(kind, n, 11 + n)
    rng = np.random.default_rng(n + 1)
    idx = np.zeros((n, 4), dtype=np.int32)
    idx[:, 0] = rng.integers(0, 2, n)
    idx[rng.random(n) < 0.1, 0] = -1                                # interior dead rows
    n_live = n - n // 7
    dev_s, dev_idx, dev_live = torch.from_numpy(s).to(cuda), torch.from_numpy(idx).to(cuda), i32(cuda, [n_live])
    live = int(rs.live_rows(n, idx, 2, n_live).sum())
    variants = [(k, None) for k in (0, 1, live - 1, live, live + 5) if k >= 0] + [(None, r) for r in (0.0, 0.3, 0.5, 1.0)]
    for k, ratio in variants:
        ref = rs.topk(s, k, ratio, idx, 2, n_live)
        before = counts()
        keep, sel = _select.topk_flags(dev_s, k, ratio, dev_idx, 2, dev_live)
        assert delta(before) == ({"hist": 4, "pick": 4, "ties": 1, "flags": 1} if n else {"pick": 4})
        assert keep.dtype == torch.uint8 and sel.cpu().tolist() == ref.sel
        np.testing.assert_array_equal(keep.cpu().numpy(), ref.keep)
        assert int(keep.sum().item()) == ref.sel[1]                 # exactly k ones
    again, sel2 = _select.topk_flags(dev_s, None, 0.5, dev_idx, 2, dev_live)
    assert torch.equal(again, _select.topk_flags(dev_s, None, 0.5, dev_idx, 2, dev_live)[0])
    # no indices, no n_live: every row is live
    ref = rs.topk(s, None, 0.3)
    keep, sel = _select.topk_flags(dev_s, None, 0.3)
    assert sel.cpu().tolist() == ref.sel
    np.testing.assert_array_equal(keep.cpu().numpy(), ref.keep)
    if kind == "equal" and n:
        assert keep.cpu().numpy().tolist() == [1] * ref.sel[1] + [0] * (n - ref.sel[1])      # the first k rows


def test_topk_mask_takes_any_float_score(cuda):
    import spconv_amd.pytorch as spconv
    s = rs.scores("normal", 500, 3)
    ref = rs.topk(s.astype(np.float16).astype(np.float32), 100)
    keep = spconv.functional.topk_mask(torch.from_numpy(s).to(cuda).half(), k=100)
    np.testing.assert_array_equal(keep.cpu().numpy(), ref.keep)


# ---------------------------------------------------------------------------------------- build
def native_build(cuda, idx, bs, shape, keep, invert, n_live=None, cap=None, rank_map=False):
    from spconv_amd.pytorch import _select
    nl = None if n_live is None else i32(cuda, [n_live])
    return _select.select_build(torch.from_numpy(np.ascontiguousarray(idx)).to(cuda), bs, shape,
                                torch.from_numpy(keep).to(cuda), invert, n_live=nl, static_num_out=cap, rank_map=rank_map)


BUILD_SHAPES = {1: [97], 2: [33, 70], 3: [5, 14, 16], 4: [5, 6, 7, 9]}


@pytest.mark.parametrize("ndim", [1, 2, 3, 4])
@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 3000, 20000])
def test_build(cuda, ndim, n):
    shape = BUILD_SHAPES[ndim]
    idx = rc.scene(2, shape, n, 5 * n + ndim, 0)                    # out-of-range rows spread through the middle
    rows = idx.shape[0]
    rng = np.random.default_rng(n + ndim)
    half = (rng.random(rows) < 0.5).astype(np.uint8) * rng.integers(1, 256, rows).astype(np.uint8)     # nonzero = keep
    n_live = rows - rows // 9
    for keep in (np.zeros(rows, np.uint8), np.ones(rows, np.uint8), half):
        for invert in (False, True):
            ref = rs.select(idx, 2, shape, keep, invert, n_live)
            before = counts()
            s = native_build(cuda, idx, 2, shape, keep, invert, n_live=None if n_live == rows else n_live)
            if n_live == rows:                                      # the eager form: count + fill
                assert delta(before) == {"count": 1, "scan": 1, **({"scatter": 1} if rows else {})}
                assert s.n_out == ref.found and s.live_rows == ref.live_rows and s.n_out_dev is None
                np.testing.assert_array_equal(s.out_indices.cpu().numpy(), ref.out_indices)
                np.testing.assert_array_equal(s.src.cpu().numpy(), ref.src)
            else:                                                   # n_live given: the static form, default bound
                assert delta(before) == {"count": 1, "scan": 1, "scatter": 1}
                check_static(s, ref, rows, max(rows, 1), ndim)
            np.testing.assert_array_equal(s.rows.cpu().numpy(), ref.rows)
    # the eager form proper, with every row in place
    ref = rs.select(idx, 2, shape, half, False)
    before = counts()
    s = native_build(cuda, idx, 2, shape, half, False)
    assert delta(before) == {"scan": 1, **({"count": 1, "scatter": 1} if rows else {})}
    assert s.n_out == ref.found == ref.live and s.live_rows == ref.live_rows and s.n_out_dev is None
    np.testing.assert_array_equal(s.out_indices.cpu().numpy(), ref.out_indices)
    np.testing.assert_array_equal(s.src.cpu().numpy(), ref.src)
    np.testing.assert_array_equal(s.rows.cpu().numpy(), ref.rows)
    # static form with room to spare and with a bound that cuts
    for cap in (ref.found + 9, max(ref.found - 5, 1)):
        cut = rs.select(idx, 2, shape, half, False, n_live, cap=cap)
        s = native_build(cuda, idx, 2, shape, half, False, n_live=n_live, cap=cap)
        check_static(s, cut, rows, cap, ndim)
        np.testing.assert_array_equal(s.rows.cpu().numpy(), cut.rows)          # cut rows in row order: -1


SCAN_ROWS = 66000           # 258 workgroups of 256 rows: the one-workgroup scans carry into a second round of 256 counts


@pytest.mark.parametrize("what", ["build_eager", "build_static_cut", "flags"])
def test_scan_carries_into_a_second_round(cuda, what):
    """select_scan_kernel (and the tie scan of the flags) walk the workgroups' counts 256 at a time and carry the sum
    from round to round: from 257 workgroups on there is a second round, which no smaller case reaches"""
    from spconv_amd.pytorch import _select
    n = SCAN_ROWS
    assert (n + 255) // 256 > 256
    if what == "flags":
        s = rs.scores("equal", n, 3)                                # every row ties: the kept rows are the first k
        s[::3] = 0.25
        for k in (1, n // 3, n - n // 3 - 1, n - n // 3, n - n // 3 + 7, n):
            ref = rs.topk(s, k)
            before = counts()
            keep, sel = _select.topk_flags(torch.from_numpy(s).to(cuda), k)
            assert delta(before) == {"hist": 4, "pick": 4, "ties": 1, "flags": 1}
            assert sel.cpu().tolist() == ref.sel
            np.testing.assert_array_equal(keep.cpu().numpy(), ref.keep)
        assert rs.topk(s, n - 5).sel[3] > 65536 // 3                # ties are taken in blocks of the second round
        return
    shape = [40, 60, 60]
    idx = rc.scene(2, shape, n - 8, 17, 0)                          # 8 rows no scene owns: n rows
    rows = idx.shape[0]
    assert rows == n
    keep = (np.random.default_rng(18).random(rows) < 0.6).astype(np.uint8)
    keep[-700:] = 1                                                 # selected rows in the last blocks of the second round
    if what == "build_eager":
        ref = rs.select(idx, 2, shape, keep, False)
        before = counts()
        s = native_build(cuda, idx, 2, shape, keep, False)
        assert delta(before) == {"count": 1, "scan": 1, "scatter": 1}
        assert s.n_out == ref.found == ref.live and s.live_rows == ref.live_rows and s.n_out_dev is None
        np.testing.assert_array_equal(s.out_indices.cpu().numpy(), ref.out_indices)
        np.testing.assert_array_equal(s.src.cpu().numpy(), ref.src)
        np.testing.assert_array_equal(s.rows.cpu().numpy(), ref.rows)
        assert int(ref.rows[256 * 256:].max()) == ref.live - 1      # the last output rows come from the second round
    else:
        n_live = rows - 100
        found = rs.select(idx, 2, shape, keep, False, n_live).found
        cap = found - 100                                           # cuts inside the second round's rows
        ref = rs.select(idx, 2, shape, keep, False, n_live, cap=cap)
        assert ref.src[-1] >= 256 * 256
        s = native_build(cuda, idx, 2, shape, keep, False, n_live=n_live, cap=cap)
        check_static(s, ref, rows, cap, 3)
        np.testing.assert_array_equal(s.rows.cpu().numpy(), ref.rows)


def test_build_of_no_rows(cuda):
    shape = BUILD_SHAPES[3]
    idx, keep = np.zeros((0, 4), np.int32), np.zeros((0,), np.uint8)
    ref = rs.select(idx, 2, shape, keep)
    s = native_build(cuda, idx, 2, shape, keep, False)
    assert s.n_out == 0 and s.live_rows == 0 and tuple(s.out_indices.shape) == (0, 4) and tuple(s.rows.shape) == (0,)
    check_static(native_build(cuda, idx, 2, shape, keep, True, cap=4), ref, 0, 4, 3)
    # every row dead
    idx = np.full((300, 4), -1, np.int32)
    s = native_build(cuda, idx, 2, shape, np.ones((300,), np.uint8), False)
    assert s.n_out == 0 and s.live_rows == 0 and bool((s.rows == -1).all())


def check_static(s, ref, rows, cap, ndim):
    assert s.n_out == cap and s.live_rows is None
    assert s.n_out_dev.cpu().tolist() == [ref.found, 0, ref.live]
    out, src = s.out_indices.cpu().numpy(), s.src.cpu().numpy()
    assert out.shape == (cap, ndim + 1) and src.shape == (cap,)
    np.testing.assert_array_equal(out[:ref.live], ref.out_indices)
    np.testing.assert_array_equal(src[:ref.live], ref.src)
    assert bool((out[ref.live:] == -1).all()) and bool((src[ref.live:] == -1).all())


def tensor_of(cuda, idx, feat, shape, bs, tag):
    import spconv_amd.pytorch as spconv
    from spconv_amd.pytorch import ops
    x = spconv.SparseConvTensor(feat.to(cuda), torch.from_numpy(idx).to(cuda), shape, bs)
    if tag:
        assert ops.attach_rank_map(x.indices, bs, shape)
    return x


def test_rank_map_of_a_subset(cuda):
    import spconv_amd.pytorch as spconv
    from spconv_amd.pytorch import ops
    F = spconv.functional
    bs, shape, C = 2, [6, 14, 16], 16
    idx = rs.sorted_scene(bs, shape, 900, 21)
    feat = rc.features(idx.shape[0], C, torch.float16, 22) * 0.25
    keep = torch.from_numpy(np.random.default_rng(23).random(idx.shape[0]) < 0.5).to(cuda)
    x = tensor_of(cuda, idx, feat, shape, bs, tag=True)
    before = counts()
    out = F.sparse_select(x, keep)
    assert delta(before) == {"count": 1, "scan": 1, "scatter": 1, "map": 1}
    n_out = int(keep.sum().item())
    assert out.features.shape[0] == n_out and ops._rankmap_of(out.indices, bs, shape, n_out, 27) is not None
    torch.manual_seed(0)
    conv = spconv.SubMConv3d(C, C, 3, bias=False).to(cuda).half().eval()
    plain = spconv.SparseConvTensor(out.features, out.indices.clone(), shape, bs)
    assert ops._rankmap_of(plain.indices, bs, shape, n_out, 27) is None          # the hash build
    with torch.no_grad():
        got, want = conv(out), conv(plain)
    assert torch.equal(bits(got.features), bits(want.features))
    # the static form tags the bounded tensor; its SubM layer agrees on the live rows
    x.n_live_dev = i32(cuda, [idx.shape[0]])
    st = F.sparse_select(x, keep, static_num_out=n_out + 30)
    assert ops._rankmap_of(st.indices, bs, shape, n_out + 30, 27) is not None and int(st.n_live_dev.item()) == n_out
    with torch.no_grad():
        got = conv(st)
    assert torch.equal(bits(got.features[:n_out]), bits(want.features))
    # a shuffled input carries no map: the output is left untagged
    perm = np.random.default_rng(24).permutation(idx.shape[0])
    y = tensor_of(cuda, idx[perm], feat[perm], shape, bs, tag=False)
    before = counts()
    out = F.sparse_select(y, keep)
    assert delta(before) == {"count": 1, "scan": 1, "scatter": 1}
    assert getattr(out.indices, "_spx_rankmap", None) is None


# ---------------------------------------------------------------------------------------- features and autograd
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, torch.float32], ids=lambda d: str(d).split(".")[1])
@pytest.mark.parametrize("C", [3, 16])
def test_select_forward_and_backward(cuda, dtype, C):
    import spconv_amd.pytorch as spconv
    F = spconv.functional
    bs, shape = 2, [5, 14, 16]
    idx = rc.scene(bs, shape, 700, 31, 0)
    n = idx.shape[0]
    feat = rc.features(n, C, dtype, 32)
    feat[3, 0] = -0.0
    keep = np.random.default_rng(33).random(n) < 0.5
    keep[3] = True
    for invert in (False, True):
        ref = rs.select(idx, bs, shape, keep, invert)
        x = spconv.SparseConvTensor(feat.to(cuda).requires_grad_(True), torch.from_numpy(idx).to(cuda), shape, bs, benchmark=True)
        x.indice_dict["k"] = object()
        out = F.sparse_select(x, torch.from_numpy(keep).to(cuda), invert)
        assert out.indice_dict == {} and out.spatial_shape == shape and out.batch_size == bs and out.benchmark
        assert out.n_live_dev is None and out.grid.numel() == 0
        np.testing.assert_array_equal(out.indices.cpu().numpy(), ref.out_indices)
        assert torch.equal(bits(out.features), bits(feat[torch.from_numpy(ref.src)]))
        dout = rc.features(ref.live, C, dtype, 34)
        out.features.backward(dout.to(cuda))
        want = torch.zeros((n, C), dtype=dtype)
        want[torch.from_numpy(ref.src)] = dout
        assert torch.equal(bits(x.features.grad), bits(want))


def test_select_gradcheck_f64(cuda):
    import spconv_amd.pytorch as spconv
    bs, shape = 1, [4, 5, 6]
    idx = rc.scene(bs, shape, 40, 41, 0)
    n = idx.shape[0]
    keep = torch.from_numpy(np.random.default_rng(42).random(n) < 0.6).to(cuda)
    dev_idx = torch.from_numpy(idx).to(cuda)
    feat = rc.features(n, 3, torch.float64, 43).to(cuda).requires_grad_(True)

    def fn(f):
        return spconv.functional.sparse_select(spconv.SparseConvTensor(f, dev_idx, shape, bs), keep).features

    assert torch.autograd.gradcheck(fn, (feat,), eps=1e-6, atol=1e-9, rtol=1e-7)


def test_refusals(cuda):
    import spconv_amd.pytorch as spconv
    F = spconv.functional
    idx = torch.from_numpy(rs.sorted_scene(1, [4, 5, 6], 20, 0)).to(cuda)
    keep = torch.ones(20, dtype=torch.bool, device=cuda)
    with pytest.raises(NotImplementedError, match="float16"):
        F.sparse_select(spconv.SparseConvTensor(torch.zeros((20, 4), dtype=torch.int8, device=cuda), idx, [4, 5, 6], 1), keep)
    from spconv_amd.pytorch import _select
    with pytest.raises(NotImplementedError, match="int32"):
        _select.select_build(idx.long(), 1, [4, 5, 6], keep)
    with pytest.raises(NotImplementedError, match="int32"):
        _select.topk_flags(torch.zeros(20, device=cuda), 3, None, idx.long(), 1)
    with pytest.raises(ValueError, match="one flag per row"):
        F.sparse_select(spconv.SparseConvTensor(torch.zeros((20, 4), device=cuda), idx, [4, 5, 6], 1), keep[:10])


# ---------------------------------------------------------------------------------------- prune
@pytest.fixture(scope="module")
def prune_scene():
    bs, shape, C = 2, [8, 30, 30], 16
    idx = rs.sorted_scene(bs, shape, 3000, 51)
    return bs, shape, C, idx, rc.features(idx.shape[0], C, torch.float16, 52)


def test_prune_sides_are_disjoint_and_complete(cuda, prune_scene):
    import spconv_amd.pytorch as spconv
    F = spconv.functional
    bs, shape, C, idx, feat = prune_scene
    n = idx.shape[0]
    x = tensor_of(cuda, idx, feat, shape, bs, tag=True)
    kept, dropped = F.sparse_prune(x, ratio=0.5, return_dropped=True)
    ref = rs.topk(rs.score(feat, "absmean"), None, 0.5)
    assert kept.features.shape[0] == n // 2 and dropped.features.shape[0] == n - n // 2
    np.testing.assert_array_equal(kept.indices.cpu().numpy(), idx[ref.keep != 0])
    np.testing.assert_array_equal(dropped.indices.cpu().numpy(), idx[ref.keep == 0])
    assert torch.equal(bits(kept.features), bits(feat[torch.from_numpy(ref.keep != 0)]))
    both = F.sparse_add(kept, dropped)
    np.testing.assert_array_equal(both.indices.cpu().numpy(), idx)
    assert torch.equal(bits(both.features), bits(feat))
    # score = "absmax", and a tensor of one value per row
    ref = rs.topk(rs.score(feat, "absmax"), 700)
    np.testing.assert_array_equal(F.sparse_prune(x, k=700, score="absmax").indices.cpu().numpy(), idx[ref.keep != 0])
    pred = rs.scores("normal", n, 53)
    ref = rs.topk(pred, None, 0.25)
    got = F.sparse_prune(x, ratio=0.25, score=torch.from_numpy(pred).to(cuda).reshape(n, 1).requires_grad_(True))
    np.testing.assert_array_equal(got.indices.cpu().numpy(), idx[ref.keep != 0])


def test_module_between_two_subm_layers_equals_the_torch_composite(cuda, prune_scene):
    import spconv_amd.pytorch as spconv
    bs, shape, C, idx, feat = prune_scene
    n = idx.shape[0]
    torch.manual_seed(3)
    net = spconv.SparseSequential(spconv.SubMConv3d(C, C, 3, bias=False, indice_key="a"), spconv.SparsePrune(ratio=0.5),
                                  spconv.SubMConv3d(C, C, 3, bias=False, indice_key="b")).to(cuda).half().eval()
    with torch.no_grad():
        mid = net[0](tensor_of(cuda, idx, feat * 0.25, shape, bs, tag=False))
        # the composite's selection is the native one only for scores without ties: the threshold's neighbours differ by
        # more than both evaluations can err
        s64 = rs.score_f64(mid.features.cpu(), "absmean")
        order = np.argsort(-s64, kind="stable")
        gap = s64[order[n // 2 - 1]] - s64[order[n // 2]]
        assert gap > 4 * (C + 2) * 2.0 ** -24 * s64[order[n // 2 - 1]]
        score = mid.features.abs().float().mean(1)
        mask = torch.zeros(n, dtype=torch.bool, device=cuda)
        mask[torch.topk(score, n // 2).indices] = True
        want = net[2](spconv.SparseConvTensor(mid.features[mask], mid.indices[mask], shape, bs))
        for tag in (False, True):                                   # hash-table and rank-map rulebooks behind the prune
            got = net(tensor_of(cuda, idx, feat * 0.25, shape, bs, tag=tag))
            assert torch.equal(got.indices, want.indices)
            assert torch.equal(bits(got.features), bits(want.features))


# ---------------------------------------------------------------------------------------- capture
def test_prune_and_subm_are_captured_in_one_graph(cuda):
    import spconv_amd.pytorch as spconv
    from spconv_amd.pytorch import ops
    F = spconv.functional
    bs, shape, C, cap = 2, [6, 14, 16], 16, 4096
    scenes = []
    for s in range(2):
        idx = rs.sorted_scene(bs, shape, 700 + 300 * s, 60 + s)
        scenes.append((idx, rc.features(idx.shape[0], C, torch.float16, 62 + s) * 0.25))
    idx_buf = torch.full((cap, 4), -1, dtype=torch.int32, device=cuda)
    feat_buf = torch.zeros((cap, C), dtype=torch.float16, device=cuda)
    live = torch.zeros((1,), dtype=torch.int32, device=cuda)
    torch.manual_seed(1)
    conv = spconv.SubMConv3d(C, C, 3, bias=False).to(cuda).half().eval()
    owner = spconv.SparsePrune(ratio=0.5)

    def load(idx, feat):
        n = idx.shape[0]
        idx_buf.fill_(-1)
        feat_buf.zero_()
        idx_buf[:n].copy_(torch.from_numpy(idx))
        feat_buf[:n].copy_(feat)
        live.fill_(n)

    def forward():
        x = spconv.SparseConvTensor(feat_buf, idx_buf, shape, bs)
        x.n_live_dev = live
        ops.attach_rank_map(idx_buf, bs, shape, check=False)        # the scenes are in key order
        mid = owner(x)
        return mid, conv(mid)

    eager = []
    with torch.no_grad():
        for idx, feat in scenes:
            m = F.sparse_prune(spconv.SparseConvTensor(feat.to(cuda), torch.from_numpy(idx).to(cuda), shape, bs), ratio=0.5)
            eager.append((m.indices.clone(), m.features.clone(), conv(m).features.clone()))
    load(*scenes[0])
    side = torch.cuda.Stream(device=cuda)
    side.wait_stream(torch.cuda.current_stream(cuda))
    with torch.cuda.stream(side), torch.no_grad():
        forward()
    torch.cuda.current_stream(cuda).wait_stream(side)
    torch.cuda.synchronize(cuda)
    graph = torch.cuda.CUDAGraph()
    with torch.no_grad(), torch.cuda.graph(graph):              # one stream, no forked branches
        mid, out = forward()
    assert mid.features.shape[0] == cap // 2                        # the bound that follows from the ratio
    assert ops._rankmap_of(mid.indices, bs, shape, cap // 2, 27) is not None
    for s in (1, 0, 1):
        load(*scenes[s])
        graph.replay()
        e_idx, e_mid, e_out = eager[s]
        n = int(mid.n_live_dev.item())
        assert n == e_idx.shape[0] == scenes[s][0].shape[0] // 2
        assert owner._static_n_out_dev.cpu().tolist() == [n, 0, n]
        assert torch.equal(mid.indices[:n], e_idx) and bool((mid.indices[n:] == -1).all())
        assert torch.equal(bits(mid.features[:n]), bits(e_mid)) and not bool(mid.features[n:].any())
        assert torch.equal(bits(out.features[:n]), bits(e_out))


class Pruned(torch.nn.Module):
    """a SubM layer, the prune, a SubM layer"""

    def __init__(self, C, static_num_out=None):
        super().__init__()
        import spconv_amd.pytorch as spconv
        self.conv0 = spconv.SubMConv3d(C, C, 3, bias=False, indice_key="s0")
        self.prune = spconv.SparsePrune(ratio=0.5, static_num_out=static_num_out)
        self.head = spconv.SubMConv3d(C, C, 3, bias=False, indice_key="h0")

    def forward(self, x):
        return self.head(self.prune(self.conv0(x)))


def test_bounded_module_under_static_inference(cuda):
    import spconv_amd.pytorch as spconv
    from spconv_amd.pytorch.static import StaticInference
    bs, shape, C = 2, [6, 14, 16], 16
    idx = rs.sorted_scene(bs, shape, 400, 91)                       # distinct, in key order: the entry sort moves nothing
    found = idx.shape[0] // 2
    feat = (rc.features(idx.shape[0], C, torch.float16, 92) * 0.25).to(cuda)
    dev_idx = torch.from_numpy(idx).to(cuda)
    torch.manual_seed(2)
    net = Pruned(C).to(cuda).half().eval()
    with torch.no_grad():
        eager = net(spconv.SparseConvTensor(feat, dev_idx, shape, bs))
    assert eager.features.shape[0] == found
    for bound, over in ((found + 20, {}), (found - 7, {"prune": found})):
        net.prune.static_num_out = bound
        runner = StaticInference(net, max_voxels=idx.shape[0] + 50, in_channels=C, spatial_shape=shape, batch_size=bs,
                                 dtype=torch.float16)
        try:
            out = runner(feat, dev_idx)
            live = min(found, bound)
            assert int(out.n_live_dev.item()) == live
            assert runner.counts()["prune"][0] == found and runner.bounds["prune"] == bound
            assert runner.overflowed() == over
            assert torch.equal(out.indices[:live], eager.indices[:live])
            if not over:
                assert torch.equal(bits(out.features[:live]), bits(eager.features))
        finally:
            runner.release_bounds()
