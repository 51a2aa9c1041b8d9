"""Voxel query and neighbour grouping on the kernels of csrc/query.hip (spconv_amd/pytorch/_query.py,
spatial.VoxelQueryAndGroup) against the numpy restatement tests/refquery.py, over the scenes of tests/queryscenes.py
(whose conditions test_refquery.py asserts on the CPU).

Every comparison is bit for bit: the rows and counts are integers, the offsets float32 arithmetic in which numpy rounds
every operation on its own (the contract), the forward moves rows unchanged, and the gradient is a sequential float32
(float64) sum in ascending entry that numpy reproduces; torch's CPU cast is the one round-to-nearest-even into float16 /
bfloat16.  The one tolerance is gradcheck's own, in float64."""
import numpy as np
import pytest
import torch

import queryscenes as qs
import refquery as rq

pytestmark = pytest.mark.gpu

DTYPES = {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32, "f64": torch.float64}
CONFIGS = [(name, radius) for name in qs.CASES for radius in qs.CASES[name]["radii"]]
B, M = qs.B, qs.M


def bits(t):
    t = t.detach().cpu().contiguous()
    return t.view({1: torch.int8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()]).numpy()


def tensor_of(cuda, idx, shape, C=4, dtype=torch.float32, n_live=None, ranked=False, seed=0):
    """a SparseConvTensor over `idx`; ranked: a rank map is built from all rows (and vouched for)"""
    import spconv_amd.pytorch as spconv
    from spconv_amd import _lib
    from spconv_amd.pytorch import _rulebook
    didx = torch.from_numpy(np.ascontiguousarray(idx)).to(cuda)
    if ranked:
        L, sp = _lib.load(), _lib.ints(shape)
        nbytes = int(L.spx_rankmap_bytes(len(shape), B, sp))
        cells = torch.empty((nbytes // 4,), dtype=torch.int32, device=cuda)
        bad = torch.zeros((1,), dtype=torch.int32, device=cuda)
        _lib.check(L.spx_rankmap_from_sorted(didx.data_ptr(), int(didx.shape[0]), len(shape), B, sp, cells.data_ptr(),
                                             nbytes, bad.data_ptr(), _rulebook._stream(didx)))
        assert int(bad.item()) == 0                     # the rows are in ascending, unique key order
        _rulebook._tag_rank_map(didx, cells, B, shape, int(didx.shape[0]))
    g = torch.Generator().manual_seed(seed)
    feat = torch.randn((idx.shape[0], C), generator=g, dtype=torch.float64).to(dtype).to(cuda)
    x = spconv.SparseConvTensor(feat, didx, shape, B)
    if n_live is not None:
        x.n_live_dev = torch.tensor([n_live], dtype=torch.int32, device=cuda)
    return x


def run_query(cuda, sc, x, radius=None, pad="none", n_queries=None, with_groups=False, pts=None, bid=None):
    from spconv_amd.pytorch import functional as F
    pts = sc.pts if pts is None else pts
    bid = sc.bid if bid is None else bid
    nq = None if n_queries is None else torch.tensor([n_queries], dtype=torch.int32, device=cuda)
    return F.voxel_query(torch.from_numpy(pts).to(cuda), torch.from_numpy(bid).to(cuda), x, sc.vs, sc.range, sc.qrange,
                         sc.nsample, radius, pad, True, nq, with_groups)


def assert_neighbors(nb, want):
    rows, count, offsets = want[:3]
    assert nb.rows.dtype == torch.int32 and nb.count.dtype == torch.int32 and nb.offsets.dtype == torch.float32
    np.testing.assert_array_equal(nb.count.cpu().numpy(), count)
    np.testing.assert_array_equal(nb.rows.cpu().numpy(), rows)
    np.testing.assert_array_equal(bits(nb.offsets), offsets.view(np.int32))


# ------------------------------------------------------------------------------------------------ query

@pytest.mark.parametrize("pad", ["none", "first"])
@pytest.mark.parametrize("form", ["rank", "hash"])
@pytest.mark.parametrize("name,radius", CONFIGS)
def test_query_bit_for_bit(cuda, name, radius, form, pad):
    from spconv_amd import _lib
    sc = qs.scene(name)
    x = tensor_of(cuda, sc.level, sc.shape, ranked=form == "rank")
    key = b"query/ranked" if form == "rank" else b"query/hash"
    before = _lib.load().spx_launch_count(key)
    nb = run_query(cuda, sc, x, radius, pad)
    assert _lib.load().spx_launch_count(key) == before + 1
    assert nb.groups is None and nb.num_voxels == sc.n
    assert tuple(nb.rows.shape) == (M, sc.nsample) and tuple(nb.offsets.shape) == (M, sc.nsample, sc.ndim)
    assert_neighbors(nb, sc.ref(radius, pad))
    from spconv_amd.pytorch import functional as F
    plain = F.voxel_query(torch.from_numpy(sc.pts).to(cuda), torch.from_numpy(sc.bid).to(cuda), x, sc.vs, sc.range,
                          sc.qrange, sc.nsample, radius, pad)                   # (offsets only on request)
    assert plain.offsets is None and torch.equal(plain.rows, nb.rows) and torch.equal(plain.count, nb.count)


@pytest.mark.parametrize("name,radius", CONFIGS)
def test_rank_and_hash_forms_agree_on_a_key_ordered_level(cuda, name, radius):
    sc = qs.scene(name)
    ranked = run_query(cuda, sc, tensor_of(cuda, sc.level, sc.shape, ranked=True), radius, "first")
    hashed = run_query(cuda, sc, tensor_of(cuda, sc.level, sc.shape), radius, "first")
    assert torch.equal(ranked.rows, hashed.rows) and torch.equal(ranked.count, hashed.count)
    assert torch.equal(ranked.offsets.view(torch.int32), hashed.offsets.view(torch.int32))
    assert int((ranked.count > 0).sum()) > 2000


@pytest.mark.parametrize("name,radius", CONFIGS)
def test_hash_form_on_a_row_shuffled_level(cuda, name, radius):
    sc = qs.scene(name)
    perm = np.random.default_rng(31).permutation(sc.n)
    inverse = np.empty(sc.n, dtype=np.int64)
    inverse[perm] = np.arange(sc.n)
    rows, count, offsets = sc.ref(radius)[:3]
    want_rows = np.where(rows >= 0, inverse[np.clip(rows, 0, None)], -1).astype(np.int32)
    shuffled = sc.level[perm]
    nb = run_query(cuda, sc, tensor_of(cuda, shuffled, sc.shape), radius)
    assert_neighbors(nb, (want_rows, count, offsets))
    got = nb.rows.cpu().numpy()
    keys = np.where(got >= 0, rq.keys_of(shuffled, sc.shape)[np.clip(got, 0, None)], np.iinfo(np.int64).max)
    assert (np.diff(keys, axis=1) >= 0).all() and (np.diff(keys, axis=1)[got[:, 1:] >= 0] > 0).all()     # ascending key
    # a coordinate that occurs twice goes to the lowest row: every row again, in another order, behind the first set
    twice = np.concatenate([shuffled, sc.level[np.random.default_rng(32).permutation(sc.n)]])
    assert_neighbors(run_query(cuda, sc, tensor_of(cuda, twice, sc.shape), radius), (want_rows, count, offsets))


@pytest.mark.parametrize("form", ["rank", "hash"])
@pytest.mark.parametrize("name,radius", CONFIGS)
def test_device_query_count_and_live_count(cuda, name, radius, form):
    sc = qs.scene(name)
    x = tensor_of(cuda, sc.level, sc.shape, ranked=form == "rank")
    nb = run_query(cuda, sc, x, radius, "first", n_queries=sc.n_queries)
    assert_neighbors(nb, sc.ref(radius, "first", None, sc.n_queries))
    assert bool((nb.rows[sc.n_queries:] == -1).all()) and bool((nb.count[sc.n_queries:] == 0).all())
    assert nb.n_queries is not None and nb.n_live is None
    x = tensor_of(cuda, sc.level, sc.shape, ranked=form == "rank", n_live=sc.n_live)         # 100 dead rows
    nb = run_query(cuda, sc, x, radius, "first")
    assert_neighbors(nb, sc.ref(radius, "first", sc.n_live))
    assert int(nb.rows.max()) < sc.n_live and nb.n_live is x.n_live_dev


@pytest.mark.parametrize("form", ["rank", "hash"])
@pytest.mark.parametrize("name,radius", [("A", 0.5), ("D", None), ("E", 1.0), ("2D", None)])
def test_the_result_does_not_depend_on_the_group_width(cuda, name, radius, form):
    from spconv_amd.pytorch import _query
    sc = qs.scene(name)
    x = tensor_of(cuda, sc.level, sc.shape, ranked=form == "rank", n_live=sc.n_live)
    want = sc.ref(radius, "first", sc.n_live)
    ndim, vsize, crange = _query._geometry(sc.vs, sc.range)
    queries, bid = torch.from_numpy(sc.pts).to(cuda), torch.from_numpy(sc.bid).to(cuda)
    rankmap = _query.level_rankmap(x.indices, B, sc.shape)
    assert (rankmap is not None) == (form == "rank")
    ws = None if form == "rank" else _query._ws(_query.query_ws_bytes(M, sc.nsample, ndim, sc.n, False), cuda)
    for width in (1, 2, 4, 8, 16, 32, 64):
        rows = torch.full((M, sc.nsample), -7, dtype=torch.int32, device=cuda)
        count = torch.full((M,), -7, dtype=torch.int32, device=cuda)
        offsets = torch.full((M, sc.nsample, ndim), float("nan"), device=cuda)
        _query.voxel_query_into(queries, bid, None, _query._floats(vsize), _query._floats(crange), x.indices, x.n_live_dev,
                                B, sc.shape, rankmap, sc.qrange, sc.nsample, _query.squared_radius(radius), True, rows,
                                count, offsets, ws, group_width=width)
        assert_neighbors(_query.VoxelNeighbors(rows, count, offsets, None, sc.n), want)


@pytest.mark.parametrize("form", ["rank", "hash"])
def test_widest_window_and_nsample_one_and_128(cuda, form):
    """range 15 on every axis (31-cell runs, 29 791 cells, far beyond the grid on every side) and the ends of nsample"""
    sc = qs.scene("A")
    x = tensor_of(cuda, sc.level, sc.shape, ranked=form == "rank")
    from spconv_amd.pytorch import functional as F
    pts, bid = sc.pts[:400], sc.bid[:400]
    for qrange, nsample, radius in (((15, 15, 15), 128, None), ((15, 15, 15), 1, 1.0), ((0, 0, 0), 1, None),
                                    ((0, 0, 15), 128, None)):
        want = rq.query(pts, bid, None, sc.vs, sc.lo, sc.level, None, B, sc.shape, list(qrange), nsample, radius, "first")
        nb = F.voxel_query(torch.from_numpy(pts).to(cuda), torch.from_numpy(bid).to(cuda), x, sc.vs, sc.range, qrange,
                           nsample, radius, "first", True)
        assert_neighbors(nb, want)
        assert int((nb.count > 0).sum()) > 150


@pytest.mark.parametrize("form", ["rank", "hash"])
def test_no_queries_no_valid_query_and_an_empty_level(cuda, form):
    from spconv_amd.pytorch import functional as F
    sc = qs.scene("A")
    x = tensor_of(cuda, sc.level, sc.shape, ranked=form == "rank")
    none = run_query(cuda, sc, x, None, "first", with_groups=True, pts=sc.pts[:0], bid=sc.bid[:0])
    assert tuple(none.rows.shape) == (0, sc.nsample) and tuple(none.count.shape) == (0,) and none.groups is None
    assert tuple(F.group_voxels(x.features, none).shape) == (0, sc.nsample, 4)
    for pts, bid, nq in ((sc.pts, sc.bid, 0), (sc.pts + np.float32(100.0), sc.bid, None),
                         (sc.pts, np.full(M, B, dtype=np.int32), None)):
        nb = run_query(cuda, sc, x, None, "first", n_queries=nq, pts=pts, bid=bid)
        assert bool((nb.rows == -1).all()) and bool((nb.count == 0).all()) and bool((nb.offsets == 0).all())
        assert bool((F.group_voxels(x.features, nb) == 0).all())
    empty = tensor_of(cuda, sc.level[:0], sc.shape)
    nb = run_query(cuda, sc, empty, None, "first")
    assert bool((nb.rows == -1).all()) and nb.num_voxels == 0
    assert bool((F.group_voxels(empty.features, nb) == 0).all())


# ------------------------------------------------------------------------------------------------ grouping

@pytest.fixture(scope="module")
def main(cuda):
    """scene A on the device: hash form, no radius, empty slots left at -1, groups built (shared, never modified)"""
    sc = qs.scene("A")
    x = tensor_of(cuda, sc.level, sc.shape)
    nb = run_query(cuda, sc, x, None, "none", with_groups=True)
    rows = sc.ref(None)[0]
    assert_neighbors(nb, sc.ref(None))
    return sc, x, nb, rows


def features(n, C, name, seed, cuda):
    g = torch.Generator().manual_seed(seed)
    host = torch.randn((n, C), generator=g, dtype=torch.float64).to(DTYPES[name])
    return host, host.to(cuda)


def raised(host, name):
    """the elements in the accumulator's type (exact)"""
    return host.double().numpy() if name == "f64" else host.float().numpy()


FWD_CASES = [(C, name) for C in (1, 3, 16, 64, 100) for name in ("f16", "bf16", "f32")] + [(3, "f64")]


@pytest.mark.parametrize("C,name", FWD_CASES)
def test_group_forward_moves_the_bits(cuda, main, C, name):
    from spconv_amd import _lib
    from spconv_amd.pytorch import functional as F
    sc, x, nb, rows = main
    host, dev = features(sc.n, C, name, 100 + C, cuda)
    host[::7] = float("nan")                                    # (moved, not computed with: payloads survive)
    dev = host.to(cuda)
    before = _lib.load().spx_launch_count(b"query/group_fwd")
    got = F.group_voxels(dev, nb)
    assert _lib.load().spx_launch_count(b"query/group_fwd") == before + 1
    assert got.dtype == DTYPES[name] and tuple(got.shape) == (M, sc.nsample, C)
    assert np.array_equal(bits(got), rq.group(bits(host), rows))
    assert int((rows < 0).sum()) > 1000 and int((rows >= 0).sum()) > 10000


@pytest.mark.parametrize("C,name", [(16, "f16"), (64, "f32"), (4, "f64"), (8, "bf16")])
def test_group_forward_from_a_misaligned_base_pointer(cuda, main, C, name):
    """rows whose bytes are a multiple of 16 but whose base is not aligned to 16: the element path"""
    from spconv_amd.pytorch import functional as F
    sc, x, nb, rows = main
    host, _ = features(sc.n, C, name, 300 + C, cuda)
    flat = torch.empty((sc.n * C + 1,), dtype=DTYPES[name], device=cuda)
    dev = flat[1:].view(sc.n, C)
    dev.copy_(host)
    assert dev.data_ptr() % 16 != 0 and dev.is_contiguous()
    assert np.array_equal(bits(F.group_voxels(dev, nb)), rq.group(bits(host), rows))


def test_transposed_list(main):
    sc, x, nb, rows = main
    offsets, lst = rq.transposed(rows, sc.n)
    g = nb.groups
    assert g.num_voxels == sc.n and tuple(g.offsets.shape) == (sc.n + 1,) and tuple(g.list.shape) == (M * sc.nsample,)
    np.testing.assert_array_equal(g.offsets.cpu().numpy(), offsets)
    np.testing.assert_array_equal(g.list.cpu().numpy()[:offsets[-1]], lst)
    sizes = np.diff(offsets)
    assert sizes.max() >= 600 and (sizes[[0, 1, sc.n - 2, sc.n - 1]] == 0).all()


BWD_CASES = [(3, "f16"), (3, "bf16"), (3, "f32"), (3, "f64"), (16, "f16"), (64, "f16"), (64, "f32"), (100, "bf16"),
             (260, "f32")]      # 260: 65 pieces, the 64 lanes of a group take a second round


@pytest.mark.parametrize("C,name", BWD_CASES)
def test_backward_bit_for_bit_and_identical_run_to_run(cuda, main, C, name):
    from spconv_amd import _lib
    from spconv_amd.pytorch import functional as F
    sc, x, nb, rows = main
    host, ddout = features(M * sc.nsample, C, name, 200 + C, cuda)
    vfeat = features(sc.n, C, name, 1, cuda)[1].requires_grad_(True)
    acc = np.float64 if name == "f64" else np.float32
    want = torch.from_numpy(rq.group_backward(raised(host, name), rows, sc.n, None, acc)).to(DTYPES[name])
    grads = []
    for _ in range(2):
        before = _lib.load().spx_launch_count(b"query/group_bwd")
        out = F.group_voxels(vfeat, nb)
        (grad,) = torch.autograd.grad(out, vfeat, ddout.view(M, sc.nsample, C))
        assert _lib.load().spx_launch_count(b"query/group_bwd") == before + 1
        grads.append(grad)
    np.testing.assert_array_equal(bits(grads[0]), bits(want))
    np.testing.assert_array_equal(bits(grads[0]), bits(grads[1]))
    assert bool((grads[0][[0, 1, sc.n - 2, sc.n - 1]] == 0).all())        # empty groups at both ends
    assert int((grads[0] != 0).any(dim=1).sum()) > 300


@pytest.mark.parametrize("C,name", [(8, "f32"), (20, "f16")])
def test_backward_with_padded_slots_and_behind_the_live_count(cuda, C, name):
    """pad = first: the repeated slots are entries of their voxel's group like any other.  Then the groups are built
    WITHOUT a live count and the backward is handed one: rows at or beyond it get zeros although their groups hold
    entries."""
    from spconv_amd.pytorch import _query
    sc = qs.scene("A")
    nb = run_query(cuda, sc, tensor_of(cuda, sc.level, sc.shape, ranked=True), None, "first", with_groups=True)
    rows = sc.ref(None, "first")[0]
    assert_neighbors(nb, sc.ref(None, "first"))
    host, ddout = features(M * sc.nsample, C, name, 400 + C, cuda)
    sizes = np.diff(nb.groups.offsets.cpu().numpy())
    assert (sizes[sc.n_live:] > 0).sum() > 30
    for n_live in (None, sc.n_live, sc.n + 5):
        count = None if n_live is None else torch.tensor([n_live], dtype=torch.int32, device=cuda)
        got = _query.group_bwd(ddout.view(M, sc.nsample, C), nb._replace(n_live=count))
        want = torch.from_numpy(rq.group_backward(raised(host, name), rows, sc.n, n_live)).to(DTYPES[name])
        np.testing.assert_array_equal(bits(got), bits(want))
        if n_live == sc.n_live:
            assert bool((got[n_live:] == 0).all())


def small_case(cuda, m=200):
    """about 60 voxels of a [4, 5, 6] grid and m queries around them, float64 features"""
    import spconv_amd.pytorch as spconv
    rng = np.random.default_rng(77)
    shape, vs, lo = [4, 5, 6], [0.3, 0.25, 0.5], [-1.0, 0.5, 2.0]
    rng_xyz = lo + [lo[j] + shape[2 - j] * vs[j] for j in range(3)]
    cells = qs.all_cells(shape)
    idx = cells[np.sort(rng.choice(len(cells), 60, replace=False))]
    v = idx[rng.integers(0, 60, m)]
    pts = ((v[:, 1:][:, ::-1] + rng.random((m, 3))) * np.array(vs) + np.array(lo)).astype(np.float32)
    didx = torch.from_numpy(idx).to(cuda)
    return (spconv, shape, vs, rng_xyz, didx, torch.from_numpy(pts).to(cuda),
            torch.from_numpy(v[:, 0].astype(np.int32)).to(cuda))


def test_gradcheck_group_voxels(cuda):
    spconv, shape, vs, rng_xyz, didx, pts, bid = small_case(cuda)
    feat = (torch.randperm(60 * 3, generator=torch.Generator().manual_seed(5)).double().reshape(60, 3) * 0.01).to(cuda)
    x = spconv.SparseConvTensor(feat, didx, shape, B)
    for pad, radius in (("none", None), ("first", 0.6)):
        nb = spconv.functional.voxel_query(pts, bid, x, vs, rng_xyz, (1, 1, 1), 6, radius, pad, with_groups=True)
        assert int((nb.rows >= 0).sum()) > 400 and int((nb.count < 6).sum()) > 10
        fn = lambda f: spconv.functional.group_voxels(f, nb)
        assert torch.autograd.gradcheck(fn, (feat.clone().requires_grad_(True),))


def test_voxel_query_and_group_module(cuda):
    import spconv_amd.pytorch as spconv
    sc = qs.scene("A")
    x = tensor_of(cuda, sc.level, sc.shape, C=16, dtype=torch.float16, ranked=True)
    x.features.requires_grad_(True)
    queries, bid = torch.from_numpy(sc.pts).to(cuda), torch.from_numpy(sc.bid).to(cuda)
    rows, count, offsets = sc.ref(0.5, "first")[:3]
    head = spconv.VoxelQueryAndGroup(sc.qrange, sc.nsample, 0.5, vsize_xyz=sc.vs, coors_range_xyz=sc.range)
    out, got_count = head(x, queries, bid)
    assert tuple(out.shape) == (M, sc.nsample, 3 + 16) and out.dtype == torch.float16
    nb = spconv.functional.voxel_query(queries, bid, x, sc.vs, sc.range, sc.qrange, sc.nsample, 0.5, "first", True)
    parts = torch.cat([nb.offsets.to(torch.float16), spconv.functional.group_voxels(x.features.detach(), nb)], dim=2)
    assert torch.equal(out.view(torch.int16), parts.view(torch.int16))
    np.testing.assert_array_equal(got_count.cpu().numpy(), count)
    want = np.concatenate([bits(torch.from_numpy(offsets).to(torch.float16)),
                           rq.group(bits(x.features), rows)], axis=2)
    assert np.array_equal(bits(out), want)
    (grad,) = torch.autograd.grad(out, x.features, torch.ones_like(out))           # every entry counts one per column
    sizes = np.diff(rq.transposed(rows, sc.n)[0]).astype(np.float32)
    np.testing.assert_array_equal(grad.float().cpu().numpy(),
                                  torch.from_numpy(np.repeat(sizes[:, None], 16, axis=1)).half().float().numpy())
    plain, _ = spconv.VoxelQueryAndGroup(sc.qrange, sc.nsample, 0.5, False, vsize_xyz=sc.vs,
                                         coors_range_xyz=sc.range)(x, queries, bid)
    assert torch.equal(plain.view(torch.int16), parts[:, :, 3:].contiguous().view(torch.int16))


# ------------------------------------------------------------------------------------------------ capture

def test_capture_query_groups_and_grouping_in_one_graph(cuda):
    """voxel_query_into + point_groups + the grouping forward and backward on ONE stream in one graph, replayed on a
    second set of queries copied into the static buffers.  The backward is the call GroupFunction.backward makes
    (group_bwd), issued by the capturing thread: the autograd engine would run it on its device thread and order it
    against the stream on which the leaf's gradient accumulator was first made -- the default stream of an earlier
    eager step -- which forks the capture onto a stream that never joins it."""
    from spconv_amd.pytorch import _query
    sc = qs.scene("A")
    x = tensor_of(cuda, sc.level, sc.shape, C=16, dtype=torch.float16, ranked=True, n_live=sc.n_live)
    ndim, vsize, crange = _query._geometry(sc.vs, sc.range)
    rankmap = _query.level_rankmap(x.indices, B, sc.shape)
    sets = [(sc.pts, sc.bid), (np.roll(sc.pts, 977, axis=0) * np.float32(0.999), np.roll(sc.bid, 977))]
    queries = torch.empty((M, 4), dtype=torch.float32, device=cuda)
    bid = torch.empty((M,), dtype=torch.int32, device=cuda)
    rows = torch.empty((M, sc.nsample), dtype=torch.int32, device=cuda)
    count = torch.empty((M,), dtype=torch.int32, device=cuda)
    offsets = torch.empty((M, sc.nsample, ndim), dtype=torch.float32, device=cuda)
    vfeat = x.features.detach().clone()
    dout = features(M * sc.nsample, 16, "f16", 9, cuda)[1].view(M, sc.nsample, 16)

    def step():
        _query.voxel_query_into(queries, bid, None, _query._floats(vsize), _query._floats(crange), x.indices, x.n_live_dev,
                                B, sc.shape, rankmap, sc.qrange, sc.nsample, _query.squared_radius(0.5), False, rows, count,
                                offsets, None)
        nb = _query.VoxelNeighbors(rows, count, offsets, _query.neighbor_groups(rows, sc.n, x.n_live_dev), sc.n, None,
                                   x.n_live_dev)
        return _query.group_voxels(vfeat, nb), _query.group_bwd(dout, nb)

    def load(k):
        queries.copy_(torch.from_numpy(sets[k][0]))
        bid.copy_(torch.from_numpy(sets[k][1]))
    eager = []
    for k in (0, 1):
        load(k)
        out, grad = step()
        want = rq.query(sets[k][0], sets[k][1], None, sc.vs, sc.lo, sc.level, sc.n_live, B, sc.shape, sc.qrange,
                        sc.nsample, 0.5)
        assert_neighbors(_query.VoxelNeighbors(rows, count, offsets, None, sc.n), want)
        eager.append((rows.clone(), count.clone(), offsets.clone(), out.clone(), grad.clone()))
    assert not torch.equal(eager[0][0], eager[1][0])
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out, grad = step()
    for k in (1, 0, 1):
        load(k)
        graph.replay()
        torch.cuda.synchronize()
        for got, want in zip((rows, count, offsets, out, grad), eager[k]):
            np.testing.assert_array_equal(bits(got), bits(want))
