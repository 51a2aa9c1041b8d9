"""Trilinear devoxelisation on the kernels of csrc/interp.hip (spconv_amd/pytorch/_interp.py, spatial.TrilinearDevoxelize,
StaticPointToVoxel.point_corners) against the numpy restatement tests/refinterp.py.

Bit for bit: the corner rows and weights (numpy float32 arithmetic rounds every multiply, add, subtract and divide on
its own, which is the contract), the forward (a sequential float32 sum in ascending corner index; torch's CPU cast is the
one round-to-nearest-even into float16 / bfloat16) and the gradient in the voxel rows (a sequential sum over the
transposed corner list, entry by entry).

The forward is also held to an independent float64 composite.  The bound is written down here, not measured: with
S = sum_c |w_c x_c| of a point's K corners, each product carries one fp32 rounding (2^-24 of its magnitude) and each of
the K additions one more on a partial sum no larger than S, so the accumulator is within (K + 1) 2^-24 S of the exact
sum (first order); the rounding into the output type adds half an ulp of the stored value:
2^-(m + 1) (|exact| + accumulator error) for m mantissa bits, or half the smallest subnormal."""
import functools

import numpy as np
import pytest
import torch

import refinterp as ri

pytestmark = pytest.mark.gpu

DTYPES = {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32, "f64": torch.float64}
MANT = {"f16": (10, 2.0 ** -24), "bf16": (7, 2.0 ** -133), "f32": (23, 2.0 ** -149)}     # mantissa bits, least subnormal
GRID3, B, VS, LO3 = [8, 20, 24], 2, 0.3, [-1.7, 2.3, 0.4]      # zyx extents; the lower bound (xyz) is not zero
N, NV, LONG_RUN = 5000, 700, (1850, 2250)                       # points, live voxels, the run of points in one voxel
N_TAIL = 300                                                    # rows behind the device point count
LONG_CELL = [1, 4, 10, 12]                                      # (batch, zyx) of the voxel that holds 600 points


def bits(t):
    t = t.detach().cpu().contiguous()
    return t.view({1: torch.int8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()]).numpy()


def geometry(ndim):
    shape = GRID3[3 - ndim:]
    lo = LO3[:ndim]
    hi = [lo[j] + shape[ndim - 1 - j] * VS for j in range(ndim)]
    return shape, [VS] * ndim, lo, lo + hi


def keys_of(idx, shape):
    key = idx[:, 0].astype(np.int64)
    for d, s in enumerate(shape):
        key = key * s + idx[:, 1 + d]
    return key


def reserved(idx, shape):
    """the two corners of the key space no point comes near: the cells around the smallest and the largest key"""
    ndim = len(shape)
    low = (idx[:, 0] == 0) & np.all(idx[:, 1:] <= np.array([1, 2, 3][3 - ndim:]), axis=1)
    high = (idx[:, 0] == B - 1) & np.all(idx[:, 1:] >= np.array(shape) - np.array([2, 3, 4][3 - ndim:]), axis=1)
    return low | high


def all_cells(shape):
    grids = np.meshgrid(np.arange(B), *[np.arange(s) for s in shape], indexing="ij")
    return np.stack([g.reshape(-1) for g in grids], axis=1).astype(np.int32)        # key order


def make_level(ndim, nv, seed, ends=True):
    """nv cells in key order; ends: the smallest and the largest two keys of the grid are among them, inside zones that
    hold no other voxel and no point (empty groups at both ends of the transposed list); so are a border cell at each
    end of every axis and the 3^ndim block around LONG_CELL (points with every corner present)"""
    shape = geometry(ndim)[0]
    cells = all_cells(shape)
    rng = np.random.default_rng(seed)
    if not ends:
        return cells[np.sort(rng.choice(len(cells), nv, replace=False))], shape
    free = np.nonzero(~reserved(cells, shape))[0]
    k = keys_of(cells, shape)
    forced = [0, 1, len(cells) - 2, len(cells) - 1]
    border = [int(np.nonzero(k == keys_of(np.array([[1] + [0] * ndim]), shape)[0])[0][0]),
              int(np.nonzero(k == keys_of(np.array([[0] + [s - 1 for s in shape]]), shape)[0])[0][0])]
    centre = np.array([LONG_CELL[0]] + LONG_CELL[4 - ndim:])
    block = np.nonzero((cells[:, 0] == centre[0]) & (np.abs(cells[:, 1:] - centre[1:]) <= 1).all(axis=1))[0]
    assert len(block) == 3 ** ndim
    fixed = np.concatenate([forced, border, block])
    pick = np.concatenate([fixed, rng.choice(np.setdiff1d(free, fixed), nv - len(fixed), replace=False)])
    return cells[np.sort(pick)], shape


def make_points(ndim, level, seed, n=N, long_cell=None):
    """points [n, 4] fp32 and batch ids [n]: jittered inside the level's voxels (never those of the reserved zones), with
    the special cases of the issue in fixed slots (n >= 800); long_cell: 600 of them inside that one voxel"""
    shape, vs, lo, _ = geometry(ndim)
    rng = np.random.default_rng(seed)
    usable = level[~reserved(level, shape)]
    v = usable[rng.integers(0, len(usable), n)]
    cell = v[:, 1:][:, ::-1].astype(np.float64)                                     # xyz
    f32 = np.float32
    pts = np.zeros((n, 4), dtype=f32)
    pts[:, :ndim] = ((cell + rng.random((n, ndim))) * VS + np.array(lo)).astype(f32)
    pts[:, ndim:] = rng.standard_normal((n, 4 - ndim)).astype(f32)                  # columns that are no coordinates
    bid = v[:, 0].astype(np.int32)
    c32, lo32 = cell.astype(f32), np.array(lo, dtype=f32)
    pts[0:200, :ndim] = (c32[0:200] + f32(0.5)) * f32(VS) + lo32                    # on voxel centres
    on_face = rng.random((200, ndim)) < 0.6
    pts[200:400, :ndim] = np.where(on_face, c32[200:400] * f32(VS) + lo32, pts[200:400, :ndim])     # on cell faces
    for s, b_, corner in ((400, 1, [0] * ndim), (450, 0, [e - 1 for e in shape[::-1]])):            # in border cells
        pts[s:s + 50, :ndim] = ((np.array(corner) + rng.random((50, ndim))) * VS + np.array(lo)).astype(f32)
        bid[s:s + 50] = b_
    ext = np.array(shape[::-1], dtype=np.float64)
    for i in range(500, 600):                                                       # outside the range, one axis each
        j = int(rng.integers(0, ndim))
        pts[i, j] = f32(lo[j] - 0.05) if i % 2 else f32(lo[j] + ext[j] * VS + 0.05)
    pts[600:610, :ndim] = lo32                                                      # exactly on the lower bound
    bid[600:610] = 1
    for i in range(610, 660):
        pts[i, int(rng.integers(0, ndim))] = np.nan
    pts[660:665, 0] = np.inf
    bid[700:750] = -1
    bid[750:800] = B
    if long_cell is not None:                                                       # 600 points in ONE voxel: a run and 200 scattered
        lo_run, hi_run = LONG_RUN
        where = np.r_[lo_run:hi_run, rng.choice(np.r_[800:lo_run, hi_run:n - N_TAIL], 200, replace=False)]
        pts[where, :ndim] = ((long_cell[1:][::-1] + rng.random((len(where), ndim))) * VS + np.array(lo)).astype(f32)
        bid[where] = long_cell[0]
    return pts, bid


class Scene:
    """the main case of one dimensionality: points, and the level in two forms -- computed once, never modified.
    `full` (hash form): the live rows in key order, six rows dead by batch index -1 (three of them below the live count),
    then GHOST rows behind the live count: coordinates that no live row holds and that many points surround, so a lookup
    that ignored the count would return them.  `ordered` (rank form): the live rows and the -1 rows; the rank map
    describes all NV rows, the live count cuts off the 40 highest keys, whose voxels points surround as well."""

    def __init__(self, ndim):
        self.ndim = ndim
        live, self.shape = make_level(ndim, NV, 10 + ndim)
        self.vs, self.lo, self.range = geometry(ndim)[1:]
        long_cell = np.array([LONG_CELL[0]] + LONG_CELL[4 - ndim:])
        self.pts, self.bid = make_points(ndim, live, 20 + ndim, long_cell=long_cell)
        self.n_points = N - N_TAIL
        self.long_row = int(np.nonzero(keys_of(live, self.shape) == keys_of(long_cell[None], self.shape)[0])[0][0])
        dead = np.full((6, ndim + 1), -1, dtype=np.int32)
        self.ghosts = self._ghosts(live)
        self.ordered = np.concatenate([live, dead])
        self.full = np.concatenate([live, dead, self.ghosts])
        self.n_live = NV + 3                                        # of `full`
        self.n_live_ordered = NV - 40                               # of `ordered`

    def _ghosts(self, live, count=8):
        """the `count` cells without a live row that are a corner of the most points (outside the reserved zones)"""
        cells = all_cells(self.shape)                               # key order: row = key
        rows, _ = ri.corners(self.pts, self.bid, self.n_points, self.vs, self.lo, cells, None, B, self.shape, False)
        keys, counts = np.unique(rows[rows >= 0], return_counts=True)
        free = ~np.isin(keys, keys_of(live, self.shape)) & ~reserved(cells[keys], self.shape)
        top = keys[free][np.argsort(-counts[free], kind="stable")[:count]]
        assert len(top) == count and counts[free].max() >= 5
        return cells[np.sort(top)]

    @functools.lru_cache(maxsize=None)
    def ref(self, normalize, full=True, honour_live=True):
        idx, n_live = (self.full, self.n_live) if full else (self.ordered, self.n_live_ordered)
        return ri.corners(self.pts, self.bid, self.n_points, self.vs, self.lo, idx, n_live if honour_live else None, B,
                          self.shape, normalize)


@functools.lru_cache(maxsize=None)
def scene(ndim):
    return Scene(ndim)


def tensor_of(cuda, idx, shape, C=4, dtype=torch.float32, n_live=None, ranked_rows=None, seed=0):
    """a SparseConvTensor over `idx`; ranked_rows: the leading rows a rank map is built from (and vouched for)"""
    import spconv_amd.pytorch as spconv
    from spconv_amd import _lib
    from spconv_amd.pytorch import _rulebook
    didx = torch.from_numpy(np.ascontiguousarray(idx)).to(cuda)
    if ranked_rows is not None:
        L, sp = _lib.load(), _lib.ints(shape)
        nbytes = int(L.spx_rankmap_bytes(len(shape), B, sp))
        cells = torch.empty((nbytes // 4,), dtype=torch.int32, device=cuda)
        bad = torch.zeros((1,), dtype=torch.int32, device=cuda)
        _lib.check(L.spx_rankmap_from_sorted(didx.data_ptr(), ranked_rows, len(shape), B, sp, cells.data_ptr(), nbytes,
                                             bad.data_ptr(), _rulebook._stream(didx)))
        assert int(bad.item()) == 0                     # the rows are in ascending, unique key order
        _rulebook._tag_rank_map(didx, cells, B, shape, int(didx.shape[0]))
    g = torch.Generator().manual_seed(seed)
    feat = torch.randn((idx.shape[0], C), generator=g, dtype=torch.float64).to(dtype).to(cuda)
    x = spconv.SparseConvTensor(feat, didx, shape, B)
    if n_live is not None:
        x.n_live_dev = torch.tensor([n_live], dtype=torch.int32, device=cuda)
    return x


def run_corners(cuda, sc, x, normalize, pts=None, bid=None, n_points="scene", with_groups=False):
    from spconv_amd.pytorch import functional as F
    pts = sc.pts if pts is None else pts
    bid = sc.bid if bid is None else bid
    if isinstance(n_points, str):
        n_points = sc.n_points
    npt = None if n_points is None else torch.tensor([n_points], dtype=torch.int32, device=cuda)
    dbid = None if bid is None else torch.from_numpy(bid).to(cuda)
    return F.point_corners(torch.from_numpy(pts).to(cuda), dbid, x, sc.vs, sc.range, normalize, npt, with_groups)


def bits_t(t):
    return t.view(torch.int32)


def assert_corners(c, rows, weights):
    assert c.rows.dtype == torch.int32 and c.weights.dtype == torch.float32
    np.testing.assert_array_equal(c.rows.cpu().numpy(), rows)
    np.testing.assert_array_equal(bits(c.weights), weights.view(np.int32))


# ------------------------------------------------------------------------------------------------ corners

def test_the_scene_holds_the_cases_it_claims():
    sc = scene(3)
    rows, w = sc.ref(True)
    assert (rows[sc.n_points:] == -1).all() and (rows[500:600] == -1).all() and (rows[610:665] == -1).all()
    assert (rows[700:800] == -1).all() and (w[rows < 0] == 0).all()
    real = rows[800:sc.n_points]
    assert ((real >= 0).sum(axis=1) == 8).sum() > 20 and ((real >= 0).sum(axis=1) < 8).sum() > 1000
    assert (rows[400:500] >= 0).any(axis=1).all() and ((rows[400:500] >= 0).sum(axis=1) <= 4).any()     # border cells
    assert rows.max() < NV and not np.isin(rows, [0, 1, NV - 2, NV - 1]).any()                          # both ends empty
    assert (rows == sc.long_row).any(axis=1).sum() >= 600
    assert (w[0:200].max(axis=1) > 0.99).all()                                                          # on centres
    for ndim in (2, 3):                     # rows behind the live count WOULD be found: ignoring the count shows
        sc = scene(ndim)
        for full, first_dead in ((True, NV + 6), (False, sc.n_live_ordered)):
            blind = sc.ref(True, full, False)[0]
            assert (blind >= first_dead).sum() > 30 and (sc.ref(True, full)[0] != blind).sum() > 30
            assert sc.ref(True, full)[0].max() < first_dead


@pytest.mark.parametrize("form", ["rank", "hash"])
@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("ndim", [2, 3])
def test_corners_bit_for_bit(cuda, ndim, normalize, form):
    from spconv_amd import _lib
    sc = scene(ndim)
    if form == "rank":
        x = tensor_of(cuda, sc.ordered, sc.shape, n_live=sc.n_live_ordered, ranked_rows=len(sc.ordered))
        key, want = b"interp/corners_ranked", sc.ref(normalize, False)
    else:
        x = tensor_of(cuda, sc.full, sc.shape, n_live=sc.n_live)
        key, want = b"interp/corners_hash", sc.ref(normalize, True)
    before = _lib.load().spx_launch_count(key)
    c = run_corners(cuda, sc, x, normalize)
    assert _lib.load().spx_launch_count(key) == before + 1
    assert c.groups is None and c.num_voxels == x.indices.shape[0] and tuple(c.rows.shape) == (N, 1 << ndim)
    assert_corners(c, *want)
    if normalize:
        w = want[1].astype(np.float64).sum(axis=1)
        assert np.abs(w[(want[0] >= 0).any(axis=1)] - 1).max() <= 2 * 2.0 ** -23


@pytest.mark.parametrize("ndim", [2, 3])
def test_rank_and_hash_forms_agree_on_a_key_ordered_level(cuda, ndim):
    sc = scene(ndim)
    ranked = run_corners(cuda, sc, tensor_of(cuda, sc.ordered, sc.shape, ranked_rows=len(sc.ordered)), True, n_points=None)
    hashed = run_corners(cuda, sc, tensor_of(cuda, sc.ordered, sc.shape), True, n_points=None)
    assert torch.equal(ranked.rows, hashed.rows) and torch.equal(bits_t(ranked.weights), bits_t(hashed.weights))
    assert int((ranked.rows >= 0).sum()) > 5000


def test_hash_form_on_permuted_rows_and_on_duplicates(cuda):
    sc = scene(3)
    rng = np.random.default_rng(31)
    live = sc.ordered[:NV]
    perm = rng.permutation(NV)
    rows_sorted, w_sorted = ri.corners(sc.pts, sc.bid, None, sc.vs, sc.lo, live, None, B, sc.shape, True)
    got = run_corners(cuda, sc, tensor_of(cuda, live[perm], sc.shape), True, n_points=None)
    inverse = np.empty(NV, dtype=np.int64)
    inverse[perm] = np.arange(NV)
    want_rows = np.where(rows_sorted >= 0, inverse[np.clip(rows_sorted, 0, None)], -1)
    assert_corners(got, want_rows.astype(np.int32), w_sorted)          # that permutation's row numbers, the same weights
    # a coordinate that occurs twice goes to the lowest row: every row of the level again, in another order, behind it
    twice = np.concatenate([live[perm], live[rng.permutation(NV)]])
    got = run_corners(cuda, sc, tensor_of(cuda, twice, sc.shape), True, n_points=None)
    assert_corners(got, want_rows.astype(np.int32), w_sorted)
    assert int(got.rows.max()) < NV
    want = ri.corners(sc.pts, sc.bid, None, sc.vs, sc.lo, twice, None, B, sc.shape, True)
    assert_corners(got, *want)


@pytest.mark.parametrize("form", ["rank", "hash"])
@pytest.mark.parametrize("nv", [1, 255, 256, 257])
def test_small_levels(cuda, nv, form):
    sc = scene(3)
    level, shape = make_level(3, nv, 40 + nv, ends=False)
    pts, bid = make_points(3, level, 50 + nv, n=1200) if nv > 1 else (None, None)
    if nv == 1:                                                 # points all around the one voxel, most of them too far away
        rng = np.random.default_rng(3)
        pts = np.zeros((1200, 4), dtype=np.float32)
        pts[:, :3] = ((level[0, 1:][::-1] + rng.uniform(-1.5, 2.5, (1200, 3))) * VS + np.array(sc.lo)).astype(np.float32)
        bid = np.full(1200, level[0, 0], dtype=np.int32)
    x = tensor_of(cuda, level, shape, ranked_rows=nv if form == "rank" else None)
    for normalize in (False, True):
        want = ri.corners(pts, bid, None, sc.vs, sc.lo, level, None, B, shape, normalize)
        assert (want[0] >= 0).sum() > 20
        assert_corners(run_corners(cuda, sc, x, normalize, pts, bid, None), *want)


@pytest.mark.parametrize("form", ["rank", "hash"])
def test_no_points_and_no_valid_point(cuda, form):
    from spconv_amd.pytorch import functional as F
    sc = scene(3)
    x = tensor_of(cuda, sc.ordered, sc.shape, ranked_rows=len(sc.ordered) if form == "rank" else None)
    none = run_corners(cuda, sc, x, True, sc.pts[:0], sc.bid[:0], None, with_groups=True)
    assert tuple(none.rows.shape) == (0, 8) and tuple(none.weights.shape) == (0, 8) and none.groups is None
    out = F.voxels_to_points_trilinear(x.features, none)
    assert tuple(out.shape) == (0, 4)
    for pts, bid, n_points in ((sc.pts, sc.bid, 0),                                      # a device count of zero
                               (sc.pts + np.float32(100.0), sc.bid, None),              # every point outside the range
                               (sc.pts, np.full(N, B, dtype=np.int32), None)):          # every batch id outside
        c = run_corners(cuda, sc, x, True, pts, bid, n_points)
        assert bool((c.rows == -1).all()) and bool((c.weights == 0).all())
        assert bool((F.voxels_to_points_trilinear(x.features, c) == 0).all())
    empty = tensor_of(cuda, sc.ordered[:0], sc.shape)                                    # a level without rows
    c = run_corners(cuda, sc, empty, True)
    assert bool((c.rows == -1).all()) and c.num_voxels == 0
    assert bool((F.voxels_to_points_trilinear(empty.features, c) == 0).all())


# ------------------------------------------------------------------------------------------------ forward

@pytest.fixture(scope="module")
def main(cuda):
    """the main 3-d case on the device: hash form over the level with dead rows, groups built (shared, never modified)"""
    sc = scene(3)
    x = tensor_of(cuda, sc.full, sc.shape, n_live=sc.n_live)
    c = run_corners(cuda, sc, x, True, with_groups=True)
    rows, w = sc.ref(True)
    assert_corners(c, rows, w)
    return sc, x, c, rows, w


def features(n, C, name, seed, cuda):
    g = torch.Generator().manual_seed(seed)
    host = torch.randn((n, C), generator=g, dtype=torch.float64).to(DTYPES[name])
    return host, host.to(cuda)


def raised(host, name):
    """the elements in the accumulator's type (exact)"""
    return host.double().numpy() if name == "f64" else host.float().numpy()


@pytest.mark.parametrize("name", ["f16", "bf16", "f32", "f64"])
@pytest.mark.parametrize("C", [1, 3, 8, 20, 64])
def test_forward_bit_for_bit(cuda, main, C, name):
    from spconv_amd import _lib
    from spconv_amd.pytorch import functional as F
    sc, x, c, rows, w = main
    host, dev = features(len(sc.full), C, name, 100 + C, cuda)
    acc = np.float64 if name == "f64" else np.float32
    want = torch.from_numpy(ri.forward(raised(host, name), rows, w, acc)).to(DTYPES[name])
    before = _lib.load().spx_launch_count(b"interp/fwd")
    got = F.voxels_to_points_trilinear(dev, c)
    assert _lib.load().spx_launch_count(b"interp/fwd") == before + 1
    assert got.dtype == DTYPES[name] and tuple(got.shape) == (N, C)
    np.testing.assert_array_equal(bits(got), bits(want))
    assert bool((got[sc.n_points:] == 0).all()) and int((got != 0).any(dim=1).sum()) > 3000


@pytest.mark.parametrize("ndim", [2, 3])
@pytest.mark.parametrize("name", ["f16", "bf16", "f32"])
def test_forward_against_a_float64_composite(cuda, ndim, name):
    from spconv_amd.pytorch import functional as F
    sc = scene(ndim)
    K, C = 1 << ndim, 20
    x = tensor_of(cuda, sc.full, sc.shape, n_live=sc.n_live)
    c = run_corners(cuda, sc, x, True)
    host, dev = features(len(sc.full), C, name, 7, cuda)
    got = F.voxels_to_points_trilinear(dev, c).double()
    rows, w = c.rows.long(), c.weights.double()                   # the composite a user would write, in float64
    terms = w.unsqueeze(2) * dev.double()[rows.clamp_min(0)] * (rows >= 0).unsqueeze(2)
    exact, mag = terms.sum(dim=1), terms.abs().sum(dim=1)
    m, least = MANT[name]
    acc_err = (K + 1) * 2.0 ** -24 * mag
    bound = acc_err + torch.clamp(2.0 ** -(m + 1) * (exact.abs() + acc_err), min=least / 2)
    excess = ((got - exact).abs() - bound).max().item()
    print(f"{name} ndim {ndim}: max |err| {(got - exact).abs().max().item():.3e}, max err / bound "
          f"{((got - exact).abs() / bound.clamp_min(1e-300)).max().item():.3f}")
    assert excess <= 0, excess


@pytest.mark.parametrize("name,C", [("f16", 20), ("f32", 64), ("bf16", 3)])
def test_forward_does_not_depend_on_the_row_order(cuda, name, C):
    from spconv_amd.pytorch import functional as F
    sc = scene(3)
    live = sc.ordered[:NV]
    perm = np.random.default_rng(9).permutation(NV)
    host, dev = features(NV, C, name, 11, cuda)
    x_key = tensor_of(cuda, live, sc.shape, ranked_rows=NV)
    x_perm = tensor_of(cuda, live[perm], sc.shape)
    out_key = F.voxels_to_points_trilinear(dev, run_corners(cuda, sc, x_key, True))
    out_perm = F.voxels_to_points_trilinear(dev[torch.from_numpy(perm).to(cuda)], run_corners(cuda, sc, x_perm, True))
    np.testing.assert_array_equal(bits(out_key), bits(out_perm))
    assert int((out_key != 0).any(dim=1).sum()) > 3000


# ------------------------------------------------------------------------------------------------ backward

def test_transposed_list(main):
    sc, x, c, rows, w = main
    n = len(sc.full)
    offsets, lst = ri.transposed(rows, n)
    g = c.groups
    assert g.num_voxels == n and tuple(g.offsets.shape) == (n + 1,) and tuple(g.list.shape) == (N * 8,)
    np.testing.assert_array_equal(g.offsets.cpu().numpy(), offsets)
    np.testing.assert_array_equal(g.list.cpu().numpy()[:offsets[-1]], lst)
    sizes = np.diff(offsets)
    assert sizes[sc.long_row] >= 600 and (sizes[[0, 1, NV - 2, NV - 1]] == 0).all() and (sizes[NV:] == 0).all()
    group = lst[offsets[sc.long_row]:offsets[sc.long_row + 1]]
    assert group[0] // 2048 != group[-1] // 2048                     # the group's entries come from several sort blocks


BWD_CASES = [(C, name) for C in (3, 8) for name in ("f16", "bf16", "f32", "f64")] + [
    (64, "f32"),        # 16 pieces: a group of 16 lanes
    (64, "f16"),        # 8 pieces
    (260, "f32"),       # 65 pieces: the 64 lanes of a group take a second round
    (67, "f16"),        # the element path, 67 > 64 elements: a second round as well
    (20, "bf16")]       # the element path (40 bytes)


@pytest.mark.parametrize("C,name", BWD_CASES)
def test_backward_bit_for_bit_and_identical_run_to_run(cuda, main, C, name):
    from spconv_amd import _lib
    from spconv_amd.pytorch import functional as F
    sc, x, c, rows, w = main
    n = len(sc.full)
    host, ddout = features(N, C, name, 200 + C, cuda)
    vfeat = features(n, C, name, 1, cuda)[1].requires_grad_(True)
    acc = np.float64 if name == "f64" else np.float32
    want = torch.from_numpy(ri.backward(raised(host, name), rows, w, n, sc.n_live, acc)).to(DTYPES[name])
    grads = []
    for _ in range(2):
        before = _lib.load().spx_launch_count(b"interp/bwd")
        out = F.voxels_to_points_trilinear(vfeat, c)
        (grad,) = torch.autograd.grad(out, vfeat, ddout)
        assert _lib.load().spx_launch_count(b"interp/bwd") == before + 1
        grads.append(grad)
    np.testing.assert_array_equal(bits(grads[0]), bits(want))
    np.testing.assert_array_equal(bits(grads[0]), bits(grads[1]))
    assert bool((grads[0][[0, 1, NV - 2, NV - 1]] == 0).all())        # empty voxels at both ends
    assert bool((grads[0][NV:] == 0).all())                           # dead rows: batch index -1, past the live count
    assert bool((grads[0][sc.long_row] != 0).all())


def group_lengths_table():
    """a corner table of 24 points over 10 voxels in which voxel v is a corner of exactly v points (v = 0 .. 9), the
    corners of a point all different voxels, the other slots empty"""
    n, N, K = 10, 24, 8
    rows = np.full((N, K), -1, np.int32)
    used = np.zeros(N, np.int64)
    for v in range(n):
        for t in range(v):
            i = (3 * v + t) % N
            rows[i, used[i]] = v
            used[i] += 1
    w = np.random.default_rng(12).random((N, K)).astype(np.float32) * (rows >= 0)
    assert np.diff(ri.transposed(rows, n)[0]).tolist() == list(range(n))
    return n, rows, w


@pytest.mark.parametrize("C", [3, 8])
@pytest.mark.parametrize("name", ["f16", "f32"])
def test_backward_every_group_length_0_to_9(cuda, name, C):
    """the walk fetches four list entries at a time: every group length from 0 to 9 crosses each of its boundaries
    (an empty group, a partial first round, exactly one and two rounds, a partial last round)"""
    from spconv_amd.pytorch import _interp
    n, rows, w = group_lengths_table()
    dev_rows = torch.from_numpy(rows).to(cuda)
    groups = _interp.corner_groups(dev_rows, n)
    np.testing.assert_array_equal(groups.offsets.cpu().numpy(), ri.transposed(rows, n)[0])
    c = _interp.PointCorners(dev_rows, torch.from_numpy(w).to(cuda), groups, n)
    host, ddout = features(rows.shape[0], C, name, 400 + C, cuda)
    got = _interp.interp_bwd(ddout, c)
    want = torch.from_numpy(ri.backward(raised(host, name), rows, w, n)).to(DTYPES[name])
    np.testing.assert_array_equal(bits(got), bits(want))
    assert bool((got[0] == 0).all()) and bool((got[1:] != 0).any(dim=1).all())


@pytest.mark.parametrize("name,C", [("f32", 8), ("f16", 20)])
def test_backward_gives_zeros_to_rows_behind_the_live_count_whose_groups_are_not_empty(cuda, name, C):
    """corners and groups built WITHOUT a live count find the ghost rows; the backward is then handed a count"""
    from spconv_amd.pytorch import _interp
    sc = scene(3)
    n = len(sc.full)
    blind = run_corners(cuda, sc, tensor_of(cuda, sc.full, sc.shape), True, with_groups=True)
    rows, w = sc.ref(True, True, False)
    assert_corners(blind, rows, w)
    sizes = np.diff(blind.groups.offsets.cpu().numpy())
    assert (sizes[NV + 6:] >= 5).all() and sizes[sc.n_live - 1] == 0          # ghost groups hold entries
    host, ddout = features(N, C, name, 300 + C, cuda)
    acc = np.float32
    for n_live in (sc.n_live, NV + 8, None):
        dev_count = None if n_live is None else torch.tensor([n_live], dtype=torch.int32, device=cuda)
        got = _interp.interp_bwd(ddout, blind._replace(n_live=dev_count))
        want = torch.from_numpy(ri.backward(raised(host, name), rows, w, n, n_live, acc)).to(DTYPES[name])
        np.testing.assert_array_equal(bits(got), bits(want))
        first_dead = n if n_live is None else n_live
        assert bool((got[first_dead:] == 0).all()) and bool((got[NV + 6:first_dead] != 0).any(dim=1).all())


def test_backward_needs_groups(cuda, main):
    from spconv_amd.pytorch import functional as F
    sc, x, c, rows, w = main
    vfeat = x.features.clone().requires_grad_(True)
    with pytest.raises(ValueError, match="with_groups"):
        F.voxels_to_points_trilinear(vfeat, c._replace(groups=None))
    with pytest.raises(ValueError, match="one row per voxel"):
        F.voxels_to_points_trilinear(vfeat[:5], c)
    with pytest.raises(NotImplementedError, match="float16, bfloat16, float32 or float64"):
        F.voxels_to_points_trilinear(vfeat.detach().to(torch.int32), c)


def small_case(cuda):
    """about 30 voxels of a [4, 5, 6] grid and 40 points around them, float64 features"""
    import spconv_amd.pytorch as spconv
    rng = np.random.default_rng(77)
    shape, vs, lo = [4, 5, 6], [0.3, 0.25, 0.5], [-1.0, 0.5, 2.0]
    rng_xyz = lo + [lo[j] + shape[2 - j] * vs[j] for j in range(3)]
    cells = all_cells(shape)
    idx = cells[np.sort(rng.choice(len(cells), 30, replace=False))]
    v = idx[rng.integers(0, 30, 40)]
    pts = ((v[:, 1:][:, ::-1] + rng.random((40, 3))) * np.array(vs) + np.array(lo)).astype(np.float32)
    didx = torch.from_numpy(idx).to(cuda)
    return (spconv, shape, vs, rng_xyz, didx, torch.from_numpy(pts).to(cuda),
            torch.from_numpy(v[:, 0].astype(np.int32)).to(cuda))


def test_gradcheck_voxels_to_points_trilinear(cuda):
    spconv, shape, vs, rng_xyz, didx, pts, bid = small_case(cuda)
    feat = (torch.randperm(30 * 3, generator=torch.Generator().manual_seed(5)).double().reshape(30, 3) * 0.01).to(cuda)
    x = spconv.SparseConvTensor(feat, didx, shape, B)
    for normalize in (False, True):
        c = spconv.functional.point_corners(pts, bid, x, vs, rng_xyz, normalize, with_groups=True)
        assert int((c.rows >= 0).sum()) > 60
        fn = lambda f: spconv.functional.voxels_to_points_trilinear(f, c)
        assert torch.autograd.gradcheck(fn, (feat.clone().requires_grad_(True),), eps=1e-6, atol=1e-9, rtol=1e-7)


def test_gradcheck_module_behind_a_subm_layer(cuda):
    spconv, shape, vs, rng_xyz, didx, pts, bid = small_case(cuda)
    torch.manual_seed(3)
    conv = spconv.SubMConv3d(3, 4, 3, bias=True).to(cuda).double()
    head = spconv.TrilinearDevoxelize(vs, rng_xyz)
    feat = torch.randn((30, 3), dtype=torch.float64, device=cuda)
    names = [n for n, _ in conv.named_parameters()]
    params = [p.detach().clone().requires_grad_(True) for _, p in conv.named_parameters()]

    def f(features, *values):
        y = torch.func.functional_call(conv, dict(zip(names, values)), (spconv.SparseConvTensor(features, didx, shape, B),))
        return head(y, pts, bid)
    out = f(feat, *params)
    assert tuple(out.shape) == (40, 4) and int((out != 0).any(dim=1).sum()) == 40
    assert torch.autograd.gradcheck(f, [feat.clone().requires_grad_(True)] + params, eps=1e-6, atol=1e-6)


# ------------------------------------------------------------------------------------------------ capture

def cloud(n, seed):
    rng = np.random.default_rng(seed)
    xyz = rng.uniform([-0.5, 0, 0], [16.5, 16, 8], (n, 3))                   # (a few points outside the range)
    return torch.from_numpy(np.concatenate([xyz, rng.uniform(0, 1, (n, 1))], axis=1).astype(np.float32))


def test_capture_voxeliser_corners_subm_and_interpolation_in_one_graph(cuda):
    import spconv_amd.pytorch as spconv
    from spconv_amd.pytorch.utils import StaticPointToVoxel
    vsize, crange, grid = [0.5, 0.5, 0.5], [0.0, 0.0, 0.0, 16.0, 16.0, 8.0], [16, 32, 32]
    gen = StaticPointToVoxel(vsize, crange, 4, 4000, 5, 3000, key_order=True, mean_dtype=torch.float16, keep_voxels=False,
                             device=cuda)
    torch.manual_seed(0)
    conv = spconv.SubMConv3d(4, 16, 3).to(cuda).half().eval()
    scenes = [cloud(3000, 1).to(cuda), cloud(1200, 2).to(cuda)]

    def head():
        gen.run()
        corners = gen.point_corners()
        x = spconv.SparseConvTensor(gen.mean, gen.indices, grid, 1)
        x.n_live_dev = gen.n_voxels[0:1]
        return corners, spconv.functional.voxels_to_points_trilinear(conv(x).features, corners)
    eager = []
    with torch.no_grad():
        for pc in scenes:
            gen.load(pc)
            corners, out = head()
            nv, n = int(gen.n_voxels[0]), pc.shape[0]
            assert corners.n_points is gen.n_points and corners.groups is None
            # the corners against the reference, over the voxeliser's own level
            want = ri.corners(pc.cpu().numpy(), None, None, vsize, crange[:3], gen.indices[:nv].cpu().numpy(), None, 1, grid)
            assert_corners(corners._replace(rows=corners.rows[:n], weights=corners.weights[:n]), *want)
            assert bool((corners.rows[n:] == -1).all()) and bool((out[n:] == 0).all())
            eager.append((out.clone(), corners.rows.clone(), nv))
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            corners, out = head()
    assert eager[0][2] > eager[1][2] > 500 and int((eager[1][0] != 0).any(dim=1).sum()) > 1000
    for k in (0, 1, 0):               # the 1200-point scene finds the 3000-point scene's rows behind its counts
        gen.load(scenes[k])
        graph.replay()
        torch.cuda.synchronize()
        want, want_rows, nv = eager[k]
        assert int(gen.n_voxels[0]) == nv
        assert torch.equal(corners.rows, want_rows)
        np.testing.assert_array_equal(bits(out), bits(want))


def test_static_corners_with_groups_feed_a_gradient(cuda):
    import spconv_amd.pytorch as spconv
    from spconv_amd.pytorch.utils import StaticPointToVoxel
    vsize, crange = [0.5, 0.5, 0.5], [0.0, 0.0, 0.0, 16.0, 16.0, 8.0]
    gen = StaticPointToVoxel(vsize, crange, 4, 2000, 5, 1500, key_order=False, device=cuda)     # first-seen order: hash form
    pc = cloud(1200, 4).to(cuda)
    torch.manual_seed(8)
    gen(pc)
    nv = int(gen.n_voxels[0])
    c = gen.point_corners(with_groups=True)
    want = ri.corners(pc.cpu().numpy(), None, None, vsize, crange[:3], gen.indices.cpu().numpy(), nv, 1, gen.grid_size)
    assert_corners(c._replace(rows=c.rows[:1200], weights=c.weights[:1200]), *want)
    vfeat = torch.randn((gen.max_num_voxels, 8), device=cuda, requires_grad=True)
    dout = torch.randn((gen.max_num_points, 8), device=cuda)
    (grad,) = torch.autograd.grad(spconv.functional.voxels_to_points_trilinear(vfeat, c), vfeat, dout)
    rows = np.full((gen.max_num_points, 8), -1, dtype=np.int32)
    w = np.zeros((gen.max_num_points, 8), dtype=np.float32)
    rows[:1200], w[:1200] = want
    ref = ri.backward(dout.cpu().numpy(), rows, w, gen.max_num_voxels, nv)
    np.testing.assert_array_equal(bits(grad), torch.from_numpy(ref).view(torch.int32).numpy())
    assert bool((grad[nv:] == 0).all()) and int((grad != 0).any(dim=1).sum()) > 500
