"""GPU: every path of the hash-table rulebook builders (csrc/rulebook_subm.hip, csrc/rulebook_conv.hip) against pairs derived from the coordinates.

test_gpu_rulebook.py holds the builders to the oracle on whichever path the default dispatch picks for its sizes.  Here
every dispatch decision of spx_subm_rulebook and spx_conv_rulebook_count / _fill / _static is reached on purpose --
through the library's options, the kernel volume or the row count -- and PROVEN reached: a case reads the rulebook/<pass>
launch counters (include/spconv_amd.h) before and after its build and asserts that the pass it is about ran and that
the pass it replaces did not.  Every artefact (coordinates, Native lists, counts, both dense tables, mask words) is then
compared bit for bit with refrulebook.py, which shares no code with the oracle or the library; at the two sizes where
that reference is too slow (131 k voxels, 70 k voxels x 125 offsets) with the oracle, which test_refrulebook.py ties to
it.  No tolerances anywhere.

Every build runs over a workspace full of a byte pattern (0xA5) instead of whatever the allocator hands out: a pass
that reads a word no earlier pass of the same build wrote shows as a mismatch, every time."""
import contextlib
import functools

import numpy as np
import pytest
import torch

import refrulebook
from test_gpu_rulebook import CONV_CASES, _far_corner_scene
from test_refrulebook import holes
from util import assert_rulebook_equal, dense_scene, gpu_rulebook, oracle_rulebook, scene, to_np

pytestmark = pytest.mark.gpu

PASSES = ("subm_probe3", "subm_probe4", "subm_probe5", "subm_mask_pass", "subm_lists", "native_lists_v1", "conv3/1",
          "conv3/2", "conv3/4", "conv3/8", "conv_generic", "conv_lists_v1", "conv_shrunk", "conv_retry", "conv3_shares/1",
          "conv3_shares/2", "conv3_shares/4", "conv3_shares/8")
DEFAULTS = {"SPX_SUBM_PROBE": 5, "SPX_SUBM_MASK_PASS": -1, "SPX_CONV_V": 3, "SPX_TEST_CONV3_SHARES": 0}


def counters():
    from spconv_amd import _lib
    L = _lib.load()
    got = {p: int(L.spx_launch_count(f"rulebook/{p}".encode())) for p in PASSES}
    assert min(got.values()) >= 0, got
    return got


def ran(before, sized_by_history=False, **expect):
    """Which counters moved since `before`, and by how much: exactly the ones named.  sized_by_history: the two-call
    form sizes its table by what the geometry produced last time, in this process -- a case that is not about that lets
    conv_shrunk and conv_retry move, and every retry is one more count pass."""
    after = counters()
    moved = {p: after[p] - before[p] for p in PASSES if after[p] != before[p]}
    want = {p.replace("__", "/"): v for p, v in expect.items() if v}
    if sized_by_history:
        retries = moved.pop("conv_retry", 0)
        assert moved.pop("conv_shrunk", 0) in (retries, retries + 1)
        for p in want:
            if p.startswith("conv3"):
                want[p] += retries
    assert moved == want, (moved, want)


@contextlib.contextmanager
def options(**values):
    from spconv_amd import _lib
    L = _lib.load()
    assert set(values) <= set(DEFAULTS)
    try:
        for name, v in values.items():
            _lib.check(L.spx_set_option(name.encode(), int(v)))
        yield
    finally:
        for name in values:
            _lib.check(L.spx_set_option(name.encode(), DEFAULTS[name]))


@pytest.fixture(autouse=True)
def stale_workspace(monkeypatch):
    from spconv_amd.pytorch import _rulebook
    monkeypatch.setattr(_rulebook, "_ws", lambda nbytes, device: torch.full((max(int(nbytes), 16),), 0xA5,
                                                                            dtype=torch.uint8, device=device))


# ------------------------------------------------------------------------------------------------------------ scenes
def dense_box(nd, n, seed):
    """Exactly n rows of one batch item, in random order, filling 40 % of a box at the low corner of a grid three times
    its size: about 0.4 (kv - 1) neighbours per row at any n."""
    side = max(3, int(np.ceil((2.5 * n) ** (1.0 / nd))))
    shape = [3 * side] * nd
    idx = dense_scene(shape, n, 1, seed)
    assert idx.shape[0] == n
    return idx, 1, shape


SUBM_KERNELS = {                      # name: (ksize, dilation)
    "k27": ([3, 3, 3], [1, 1, 1]),
    "k45": ([5, 3, 3], [1, 1, 1]),                   # two mask words
    "k81": ([3, 3, 3, 3], [1, 1, 1, 1]),             # 4-d, three mask words
    "k125": ([5, 5, 5], [1, 1, 1]),                  # four mask words, the largest list state of subm_probe5_kernel
    "k175": ([5, 5, 7], [1, 1, 1]),                  # six mask words: beyond 128, the first form
    "k1": ([1, 1, 1], [1, 1, 1]),                    # the identity alone: the first form
    "k313": ([3, 1, 3], [1, 1, 1]),
    "d2": ([3, 3, 3], [2, 2, 2]),
}


@functools.lru_cache(maxsize=None)
def subm_problem(kernel, kind, n):
    """(idx, bs, shape, reference) -- shared by the cases that differ in the path only; nobody writes to it."""
    ksize, dil = SUBM_KERNELS[kernel]
    nd = len(ksize)
    if kind == "dense":
        idx, bs, shape = dense_box(nd, n, seed=n % 97)
    elif kind == "holes":
        assert nd == 3
        idx, bs, shape = dense_box(nd, n - 70, seed=9)
        idx = holes(idx, bs)
    else:
        assert kind == "far" and nd == 3
        bs, shape = 2, [3000, 2500, 2000]
        idx = _far_corner_scene(shape, n // 2, bs, seed=2)
        assert int(idx[:, 1].max()) * shape[1] * shape[2] > 2 ** 32          # int64 keys
    assert idx.shape[0] == n
    pad = [(k // 2) * d for k, d in zip(ksize, dil)]
    ref = refrulebook.rulebook(idx, bs, shape, ksize, [1] * nd, pad, dil, True)
    kv = int(np.prod(ksize))
    if kv > 1 and kind != "far":
        # dense: more than four pairs per row -- or, where the kernel has fewer than 16 neighbour sites ([3, 1, 3]), a
        # quarter of them occupied
        assert ref["num"].sum() > min(2 * n, (kv // 2) * n // 4), (int(ref["num"].sum()), n)
    elif kv > 1:
        assert ref["num"].sum() > n // 2
    if kind == "holes":
        live = (idx[:, 0] >= 0) & (idx[:, 0] < bs)
        assert (~live).sum() == 2 and np.unique(idx[live], axis=0).shape[0] < live.sum()
    for a in ref.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return idx, bs, shape, ref


def run_subm(kernel, kind, n, path, mask_pass, native):
    ksize, dil = SUBM_KERNELS[kernel]
    nd, kv = len(ksize), int(np.prod(ksize))
    idx, bs, shape, ref = subm_problem(kernel, kind, n)
    pad = [(k // 2) * d for k, d in zip(ksize, dil)]
    first_form = kv > 128 or kv == 1
    assert first_form == (path == "probe3")
    opts = {}
    if path == "probe4":
        opts["SPX_SUBM_PROBE"] = 4
    if mask_pass is not None:
        opts["SPX_SUBM_MASK_PASS"] = mask_pass
    # (tables below 1024 slots -- up to 128 rows -- take the fourth form whatever the option says)
    probe = "subm_probe3" if first_form else ("subm_probe4" if path == "probe4" or n <= 128 else "subm_probe5")
    with options(**opts):
        before = counters()
        rb, _ = gpu_rulebook(idx, bs, shape, ksize, [1] * nd, pad, dil, True, need_bwd_table=True, need_native=native)
        ran(before, **{probe: 1, "subm_mask_pass": int(bool(mask_pass) and not first_form),
                       "subm_lists": int(native and not first_form),
                       "native_lists_v1": int(native and first_form and kv > 1)})
    assert (rb._pair_native is not None) == native
    assert rb.pair_bwd is not None
    assert_rulebook_equal(rb, ref, True)


SWEEP = (129, 255, 256, 257, 2047, 2048, 2049, 4097)      # one workgroup, the 2048-row blocks of the list passes
SUBM_MATRIX = []
for _path in ("probe5", "probe4"):
    for _n in ((128,) if _path == "probe5" else ()) + SWEEP:                # 128 / 129: the smallest fifth-form table
        SUBM_MATRIX += [("k27", "dense", _n, _path, 0, True), ("k27", "dense", _n, _path, 1, False)]
    for _k in ("k45", "k81", "k125", "k313", "d2"):
        SUBM_MATRIX += [(_k, "dense", 257, _path, 0, True), (_k, "dense", 257, _path, 1, False)]
        SUBM_MATRIX += [(_k, "dense", 2049, _path, _mp, _nat) for _mp in (0, 1) for _nat in (True, False)]
    for _kind, _n in (("holes", 470), ("far", 800)):
        SUBM_MATRIX += [("k27", _kind, _n, _path, 0, True), ("k27", _kind, _n, _path, 1, True)]
for _n in SWEEP[1:]:
    SUBM_MATRIX += [("k175", "dense", _n, "probe3", None, True), ("k175", "dense", _n, "probe3", None, False)]
SUBM_MATRIX += [("k1", "dense", _n, "probe3", None, _nat) for _n in (257, 2049) for _nat in (True, False)]
SUBM_MATRIX += [("k175", "holes", 470, "probe3", None, True), ("k175", "far", 800, "probe3", None, True)]


@pytest.mark.parametrize("kernel,kind,n,path,mask_pass,native", SUBM_MATRIX,
                         ids=[f"{p}-{k}-{s}-n{n}-mp{m}-{'native' if nat else 'tables'}" for k, s, n, p, m, nat in SUBM_MATRIX])
def test_subm_path(cuda, kernel, kind, n, path, mask_pass, native):
    run_subm(kernel, kind, n, path, mask_pass, native)


@pytest.mark.parametrize("n,probe", [(131072, "subm_probe5"), (131073, "subm_probe4")])
def test_subm_largest_fifth_form_table(cuda, n, probe):
    """Default options, kv = 27: 131 072 rows are the last with a table of 2^19 slots (64 KB of occupancy bits in LDS),
    one row more takes the fourth form.  Against the oracle (refrulebook takes minutes here)."""
    shape = [64, 128, 128]
    idx = scene(shape, n, 1, seed=1)
    assert idx.shape[0] == n
    ref = oracle_rulebook(idx, 1, shape, [3] * 3, [1] * 3, [1] * 3, [1] * 3, True)
    assert ref["num"].sum() > n
    before = counters()
    rb, _ = gpu_rulebook(idx, 1, shape, [3] * 3, [1] * 3, [1] * 3, [1] * 3, True, need_bwd_table=True)
    ran(before, **{probe: 1, "subm_lists": 1})
    assert_rulebook_equal(rb, ref, True)


def test_subm_full_bit_map_and_largest_list_state(cuda):
    """kv = 125 at 70 000 rows: the full 64 KB bit map (a table of 2^19 slots) beside 62 x 40 bytes of list state, four
    mask words.  Against the oracle."""
    shape, n, ks = [48, 96, 96], 70_000, [5, 5, 5]
    idx = scene(shape, n, 1, seed=4)
    ref = oracle_rulebook(idx, 1, shape, ks, [1] * 3, [2] * 3, [1] * 3, True)
    assert ref["num"].sum() > 2 * n
    before = counters()
    rb, _ = gpu_rulebook(idx, 1, shape, ks, [1] * 3, [2] * 3, [1] * 3, True, need_bwd_table=True)
    ran(before, subm_probe5=1, subm_lists=1)
    assert_rulebook_equal(rb, ref, True)


# ------------------------------------------------------------------------------------------- strided / transposed
CONV_GEOMS = {                        # name: (shape, n per batch item, bs, ksize, stride, padding, dilation, transposed, out_padding)
    "mj8": CONV_CASES[0] + (None,),                                        # k3 s2 p1
    "mj4": CONV_CASES[9] + (None,),                                        # 2-d k3 s2
    "mj2": ([19, 18, 17], 1500, 2, [3, 2, 2], [2, 2, 2], [1, 0, 0], [1, 1, 1], False, None),
    "mj1": CONV_CASES[1] + (None,),                                        # k2 s2
    "mj1s3": CONV_CASES[3] + (None,),                                      # k3 s3 p2
    # generic only
    "1d": ([301], 140, 2, [3], [2], [1], [1], False, None),               # two candidates of three offsets: no gain
    "4d": ([9, 8, 7, 6], 900, 1, [3] * 4, [2] * 4, [1] * 4, [1] * 4, False, None),        # 81 offsets
    "tr": ([10, 9, 9], 500, 2, [3] * 3, [2] * 3, [1] * 3, [1] * 3, True, [1, 1, 1]),
    "tr0": ([10, 9, 9], 500, 1, [2] * 3, [2] * 3, [0] * 3, [1] * 3, True, [1, 0, 1]),
    "s1": CONV_CASES[4] + (None,),                                         # stride 1
    "d2": ([31, 30, 29], 1200, 1, [3] * 3, [2] * 3, [2] * 3, [2] * 3, False, None),       # 27 candidates
    "k216": ([19, 18, 17], 500, 1, [6] * 3, [2] * 3, [2] * 3, [1] * 3, False, None),      # beyond 128 offsets
}
assert CONV_GEOMS["mj8"][3:5] == ([3] * 3, [2] * 3) and CONV_GEOMS["mj4"][3] == [3, 3] and CONV_GEOMS["mj1"][3] == [2] * 3
assert CONV_GEOMS["mj1s3"][4] == [3] * 3 and CONV_GEOMS["s1"][4:6] == ([1] * 3, [1] * 3)
COMPACT = {"mj8": 8, "mj4": 4, "mj2": 2, "mj1": 1, "mj1s3": 1}


@functools.lru_cache(maxsize=None)
def conv_problem(geom, kind, n):
    shape, n_geom, bs, ks, st, pd, dl, tr, op = CONV_GEOMS[geom]
    if kind == "uniform":
        idx = scene(shape, n_geom, bs, seed=11)
    elif kind == "sparse":                         # exactly n rows, far apart: more outputs than inputs
        bs, shape = 1, [40, 40, 40]
        idx = scene(shape, n, 1, seed=n % 89)
        assert idx.shape[0] == n
    elif kind == "holes":
        bs, shape = 1, [36, 36, 36]
        idx = holes(dense_scene(shape, 400, 1, seed=9), 1)
        assert idx.shape[0] == 470
    else:
        assert kind == "far"
        bs, shape = 1, [4000, 4000, 4000]
        idx = _far_corner_scene(shape, 400, 1, seed=4)
    ref = refrulebook.rulebook(idx, bs, shape, ks, st, pd, dl, False, tr, op)
    if kind == "sparse":
        assert ref["n_out"] > ref["n_in"]
    if kind == "holes":
        live = (idx[:, 0] >= 0) & (idx[:, 0] < bs)
        assert (~live).sum() == 2 and np.unique(idx[live], axis=0).shape[0] < live.sum()
    if kind == "far":
        assert int(np.prod(ref["out_shape"], dtype=np.int64)) > 2 ** 32
    assert ref["n_out"] > 0 and ref["num"].sum() > ref["n_in"] // 2
    for a in ref.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return idx, bs, shape, ref


def run_conv(geom, kind, n, gen, shares, native=True):
    _, _, _, ks, st, pd, dl, tr, op = CONV_GEOMS[geom]
    idx, bs, shape, ref = conv_problem(geom, kind, n)
    kv = int(np.prod(ks))
    mj = COMPACT.get(geom, 0) if gen == 3 else 0
    # the grid.y of the compact passes: what the option forces, at most mj; by size (0) these scenes get mj.  Counted
    # by the count pass and by the fill pass, which must launch the same
    eff = min(shares, mj) if shares else mj
    with options(SPX_CONV_V=gen, SPX_TEST_CONV3_SHARES=shares):
        before = counters()
        rb, out_shape = gpu_rulebook(idx, bs, shape, ks, st, pd, dl, False, tr, op, need_native=native)
        # the count pass and the fill pass each say which passes they took
        ran(before, sized_by_history=True,
            **{(f"conv3/{mj}" if mj else "conv_generic"): 2, f"conv3_shares/{eff}": 2 * int(mj > 0),
               "conv_lists_v1": int(native and kv > 128)})
    assert list(out_shape) == list(ref["out_shape"])
    assert_rulebook_equal(rb, ref, False)


CONV_MATRIX = []
for _g in COMPACT:
    CONV_MATRIX += [(_g, "uniform", 0, 3, _s) for _s in (0, 1, 2, 4)] + [(_g, "uniform", 0, 2, 0)]
CONV_MATRIX += [(_g, "uniform", 0, _gen, 0) for _g in ("1d", "4d", "tr", "tr0", "s1", "d2", "k216") for _gen in (3, 2)]
CONV_MATRIX += [("mj8", "sparse", _n, _gen, _s) for _n in (255, 256, 257, 2047, 2049) for _gen, _s in ((3, 0), (3, 2), (2, 0))]
CONV_MATRIX += [("mj8", _kind, 0, _gen, _s) for _kind in ("holes", "far") for _gen, _s in ((3, 0), (3, 2), (2, 0))]


@pytest.mark.parametrize("geom,kind,n,gen,shares", CONV_MATRIX,
                         ids=[f"{g}-{k}{n or ''}-v{gen}-shares{s}" for g, k, n, gen, s in CONV_MATRIX])
def test_conv_path(cuda, geom, kind, n, gen, shares):
    run_conv(geom, kind, n, gen, shares)


def test_conv_beyond_128_offsets_without_lists(cuda):
    """[6, 6, 6]: the tables alone (inference) launch no list pass; the lists derived later equal the reference's."""
    run_conv("k216", "uniform", 0, 3, 0, native=False)


# ----------------------------------------------------------------------------------------- the expected-size table
def slots(entries):
    """Slots of a table sized for `entries`: the power of two from 256 that leaves it at most half full."""
    cap = 256
    while cap < 2 * entries:
        cap *= 2
    return cap


def expected(n_in, n_out_last):
    """Outputs the two-call form expects from n_in inputs after a build of the same geometry and size gave n_out_last:
    the last ratio in 64ths, rounded up and one more, + 25 % + 4096."""
    ratio_x64 = (n_out_last * 64 + n_in - 1) // n_in + 1
    return n_in * ratio_x64 // 64 * 5 // 4 + 4096


def clustered(n, origin, seed):
    """A full 16 x 32 x (n / 512) block in random row order: few outputs per input."""
    assert n % 512 == 0
    g = np.stack(np.unravel_index(np.random.default_rng(seed).permutation(n), (16, 32, n // 512)), -1)
    return np.ascontiguousarray(np.concatenate([np.zeros((n, 1), np.int64), g + np.asarray(origin)], 1).astype(np.int32))


def separated(n, extent, origin, seed):
    """Stride-aligned inputs four cells apart (k = 3, s = 2, p = 1): an odd coordinate reaches two outputs along its axis,
    an even one a single output, and no two inputs share an output.  Half the rows are (odd, odd, even): four outputs,
    half (even, even, even): one -- 2.5 outputs per input."""
    grid = [(s - 3) // 4 + 1 for s in extent]
    assert int(np.prod(grid)) >= n and n % 2 == 0
    g = np.stack(np.unravel_index(np.random.default_rng(seed).choice(int(np.prod(grid)), n, replace=False), grid), -1)
    c = 4 * g + 2
    c[: n // 2, :2] -= 1
    c = c[np.random.default_rng(seed + 1).permutation(n)]
    assert (c < np.asarray(extent)).all()
    return np.ascontiguousarray(np.concatenate([np.zeros((n, 1), np.int64), c + np.asarray(origin)], 1).astype(np.int32))


@pytest.mark.parametrize("shape,origin,wide", [([101, 99, 107], [0, 0, 0], False),
                                               ([4001, 3999, 4003], [3880, 3880, 3880], True)])
def test_expected_size_table_grows_and_holds(cuda, shape, origin, wide):
    """The two-call form sizes its table for the ratio the geometry gave last time (a process-wide cache: these grids
    are used by no other test).  First build: a clustered scene, no expectation yet.  Second: the same number of
    inputs, separated, with more outputs than the expected table has SLOTS: the count pass overflows and runs again at
    the guaranteed size.  Third: the first scene again, now on a table shrunk to the second build's ratio, which holds.
    wide: the same at the far corner of a grid whose output keys take 64 bits -- a shrunk table keeps its values behind
    the shrunk keys."""
    n, ks, st, pd, dl = 16384, [3] * 3, [2] * 3, [1] * 3, [1] * 3
    a, b = clustered(n, origin, seed=1), separated(n, [101, 99, 107], origin, seed=2)
    ref_a = refrulebook.rulebook(a, 1, shape, ks, st, pd, dl, False)
    ref_b = refrulebook.rulebook(b, 1, shape, ks, st, pd, dl, False)
    out_cells = int(np.prod(ref_a["out_shape"], dtype=np.int64))
    assert (out_cells > 2 ** 32) == wide
    assert ref_b["n_out"] == 5 * n // 2 and ref_a["n_out"] < n // 4
    bound = slots(8 * n)                                                  # the guaranteed size: eight candidates per input
    expect_b = expected(n, ref_a["n_out"])
    assert expect_b < ref_b["n_out"] and slots(expect_b) < ref_b["n_out"]          # cannot hold the second build
    assert slots(expected(n, ref_b["n_out"])) < bound                               # the third build shrinks ...
    assert expected(n, ref_b["n_out"]) > ref_a["n_out"]                             # ... and holds
    for idx, ref, moved in ((a, ref_a, {}), (b, ref_b, {"conv_shrunk": 1, "conv_retry": 1}), (a, ref_a, {"conv_shrunk": 1})):
        before = counters()
        rb, _ = gpu_rulebook(idx, 1, shape, ks, st, pd, dl, False)
        ran(before, conv3__8=2 + moved.get("conv_retry", 0), conv3_shares__8=2 + moved.get("conv_retry", 0), **moved)
        assert_rulebook_equal(rb, ref, False)


@pytest.mark.parametrize("gen", [3, 2])
@pytest.mark.parametrize("slack", [37, -37])
def test_static_form_around_the_true_count(cuda, slack, gen):
    """spx_conv_rulebook_static with a bound a little above and a little below the number of outputs: the table is sized
    for the bound (compact passes), the first `bound` outputs of the reference survive with exactly their pairs."""
    shape, bs, ks, st, pd, dl = [24, 24, 24], 1, [3] * 3, [2] * 3, [1] * 3, [1] * 3
    idx = scene(shape, 4000, bs, 5)
    ref = refrulebook.rulebook(idx, bs, shape, ks, st, pd, dl, False)
    n_out, cap = ref["n_out"], ref["n_out"] + slack
    live = min(n_out, cap)
    with options(SPX_CONV_V=gen):
        before = counters()
        rb, _ = gpu_rulebook(idx, bs, shape, ks, st, pd, dl, False, static_num_out=cap)
        ran(before, **({"conv3__8": 2, "conv3_shares__8": 2, "conv_shrunk": 1} if gen == 3 else {"conv_generic": 2}))
    assert rb.n_out == cap and to_np(rb.n_out_dev).tolist() == [n_out, 0]          # the count found, not the bound
    oi, pf, pb = to_np(rb.out_indices), to_np(rb.pair_fwd), to_np(rb.pair_bwd)
    np.testing.assert_array_equal(oi[:live], ref["out_inds"][:live])
    np.testing.assert_array_equal(pf[:, :live], ref["fwd"][:, :live])
    assert (oi[live:] == -1).all() and (pf[:, live:] == -1).all()
    np.testing.assert_array_equal(pb, np.where(ref["bwd"] < cap, ref["bwd"], -1))
    mf, mb = to_np(rb.mask_fwd).view(np.uint32), to_np(rb.mask_bwd).view(np.uint32)
    np.testing.assert_array_equal(mf[:live], ref["mfwd"][:live])
    assert (mf[live:] == 0).all()
    kbit = (np.uint32(1) << np.arange(27, dtype=np.uint32))[:, None]
    np.testing.assert_array_equal(mb[:, 0], ((pb >= 0) * kbit).sum(0).astype(np.uint32))
    # the Native lists hold exactly the surviving pairs, in the reference's order
    nat, num = to_np(rb.pair_native), to_np(rb.num_per_loc)
    for k in range(27):
        full = ref["pair"][:, k, :ref["num"][k]]
        keep = full[:, full[1] < cap]
        assert num[k] == keep.shape[1]
        np.testing.assert_array_equal(nat[:, k, :num[k]], keep)
        assert (nat[:, k, num[k]:] == -1).all()
