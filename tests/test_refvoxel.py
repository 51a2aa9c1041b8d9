"""CPU: tests/refvoxel.py, the float32 numpy reference of the voxelisers, against the sequential restatement
(oracle.point2voxel) and the reference's own code executed (tests/golden/p2v_ref.npz); the teeth of its comparison; the
conditions the inputs of tests/test_gpu_voxel_matrix.py must meet to prove anything; and the coverage of its tables."""
import math
import os

import numpy as np
import pytest
import torch

import oracle
import refvoxel
import test_gpu_voxel_matrix as M
from refvoxel import assert_voxels_equal


def _u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ------------------------------------------------------------------------------------------------ against the restatement
def _finite_cloud(name):
    if name == "wide4":
        return M.cloud(("dup", name, 3000, 5, 65))[0]
    if name.startswith("r"):
        return M.cloud(("uniform", name, 3000, len(M.GRIDS[name]) + 1, 3))[0]
    if name in M.LATTICE:
        return M.cloud(("lattice", name))[0]
    return M.cloud(("rand", name, 3000, len(M.GRIDS[name]) + 2, 3))[0]


@pytest.mark.parametrize("name", sorted(M.GEOMS))
def test_reference_equals_the_sequential_restatement(name):
    geom = M.geometry(name)
    pts = _finite_cloud(name)
    found = refvoxel.voxelize(pts, geom, pts.shape[0] + 1, 1)["found"]
    assert found > 3
    for max_voxels in (found + 5, max(found // 3, 1)):
        for empty_mean in (False, True):
            got = refvoxel.voxelize(pts, geom, max_voxels, 2, empty_mean=empty_mean)
            v, i, c, pid = oracle.point2voxel(pts, [float(x) for x in geom.vsize],
                                              [float(x) for x in geom.lo] + [float(x) for x in geom.hi], list(geom.grid),
                                              max_voxels, 2, empty_mean)
            assert got["found"] == found and got["kept"] == min(found, max_voxels) == i.shape[0]
            assert_voxels_equal(refvoxel.oneshot_view(got), {"voxels": v, "indices": i, "num": c, "pid": pid, "kept": i.shape[0]})
            assert (pid == -1).any() and c.max() == 2


@pytest.mark.parametrize("tag", ["plain", "mean", "capped_mean"])
def test_reference_equals_the_reference_code_executed(tag):
    d = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "p2v_ref.npz"))
    mv, mp, mean = (int(v) for v in d[f"{tag}_args"])
    vs, cr, grid = d["vsize"].astype(np.float32), d["coors_range"].astype(np.float32), d["grid_size"]
    geom = refvoxel.Geometry(3, vs, cr[:3], cr[3:], tuple(int(g) for g in grid))
    got = refvoxel.voxelize(d["points"], geom, mv, mp)
    np.testing.assert_array_equal(got["indices"], d[f"{tag}_indices"])
    np.testing.assert_array_equal(got["num"], d[f"{tag}_num"])
    np.testing.assert_array_equal(got["pid"], d[f"{tag}_pid"])
    stored = np.arange(mp)[None, :] < got["num"][:, None]
    np.testing.assert_array_equal(_u32(got["voxels"])[stored], _u32(d[f"{tag}_voxels"])[stored])
    if not mean:
        np.testing.assert_array_equal(_u32(got["voxels"]), _u32(d[f"{tag}_voxels"]))
    # the first voxel's fill starts from a zero accumulator in the reference's loop too
    filled = refvoxel.voxelize(d["points"], geom, mv, mp, empty_mean=True)
    if mean:
        np.testing.assert_array_equal(_u32(filled["voxels"][0]), _u32(d[f"{tag}_voxels"][0]))


def test_float64_would_be_the_wrong_reference():
    """On the lattice a float64 floor-divide lands in another cell than the float32 one."""
    for name in M.LATTICE:
        g = M.geometry(name)
        x = M.lattice_values(name)
        f32 = np.floor((x - g.lo[-1]) / g.vsize[-1])
        f64 = np.floor((x.astype(np.float64) - float(g.lo[-1])) / float(g.vsize[-1]))
        assert f32.dtype == np.float32 and int((f32 != f64).sum()) >= 20, name


# ----------------------------------------------------------------------------------------------------------------- bf16
def test_bf16_rule_equals_torch():
    rng = np.random.default_rng(0)
    u = rng.integers(0, 1 << 32, 4000, dtype=np.uint64).astype(np.uint32)
    hi = rng.integers(0, 1 << 16, 600, dtype=np.uint64).astype(np.uint32) << 16
    ties = np.concatenate([hi | 0x8000, hi | 0x7FFF, hi | 0x8001, hi])           # exact ties and their neighbours
    special = np.array([0x7F800000, 0xFF800000, 0x7FC00000, 0x7F800001, 0x7FFFFFFF, 0x7F7FFFFF, 0xFF7FFFFF, 0x7F7F8000,
                        0x00000000, 0x80000000, 0x00000001, 0x00008000, 0x00018000, 0x3F808000, 0x3F818000], np.uint32)
    bits = np.concatenate([u, ties.astype(np.uint32), special])
    x = bits.view(np.float32)
    want = torch.from_numpy(x.copy()).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    got = refvoxel.round_bf16(x)
    nan = np.isnan(x)
    assert nan.any() and np.isinf(x).any()
    np.testing.assert_array_equal(got[~nan], want[~nan])
    assert ((got[nan] & 0x7F80) == 0x7F80).all() and ((got[nan] & 0x007F) != 0).all()        # NaN kept NaN
    assert ((want[nan] & 0x7F80) == 0x7F80).all() and ((want[nan] & 0x007F) != 0).all()


# ------------------------------------------------------------------------------------------------------------ rank map
def _encode_rank_map(keys, cells):
    W = refvoxel.rank_map_words(cells)
    buf = np.zeros((refvoxel.rank_map_int32s(cells),), np.uint32)
    bits = np.zeros((W,), np.uint32)
    np.bitwise_or.at(bits, keys >> 5, (np.uint32(1) << (keys & 31).astype(np.uint32)))
    pop = np.array([bin(int(b)).count("1") for b in bits], np.int64)
    nblk = (W + 2047) // 2048
    for b in range(nblk):
        p = pop[b * 2048:(b + 1) * 2048]
        buf[2 * b * 2048 + 1:2 * min((b + 1) * 2048, W):2] = np.cumsum(p) - p
    buf[0:2 * W:2] = bits
    tot = np.array([pop[b * 2048:(b + 1) * 2048].sum() for b in range(nblk)])
    buf[(W * 8 + 255) // 256 * 64:][:nblk] = np.cumsum(tot) - tot
    return buf.view(np.int32)


@pytest.mark.parametrize("cells", [31, 32, 33, 65535, 65536, 65537, 3 * 65536 + 1])
def test_rank_map_decoder(cells):
    rng = np.random.default_rng(cells)
    keys = np.unique(np.concatenate([rng.integers(0, cells, min(cells, 5000)), [0, cells - 1]])).astype(np.int64)
    got, rank = refvoxel.decode_rank_map(_encode_rank_map(keys, cells), cells)
    assert np.array_equal(got, keys) and np.array_equal(rank, np.arange(keys.shape[0]))
    buf = _encode_rank_map(keys, cells)
    buf[1] += 1                                                                  # a wrong prefix shows in the ranks
    assert not np.array_equal(refvoxel.decode_rank_map(buf, cells)[1], np.arange(keys.shape[0]))


# ------------------------------------------------------------------------------ section 5: conditions on the inputs
def test_geometries_and_rank_cells():
    for name in M.GEOMS:
        M.geometry(name)                                                          # (asserts the grid)
    for (name, batch), cells in M.RANK_CELLS.items():
        assert batch * math.prod(M.GRIDS[name]) == cells
    assert sorted(M.RANK_CELLS.values()) == [31, 32, 33, 65535, 65536, 65537, 3 * 65536 + 1]
    assert math.prod(M.GRIDS["wide4"]) > 2 ** 32 and math.prod(M.GRIDS["lat0.05"]) > 0x7FFFFFE0


@pytest.mark.parametrize("name", M.LATTICE)
def test_lattice_clouds_have_teeth(name):
    """At 20 points or more of the lattice, multiplying by the reciprocal lands in another cell than dividing: a kernel
    that did so would fail.  (vsize 0.2 / lo -2 / 20 cells has no such point: d3's z axis is no lattice case.)"""
    g = M.geometry(name)
    x = M.lattice_values(name)
    d = x - g.lo[-1]
    vs = g.vsize[-1]
    inside = (np.floor(d / vs) >= 0) & (np.floor(d / vs) < g.grid[-1])
    differ = np.floor(d / vs) != np.floor(d * (np.float32(1) / vs))
    assert d.dtype == np.float32 and int((differ & inside).sum()) >= 20, int((differ & inside).sum())
    pts, _ = M.cloud(("lattice", name))
    assert pts.shape[0] == 3 * x.shape[0] <= 15000
    for axis in range(3):                                                         # each axis in turn, the others mid-cell
        part = pts[axis * x.shape[0]:(axis + 1) * x.shape[0]]
        assert np.array_equal(part[:, axis], x)
        others = np.delete(part[:, :3], axis, axis=1)
        frac = (others.astype(np.float64) - float(g.lo[-1])) / float(M.GEOMS[name][0][0]) % 1.0
        assert (np.abs(frac - 0.5) < 0.01).all()
    res = refvoxel.voxelize(pts, g, 20000, 4)
    assert res["found"] <= 20000 and (res["pid"] == -1).any() and (res["pid"] >= 0).any()


def _scene0(c_or_g):
    if "scenes" in c_or_g:
        return M.static_reference(c_or_g, 0)
    return M.oneshot_reference(c_or_g)


_CAP_CASES = [c for c in M.ONESHOT + M.STATIC if c["capped"] is not None]


@pytest.mark.parametrize("c", _CAP_CASES, ids=[c["id"] for c in _CAP_CASES])
def test_cap_conditions(c):
    """Every capped case overflows the cap; every uncapped one does not, fills a voxel and drops a point.  (capped=None:
    a hand-built cloud, whose own properties are asserted in this file.)"""
    res = _scene0(c)
    if c["capped"]:
        assert res["found"] > c["max_voxels"] == res["kept"]
    else:
        assert res["found"] <= c["max_voxels"] and res["num"].max() == c["max_points"] and (res["pid"] == -1).any()


def test_sort_width_clouds():
    assert 257 < M.FOUND_D3 < 4000
    big = [g for g in M.STATIC if g["row"] == "sortwidth" and g["geom"] == "sort"]
    assert sorted({g["max_voxels"] for g in big}) == [65535, 65536, 65537, 70000]
    for g in big:
        assert M.cloud(g["scenes"][0][0])[0].shape[0] == 200000
        assert M.static_reference(g, 0)["found"] > 70000
    exact = [c for c in M.ONESHOT + M.STATIC if c["row"] == "caps"]
    assert {M.FOUND_D3 - c["max_voxels"] for c in exact if c["max_voxels"] > 1 and c["max_points"] > 1} == {0, 1}


def test_static_groups_run_largest_first_and_end_empty():
    for g in M.STATIC:
        lives = [M.cloud(spec)[0].shape[0] if live is None else live for spec, live, _ in g["scenes"]]
        assert lives == sorted(lives, reverse=True) and lives[-1] == 0 and lives[0] <= g["n_cap"], g["id"]
        for spec, _, _ in g["scenes"]:
            assert M.cloud(spec)[0].shape[1] == g["nfeat"]
    sizes = {(g["n_cap"], live) for g in M.STATIC if g["row"] == "sizes" for _, live, _ in g["scenes"]}
    assert sizes == {(n, live) for n in (1, 256, 257, 2048, 2049) for live in (0, 1, n - 1, n)}
    one = {M.cloud(c["cloud"])[0].shape[0] for c in M.ONESHOT if c["row"] == "sizes"}
    assert one == {1, 255, 256, 257, 2047, 2048, 2049, 4097}
    assert max(M.cloud(spec)[0].shape[0] for g in M.STATIC for spec, _, _ in g["scenes"]) == 200000


def test_hand_built_clouds():
    d3 = M.geometry("d3")
    # non-finite: the 15 points with a bad coordinate are dropped, the feature specials are stored bit for bit
    for payload in (False, True):
        pts, _ = M.cloud(("nonfinite", payload))
        res = refvoxel.voxelize(pts, d3, 1000, 4, empty_mean=True, mean_dtype="f32")
        bad = ~np.isfinite(pts[:, :3]).all(axis=1) | (np.abs(pts[:, :3]) > 1e38).any(axis=1)
        assert bad.sum() == 15 and (res["pid"][bad] == -1).all()
        clean = refvoxel.voxelize(pts[~bad], d3, 1000, 4)
        assert clean["found"] == res["found"] and np.array_equal(clean["indices"], res["indices"])
        stored = _u32(res["voxels"])[np.arange(4)[None, :] < res["num"][:, None]]
        for bits in (0x7FC12345 if payload else 0x7FC00000, 0x7F800000, 0x80000000, int(_u32(np.float32(1e-40).reshape(1))[0])):
            assert (stored[:, 3] == bits).sum() >= 1, hex(bits)
        assert 0 < _u32(np.float32(1e-40).reshape(1))[0] < 0x00800000                         # a denormal
        assert np.isnan(res["mean"][:, 3]).sum() == 1 and np.isinf(res["mean"][:, 3]).sum() == 1
    # heavy: one voxel of 5000 points
    pts, _ = M.cloud(("heavy",))
    res = refvoxel.voxelize(pts, d3, 200, 6000)
    assert pts.shape[0] == 5100 and res["num"].max() == 5000 and res["found"] <= 200
    # batch: scene 1 empty, strays dropped, one cell occupied in scenes 0 and 2
    pts, ids = M.cloud(("batch3",))
    res = refvoxel.voxelize(pts, d3, 4000, 5, batch_ids=ids, batch_size=3, lead=True)
    assert set(res["indices"][:, 0]) == {0, 2} and (res["pid"][(ids < 0) | (ids > 2)] == -1).all()
    assert res["pid"][0] != res["pid"][1] and np.array_equal(res["indices"][res["pid"][0], 1:], res["indices"][res["pid"][1], 1:])
    assert (ids == 3).any() and (ids == -1).any()


def test_rounding_cloud_hits_the_ties():
    pts, _ = M.cloud(("rounding",))
    d3 = M.geometry("d3")
    rows = {}
    for dt in ("f32", "f16", "bf16"):
        res = refvoxel.voxelize(pts, d3, 1000, 4, key_order=True, mean_dtype=dt)
        a, b, c = (int(res["pid"][np.flatnonzero(np.isclose(pts[:, 0], x))[0]]) for x in (6.05, 6.25, 6.45))
        assert res["num"][a] == 2 and res["num"][b] == 2 and res["num"][c] == 3
        rows[dt] = (res["mean"][a], res["mean"][b], res["mean"][c])
    A32, B32, C32 = rows["f32"]
    assert list(A32[3:]) == [1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8]         # exact in fp32
    A16, B16, _ = rows["f16"]
    assert float(A16[3]) == 1.0 and float(A16[4]) == 1 + 2.0 ** -9                                  # tie down, tie up
    assert np.isposinf(B16[3]) and np.isneginf(B16[4]) and np.isposinf(B16[5]) and float(B16[6]) == 65504.0
    Ab, Bb, _ = rows["bf16"]
    f = lambda u: np.array([int(u) << 16], np.uint32).view(np.float32)[0]
    assert f(Ab[5]) == 1.0 and f(Ab[6]) == 1 + 2.0 ** -6 and np.isfinite(f(Bb[3])) and np.isfinite(f(Bb[4]))
    assert float(C32[3]) != (0.1 + 0.2 + 0.7) / 3 and np.float64(C32[3]) * 3 != np.float64(np.float32(0.1) + np.float32(0.2) + np.float32(0.7))


# ------------------------------------------------------------------------------------------------------ checker teeth
def _reference_output():
    pts, _ = M.cloud(("nonfinite", False))
    res = refvoxel.voxelize(pts, M.geometry("d3"), 1000, 4, mean_dtype="f16", lead=True, key_order=True)
    return refvoxel.static_view(res, 1000, 400), res["kept"]


def _copy(d):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in d.items()}


def test_checker_accepts_the_reference_itself():
    want, _ = _reference_output()
    assert_voxels_equal(_copy(want), want)


def _swap_points(got, kept):
    v = int(np.flatnonzero(got["num"] >= 2)[0])
    got["voxels"][v, [0, 1]] = got["voxels"][v, [1, 0]]


def _swap_voxels(got, kept):
    for name in ("voxels", "indices", "num", "mean"):
        got[name][[0, 1]] = got[name][[1, 0]]
    pid = got["pid"]
    got["pid"] = np.where(pid == 0, 1, np.where(pid == 1, 0, pid))


def _count(got, kept):
    got["num"][kept - 1] += 1


def _stale_row(got, kept):
    got["indices"][kept + 3] = got["indices"][0]


def _mean_ulp(got, kept):
    m = got["mean"].view(np.uint16)
    m[2, 1] += 1


def _minus_zero(got, kept):
    bits = got["voxels"].view(np.uint32)
    at = np.argwhere(bits == 0x80000000)
    assert at.shape[0] > 0
    bits[tuple(at[0])] = 0


@pytest.mark.parametrize("alter", [_swap_points, _swap_voxels, _count, _stale_row, _mean_ulp, _minus_zero],
                         ids=lambda f: f.__name__.strip("_"))
def test_checker_rejects(alter):
    want, kept = _reference_output()
    got = _copy(want)
    alter(got, kept)
    with pytest.raises(AssertionError):
        assert_voxels_equal(got, want)


def test_checker_rejects_a_missing_or_extra_output():
    want, _ = _reference_output()
    got = _copy(want)
    del got["mean"]
    with pytest.raises(AssertionError):
        assert_voxels_equal(got, want)
    with pytest.raises(AssertionError):
        assert_voxels_equal(want, got)


# ------------------------------------------------------------------------------------------------------- case coverage
def test_cases_cover_every_path():
    one = [M.oneshot_path(c) for c in M.ONESHOT]
    static = [p for g in M.STATIC for p in M.static_paths(g)]
    assert {p["passes"] for p in static} == {1, 2, 3, 4} and {p["passes"] for p in one} == {4}
    for paths in (one, static):
        assert {p["table"] for p in paths} == {"packed", "wide"}
        for ndim in (1, 2, 3, 4):
            assert {p["key_order"] for p in paths if p["ndim"] == ndim} == {False, True}, ndim
    assert {p["empty_mean"] for p in one} == {0, 1} and {p["empty_mean"] for p in static} == {0, 1}
    # (empty_mean = 2, one-shot only, is test_quirk_fill_with_seventy_features)
    assert {(p["mean"], p["keep_voxels"]) for p in static} >= {(m, k) for m in ("f32", "f16", "bf16") for k in (True, False)}
    assert (None, True) in {(p["mean"], p["keep_voxels"]) for p in static}
    # the pass count follows the code's rule at the digit edges
    assert [refvoxel.radix_passes(v) for v in (1, 255, 256, 65535, 65536, (1 << 24) - 1, 1 << 24, 1 << 30)] == [1, 1, 2, 2, 3, 3, 4, 4]
    # only combinations that construct are cases, and what the constructor refuses is none
    for g in M.STATIC:
        assert M.static_constructs(g["geom"], g["batch_size"], g["max_voxels"], g["key_order"]), g["id"]
    for geom, batch, max_voxels, key in M.REJECTED:
        assert not M.static_constructs(geom, batch, max_voxels, key)
        assert not any((g["geom"], g["batch_size"], g["max_voxels"], g["key_order"]) == (geom, batch, max_voxels, key)
                       for g in M.STATIC)
    rows = {c["row"] for c in M.ONESHOT} | {g["row"] for g in M.STATIC}
    assert rows == {"dims", "sizes", "sortwidth", "caps", "heavy", "lattice", "nonfinite", "batch", "rankmap", "rounding"}
    ids = [c["id"] for c in M.ONESHOT + M.STATIC]
    assert len(ids) == len(set(ids))
