"""GPU: both voxelisers (spx_point2voxel through PointToVoxel, spx_point2voxel_static through StaticPointToVoxel)
against tests/refvoxel.py, the float32 numpy statement of their contract, at every edge of the pipeline: dimensions 1-4,
feature widths, block edges of the point count, every radix pass count of the static sort and the digit edges of its
drop key, word and block edges of the rank map, points on the cell lattice, non-finite input, one heavy voxel, the
caps, scene batches, the rounding of the mean rows, reuse of buffers, repeatability and graph replay.

The tables (ONESHOT, STATIC) and the clouds are plain numpy and import without a GPU: tests/test_refvoxel.py checks the
reference, the conditions the inputs must meet and the coverage of the tables on the CPU.  Every case compares every
output through refvoxel.assert_voxels_equal.

A case names whether its cloud overflows the voxel cap (`capped` True / False; test_refvoxel.py asserts found >
max_voxels, or found <= max_voxels with a full voxel and a dropped point).  Hand-built clouds (block-edge sizes down to
one point, lattice, non-finite, heavy, rounding) carry `capped=None`: their own properties are asserted instead."""
import functools
import math

import numpy as np
import pytest
import torch

import refvoxel
from refvoxel import assert_voxels_equal

pytestmark = pytest.mark.gpu

# ------------------------------------------------------------------------------------------------------- geometries (xyz)
GEOMS = {
    "d1": ([0.3], [-1.0, 28.1]),                                                       # grid [97]
    "d2": ([0.05, 0.075], [-1.0, -3.0, 2.5, -0.525]),                                  # grid [33, 70] (zyx)
    "d3": ([0.1, 0.1, 0.2], [0, -4, -2, 8, 4, 2]),                                     # grid [20, 80, 80]
    "d4": ([0.5, 0.4, 0.3, 0.2], [0, -1, -2, 1, 4.5, 1.8, -0.2, 2.0]),                 # grid [5, 6, 7, 9]
    "wide4": ([0.01] * 4, [0.0] * 4 + [3.0] * 4),                                      # 300^4 cells > 2^32
    "sort": ([0.1] * 3, [0, 0, 0, 6.4, 6.4, 3.2]),                                     # grid [32, 64, 64]
    "lat0.1": ([0.1] * 3, [0.0] * 3 + [70.4] * 3),                                     # 704 cells an axis
    "lat0.05": ([0.05] * 3, [-40.0] * 3 + [40.0] * 3),                                 # 1600 (1600^3 cells: beyond a rank map)
    "lat0.075": ([0.075] * 3, [-3.0] * 3 + [27.0] * 3),                                # 400
    "lat0.3": ([0.3] * 3, [-1.0] * 3 + [28.1] * 3),                                    # 97
    # rank-map edges: batch x grid cells (vsize 0.5: the grid is exact)
    "r31": ([0.5], [0, 15.5]), "r32": ([0.5, 0.5], [0, 0, 4.0, 2.0]), "r11": ([0.5], [0, 5.5]),
    "r65535": ([0.5, 0.5], [0, 0, 128.5, 127.5]), "r32768": ([0.5, 0.5], [0, 0, 128.0, 64.0]),
    "r65537": ([0.5], [0, 32768.5]), "r28087": ([0.5], [0, 14043.5]),
}
GRIDS = {"d1": (97,), "d2": (33, 70), "d3": (20, 80, 80), "d4": (5, 6, 7, 9), "wide4": (300,) * 4, "sort": (32, 64, 64),
         "lat0.1": (704,) * 3, "lat0.05": (1600,) * 3, "lat0.075": (400,) * 3, "lat0.3": (97,) * 3,
         "r31": (31,), "r32": (4, 8), "r11": (11,), "r65535": (255, 257), "r32768": (128, 256), "r65537": (65537,),
         "r28087": (28087,)}
LATTICE = ("lat0.1", "lat0.05", "lat0.075", "lat0.3")
RANK_CELLS = {("r31", 1): 31, ("r32", 1): 32, ("r11", 3): 33, ("r65535", 1): 65535, ("r32768", 2): 65536,
              ("r65537", 1): 65537, ("r28087", 7): 3 * 65536 + 1}


@functools.lru_cache(maxsize=None)
def geometry(name):
    g = refvoxel.meta(*GEOMS[name])
    assert g.grid == GRIDS[name], (name, g.grid)
    return g


# ----------------------------------------------------------------------------------------------------------------- clouds
def _frozen(pts, ids=None):
    pts = np.ascontiguousarray(pts, np.float32)
    pts.setflags(write=False)
    if ids is not None:
        ids = np.ascontiguousarray(ids, np.int32)
        ids.setflags(write=False)
    return pts, ids


def _rand(name, n, nfeat, seed):
    """Uniform over the range widened by a tenth on every side (points outside), the first half drawn into a twentieth of
    the range around its middle (several points per voxel); features in [0, 1)."""
    vs, rng_xyz = GEOMS[name]
    ndim = len(vs)
    lo, hi = np.asarray(rng_xyz[:ndim], np.float64), np.asarray(rng_xyz[ndim:], np.float64)
    rng = np.random.default_rng(seed)
    pts = rng.uniform(0.0, 1.0, (n, nfeat))
    pts[:, :ndim] = lo - 0.1 * (hi - lo) + pts[:, :ndim] * 1.2 * (hi - lo)
    mid = 0.5 * (lo + hi)
    pts[: n // 2, :ndim] = mid + (pts[: n // 2, :ndim] - mid) * 0.05
    return pts.astype(np.float32)


def _uniform(name, n, nfeat, seed):
    """Uniform over the range widened by one percent."""
    vs, rng_xyz = GEOMS[name]
    ndim = len(vs)
    lo, hi = np.asarray(rng_xyz[:ndim], np.float64), np.asarray(rng_xyz[ndim:], np.float64)
    pts = np.random.default_rng(seed).uniform(0.0, 1.0, (n, nfeat))
    pts[:, :ndim] = lo - 0.01 * (hi - lo) + pts[:, :ndim] * 1.02 * (hi - lo)
    return pts.astype(np.float32)


def _background(n, nfeat, seed):
    """A d3 cloud that stays below x = 3.7: the cells the hand-built points use lie at x >= 6."""
    pts = _rand("d3", n, nfeat, seed)
    pts[:, 0] *= np.float32(0.4)
    return pts


def lattice_values(name):
    """One axis of a lattice geometry: every lo + k * vsize, k = 0 .. grid, its float32 neighbours on both sides, and
    both range ends with theirs."""
    g = geometry(name)
    lo, hi, vs, N = float(g.lo[-1]), float(g.hi[-1]), float(GEOMS[name][0][0]), g.grid[-1]
    edge = np.concatenate([(lo + np.arange(N + 1, dtype=np.float64) * vs), [lo, hi]]).astype(np.float32)
    return np.concatenate([edge, np.nextafter(edge, np.float32(-np.inf)), np.nextafter(edge, np.float32(np.inf))])


def _lattice(name):
    g = geometry(name)
    vals = lattice_values(name)
    vs, lo = float(GEOMS[name][0][0]), float(g.lo[-1])
    rng = np.random.default_rng(11)
    parts = []
    for axis in range(3):
        pts = np.empty((vals.shape[0], 4), np.float64)
        pts[:, :3] = lo + ((np.arange(vals.shape[0]) % 37)[:, None] + 0.5) * vs          # the other axes: mid-cell
        pts[:, 3] = rng.uniform(0, 1, vals.shape[0])
        pts = pts.astype(np.float32)
        pts[:, axis] = vals
        parts.append(pts)
    return np.concatenate(parts)


NONFINITE = (np.float32(np.nan), np.float32(np.inf), np.float32(-np.inf), np.float32(3e38), np.float32(-3e38))


def _nonfinite(payload):
    """300 background points; 15 points with one bad coordinate each (dropped); four cells of two points whose feature
    column 3 holds NaN, inf, -0.0 and a denormal (stored bit for bit).  payload: the NaN carries a payload (for calls
    that only store it: the payload of a COMPUTED NaN is not part of the contract)."""
    bg = _background(300, 5, 21)
    bad = np.tile(np.array([4.05, 0.05, 0.1, 0.5, 0.5], np.float32), (15, 1))
    for col in range(3):
        for k, v in enumerate(NONFINITE):
            bad[col * 5 + k, col] = v
    nan = np.array([0x7FC12345 if payload else 0x7FC00000], np.uint32).view(np.float32)[0]
    special = [nan, np.float32(np.inf), np.float32(-0.0), np.float32(1e-40)]
    feat = np.empty((8, 5), np.float32)
    for k, v in enumerate(special):
        feat[2 * k:2 * k + 2, :3] = np.array([6.05 + 0.2 * k, 0.05, 0.1], np.float32)
        feat[2 * k, 3], feat[2 * k, 4] = v, np.float32(0.25)
        feat[2 * k + 1, 3], feat[2 * k + 1, 4] = (v if k >= 2 else np.float32(1.0)), np.float32(-0.0)
    return np.concatenate([bg[:150], bad[:7], feat, bad[7:], bg[150:]])


def _heavy():
    """5000 points in the cell at x = 6.0, y = 0.0, z = 0.0 and 100 scattered, shuffled."""
    rng = np.random.default_rng(31)
    one = rng.uniform(0, 1, (5000, 4))
    one[:, :3] = np.array([6.005, 0.005, 0.005]) + one[:, :3] * np.array([0.09, 0.09, 0.19])
    pts = np.concatenate([one.astype(np.float32), _background(100, 4, 32)])
    return pts[rng.permutation(pts.shape[0])]


def _rounding():
    """400 background points and three hand-built voxels (7 features; columns 3 .. 6):
    A, two points: means 1 + 2^-11 (f16 tie, down to even), 1 + 3 * 2^-11 (f16 tie, up), 1 + 2^-8 and 1 + 3 * 2^-8 (the
    same for bf16);  B, two points: 1e5 and -1e5 (inf in f16, finite in bf16), 65520 (the f16 tie that rounds to inf);
    C, three points: a float32 division that is inexact."""
    bg = _background(400, 7, 41)
    e = lambda k: np.float32(2.0 ** k)
    one = np.float32(1)
    A = np.array([[6.05, 0.05, 0.1, one, one + e(-10), one, one + e(-7)],
                  [6.05, 0.05, 0.1, one + e(-10), one + e(-9), one + e(-7), one + e(-6)]], np.float32)
    B = np.array([[6.25, 0.05, 0.1, 1e5, -1e5, 65520.0, 65519.0]] * 2, np.float32)
    C = np.array([[6.45, 0.05, 0.1, 0.1, 0.2, 1.0, 1e-3], [6.45, 0.05, 0.1, 0.2, 0.3, 1.0, 1e-3],
                  [6.45, 0.05, 0.1, 0.7, 0.5, 2.0, 2e-3]], np.float32)
    return np.concatenate([bg[:200], A[:1], B[:1], C[:2], bg[200:], A[1:], B[1:], C[2:]])


def _batch3():
    """3000 points, scenes 0 and 2 interleaved (scene 1 stays empty), strays -1 and 3; points 0 and 1 are the same point
    in scenes 0 and 2."""
    pts = _rand("d3", 3000, 4, 51)
    pts[1] = pts[0] = np.array([4.05, 0.05, 0.1, 0.5], np.float32)
    ids = np.tile(np.array([0, 2], np.int32), 1500)
    ids[100:140], ids[2000:2031] = 3, -1
    return pts, ids


@functools.lru_cache(maxsize=None)
def cloud(spec):
    """spec -> (points, batch ids or None), read-only, made once."""
    kind, args = spec[0], spec[1:]
    if kind == "rand":
        return _frozen(_rand(*args))
    if kind == "uniform":
        return _frozen(_uniform(*args))
    if kind == "ubatch":                                        # uniform, with uniform scene ids
        name, n, nfeat, seed, batch = args
        return _frozen(_uniform(name, n, nfeat, seed), np.random.default_rng(seed + 1).integers(0, batch, n))
    if kind == "dup":                                           # the second half repeats the first, shifted by 1e-4
        name, n, nfeat, seed = args
        pts = _uniform(name, n, nfeat, seed)
        pts[n // 2:, :len(GEOMS[name][0])] = pts[: n - n // 2, :len(GEOMS[name][0])] + np.float32(1e-4)
        return _frozen(pts)
    if kind == "lattice":
        return _frozen(_lattice(*args))
    if kind == "nonfinite":
        return _frozen(_nonfinite(*args))
    if kind == "heavy":
        return _frozen(_heavy())
    if kind == "rounding":
        return _frozen(_rounding())
    if kind == "batch3":
        return _frozen(*_batch3())
    if kind == "empty":
        return _frozen(np.zeros((0, args[0]), np.float32))
    raise KeyError(kind)


def _found(spec, name, batch=1):
    pts, ids = cloud(spec)
    return refvoxel.voxelize(pts, geometry(name), pts.shape[0] + 1, 1, batch_ids=ids, batch_size=batch)["found"]


FOUND_D3 = _found(("rand", "d3", 3000, 4, 1), "d3")             # voxels of the d3 cloud most rows use


# ------------------------------------------------------------------------------------------------------------- one-shot
def _one(row, geom, spec, max_voxels, max_points, key_order=False, empty_mean=0, capped=None, tag=""):
    nfeat = cloud(spec)[0].shape[1]
    return dict(row=row, geom=geom, cloud=spec, nfeat=nfeat, max_voxels=max_voxels, max_points=max_points,
                key_order=key_order, empty_mean=empty_mean, capped=capped,
                id=f"{row}-{geom}-f{nfeat}-n{cloud(spec)[0].shape[0]}-v{max_voxels}-p{max_points}"
                   f"-{'key' if key_order else 'first'}-m{empty_mean}{tag}")


def _oneshot_cases():
    out = []
    for nd, name in enumerate(("d1", "d2", "d3", "d4"), 1):                      # dimensions x features
        for k, nfeat in enumerate((nd, nd + 1, 7)):
            for key in (False, True):
                out.append(_one("dims", name, ("rand", name, 3000, nfeat, 60 + nd), 4000, 5, key, (k + key) % 2, False))
    for key in (False, True):                                                    # beyond 2^32 cells: the wide table
        out.append(_one("dims", "wide4", ("dup", "wide4", 3000, 5, 65), 4000, 2, key, 1, False))
    for k, n in enumerate((1, 255, 256, 257, 2047, 2048, 2049, 4097)):            # block edges
        for key in (False, True):
            out.append(_one("sizes", "d3", ("rand", "d3", n, 4, 70 + k), 5000, 5, key, k % 2))
    d3 = ("rand", "d3", 3000, 4, 1)
    out += [_one("caps", "d3", d3, 1, 5, False, 1, True), _one("caps", "d3", d3, 4000, 1, False, 1, False),
            _one("caps", "d3", d3, FOUND_D3, 5, True, 1, False, "-found"),
            _one("caps", "d3", d3, FOUND_D3 - 1, 5, True, 0, True, "-found+1")]
    for mp in (3, 6000):                                                         # one voxel with 5000 points
        for key in (False, True):
            out.append(_one("heavy", "d3", ("heavy",), 200, mp, key, 1))
    for name in LATTICE:
        out.append(_one("lattice", name, ("lattice", name), 20000, 4, False, 1))
    out += [_one("nonfinite", "d3", ("nonfinite", True), 1000, 4, False, 0),
            _one("nonfinite", "d3", ("nonfinite", False), 1000, 4, True, 1)]
    return out


ONESHOT = _oneshot_cases()


@functools.lru_cache(maxsize=None)
def _oneshot_reference(k):
    c = ONESHOT[k]
    pts, _ = cloud(c["cloud"])
    return refvoxel.voxelize(pts, geometry(c["geom"]), c["max_voxels"], c["max_points"], empty_mean=bool(c["empty_mean"]),
                             key_order=c["key_order"])


def oneshot_reference(c):
    return _oneshot_reference(ONESHOT.index(c))


# --------------------------------------------------------------------------------------------------------------- static
def static_constructs(geom, batch_size, max_voxels, key_order):
    """The constructor's gates for key order (a rank map for batch x grid): at most 0xffe00000 cells, a map of at most
    1 GiB, at most 4096 cells per row."""
    if not key_order:
        return True
    cells = batch_size * math.prod(GRIDS[geom])
    return (cells <= 0xFFE00000 and cells <= 0x7FFFFFE0 and refvoxel.rank_map_int32s(cells) * 4 <= (1 << 30)
            and cells <= 4096 * max_voxels)


def _group(row, geom, nfeat, max_voxels, max_points, n_cap, scenes, key_order=True, batch_size=1, mean=None,
           keep_voxels=True, capped=None, device_tail=False, tag=""):
    """scenes: [(cloud spec, live count or None = the whole cloud, empty_mean)], largest first; they run back to back on
    ONE generator."""
    return dict(row=row, geom=geom, nfeat=nfeat, max_voxels=max_voxels, max_points=max_points, n_cap=n_cap,
                scenes=scenes, key_order=key_order, batch_size=batch_size, mean=mean, keep_voxels=keep_voxels,
                capped=capped, device_tail=device_tail,
                id=f"{row}-{geom}-b{batch_size}-f{nfeat}-cap{n_cap}-v{max_voxels}-p{max_points}"
                   f"-{'key' if key_order else 'first'}-{mean or 'nomean'}{'' if keep_voxels else '-novox'}{tag}")


def _static_groups():
    out = []
    means = ("f32", "f16", "bf16", None)
    for nd, name in enumerate(("d1", "d2", "d3", "d4"), 1):                      # dimensions x features
        for k, nfeat in enumerate((nd, nd + 1, 7)):
            for key in (False, True):
                scenes = [(("rand", name, 3000, nfeat, 60 + nd), None, 1), (("rand", name, 500, nfeat, 80 + nd), None, 0),
                          (("empty", nfeat), None, 1)]
                out.append(_group("dims", name, nfeat, 4000, 5, 3000, scenes, key, mean=means[(nd + k) % 4], capped=False))
    out.append(_group("dims", "wide4", 5, 4000, 2, 3000, [(("dup", "wide4", 3000, 5, 65), None, 1),
                                                          (("dup", "wide4", 300, 5, 66), None, 0), (("empty", 5), None, 0)],
                      False, mean="f32", capped=False))
    for k, n_cap in enumerate((1, 256, 257, 2048, 2049)):                         # block edges x live counts
        for key in (False, True):
            lives = sorted({n_cap, n_cap - 1, 1, 0}, reverse=True)
            scenes = [(("rand", "d3", n_cap, 4, 90 + k), live, (j + k) % 2) for j, live in enumerate(lives)]
            out.append(_group("sizes", "d3", 4, 3000, 5, n_cap, scenes, key, mean="f32"))
    d3, small, empty = ("rand", "d3", 3000, 4, 1), ("rand", "d3", 400, 4, 2), ("empty", 4)
    for mv in (255, 256, 257):                                                    # the drop key at the first digit edge
        for key in (False, True):
            out.append(_group("sortwidth", "d3", 4, mv, 5, 3000, [(d3, None, 1), (small, None, 0), (empty, None, 0)], key,
                              mean="f16", capped=True))
    big, less = ("uniform", "sort", 200000, 4, 3), ("uniform", "sort", 5000, 4, 4)
    for k, mv in enumerate((65535, 65536, 65537, 70000)):                         # ... at the second
        for key in (False, True):
            out.append(_group("sortwidth", "sort", 4, mv, 3, 200000, [(big, None, k % 2), (less, None, 0), (empty, None, 0)],
                              key, mean=("bf16", "f16")[k % 2], capped=True))
    for mv in ((1 << 24) - 1, 1 << 24):                                           # ... at the third: three and four passes
        out.append(_group("sortwidth", "d3", 4, mv, 5, 4096, [(("rand", "d3", 4096, 4, 5), None, 0), (empty, None, 0)], False,
                          keep_voxels=False, capped=False, device_tail=True))
    d1 = ("rand", "d1", 3000, 2, 61)                            # (one row of d3's 128 000 cells has no rank map: REJECTED)
    out += [_group("caps", "d3", 4, 1, 5, 3000, [(d3, None, 1), (empty, None, 0)], False, mean="f32", capped=True),
            _group("caps", "d1", 2, 1, 5, 3000, [(d1, None, 1), (("empty", 2), None, 0)], True, mean="f32", capped=True),
            _group("caps", "d3", 4, 4000, 1, 3000, [(d3, None, 1), (empty, None, 0)], True, mean="f32", capped=False),
            _group("caps", "d3", 4, FOUND_D3, 5, 3000, [(d3, None, 1), (empty, None, 0)], True, mean="f32", capped=False,
                   tag="-found"),
            _group("caps", "d3", 4, FOUND_D3 - 1, 5, 3000, [(d3, None, 0), (empty, None, 0)], False, mean="f32", capped=True,
                   tag="-found+1")]
    for mp in (3, 6000):
        out.append(_group("heavy", "d3", 4, 200, mp, 5100, [(("heavy",), None, 1), (small, None, 0), (empty, None, 0)],
                          mp == 3, mean="f32"))
    for name in LATTICE:                                                          # (1600^3 cells: no rank map)
        out.append(_group("lattice", name, 4, 20000, 4, 15000, [(("lattice", name), None, 1), (empty, None, 0)], False,
                          mean="f32"))
    for key in (False, True):
        out.append(_group("nonfinite", "d3", 5, 1000, 4, 400, [(("nonfinite", False), None, 1), (("empty", 5), None, 0)], key,
                          mean="f32"))
        out.append(_group("batch", "d3", 4, 4000, 5, 3000, [(("batch3",), None, 1), (empty, None, 0)], key, batch_size=3,
                          mean="f32"))
    for (name, batch), cells in RANK_CELLS.items():                               # word and block edges of the rank map
        nd = len(GRIDS[name])
        n, mv = (300, 40) if cells < 100 else (6000, 3000)
        scenes = [(("ubatch", name, n, nd + 1, 100 + nd, batch), None, 0), (("ubatch", name, n // 10, nd + 1, 110 + nd, batch), None, 0),
                  (("empty", nd + 1), None, 0)]
        out.append(_group("rankmap", name, nd + 1, mv, 3, n, scenes, True, batch_size=batch, mean="f32",
                          capped=cells >= 100))
    for mean in ("f32", "f16", "bf16"):                                           # rounding of the mean rows
        for keep in (True, False):
            out.append(_group("rounding", "d3", 7, 1000, 4, 500, [(("rounding",), None, int(keep)), (("empty", 7), None, 0)], True,
                              mean=mean, keep_voxels=keep))
    for g in out:
        assert static_constructs(g["geom"], g["batch_size"], g["max_voxels"], g["key_order"]), g["id"]
    return out


STATIC = _static_groups()
# refused by the constructor (ValueError: no rank map for that key space), therefore not cases
REJECTED = [("wide4", 1, 4000, True), ("lat0.05", 1, 20000, True), ("d3", 1, 1, True)]


@functools.lru_cache(maxsize=None)
def _static_reference(k, s):
    g = STATIC[k]
    spec, live, empty_mean = g["scenes"][s]
    pts, ids = cloud(spec)
    return refvoxel.voxelize(pts, geometry(g["geom"]), g["max_voxels"], g["max_points"], batch_ids=ids,
                             batch_size=g["batch_size"], n_live=live, empty_mean=bool(empty_mean), key_order=g["key_order"],
                             mean_dtype=g["mean"], lead=True)


def static_reference(g, s):
    """The live rows of scene s of group g (made once)."""
    return _static_reference(STATIC.index(g), s)


# ---------------------------------------------------------------------------------------------------------------- paths
def oneshot_path(c):
    grid = GRIDS[c["geom"]]
    return dict(form="oneshot", passes=4, table="packed" if refvoxel.keys_fit_u32(1, grid) else "wide", ndim=len(grid),
                key_order=c["key_order"], empty_mean=c["empty_mean"])


def static_paths(g):
    grid = GRIDS[g["geom"]]
    return [dict(form="static", passes=refvoxel.radix_passes(g["max_voxels"]), ndim=len(grid),
                 table="packed" if refvoxel.keys_fit_u32(g["batch_size"], grid) else "wide", key_order=g["key_order"],
                 keep_voxels=g["keep_voxels"], mean=g["mean"], empty_mean=em) for _, _, em in g["scenes"]]


# ------------------------------------------------------------------------------------------------------------ the GPU side
_TORCH_MEAN = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16, None: None}


def _np(t):
    if t.dtype == torch.bfloat16:
        return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)
    return t.cpu().numpy()


def _oneshot_outputs(res):
    v, i, c, pid = res
    return {"voxels": _np(v), "indices": _np(i), "num": _np(c), "pid": _np(pid), "kept": int(v.shape[0])}


def _static_outputs(gen, rows=None, cpu=True):
    kept, found = gen.n_voxels.tolist()
    out = {"kept": kept, "found": found, "indices": gen.indices[:rows], "num": gen.num_per_voxel[:rows],
           "pid": gen.pc_voxel_id}
    if gen.voxels is not None:
        out["voxels"] = gen.voxels[:rows]
    if gen.mean is not None:
        out["mean"] = gen.mean[:rows]
    return {k: (_np(v) if cpu and torch.is_tensor(v) else v) for k, v in out.items()}


def _generator(cuda, g):
    from spconv_amd.pytorch.utils import StaticPointToVoxel
    vs, rng_xyz = GEOMS[g["geom"]]
    gen = StaticPointToVoxel(vs, rng_xyz, g["nfeat"], g["max_voxels"], g["max_points"], g["n_cap"],
                             batch_size=g["batch_size"], key_order=g["key_order"], mean_dtype=_TORCH_MEAN[g["mean"]],
                             keep_voxels=g["keep_voxels"], device=cuda)
    _same_geometry(gen, geometry(g["geom"]))
    return gen


def _same_geometry(gen, geom):
    assert tuple(gen.grid_size) == geom.grid
    assert np.array_equal(np.asarray(gen.vsize, np.float32), geom.vsize)
    assert np.array_equal(np.asarray(gen.coors_range[:geom.ndim], np.float32), geom.lo)


def _load(gen, g, s, cuda):
    """Scene s into the generator's buffers; the rows behind the live count hold valid-looking points."""
    spec, live, _ = g["scenes"][s]
    pts, ids = cloud(spec)
    filler, _ = cloud(("rand", g["geom"], g["n_cap"], g["nfeat"], 999))
    gen.points.copy_(torch.tensor(filler).to(cuda))
    live = pts.shape[0] if live is None else live
    gen.load(torch.tensor(pts[:live]).to(cuda), None if ids is None else torch.tensor(ids[:live]).to(cuda))
    return live


def _check_rank_map(gen, g, want):
    """The map left behind marks exactly the kept voxels' keys, and the rank of each is its row."""
    cells = g["batch_size"] * math.prod(GRIDS[g["geom"]])
    buf = gen.indices._spx_rankmap[0]
    assert buf.numel() == refvoxel.rank_map_int32s(cells)
    keys, rank = refvoxel.decode_rank_map(buf.cpu().numpy(), cells)
    assert np.array_equal(keys, want["keys"]), "the rank map does not mark exactly the kept voxels' cells"
    assert np.array_equal(rank, np.arange(want["kept"])), "the rank of a kept voxel's key is not its row"


@pytest.mark.parametrize("c", ONESHOT, ids=[c["id"] for c in ONESHOT])
def test_oneshot_equals_the_float32_reference(cuda, c):
    from spconv_amd.pytorch.utils import PointToVoxel
    vs, rng_xyz = GEOMS[c["geom"]]
    gen = PointToVoxel(vs, rng_xyz, c["nfeat"], c["max_voxels"], c["max_points"], device=cuda, key_order=c["key_order"])
    _same_geometry(gen, geometry(c["geom"]))
    pts, _ = cloud(c["cloud"])
    got = gen.generate_voxel_with_id(torch.tensor(pts).to(cuda), True, bool(c["empty_mean"]))
    assert_voxels_equal(_oneshot_outputs(got), refvoxel.oneshot_view(oneshot_reference(c)))


@pytest.mark.parametrize("g", STATIC, ids=[g["id"] for g in STATIC])
def test_static_equals_the_float32_reference(cuda, g):
    """The scenes of a group back to back on ONE generator, largest first, the empty one last: a stale row, bit of the
    rank map or table entry of an earlier scene would show."""
    gen = _generator(cuda, g)
    for s, (_, _, empty_mean) in enumerate(g["scenes"]):
        want = static_reference(g, s)
        _load(gen, g, s, cuda)
        out = gen.run(bool(empty_mean))
        assert out is None
        if g["device_tail"]:
            # 2^24 rows: the live head and a margin are copied out, the dead tail is reduced on the device
            rows = want["kept"] + 64
            assert_voxels_equal(_static_outputs(gen, rows), refvoxel.static_view(want, rows, g["n_cap"], g["keep_voxels"]))
            assert bool((gen.indices[rows:] == -1).all()) and not bool(gen.num_per_voxel[rows:].any())
        else:
            assert_voxels_equal(_static_outputs(gen),
                                refvoxel.static_view(want, g["max_voxels"], g["n_cap"], g["keep_voxels"]))
        if g["key_order"]:
            _check_rank_map(gen, g, want)


# ----------------------------------------------------------------------------------------------- quirk fill, wide features
def test_quirk_fill_with_seventy_features(cuda, monkeypatch):
    """empty_mean = 2 (REFERENCE_QUIRKS: the accumulator carried from voxel to voxel) with 70 features: a second wave of
    p2v_mean_carry_kernel.  The fill is the sequential restatement's; everything else is refvoxel's too."""
    import oracle
    from spconv_amd import constants
    from spconv_amd.pytorch.utils import PointToVoxel
    vs, rng_xyz = GEOMS["d3"]
    geom = geometry("d3")
    pts, _ = cloud(("rand", "d3", 600, 70, 7))
    gen = PointToVoxel(vs, rng_xyz, 70, 1000, 4, device=cuda)
    monkeypatch.setattr(constants, "REFERENCE_QUIRKS", True)
    got = _oneshot_outputs(gen.generate_voxel_with_id(torch.tensor(pts).to(cuda), True, True))
    monkeypatch.setattr(constants, "REFERENCE_QUIRKS", False)
    want = refvoxel.oneshot_view(refvoxel.voxelize(pts, geom, 1000, 4))
    rv, ri, rc, rpid = oracle.point2voxel(pts, [float(v) for v in geom.vsize], [float(v) for v in geom.lo] + [float(v) for v in geom.hi],
                                          list(geom.grid), 1000, 4, True, reference_quirks=True)
    assert np.array_equal(ri, want["indices"]) and np.array_equal(rc, want["num"]) and np.array_equal(rpid, want["pid"])
    stored = np.arange(4)[None, :] < rc[:, None]
    assert np.array_equal(rv[stored].view(np.uint32), want["voxels"][stored].view(np.uint32)) and not stored.all()
    want["voxels"] = rv
    assert_voxels_equal(got, want)


# ------------------------------------------------------------------------------------------------------------------ reuse
def test_clear_voxels_false_keeps_what_the_second_call_does_not_write(cuda):
    from spconv_amd.pytorch.utils import PointToVoxel
    vs, rng_xyz = GEOMS["d3"]
    geom = geometry("d3")
    gen = PointToVoxel(vs, rng_xyz, 4, 4000, 5, device=cuda)
    first, _ = cloud(("rand", "d3", 3000, 4, 1))
    second, _ = cloud(("rand", "d3", 400, 4, 2))
    w1, w2 = refvoxel.voxelize(first, geom, 4000, 5), refvoxel.voxelize(second, geom, 4000, 5)
    assert w2["kept"] < w1["kept"] and (w2["num"] < w1["num"][:w2["kept"]]).any()
    assert_voxels_equal(_oneshot_outputs(gen.generate_voxel_with_id(torch.tensor(first).to(cuda))), refvoxel.oneshot_view(w1))
    got = _oneshot_outputs(gen.generate_voxel_with_id(torch.tensor(second).to(cuda), clear_voxels=False))
    buffer = np.zeros((4000, 5, 4), np.uint32)
    buffer[:w1["kept"]] = w1["voxels"].view(np.uint32)
    written = np.arange(5)[None, :] < w2["num"][:, None]
    buffer[:w2["kept"]][written] = w2["voxels"].view(np.uint32)[written]
    want = refvoxel.oneshot_view(w2)
    want["voxels"] = buffer[:w2["kept"]].view(np.float32)
    assert_voxels_equal(got, want)
    assert np.array_equal(gen.voxels.cpu().numpy().view(np.uint32), buffer)      # every other slot: the first call's bits


# ----------------------------------------------------------------------------------------------------------------- repeat
def test_two_runs_of_the_largest_case_are_bit_identical(cuda):
    g = next(g for g in STATIC if g["row"] == "sortwidth" and g["max_voxels"] == 70000 and g["key_order"])
    gen = _generator(cuda, g)
    _load(gen, g, 0, cuda)
    runs = []
    for _ in range(2):
        gen.run(False)
        runs.append([t.clone() for t in (gen.voxels, gen.indices, gen.num_per_voxel, gen.pc_voxel_id, gen.mean, gen.n_voxels,
                                         gen.indices._spx_rankmap[0])])
        gen.voxels.fill_(7.0)                                                    # (every output is written anew)
    for a, b in zip(*runs):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))


# ---------------------------------------------------------------------------------------------------------------- capture
def test_one_capture_replays_three_loads(cuda):
    g = _group("capture", "d3", 4, 4000, 5, 3000, [(("rand", "d3", 3000, 4, 1), None, 0), (("rand", "d3", 400, 4, 2), None, 0),
                                                   (("rand", "d3", 2049, 4, 96), 2048, 0)], True, mean="bf16")
    geom = geometry("d3")
    gen = _generator(cuda, g)
    _load(gen, g, 0, cuda)
    gen.run(False)                                                               # (first use outside the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        gen.run(False)
    for s in (1, 2, 0):
        spec, live, _ = g["scenes"][s]
        pts, _ = cloud(spec)
        want = refvoxel.voxelize(pts, geom, 4000, 5, n_live=live, key_order=True, mean_dtype="bf16", lead=True)
        _load(gen, g, s, cuda)
        graph.replay()
        assert_voxels_equal(_static_outputs(gen), refvoxel.static_view(want, 4000, 3000))
        _check_rank_map(gen, g, want)
