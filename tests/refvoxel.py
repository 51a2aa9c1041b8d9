"""An independent numpy statement of the voxelisers' contract (spx_point2voxel, spx_point2voxel_static), for the tests.

It calls neither the library nor ``oracle``.  The arithmetic that decides a point's cell is FLOAT32 on purpose: the
contract is the reference project's ``floor((x - lo) / vsize)`` in float32, and on the lattice ``lo + k * vsize`` a
float64 floor-divide lands in the neighbouring cell at a fifth of the points -- here "higher precision" is the wrong
answer.  Everything is vectorised over the points; the only Python loops run over the slots of a voxel.

  meta(vsize_xyz, range_xyz)          -> Geometry (zyx, float32 arithmetic, as Point2VoxelCommon::calc_meta_data)
  voxelize(pts, geom, ...)            -> dict: the live rows, first-seen or key order
  static_view(res, max_voxels, n_cap) -> dict: the static form's full-length buffers (dead rows behind the live ones)
  oneshot_view(res)                   -> dict: what PointToVoxel.generate_voxel_with_id returns
  round_bf16(x), mean_rows(...)       -> the mean feature rows and their rounding
  decode_rank_map(buf, cells)         -> (keys marked, rank of each) of a rank map laid out as csrc/rankmap.h says
  assert_voxels_equal(got, want)      -> the ONE comparison of every GPU case (bit views for the floats)
"""
from __future__ import annotations

import collections

import numpy as np

Geometry = collections.namedtuple("Geometry", "ndim vsize lo hi grid")      # all in zyx order; vsize / lo / hi float32

RADIX_BITS = 8               # spx_point2voxel_static sorts by voxel id in 8-bit passes
RANK_WORD_CELLS = 32         # cells per {bits, prefix} word of a rank map
RANK_BLOCK_WORDS = 2048      # words per prefix block


def meta(vsize_xyz, range_xyz) -> Geometry:
    """grid = round((hi - lo) / vsize) in float32, axes reversed to zyx."""
    ndim = len(vsize_xyz)
    assert 1 <= ndim <= 4 and len(range_xyz) == 2 * ndim
    vs = np.asarray(vsize_xyz, np.float32)[::-1].copy()
    lo = np.asarray(range_xyz[:ndim], np.float32)[::-1].copy()
    hi = np.asarray(range_xyz[ndim:], np.float32)[::-1].copy()
    q = (hi - lo) / vs
    assert q.dtype == np.float32 and (q > 0).all()
    grid = np.floor(q + np.float32(0.5)).astype(np.int64)
    return Geometry(ndim, vs, lo, hi, tuple(int(g) for g in grid))


def cell_coordinates(pts: np.ndarray, geom: Geometry):
    """-> (coordinates [n, ndim] int64 (0 where the point is outside), inside [n] bool).  Coordinate j comes from point
    column ndim - 1 - j; a point is inside iff every v = floor((x - lo) / vsize) has v >= 0 and v < grid, in float32:
    NaN and +-inf fail."""
    assert pts.dtype == np.float32 and pts.ndim == 2 and pts.shape[1] >= geom.ndim
    n = pts.shape[0]
    coor = np.zeros((n, geom.ndim), np.int64)
    inside = np.ones((n,), bool)
    with np.errstate(all="ignore"):
        for j in range(geom.ndim):
            v = np.floor((pts[:, geom.ndim - 1 - j] - np.float32(geom.lo[j])) / np.float32(geom.vsize[j]))
            assert v.dtype == np.float32
            ok = (v >= np.float32(0)) & (v < np.float32(geom.grid[j]))
            coor[:, j] = np.where(ok, v, np.float32(0)).astype(np.int64)
            inside &= ok
    coor[~inside] = 0
    return coor, inside


def linear_keys(batch, coor, grid) -> np.ndarray:
    """int64, batch-major, last axis fastest."""
    key = np.asarray(batch, np.int64).copy()
    for j, g in enumerate(grid):
        key = key * int(g) + coor[:, j]
    return key


def round_bf16(x: np.ndarray) -> np.ndarray:
    """float32 -> bfloat16 bits (uint16), nearest-even by the integer rule on the bits; NaN stays NaN."""
    x = np.ascontiguousarray(x, np.float32)
    u = x.view(np.uint32).astype(np.uint64)
    r = ((u + np.uint64(0x7FFF) + ((u >> np.uint64(16)) & np.uint64(1))) >> np.uint64(16)).astype(np.uint16)
    return np.where(np.isnan(x), np.uint16(0x7FC0), r)              # (the quiet NaN torch's conversion gives)


def slot_sums(voxels: np.ndarray, num: np.ndarray) -> np.ndarray:
    """Stored points j = 0 .. num - 1 of every voxel added in that order in float32: [V, F]."""
    acc = np.zeros((voxels.shape[0], voxels.shape[2]), np.float32)
    with np.errstate(all="ignore"):
        for j in range(int(num.max()) if num.size else 0):
            live = num > j
            acc[live] = acc[live] + voxels[live, j]
    assert acc.dtype == np.float32
    return acc


def mean_rows(voxels: np.ndarray, num: np.ndarray, dtype: str) -> np.ndarray:
    """The mean feature rows in `dtype` ("f32" -> float32, "f16" -> float16, "bf16" -> uint16 bits); a voxel without
    points has a zero row."""
    with np.errstate(all="ignore"):
        mean = slot_sums(voxels, num) / np.maximum(num, 1).astype(np.float32)[:, None]
    mean[num <= 0] = 0
    assert mean.dtype == np.float32
    if dtype == "f32":
        return mean
    if dtype == "f16":
        with np.errstate(all="ignore"):
            return mean.astype(np.float16)
    assert dtype == "bf16", dtype
    return round_bf16(mean)


def voxelize(pts: np.ndarray, geom: Geometry, max_voxels: int, max_points: int, *, batch_ids=None, batch_size: int = 1,
             n_live=None, empty_mean: bool = False, key_order: bool = False, mean_dtype=None, lead: bool = False):
    """The live rows.  dict: voxels [kept, max_points, F] float32, indices [kept, ndim (+ 1 with lead: the batch index in
    front)] int32, num [kept] int32, pid [n] int64 (-1: no voxel), keys [kept] int64, found, kept, and mean [kept, F]
    with mean_dtype.  n_live: rows behind it are no points (pid is then n_live long)."""
    pts = np.ascontiguousarray(pts, np.float32)
    if n_live is not None:
        pts = pts[:n_live]
        batch_ids = None if batch_ids is None else np.asarray(batch_ids)[:n_live]
    n, nfeat = pts.shape
    coor, inside = cell_coordinates(pts, geom)
    batch = np.zeros((n,), np.int64) if batch_ids is None else np.asarray(batch_ids, np.int64)
    inside = inside & (batch >= 0) & (batch < batch_size)
    key = linear_keys(np.where(inside, batch, 0), coor, geom.grid)
    # first-seen numbering; the cap keeps the first max_voxels voxels in that order
    live = np.flatnonzero(inside)
    uniq, first, inverse = np.unique(key[live], return_index=True, return_inverse=True)
    by_first = np.argsort(first, kind="stable")
    number = np.empty_like(by_first)
    number[by_first] = np.arange(by_first.shape[0])
    found = int(uniq.shape[0])
    kept = min(found, int(max_voxels))
    pid = np.full((n,), -1, np.int64)
    vid = number[inverse.reshape(-1)]
    pid[live] = np.where(vid < kept, vid, -1)
    first_point = live[first[by_first[:kept]]]                      # the point that opened voxel v
    if key_order:
        order = np.argsort(key[first_point], kind="stable")
        rank = np.empty_like(order)
        rank[order] = np.arange(kept)
        pid = np.where(pid >= 0, rank[np.maximum(pid, 0)], -1)
        first_point = first_point[order]
    # slot of a point inside its voxel: its rank in a stable sort by voxel id
    member = np.flatnonzero(pid >= 0)
    srt = member[np.argsort(pid[member], kind="stable")]
    counts = np.bincount(pid[member], minlength=kept).astype(np.int64)
    start = np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.int64) if kept else np.zeros((0,), np.int64)
    slot = np.arange(srt.shape[0]) - start[pid[srt]]
    stored = slot < max_points
    bits = np.zeros((kept, int(max_points), nfeat), np.uint32)
    bits[pid[srt][stored], slot[stored]] = pts.view(np.uint32)[srt[stored]]       # bit for bit
    voxels = bits.view(np.float32)
    num = np.minimum(counts, max_points).astype(np.int32)
    res = {"found": found, "kept": kept, "num": num, "pid": pid, "keys": key[first_point]}
    idx = coor[first_point].astype(np.int32)
    if lead:
        idx = np.concatenate([batch[first_point].astype(np.int32)[:, None], idx], axis=1)
    res["indices"] = np.ascontiguousarray(idx).reshape(kept, geom.ndim + int(bool(lead)))
    if mean_dtype is not None:
        res["mean"] = mean_rows(voxels, num, mean_dtype)
    if empty_mean:
        with np.errstate(all="ignore"):
            fill = slot_sums(voxels, num) / np.maximum(num, 1).astype(np.float32)[:, None]
        empty = (np.arange(max_points)[None, :] >= num[:, None]) & (num > 0)[:, None]
        voxels = np.where(empty[:, :, None], fill[:, None, :], voxels)
    res["voxels"] = np.ascontiguousarray(voxels, np.float32)
    return res


def oneshot_view(res: dict) -> dict:
    """What PointToVoxel.generate_voxel_with_id returns: the live rows and the per-point ids."""
    return {k: res[k] for k in ("voxels", "indices", "num", "pid", "kept")}


def static_view(res: dict, max_voxels: int, n_cap: int, keep_voxels: bool = True) -> dict:
    """The static form's buffers at full length: live rows first, every row behind them dead -- indices -1 in every
    column, count 0, voxels and mean all-zero bits -- and pc_voxel_id -1 behind the live points."""
    kept = res["kept"]

    def pad(a, rows, value):
        out = np.full((rows,) + a.shape[1:], value, a.dtype)
        out[:a.shape[0]] = a
        return out
    out = {"found": res["found"], "kept": kept, "indices": pad(res["indices"], max_voxels, -1),
           "num": pad(res["num"], max_voxels, 0), "pid": pad(res["pid"], n_cap, -1)}
    if keep_voxels:
        out["voxels"] = pad(res["voxels"], max_voxels, 0)
    if "mean" in res:
        out["mean"] = pad(res["mean"], max_voxels, 0)
    return out


def radix_passes(max_voxels: int) -> int:
    """The eight-bit passes spx_point2voxel_static sorts with: the bytes of the drop key max_voxels."""
    passes = 1
    while passes < 4 and (int(max_voxels) >> (passes * RADIX_BITS)) != 0:
        passes += 1
    return passes


def keys_fit_u32(batch_size: int, grid) -> bool:
    """The packed form of the hash table: every key of batch x grid below 2**32 - 1."""
    v = max(int(batch_size), 1)
    for g in grid:
        v *= max(int(g), 1)
    return v <= 0xFFFFFFFF


def rank_map_words(cells: int) -> int:
    return (int(cells) + RANK_WORD_CELLS - 1) // RANK_WORD_CELLS


def rank_map_int32s(cells: int) -> int:
    """int32 elements of a rank-map buffer: W {bits, prefix} words padded to 256 bytes, then one int32 per block of 2048
    words, padded to 256 bytes."""
    W = rank_map_words(cells)
    up = lambda b: (b + 255) // 256 * 256
    return (up(W * 8) + up((W + RANK_BLOCK_WORDS - 1) // RANK_BLOCK_WORDS * 4)) // 4


def decode_rank_map(buf: np.ndarray, cells: int):
    """-> (keys marked, ascending; rank of each): rank = blockoff[key >> 16] + prefix[key >> 5] + popcount of the bits
    below the key's own in its word."""
    W = rank_map_words(cells)
    buf = np.ascontiguousarray(buf).view(np.uint32).reshape(-1)
    assert buf.shape[0] >= rank_map_int32s(cells), "buffer shorter than the layout"
    words = buf[:2 * W].reshape(W, 2)
    bits, prefix = words[:, 0], words[:, 1].astype(np.int64)
    blockoff = buf[(W * 8 + 255) // 256 * 64:][:(W + RANK_BLOCK_WORDS - 1) // RANK_BLOCK_WORDS].view(np.int32).astype(np.int64)
    table = ((bits[:, None] >> np.arange(32, dtype=np.uint32)[None, :]) & 1).astype(bool)      # [W, 32], bit b = cell
    keys = np.flatnonzero(table.reshape(-1)).astype(np.int64)
    below = np.cumsum(table, axis=1) - table                        # set bits below each bit of its word
    rank = blockoff[keys >> 16] + prefix[keys >> 5] + below.reshape(-1)[keys]
    return keys, rank


def _bits(a: np.ndarray) -> np.ndarray:
    a = np.ascontiguousarray(a)
    if a.dtype.kind == "f":
        return a.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])
    return a


def assert_voxels_equal(got: dict, want: dict) -> None:
    """Every output of `want` is in `got` and equal: same shape, same dtype, same bits (floats are compared through
    their integer views, so -0.0 != +0.0 and a NaN equals only the same NaN); `got` holds nothing else."""
    assert set(got) == set(want), f"outputs differ: got {sorted(got)}, want {sorted(want)}"
    for name in ("kept", "found"):
        if name in want:
            assert int(got[name]) == int(want[name]), f"{name}: got {got[name]}, want {want[name]}"
    for name in sorted(set(want) - {"kept", "found"}):
        g, w = np.asarray(got[name]), np.asarray(want[name])
        assert g.shape == w.shape, f"{name}: shape {g.shape}, want {w.shape}"
        assert g.dtype == w.dtype, f"{name}: dtype {g.dtype}, want {w.dtype}"
        gb, wb = _bits(g), _bits(w)
        if not np.array_equal(gb, wb):
            bad = np.argwhere(gb != wb)
            at = tuple(int(v) for v in bad[0])
            raise AssertionError(f"{name}: {bad.shape[0]} of {gb.size} elements differ, first at {at}: "
                                 f"got {g[at]!r} (bits {int(gb[at]):#x}), want {w[at]!r} (bits {int(wb[at]):#x})")
