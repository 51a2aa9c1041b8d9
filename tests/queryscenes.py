"""The scenes of the voxel-query tests (test_refquery.py on the CPU, test_gpu_query.py on the device): levels in key
order and 3000 queries each, with the special cases in fixed slots.  Built once, never modified."""
import functools

import numpy as np

import refquery as rq

B, VS, M = 2, 0.25, 3000
LO3 = [-1.75, 2.25, 0.5]            # xyz; multiples of the voxel size, so voxel centres are exact in float32
N_TAIL, N_DEAD = 300, 100           # queries behind the device count; rows behind the live count
LONG_RUN = (1850, 2250)             # with 200 scattered slots: the 600 queries inside one voxel

# name: grid (zyx), live voxels, query_range (zyx), nsample, radii, the cell of the long group, the cell whose window is
# empty, the reach (zyx) no other voxel or query comes nearer than to the reserved ends and to the empty cell
CASES = {
    "A": dict(grid=[8, 20, 24], nv=700, qrange=(1, 2, 3), nsample=8, radii=(None, 0.5), long=(0, 5, 14, 16),
              empty=(1, 4, 10, 12), reach=(1, 2, 3), seed=1),
    "D": dict(grid=[6, 9, 70], nv=900, qrange=(1, 1, 15), nsample=16, radii=(None,), long=(0, 3, 4, 40),
              empty=(1, 2, 4, 30), reach=(1, 4, 15), seed=2),
    "E": dict(grid=[6, 9, 70], nv=900, qrange=(0, 4, 4), nsample=8, radii=(1.0,), long=(0, 3, 4, 40),
              empty=(1, 2, 4, 30), reach=(1, 4, 15), seed=2),
    "2D": dict(grid=[20, 24], nv=150, qrange=(2, 3), nsample=8, radii=(None, 0.5), long=(0, 14, 16), empty=(1, 10, 12),
               reach=(2, 3), seed=3),
    # the windows of D and E in two dimensions, on one more 2-D level: lines of 31 cells, wider than the grid
    "2D-D": dict(grid=[20, 24], nv=150, qrange=(1, 15), nsample=16, radii=(None,), long=(0, 14, 16), empty=(1, 10, 12),
                 reach=(4, 15), seed=4),
    "2D-E": dict(grid=[20, 24], nv=150, qrange=(4, 4), nsample=8, radii=(1.0,), long=(0, 14, 16), empty=(1, 10, 12),
                 reach=(4, 15), seed=4),
}


def all_cells(shape):
    grids = np.meshgrid(np.arange(B), *[np.arange(s) for s in shape], indexing="ij")
    return np.stack([g.reshape(-1) for g in grids], axis=1).astype(np.int32)        # key order: row = key


def near(cells, centre, reach):
    return (cells[:, 0] == centre[0]) & (np.abs(cells[:, 1:] - np.array(centre[1:])) <= np.array(reach)).all(axis=1)


class Scene:
    def __init__(self, name):
        c = CASES[name]
        self.name, self.shape, self.ndim = name, c["grid"], len(c["grid"])
        self.qrange, self.nsample, self.radii = list(c["qrange"]), c["nsample"], c["radii"]
        ndim, shape, reach = self.ndim, self.shape, np.array(c["reach"])
        self.vs, self.lo = [VS] * ndim, LO3[:ndim]
        self.range = self.lo + [self.lo[j] + shape[ndim - 1 - j] * VS for j in range(ndim)]
        rng = np.random.default_rng(c["seed"])
        cells = all_cells(shape)
        first, last = [0] + [0] * ndim, [B - 1] + [s - 1 for s in shape]
        step = np.array([0] * (ndim - 1) + [1])                      # the second and the second-to-last key
        self.reserved = near(cells, first, reach + step) | near(cells, last, reach + step)
        hollow = near(cells, c["empty"], reach)
        ends = [0, 1, len(cells) - 2, len(cells) - 1]                # live voxels no query reaches: empty groups
        border = [int(rq.keys_of(np.array([[1] + [0] * ndim]), shape)[0]),
                  int(rq.keys_of(np.array([[0] + [s - 1 for s in shape]]), shape)[0]),
                  int(rq.keys_of(np.array([c["long"]]), shape)[0])]
        free = np.setdiff1d(np.nonzero(~self.reserved & ~hollow)[0], border)
        pick = np.concatenate([ends, border, rng.choice(free, c["nv"] - len(ends) - len(border), replace=False)])
        self.level = cells[np.sort(pick)]                            # key order
        self.n = len(self.level)
        self.long_cell, self.empty_cell = np.array(c["long"]), np.array(c["empty"])
        self.pts, self.bid = self._queries(rng)
        self.n_queries = M - N_TAIL
        self.n_live = self.n - N_DEAD

    def _queries(self, rng):
        ndim, shape, lo = self.ndim, self.shape, self.lo
        f32 = np.float32
        usable = self.level[~self.reserved[rq.keys_of(self.level, shape)]]
        v = usable[rng.integers(0, len(usable), M)]
        cell = v[:, 1:][:, ::-1].astype(np.float64)                                 # xyz
        pts = np.zeros((M, 4), dtype=f32)
        pts[:, :ndim] = ((cell + rng.random((M, ndim))) * VS + np.array(lo)).astype(f32)
        pts[:, ndim:] = rng.standard_normal((M, 4 - ndim)).astype(f32)              # columns that are no coordinates
        bid = v[:, 0].astype(np.int32)
        c32, lo32 = cell.astype(f32), np.array(lo, dtype=f32)
        pts[0:200, :ndim] = (c32[0:200] + f32(0.5)) * f32(VS) + lo32                # on voxel centres
        hollow = self.empty_cell[1:][::-1]                                          # a valid cell with an empty window
        pts[200:300, :ndim] = ((hollow + rng.random((100, ndim))) * VS + np.array(lo)).astype(f32)
        bid[200:300] = self.empty_cell[0]
        for s, b_, corner in ((400, 1, [0] * ndim), (450, 0, [e - 1 for e in shape[::-1]])):     # in border cells
            pts[s:s + 50, :ndim] = ((np.array(corner) + rng.random((50, ndim))) * VS + np.array(lo)).astype(f32)
            bid[s:s + 50] = b_
        ext = np.array(shape[::-1], dtype=np.float64)
        for i in range(500, 600):                                                   # outside the range, one axis each
            j = int(rng.integers(0, ndim))
            pts[i, j] = f32(lo[j] - 0.05) if i % 2 else f32(lo[j] + ext[j] * VS + 0.05)
        pts[600:610, :ndim] = lo32                                                  # exactly on the lower bound
        bid[600:610] = 1
        for i in range(610, 660):
            pts[i, int(rng.integers(0, ndim))] = np.nan
        pts[660:665, 0] = np.inf
        bid[700:750] = -1
        bid[750:800] = B
        lo_run, hi_run = LONG_RUN                                                   # 600 queries in ONE voxel
        where = np.r_[lo_run:hi_run, rng.choice(np.r_[800:lo_run, hi_run:M - N_TAIL], 200, replace=False)]
        pts[where, :ndim] = ((self.long_cell[1:][::-1] + rng.random((len(where), ndim))) * VS + np.array(lo)).astype(f32)
        bid[where] = self.long_cell[0]
        return pts, bid

    @functools.lru_cache(maxsize=None)
    def ref(self, radius=None, pad="none", n_live=None, n_queries=None):
        """rows, count, offsets, hits, rejected of tests/refquery.py over the key-ordered level"""
        if pad == "first":
            rows, count, offsets, hits, rejected = self.ref(radius, "none", n_live, n_queries)
            return rq.pad_first(rows, count, offsets)[0], count, rq.pad_first(rows, count, offsets)[1], hits, rejected
        return rq.query(self.pts, self.bid, n_queries, self.vs, self.lo, self.level, n_live, B, self.shape, self.qrange,
                        self.nsample, radius)


@functools.lru_cache(maxsize=None)
def scene(name):
    return Scene(name)
