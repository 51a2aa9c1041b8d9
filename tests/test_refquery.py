"""CPU: the numpy restatement tests/refquery.py against an independent formulation of the voxel query (all live voxels
filtered by window and radius in float64, sorted by key, truncated), and the conditions the scenes of
test_gpu_query.py must meet -- counted from the restatement alone."""
import numpy as np
import pytest

import queryscenes as qs
import refquery as rq

CONFIGS = [(name, radius) for name in qs.CASES for radius in qs.CASES[name]["radii"]]


def independent(sc, radius):
    """per query the kept rows by the other route, or None where it cannot decide (a distance within 1e-6 of the
    radius, a cell that float64 places elsewhere); also the number of hits looked at and of those left undecided"""
    ndim, shape = sc.ndim, sc.shape
    level = sc.level.astype(np.int64)
    keys = rq.keys_of(level, shape)
    centres = (level[:, 1:][:, ::-1] + 0.5) * qs.VS + np.array(sc.lo)               # xyz, float64
    lo, ext = np.array(sc.lo), np.array(shape[::-1])
    qrange_xyz = np.array(sc.qrange[::-1])
    out, looked, undecided = [], 0, 0
    for m in range(qs.M):
        q, b = sc.pts[m, :ndim].astype(np.float64), int(sc.bid[m])
        with np.errstate(invalid="ignore"):
            cell = np.floor((q - lo) / qs.VS)
        if not (0 <= b < qs.B) or not np.all((cell >= 0) & (cell < ext)):           # (false for NaN)
            out.append(np.zeros(0, dtype=np.int64))
            continue
        inside = (level[:, 0] == b) & (np.abs(level[:, 1:][:, ::-1] - cell) <= qrange_xyz).all(axis=1)
        cand = np.nonzero(inside)[0]
        if radius is not None:
            d2 = ((centres[cand] - q) ** 2).sum(axis=1)
            r2 = float(np.float32(radius)) ** 2
            looked += len(cand)
            if (np.abs(d2 - r2) <= 1e-6).any():
                undecided += int((np.abs(d2 - r2) <= 1e-6).sum())
                out.append(None)
                continue
            cand = cand[d2 < r2]
        else:
            looked += len(cand)
        out.append(cand[np.argsort(keys[cand])][:sc.nsample])
    return out, looked, undecided


@pytest.mark.parametrize("name,radius", CONFIGS)
def test_restatement_against_the_independent_formulation(name, radius):
    sc = qs.scene(name)
    rows, count, offsets, hits, rejected = sc.ref(radius)
    want, looked, undecided = independent(sc, radius)
    assert looked > 5000 and undecided < 0.01 * looked
    decided = 0
    for m in range(qs.M):
        if want[m] is None:
            continue
        decided += 1
        assert count[m] == len(want[m]), m
        assert rows[m, :count[m]].tolist() == want[m].tolist(), m
        assert (rows[m, count[m]:] == -1).all() and (offsets[m, count[m]:] == 0).all()
        kept = sc.level[rows[m, :count[m]]].astype(np.float64)
        centres = (kept[:, 1:][:, ::-1] + 0.5) * qs.VS + np.array(sc.lo)
        assert np.abs(offsets[m, :count[m]] - (centres - sc.pts[m, :sc.ndim])).max(initial=0) <= 1e-5
    assert decided > 0.9 * qs.M
    if radius == 0.5:       # the queries on voxel centres: the voxels exactly two cells away are undecidable in float64
        assert sum(w is None for w in want[:200]) >= 20


@pytest.mark.parametrize("name,radius", CONFIGS)
def test_the_scenes_hold_the_cases_they_claim(name, radius):
    sc = qs.scene(name)
    rows, count, offsets, hits, rejected = sc.ref(radius)
    ns, n = sc.nsample, sc.n
    truncated, partial = int((hits > ns).sum()), int(((hits > 0) & (hits < ns)).sum())
    print(f"{name} radius {radius}: {truncated} truncated, {partial} partial, mean hits {hits.mean():.2f}, "
          f"{int((rejected > 0).sum())} queries with a rejected cell")
    if (name, radius) in (("A", None), ("D", None), ("E", 1.0), ("2D", None), ("2D-D", None), ("2D-E", 1.0)):
        assert truncated >= 100 and partial >= 100
    if radius is not None:
        assert (rejected > 0).sum() >= 100                  # the radius turns down an occupied window cell
    assert (count == np.minimum(hits, ns)).all()
    assert (count[200:300] == 0).all()                      # valid queries whose window holds no voxel
    table = rq.live_table(sc.level, None, qs.B, sc.shape)
    for m in range(200, 300):
        assert rq.query_cell(sc.pts[m], sc.bid[m], sc.vs, sc.lo, qs.B, sc.shape) is not None
    assert (count[500:600] == 0).all() and (count[610:665] == 0).all() and (count[700:800] == 0).all()
    assert (rows[500:600] == -1).all() and (rows[700:800] == -1).all()
    assert (count[400:500] > 0).all()                       # border cells at both ends of every axis
    for s, cell in ((400, [0] * sc.ndim), (450, [e - 1 for e in sc.shape])):
        for m in range(s, s + 50):
            assert rq.query_cell(sc.pts[m], sc.bid[m], sc.vs, sc.lo, qs.B, sc.shape) == cell
    assert (count[600:610] > 0).all()                       # exactly on the lower bound: cell 0
    # both ends of the key space hold live voxels that no query reaches
    assert not np.isin(rows, [0, 1, n - 2, n - 1]).any()
    assert rq.keys_of(sc.level[:2], sc.shape).tolist() == [0, 1]
    # the long group
    sizes = np.diff(rq.transposed(rows, n)[0])
    assert sizes.max() >= 600 and (sizes[[0, 1, n - 2, n - 1]] == 0).all()
    if radius == 0.5:
        # on voxel centres, a voxel exactly two cells away along x has d2 == r2: the strict < turns it down
        exact = 0
        for m in range(200):
            cell = rq.query_cell(sc.pts[m], sc.bid[m], sc.vs, sc.lo, qs.B, sc.shape)
            for step in (-2, 2):
                v = cell[:-1] + [cell[-1] + step]
                if 0 <= v[-1] < sc.shape[-1]:
                    r = table.get(int(rq.keys_of(np.array([[sc.bid[m]] + v]), sc.shape)[0]))
                    if r is not None:
                        exact += 1
                        assert r not in rows[m]
        assert exact >= 20
    # rows behind the live count would be found: the count makes a difference
    blind, cut = rows, sc.ref(radius, "none", sc.n_live)[0]
    assert (blind >= sc.n_live).sum() > 30 and cut.max() < sc.n_live and (cut != blind).sum() > 30
    # the device query count
    tail = sc.ref(radius, "none", None, sc.n_queries)
    assert (tail[0][sc.n_queries:] == -1).all() and (tail[1][sc.n_queries:] == 0).all() and (count[sc.n_queries:] > 0).any()
    assert (tail[0][:sc.n_queries] == rows[:sc.n_queries]).all()


def test_pad_first_repeats_slot_zero():
    sc = qs.scene("A")
    rows, count, offsets, _, _ = sc.ref(None)
    prow, pcount, poff, _, _ = sc.ref(None, "first")
    assert (pcount == count).all()
    for m in range(qs.M):
        k = count[m]
        assert (prow[m, :k] == rows[m, :k]).all() and (poff[m, :k] == offsets[m, :k]).all()
        if k > 0:
            assert (prow[m, k:] == rows[m, 0]).all() and (poff[m, k:] == offsets[m, 0]).all()
        else:
            assert (prow[m] == -1).all() and (poff[m] == 0).all()


def test_gather_and_sequential_gradient():
    rows = np.array([[2, 0, -1], [2, 2, -1], [-1, -1, -1], [1, 2, 0]], dtype=np.int32)
    vfeat = np.arange(12, dtype=np.float32).reshape(4, 3)
    out = rq.group(vfeat, rows)
    assert out.shape == (4, 3, 3) and (out[0, 0] == vfeat[2]).all() and (out[2] == 0).all() and (out[0, 2] == 0).all()
    offsets, lst = rq.transposed(rows, 4)
    assert offsets.tolist() == [0, 2, 3, 7, 7] and lst.tolist() == [1, 11, 9, 0, 3, 4, 10]
    dout = np.random.default_rng(0).standard_normal((12, 3)).astype(np.float32)
    grad = rq.group_backward(dout, rows, 4)
    want2 = ((dout[0] + dout[3]) + dout[4]) + dout[10]
    assert (grad[2] == want2).all() and (grad[3] == 0).all() and (grad[1] == dout[9]).all()
    assert (rq.group_backward(dout, rows, 4, n_live=2)[2:] == 0).all()
