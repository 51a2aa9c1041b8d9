"""CPU: the numpy restatement tests/refsector.py (what test_gpu_sector.py holds the kernels to, bit for bit) against
independent float64 formulations -- the sector rule against atan2, the RoI filter against float64 distances, the quotas
against exact fractions -- and the conditions of the shared scenes (tests/sectorscenes.py)."""
import math
from fractions import Fraction

import numpy as np
import pytest

import refsample as rs
import refsector as rsec
import sectorscenes as sc

f32 = np.float32


def ring(n, seed, center=(0.0, 0.0)):
    """n float32 points at radius 0.01 .. 80 about the centre, any angle"""
    rng = np.random.default_rng(seed)
    r, t = 0.01 + rng.random(n) * 79.99, rng.random(n) * 2.0 * np.pi
    return (center[0] + r * np.cos(t)).astype(f32), (center[1] + r * np.sin(t)).astype(f32)


@pytest.mark.parametrize("center", [(0.0, 0.0), sc.CENTER])
@pytest.mark.parametrize("S", [1, 2, 3, 5, 6, 7, 8, 64])
def test_sectors_equal_atan2_away_from_the_boundaries(S, center):
    """200 000 points; the points within 1e-5 rad of a boundary (at most 28 of 200 000 at the centre (0, 0)) are left out,
    on every other one the cross-product rule is floor((atan2 + pi) / (2 pi / S)) of the float32 direction it looks at"""
    x, y = ring(200_000, 10 + S, center)
    got = rsec.sectors(x, y, S, center)
    a = (-(x - f32(center[0]))).astype(np.float64)                       # (the float32 direction, then float64 throughout)
    b = (-(y - f32(center[1]))).astype(np.float64)
    theta = np.arctan2(-b, -a) + np.pi                                   # OpenPCDet: atan2(y, x) + pi
    width = 2.0 * np.pi / S
    off = np.mod(theta, width)
    near = np.minimum(off, width - off) < 1e-5
    assert near.mean() < 1e-3, near.sum()
    want = np.minimum(np.floor(theta / width), S - 1).astype(np.int64)
    assert (got[~near] == want[~near]).all(), int((got[~near] != want[~near]).sum())
    assert got.min() == 0 and got.max() == S - 1 and len(np.unique(got)) == S


def test_boundary_table_is_exact_on_the_axes():
    for S in range(1, 65):
        tab = rsec.table(S)
        assert tab.dtype == f32 and tab.shape == (S, 2) and tab[0].tolist() == [1.0, 0.0]
        for k in range(S):
            if 4 * k % S == 0:
                assert tab[k].tolist() == list(rsec.AXES[4 * k // S]), (S, k)
            else:
                assert abs(float(tab[k, 0]) - math.cos(2 * math.pi * k / S)) < 1e-7, (S, k)
                assert abs(float(tab[k, 1]) - math.sin(2 * math.pi * k / S)) < 1e-7, (S, k)
                assert 0.0 < abs(float(tab[k, 0])) < 1.0 and 0.0 < abs(float(tab[k, 1])) < 1.0


@pytest.mark.parametrize("S", sorted(sc.SPECIAL_SECTORS))
def test_axis_and_origin_cases_by_hand(S):
    pts = sc.special()
    assert rsec.sectors(pts[:, 0], pts[:, 1], S, sc.CENTER).tolist() == sc.SPECIAL_SECTORS[S]
    # about (0, 0) with either zero: the negative x axis (OpenPCDet's dropped index S with y = +0) is sector 0, the
    # positive x axis is half a turn on, the origin is sector 0
    x = np.array([-3.0, -3.0, 3.0, 3.0, 0.0, -0.0, 0.0, -0.0], dtype=f32)
    y = np.array([0.0, -0.0, 0.0, -0.0, 0.0, 0.0, -0.0, -0.0], dtype=f32)
    assert rsec.sectors(x, y, S).tolist() == [0, 0, S // 2, S // 2, 0, 0, 0, 0]


@pytest.mark.parametrize("counts", sc.BOX_COUNTS)
def test_filter_equals_float64_distances_away_from_the_margin(counts):
    """Left out: points whose float64 margin |dist - (half diagonal + radius)| is below 1e-5 of the bound, or whose two
    nearest centres differ by less than 1e-6 relative.  Measured on these scenes: 0 of 6000 points for either set of
    boxes (the cap is 1 %)."""
    pts, bid = sc.base()
    rois, rbid = sc.boxes(counts)
    seg = rsec.sector_ids(pts, bid, sc.B, 1, rois=rois, roi_batch_ids=rbid, roi_radius=sc.RADIUS)
    left_out = 0
    for b in range(sc.B):
        mine = np.nonzero(bid == b)[0]
        bx = rois[rbid == b].astype(np.float64)
        if len(bx) == 0:
            assert (seg[mine] == -1).all()
            continue
        d = np.sqrt(((pts[mine, None, :3].astype(np.float64) - bx[None, :, :3]) ** 2).sum(axis=2))
        order = np.argsort(d, axis=1)
        near = order[:, 0]
        dmin = d[np.arange(len(mine)), near]
        bound = np.sqrt(((0.5 * bx[near, 3:6]) ** 2).sum(axis=1)) + float(f32(sc.RADIUS))
        unsure = np.abs(dmin - bound) < 1e-5 * bound
        if len(bx) > 1:
            second = d[np.arange(len(mine)), order[:, 1]]
            unsure |= (second - dmin) < 1e-6 * second
        left_out += int(unsure.sum())
        want = dmin < bound
        assert ((seg[mine] >= 0) == want)[~unsure].all()
        assert (seg[mine][seg[mine] >= 0] == b).all()
        if len(bx) >= 40:
            assert 0.1 < want.mean() < 0.9, want.mean()                  # both answers are common
    print("left out:", left_out)
    assert left_out <= 0.01 * len(pts)


def test_filter_takes_the_nearest_centre_only_and_the_lowest_index_of_a_tie():
    # a large box further away would hold the point; the small nearer one decides, and turns it down
    rois = np.array([[0, 0, 0, 1, 1, 1, 0], [6, 0, 0, 20, 20, 20, 0]], dtype=f32)
    p = np.array([[2.5, 0, 0]], dtype=f32)
    assert not rsec.roi_keep(p, rois, 0.5)[0] and rsec.roi_keep(p, rois[1:], 0.5)[0]
    # equidistant from two centres (exact in float32): the lower index decides
    tie = np.array([[-4, 0, 0, 1, 1, 1, 0], [4, 0, 0, 8, 8, 8, 0]], dtype=f32)
    o = np.zeros((1, 3), dtype=f32)
    assert not rsec.roi_keep(o, tie, 0.5)[0] and rsec.roi_keep(o, tie[::-1], 0.5)[0]
    # the bound is strict: distance 2 against half diagonal 1.5 (sizes 2, 2, 1) plus radius 0.5
    edge = np.array([[0, 0, 0, 2, 2, 1, 0.3]], dtype=f32)
    assert not rsec.roi_keep(np.array([[2, 0, 0]], dtype=f32), edge, 0.5)[0]
    assert rsec.roi_keep(np.array([[2, 0, 0]], dtype=f32), edge, 0.5001)[0]


def test_invalid_boxes_and_points_are_in_no_segment():
    pts, bid = (a.copy() for a in sc.base())
    rois, rbid = (a.copy() for a in sc.boxes(sc.BOX_COUNTS[1]))
    clean = rsec.sector_ids(pts, bid, sc.B, 6, sc.CENTER, rois, rbid, sc.RADIUS)
    rois[0, 3], rois[1, 4], rois[2, 0], rois[3, 6], rbid[4], rbid[5] = 0.0, -1.0, np.nan, np.inf, -1, sc.B
    pts[7, 0], pts[8, 1], pts[9, 2], bid[10], bid[11] = np.nan, np.inf, -np.inf, -1, sc.B
    seg = rsec.sector_ids(pts, bid, sc.B, 6, sc.CENTER, rois, rbid, sc.RADIUS, n_points=len(pts) - 300, n_rois=150)
    assert (seg[[7, 8, 9, 10, 11]] == -1).all() and (seg[-300:] == -1).all() and (clean[-300:] >= 0).any()
    ok = rsec.valid_boxes(rois, rbid, sc.B, 150)
    assert not set(range(6)) & set(np.concatenate(ok).tolist()) and max(np.concatenate(ok)) < 150
    assert (seg != clean).sum() > 50 and (seg >= 0).sum() > 500            # dropping boxes changed the answer


@pytest.mark.parametrize("S", [1, 2, 6, 64])
def test_quotas_equal_exact_fraction_ceilings(S):
    rng = np.random.default_rng(S)
    for K in (1, 2, 64, 257, 4096, 65_536):
        batch = 5
        sizes = rng.integers(0, 20_000, batch * S)
        sizes[rng.random(batch * S) < 0.2] = 0
        sizes[:S] = 0                                                    # an empty scene
        quota, slot, count = rsec.quotas(sizes, batch, S, K)
        for b in range(batch):
            nk = [int(v) for v in sizes[b * S:(b + 1) * S]]
            n = sum(nk)
            want = [0 if n == 0 else min(v, math.ceil(Fraction(v * K, n))) for v in nk]
            assert quota[b * S:(b + 1) * S].tolist() == want
            assert slot[b * S:(b + 1) * S].tolist() == [sum(want[:k]) for k in range(S)]
            assert count[b] == sum(want) <= K + S - 1
            assert count[b] >= min(n, K)
    ones = rsec.quotas([1] * S, 1, S, 1)
    assert ones[0].tolist() == [1] * S and ones[2].tolist() == [S]       # every one-point sector keeps its point


def test_packed_sampling_of_the_shared_scene():
    pts, bid = sc.base()
    idx, count, seg, quota = rsec.sector_fps(pts, bid, sc.B, 64, 6, center=sc.CENTER)
    assert (np.bincount(seg, minlength=sc.B * 6) > 200).all()            # every sector of every scene is populated
    assert (count >= 64).all() and (count <= 69).all() and quota.reshape(sc.B, 6).sum(axis=1).tolist() == count.tolist()
    for b in range(sc.B):
        row = idx[b]
        assert (row[:count[b]] >= 0).all() and (row[count[b]:] == -1).all()
        assert len(set(row[:count[b]].tolist())) == count[b] and (bid[row[:count[b]]] == b).all()
        assert (np.diff(seg[row[:count[b]]]) >= 0).all()                 # ascending sector
    # one sector and no filter: the packed row is whole-scene farthest-point sampling
    one = rsec.sector_fps(pts, bid, sc.B, 64, 1, center=sc.CENTER)
    want = rs.fps(pts, bid, sc.B, 64)
    assert np.array_equal(one[0], want[0]) and np.array_equal(one[1], want[1])
