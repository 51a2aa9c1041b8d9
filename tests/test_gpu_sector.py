"""Sectorised keypoint sampling on the kernels of csrc/sample.hip (spx_sector_ids, spx_fps_quota, spx_fps_segments;
spconv_amd/pytorch/_sample.py, spatial.SectorFPS) against the numpy restatement tests/refsector.py, over the scenes of
tests/sectorscenes.py (whose conditions test_refsector.py asserts on the CPU).

Every comparison is bit for bit: segment ids, quotas, counts and indices are integers decided by float32 arithmetic in
which numpy rounds every operation on its own (the contract)."""
import numpy as np
import pytest
import torch

import refsample as rs
import refsector as rsec
import samplescenes as ss
import sectorscenes as sc

pytestmark = pytest.mark.gpu

# the new launches are uncounted; what they must NOT do is visible: no whole-scene FPS launch, no groups but the named
KEYS = ("sample/fps", "pointvoxel/groups")


def dev(cuda, a):
    return None if a is None else torch.from_numpy(np.array(a, order="C")).to(cuda)


def count_of(cuda, n):
    return None if n is None else torch.tensor([n], dtype=torch.int32, device=cuda)


def launches():
    from spconv_amd import _lib
    return _lib.launch_counts(KEYS)


def since(before):
    now = launches()
    return {k: now[k] - before[k] for k in KEYS if now[k] != before[k]}


# ------------------------------------------------------------------------------------------------ per-segment K

SIZES = [0, 1, 2, 63, 64, 65, 1023, 1024, 1025]          # valid points per segment
QUOTAS = [1, 2, 64, 64, 257, 0, 257, 2, 64]              # (above the segment's size for 0, 1, 2, 63 and 64)


def segment_cloud(sizes, seed, nfeat=4, extent=4.0):
    """a shuffled cloud: segment g holds sizes[g] valid points and, when it has any, a NaN and an inf point as well; 60
    more points carry the ids -1 and G"""
    rng = np.random.default_rng(seed)
    G = len(sizes)
    ids = np.concatenate([np.repeat(np.arange(G), [v + 2 if v else 0 for v in sizes]), np.repeat([-1, G], 30)])
    pts = (rng.random((len(ids), nfeat)) * extent).astype(np.float32)
    start = 0
    for v in sizes:
        if v:
            pts[start, 0], pts[start + v + 1, nfeat - 2] = np.nan, np.inf
            start += v + 2
    order = rng.permutation(len(ids))
    return np.ascontiguousarray(pts[order]), ids[order].astype(np.int32)


def run_segments(cuda, pts, ids, G, quota, cap, ndim=3):
    from spconv_amd.pytorch import functional as F
    groups = F.point_groups(dev(cuda, ids), G)
    before = launches()
    s = F.farthest_point_sample_segments(dev(cuda, pts), groups, quota, cap, ndim=ndim)
    assert since(before) == {}
    assert s.idx.dtype == torch.int32 and tuple(s.idx.shape) == (G, cap) and tuple(s.count.shape) == (G,)
    np.testing.assert_array_equal(s.batch_ids.cpu().numpy(), np.repeat(np.arange(G, dtype=np.int32), cap))
    return s


def test_segments_read_their_own_k(cuda):
    pts, ids = segment_cloud(SIZES, 3)
    G = len(SIZES)
    index = rsec.segments(ids, G)
    want = rsec.fps_segments(pts, index, QUOTAS, 257)
    assert want[1].tolist() == [min(v, q) for v, q in zip(SIZES, QUOTAS)] and set(QUOTAS) == {0, 1, 2, 64, 257}
    s = run_segments(cuda, pts, ids, G, dev(cuda, np.array(QUOTAS, dtype=np.int32)), 257)
    np.testing.assert_array_equal(s.count.cpu().numpy(), want[1])
    np.testing.assert_array_equal(s.idx.cpu().numpy(), want[0])
    # the host cap clamps the device value, a negative one is 0
    wild = np.array([5, -3, 1 << 30, 257, 100, 101, -(1 << 31), 99, 65_536], dtype=np.int32)
    want = rsec.fps_segments(pts, index, wild, 100)
    assert want[1].tolist() == [0, 0, 2, 63, 64, 65, 0, 99, 100]
    s = run_segments(cuda, pts, ids, G, dev(cuda, wild), 100)
    np.testing.assert_array_equal(s.count.cpu().numpy(), want[1])
    np.testing.assert_array_equal(s.idx.cpu().numpy(), want[0])


def test_an_int_k_over_scene_groups_is_farthest_point_sample(cuda):
    from spconv_amd.pytorch import functional as F
    pts, bid = (a.copy() for a in sc.base())
    bid[3::11], bid[4::11] = -1, sc.B
    pts[5::11, 0], pts[6::11, 2] = np.nan, np.inf
    live = count_of(cuda, len(pts) - 300)
    d_pts, d_bid = dev(cuda, pts), dev(cuda, bid)
    for K in (1, 64, 1800):                              # (1800: more than the valid points of a scene)
        groups = F.scene_groups(d_bid, len(pts), sc.B, live)
        want = F.farthest_point_sample(d_pts, d_bid, sc.B, K, n_points=live, groups=groups)
        got = F.farthest_point_sample_segments(d_pts, groups, K, K)
        assert torch.equal(got.idx, want.idx) and torch.equal(got.count, want.count)
        assert torch.equal(got.batch_ids, want.batch_ids)
    assert int(want.count.max()) < 1800 and int((want.idx >= 0).sum()) == int(want.count.sum())
    few = F.farthest_point_sample_segments(d_pts, groups, 3, 8)         # an int below max_samples
    assert torch.equal(few.idx[:, :3], want.idx[:, :3]) and bool((few.idx[:, 3:] == -1).all()) and few.count.tolist() == [3] * 3


@pytest.mark.parametrize("ndim", [3, 2])
def test_segments_in_both_tiers(cuda, ndim):
    """a segment of exactly resident_points() points stays in registers, one of a point more streams staged records"""
    from spconv_amd.pytorch import _sample
    R = _sample.resident_points()
    rng = np.random.default_rng(7 + ndim)
    ids = np.repeat(np.arange(3, dtype=np.int32), [R, R + 1, 7])[rng.permutation(2 * R + 8)]
    pts = (rng.random((len(ids), ndim + 1)) * 50.0).astype(np.float32)
    want = rsec.fps_segments(pts, rsec.segments(ids, 3), [4, 4, 4], 4, ndim)
    assert want[1].tolist() == [4, 4, 4]
    s = run_segments(cuda, pts, ids, 3, dev(cuda, np.array([4, 4, 4], dtype=np.int32)), 4, ndim)
    np.testing.assert_array_equal(s.idx.cpu().numpy(), want[0])
    np.testing.assert_array_equal(s.count.cpu().numpy(), want[1])


# ------------------------------------------------------------------------------------------------ segment ids

def dirty_cloud():
    """the shared cloud with the axis points in scene 1, ids -1 and B, NaN / inf points, and 300 rows behind the count"""
    pts, bid = sc.base()
    pts = np.concatenate([pts, sc.special()])
    bid = np.concatenate([bid, np.full(len(sc.special()), 1, dtype=np.int32)])
    first = len(pts) - len(sc.special())
    pts = np.concatenate([pts, pts[:300]])
    bid = np.concatenate([bid, bid[:300]])
    bid[3::11][:400], bid[4::11][:400] = -1, sc.B
    pts[5::11, 0][:400], pts[6::11, 1][:400], pts[7::11, 2][:400] = np.nan, np.inf, -np.inf
    return pts, bid, first, len(pts) - 300


def run_ids(cuda, pts, bid, S, center=(0.0, 0.0), rois=None, rbid=None, radius=None, n_points=None, n_rois=None, ndim=3):
    from spconv_amd.pytorch import functional as F
    before = launches()
    seg = F.sector_ids(dev(cuda, pts), dev(cuda, bid), sc.B, S, center=center, rois=dev(cuda, rois),
                       roi_batch_ids=dev(cuda, rbid), roi_radius=radius, n_points=count_of(cuda, n_points),
                       n_rois=count_of(cuda, n_rois), ndim=ndim)
    assert since(before) == ({"pointvoxel/groups": 1} if rois is not None and len(rois) else {})
    assert seg.dtype == torch.int32 and tuple(seg.shape) == (len(pts),)
    return seg.cpu().numpy()


@pytest.mark.parametrize("S", [1, 2, 3, 6, 64])
def test_sector_ids_bit_for_bit(cuda, S):
    pts, bid, first, live = dirty_cloud()
    want = rsec.sector_ids(pts, bid, sc.B, S, sc.CENTER, n_points=live)
    got = run_ids(cuda, pts, bid, S, sc.CENTER, n_points=live)
    np.testing.assert_array_equal(got, want)
    assert (got[live:] == -1).all() and (got[(bid < 0) | (bid >= sc.B)] == -1).all()
    assert (got[~np.isfinite(pts[:, :3]).all(axis=1)] == -1).all()
    assert sorted(np.unique(got).tolist()) == [-1] + list(range(sc.B * S))
    assert (got[first:first + 7] - S).tolist() == sc.SPECIAL_SECTORS[S]          # scene 1: ids S .. 2 S - 1
    # about (0, 0), either zero: the negative x axis and the origin are sector 0, the positive x axis half a turn on
    x = np.array([-3.0, -3.0, 3.0, 3.0, 0.0, -0.0, 0.0, -0.0], dtype=np.float32)
    y = np.array([0.0, -0.0, 0.0, -0.0, 0.0, 0.0, -0.0, -0.0], dtype=np.float32)
    axis = np.stack([x, y, np.zeros(8, dtype=np.float32)], axis=1)
    assert run_ids(cuda, axis, None, S).tolist() == [0, 0, S // 2, S // 2, 0, 0, 0, 0]
    # two columns: the same sectors
    flat = np.ascontiguousarray(pts[:, :2])
    np.testing.assert_array_equal(run_ids(cuda, flat, bid, S, sc.CENTER, n_points=live, ndim=2),
                                  rsec.sector_ids(flat, bid, sc.B, S, sc.CENTER, n_points=live, ndim=2))


def test_sector_ids_do_not_depend_on_the_order_across_scenes(cuda):
    pts, bid = sc.base()
    rois, rbid = sc.boxes(sc.BOX_COUNTS[1])
    new_pts, new_bid, new_row = ss.interleaved(pts, bid)
    for kw in (dict(), dict(rois=rois, rbid=rbid, radius=sc.RADIUS)):
        a = run_ids(cuda, pts, bid, 6, sc.CENTER, **kw)
        b = run_ids(cuda, new_pts, new_bid, 6, sc.CENTER, **kw)
        np.testing.assert_array_equal(b[new_row], a)
        assert (a >= 0).sum() > 1000


# ------------------------------------------------------------------------------------------------ the RoI filter

@pytest.mark.parametrize("counts", sc.BOX_COUNTS)
def test_roi_filter_bit_for_bit(cuda, counts):
    """0, 1, 40 and 129 boxes per scene (129: past a staged tile of 128), in a random order across scenes"""
    from spconv_amd import _lib
    assert max(max(c) for c in sc.BOX_COUNTS) == _lib.load().spx_sector_box_tile() + 1
    pts, bid = sc.base()
    rois, rbid = sc.boxes(counts)
    want = rsec.sector_ids(pts, bid, sc.B, 6, sc.CENTER, rois, rbid, sc.RADIUS)
    got = run_ids(cuda, pts, bid, 6, sc.CENTER, rois, rbid, sc.RADIUS)
    np.testing.assert_array_equal(got, want)
    kept = [(got[bid == b] >= 0).sum() for b in range(sc.B)]
    assert all((k == 0) == (c == 0) for k, c in zip(kept, counts)), kept       # a scene without boxes keeps nothing
    assert all(k < sc.N_SCENE for k in kept)


def test_roi_filter_invalid_boxes_foreign_ids_and_a_device_count(cuda):
    pts, bid, _, live = dirty_cloud()
    rois, rbid = (a.copy() for a in sc.boxes(sc.BOX_COUNTS[1]))
    clean = rsec.sector_ids(pts, bid, sc.B, 6, sc.CENTER, rois, rbid, sc.RADIUS, n_points=live)
    rois[0, 3], rois[1, 4], rois[2, 0], rois[3, 6], rois[6, 5], rbid[4], rbid[5] = 0.0, -1.0, np.nan, np.inf, -np.inf, -1, sc.B
    want = rsec.sector_ids(pts, bid, sc.B, 6, sc.CENTER, rois, rbid, sc.RADIUS, n_points=live, n_rois=150)
    assert (want != clean).sum() > 50 and (want >= 0).sum() > 500
    got = run_ids(cuda, pts, bid, 6, sc.CENTER, rois, rbid, sc.RADIUS, n_points=live, n_rois=150)
    np.testing.assert_array_equal(got, want)
    # no boxes at all, and boxes that are all invalid: nothing is kept
    assert (run_ids(cuda, pts, bid, 6, sc.CENTER, rois[:0], rbid[:0], sc.RADIUS) == -1).all()
    bad = rois.copy()
    bad[:, 4] = 0.0
    assert (run_ids(cuda, pts, bid, 6, sc.CENTER, bad, rbid, sc.RADIUS) == -1).all()


def test_roi_filter_exact_cases(cuda):
    """float32-exact scenes: the nearest centre alone decides, a tie goes to the lower box index, the bound is strict"""
    f32 = np.float32
    zero = np.zeros(1, dtype=np.int32)
    run = lambda p, boxes, r: run_ids(cuda, np.array(p, dtype=f32), zero[:len(p)], 1, rois=np.array(boxes, dtype=f32),
                                      rbid=np.zeros(len(boxes), dtype=np.int32), radius=r).tolist()
    small_near, large_far = [0, 0, 0, 1, 1, 1, 0], [6, 0, 0, 20, 20, 20, 0]
    assert run([[2.5, 0, 0]], [small_near, large_far], 0.5) == [-1] and run([[2.5, 0, 0]], [large_far], 0.5) == [0]
    left, right = [-4, 0, 0, 1, 1, 1, 0], [4, 0, 0, 8, 8, 8, 0]
    assert run([[0, 0, 0]], [left, right], 0.5) == [-1] and run([[0, 0, 0]], [right, left], 0.5) == [0]
    edge = [0, 0, 0, 2, 2, 1, 0.3]
    assert run([[2, 0, 0]], [edge], 0.5) == [-1] and run([[2, 0, 0]], [edge], 0.5001) == [0]


# ------------------------------------------------------------------------------------------------ sector_fps

def run_sector_fps(cuda, pts, bid, B, K, S, filtered, n_points=None, n_rois=None):
    from spconv_amd.pytorch import functional as F
    rois, rbid = sc.boxes(sc.BOX_COUNTS[1]) if filtered else (None, None)
    kw = dict(center=sc.CENTER, rois=dev(cuda, rois), roi_batch_ids=dev(cuda, rbid), roi_radius=sc.RADIUS if filtered else None,
              n_points=count_of(cuda, n_points), n_rois=count_of(cuda, n_rois))
    before = launches()
    s, seg, quota = F.sector_fps(dev(cuda, pts), dev(cuda, bid), B, K, S, return_sectors=True, **kw)
    assert since(before) == {"pointvoxel/groups": 2 if filtered else 1}       # the box groups and the segment groups
    W = K + S - 1
    assert s.idx.dtype == torch.int32 and tuple(s.idx.shape) == (B, W) and tuple(s.count.shape) == (B,)
    assert tuple(seg.shape) == (len(pts),) and tuple(quota.shape) == (B * S,)
    np.testing.assert_array_equal(s.batch_ids.cpu().numpy(), np.repeat(np.arange(B, dtype=np.int32), W))
    want = rsec.sector_fps(pts, bid, B, K, S, center=sc.CENTER, rois=rois, roi_batch_ids=rbid,
                           roi_radius=sc.RADIUS if filtered else None, n_points=n_points, n_rois=n_rois)
    return s, seg, quota, want


def assert_packed(idx, count, bid, K, S):
    """no -1 below count, only -1 at or beyond it, distinct indices of the row's own scene"""
    for b in range(len(count)):
        row, c = idx[b], int(count[b])
        assert c <= K + S - 1 and (row[:c] >= 0).all() and (row[c:] == -1).all()
        assert len(set(row[:c].tolist())) == c and (bid[row[:c]] == b).all()


@pytest.mark.parametrize("filtered", [False, True])
@pytest.mark.parametrize("K,S", [(1, 6), (64, 6), (257, 3), (64, 64)])
def test_sector_fps_bit_for_bit(cuda, K, S, filtered):
    pts, bid, _, live = dirty_cloud()
    s, seg, quota, want = run_sector_fps(cuda, pts, bid, sc.B, K, S, filtered, n_points=live, n_rois=150 if filtered else None)
    np.testing.assert_array_equal(seg.cpu().numpy(), want[2])
    np.testing.assert_array_equal(quota.cpu().numpy(), want[3])
    np.testing.assert_array_equal(s.count.cpu().numpy(), want[1])
    np.testing.assert_array_equal(s.idx.cpu().numpy(), want[0])
    idx, count = s.idx.cpu().numpy(), s.count.cpu().numpy()
    assert_packed(idx, count, bid, K, S)
    kept = np.bincount(want[2][want[2] >= 0] // S, minlength=sc.B)
    assert (count >= np.minimum(kept, K)).all() and (kept > 0).all() and int(idx.max()) < live
    for b in range(sc.B):                                               # ascending sector inside a row
        assert (np.diff(want[2][idx[b, :count[b]]]) >= 0).all()
    again = run_sector_fps(cuda, pts, bid, sc.B, K, S, filtered, n_points=live, n_rois=150 if filtered else None)[0]
    assert torch.equal(s.idx, again.idx) and torch.equal(s.count, again.count)       # identical run to run


def test_one_sector_without_a_filter_is_farthest_point_sample(cuda):
    from spconv_amd.pytorch import functional as F
    pts, bid, _, live = dirty_cloud()
    d_pts, d_bid, n = dev(cuda, pts), dev(cuda, bid), count_of(cuda, live)
    for K in (1, 64, 257):
        a = F.sector_fps(d_pts, d_bid, sc.B, K, 1, center=sc.CENTER, n_points=n)
        b = F.farthest_point_sample(d_pts, d_bid, sc.B, K, n_points=n)
        assert tuple(a.idx.shape) == (sc.B, K) and torch.equal(a.idx, b.idx) and torch.equal(a.count, b.count)


def test_one_point_sectors_and_an_empty_scene(cuda):
    """every sector of scene 0 holds one point: at K = 1 each keeps it (count = S); scene 1 is empty, scene 2 is turned
    down whole by the filter (OpenPCDet would fall back to its first point: here the count is 0)"""
    from spconv_amd.pytorch import functional as F
    S = 6
    angle = (np.arange(S) + 0.5) * 2.0 * np.pi / S
    ring = np.stack([-5.0 * np.cos(angle), -5.0 * np.sin(angle), np.zeros(S)], axis=1).astype(np.float32)
    far = np.full((4, 3), 500.0, dtype=np.float32)
    pts = np.concatenate([ring[::-1], far])
    bid = np.array([0] * S + [2] * 4, dtype=np.int32)
    s, seg, quota = F.sector_fps(dev(cuda, pts), dev(cuda, bid), 3, 1, S, return_sectors=True)
    assert seg.tolist() == list(range(S))[::-1] + [2 * S + 3] * 4           # (the far points: 225 degrees, sector 3)
    assert quota.tolist() == [1] * S + [0] * S + [0, 0, 0, 1, 0, 0]
    assert s.count.tolist() == [S, 0, 1]
    assert s.idx.tolist() == [list(range(S))[::-1], [-1] * S, [S] + [-1] * (S - 1)]
    box = np.array([[0, 0, 0, 4, 4, 4, 0], [0, 0, 0, 4, 4, 4, 0]], dtype=np.float32)
    s = F.sector_fps(dev(cuda, pts), dev(cuda, bid), 3, 1, S, rois=dev(cuda, box),
                     roi_batch_ids=dev(cuda, np.array([0, 2], dtype=np.int32)), roi_radius=2.0)
    assert s.count.tolist() == [S, 0, 0] and bool((s.idx[1:] == -1).all())
    none = F.sector_fps(dev(cuda, pts[:0]), dev(cuda, bid[:0]), 3, 5, S)                # no points at all
    assert none.count.tolist() == [0, 0, 0] and tuple(none.idx.shape) == (3, 5 + S - 1) and bool((none.idx == -1).all())


def test_sector_fps_module_and_what_takes_its_samples(cuda):
    import spconv_amd.pytorch as spconv
    F = spconv.functional
    pts, bid = sc.base()
    rois, rbid = sc.boxes(sc.BOX_COUNTS[1])
    d_pts, d_bid, d_rois, d_rbid = dev(cuda, pts), dev(cuda, bid), dev(cuda, rois), dev(cuda, rbid)
    s = spconv.SectorFPS(64, 6, sc.RADIUS, sc.CENTER)(d_pts, d_bid, sc.B, d_rois, d_rbid)
    want = rsec.sector_fps(pts, bid, sc.B, 64, 6, center=sc.CENTER, rois=rois, roi_batch_ids=rbid, roi_radius=sc.RADIUS)
    np.testing.assert_array_equal(s.idx.cpu().numpy(), want[0])
    np.testing.assert_array_equal(s.count.cpu().numpy(), want[1])
    plain = spconv.SectorFPS(64, center=sc.CENTER)(d_pts, d_bid, sc.B)
    np.testing.assert_array_equal(plain.idx.cpu().numpy(), rsec.sector_fps(pts, bid, sc.B, 64, 6, center=sc.CENTER)[0])
    keys = F.gather_samples(d_pts, s)                                   # dead slots are NaN rows: invalid queries
    assert tuple(keys.shape) == (sc.B * 69, 4) and int(torch.isnan(keys[:, 0]).sum()) == sc.B * 69 - int(s.count.sum())
    nb = F.ball_query(keys, s.batch_ids, d_pts, d_bid, sc.B, 3.0, 16)
    flat = want[0].reshape(-1)
    ref = rs.ball_query(np.where((flat >= 0)[:, None], pts[np.clip(flat, 0, None), :3], np.float32(np.nan)),
                        np.repeat(np.arange(sc.B, dtype=np.int32), 69), None, pts, bid, None, sc.B, 3.0, 16)
    np.testing.assert_array_equal(nb.rows.cpu().numpy(), ref[0])
    np.testing.assert_array_equal(nb.count.cpu().numpy(), ref[1])
    assert (ref[1][flat >= 0] >= 1).all() and (ref[1][flat < 0] == 0).all()


# ------------------------------------------------------------------------------------------------ capture

def test_capture_sector_sampling_and_ball_query_in_one_graph(cuda):
    """box groups -> sector_ids -> point_groups -> quotas -> segmented FPS -> gather_samples -> ball_query on ONE stream
    in one graph, replayed on a second cloud with other device point and box counts copied into the static buffers"""
    from spconv_amd.pytorch import functional as F
    base_pts, base_bid = sc.base()
    other_pts, other_bid, _ = ss.interleaved(base_pts * np.float32(0.97), base_bid, seed=9)
    rois, rbid = sc.boxes(sc.BOX_COUNTS[1])
    sets = [(base_pts, base_bid, len(base_pts), rois, rbid, len(rois)),
            (other_pts, other_bid, len(base_pts) - 700, rois[::-1], rbid[::-1], 100)]
    N, M, K, S, NS = len(base_pts), len(rois), 96, 6, 16
    points = torch.empty((N, 4), dtype=torch.float32, device=cuda)
    bid = torch.empty((N,), dtype=torch.int32, device=cuda)
    boxes = torch.empty((M, 8), dtype=torch.float32, device=cuda)
    box_ids = torch.empty((M,), dtype=torch.int32, device=cuda)
    n_points, n_rois = (torch.empty((1,), dtype=torch.int32, device=cuda) for _ in range(2))

    def step():
        s, seg, quota = F.sector_fps(points, bid, sc.B, K, S, center=sc.CENTER, rois=boxes, roi_batch_ids=box_ids,
                                     roi_radius=sc.RADIUS, n_points=n_points, n_rois=n_rois, return_sectors=True)
        keys = F.gather_samples(points, s)
        nb = F.ball_query(keys, s.batch_ids, points, bid, sc.B, 4.0, NS, pad="first", n_points=n_points)
        return s.idx, s.count, seg, quota, keys, nb.rows, nb.count

    def load(k):
        points.copy_(dev(cuda, sets[k][0]))
        bid.copy_(dev(cuda, sets[k][1]))
        n_points.fill_(sets[k][2])
        boxes.copy_(dev(cuda, sets[k][3]))
        box_ids.copy_(dev(cuda, sets[k][4]))
        n_rois.fill_(sets[k][5])
    eager = []
    for k in (0, 1):
        load(k)
        got = [t.clone() for t in step()]
        pts_k, bid_k, live, rois_k, rbid_k, live_rois = sets[k]
        want = rsec.sector_fps(pts_k, bid_k, sc.B, K, S, center=sc.CENTER, rois=rois_k, roi_batch_ids=rbid_k,
                               roi_radius=sc.RADIUS, n_points=live, n_rois=live_rois)
        for g, w in zip(got[:4], want):
            np.testing.assert_array_equal(g.cpu().numpy(), w)
        flat = want[0].reshape(-1)
        ref = rs.ball_query(np.where((flat >= 0)[:, None], pts_k[np.clip(flat, 0, None), :3], np.float32(np.nan)),
                            np.repeat(np.arange(sc.B, dtype=np.int32), K + S - 1), None, pts_k, bid_k, live, sc.B, 4.0, NS,
                            3, "first")
        np.testing.assert_array_equal(got[5].cpu().numpy(), ref[0])
        assert int(got[5].max()) < live and int((got[6] == NS).sum()) > 20 and int((got[6] < NS).sum()) > 20
        eager.append(got)
    assert not torch.equal(eager[0][0], eager[1][0])
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = step()
    for k in (1, 0, 1):
        load(k)
        graph.replay()
        torch.cuda.synchronize()
        for got, want in zip(outs, eager[k]):
            a, b = got.cpu().contiguous(), want.cpu().contiguous()
            np.testing.assert_array_equal(a.view(torch.int32).numpy(), b.view(torch.int32).numpy())
