"""Points in rotated boxes on the kernels of csrc/roi.hip (spconv_amd/pytorch/_roi.py, spatial.RoIPointPool3d /
RoIAwarePool3d) against the numpy float32 restatement tests/refroi.py (whose conditions test_refroi.py asserts on the
CPU).

The frames are held to float64 numpy within a derived bound (the sine and cosine are the one step a host does not
reproduce).  The device's own frames are then downloaded and handed to refroi, and everything downstream of them -- the
box of every point, rows, count, hits, local, cells, the pads -- is compared bit for bit.  Every box-major call goes
through ``box_query_into`` with buffers filled with junk first."""
import functools

import numpy as np
import pytest
import torch

import refroi

pytestmark = pytest.mark.gpu

TILE, WAVES = 128, 4            # spx_points_in_boxes_tile(), spx_box_query_waves() (asserted below)
PADS = {"none": refroi.PAD_NONE, "first": refroi.PAD_FIRST, "cycle": refroi.PAD_CYCLE}


def bits(t):
    t = t.detach().cpu().contiguous()
    return t.view({4: torch.int32, 2: torch.int16}[t.element_size()]).numpy()


def dev(cuda, a):
    return None if a is None else torch.from_numpy(np.array(a, order="C")).to(cuda)


def count_of(cuda, n):
    return None if n is None else torch.tensor([n], dtype=torch.int32, device=cuda)


def junk(cuda, shape, dtype):
    t = torch.empty(shape, dtype=dtype, device=cuda)
    t.view(torch.int32).fill_(0x7fc12345 if dtype == torch.float32 else 0x12345678)
    return t


def device_frames(cuda, boxes, n_boxes=None, extra=0.0):
    """(BoxFrames on the device, the DOWNLOADED frames)"""
    from spconv_amd.pytorch import functional as F
    fr = F.boxes_to_frames(dev(cuda, boxes), count_of(cuda, n_boxes), extra)
    return fr, fr.frames.cpu().numpy()


def spoil(boxes, rows):
    """NaN, Inf, zero and negative sizes in the given rows, one kind after the other"""
    kinds = [(0, np.nan), (1, np.inf), (6, -np.inf), (3, 0.0), (4, -1.0), (5, 0.0), (2, np.nan), (5, -2.0)]
    for t, r in enumerate(rows):
        col, v = kinds[t % len(kinds)]
        boxes[r, col] = v
    return boxes


def test_constants():
    from spconv_amd import _lib
    assert _lib.load().spx_points_in_boxes_tile() == TILE and _lib.load().spx_box_query_waves() == WAVES


# ------------------------------------------------------------------------------------------------ frames

def test_frames_against_float64_numpy(cuda):
    """x, y, z and the half sizes are float32 copies / one product and one sum: bit for bit.  Cosine and sine: a
    magnitude of at most 1, so an ulp of at most 2^-24 below 1; the 4-ulp cosf / sinf of OpenCL's full profile (the
    argument reduction included: headings up to +-100) gives |c - cos| <= 4 * 2^-24, the float64 reference errs by
    2^-53.  Asserted: 4 * 2^-24.  Measured worst on an MI355X: 1.00 x 2^-24."""
    from spconv_amd.pytorch import _roi
    n, live = 1500, 1400
    rng = np.random.default_rng(23)
    b = np.zeros((n, 8), np.float32)
    b[:, :3] = rng.random((n, 3)) * 200.0 - 100.0
    b[:, 3:6] = 0.2 + rng.random((n, 3)) * 10.0
    b[:, 6] = rng.random(n) * 200.0 - 100.0
    b[:10, 6] = [0.0, -0.0, np.pi / 2, -np.pi / 2, 100.0, -100.0, np.pi, -np.pi, 1e-30, 8.0]
    bad = np.arange(20, 1300, 37)
    spoil(b, bad)
    extra = (0.25, 0.5, 1.0)
    frames = junk(cuda, (n, 8), torch.float32)
    _roi.frames_into(dev(cuda, b), count_of(cuda, live), extra, frames)
    got = frames.cpu().numpy()
    dead = np.zeros(n, bool)
    dead[bad], dead[live:] = True, True
    assert np.isnan(got[dead]).all() and np.isfinite(got[~dead]).all()        # every element written
    ok = ~dead
    c64, s64 = np.cos(b[ok, 6].astype(np.float64)), np.sin(b[ok, 6].astype(np.float64))
    want = refroi.frames_given_trig(b, got[:, 6], got[:, 7], extra, live)
    np.testing.assert_array_equal(got[ok, :6].view(np.int32), want[ok, :6].view(np.int32))
    err = max(np.abs(got[ok, 6] - c64).max(), np.abs(got[ok, 7] - s64).max())
    print(f"frames: worst |c - cos|, |s - sin| = {err / 2.0 ** -24:.2f} x 2^-24")
    assert err <= 4.0 * 2.0 ** -24
    np.testing.assert_array_equal(got[0, 6:].view(np.int32), np.array([1.0, 0.0], np.float32).view(np.int32))
    assert got[1, 6] == 1.0 and got[1, 7] == 0.0                      # (heading -0.0)
    # the public form: the same bits, NaN beyond the count
    fr, host = device_frames(cuda, b, live, extra)
    np.testing.assert_array_equal(host.view(np.int32), got.view(np.int32))
    assert fr.num_boxes == n and tuple(device_frames(cuda, b[:0])[1].shape) == (0, 8)


def test_faces_strict_in_the_plane_inclusive_in_z(cuda):
    from spconv_amd.pytorch import functional as F
    box, pts, want = refroi.faces()
    fr, host = device_frames(cuda, box)
    np.testing.assert_array_equal(host[0].view(np.int32), np.array([0, 0, 0, 2, 1, 0.5, 1, 0], np.float32).view(np.int32))
    got = F.points_in_boxes(dev(cuda, pts), None, fr, None, 1).cpu().numpy()
    np.testing.assert_array_equal(got, np.where(want, 0, -1))
    q = F.box_query(fr, None, dev(cuda, pts), None, 1, 16, with_local=True)
    assert int(q.hits[0]) == int(want.sum()) == int(q.count[0])
    np.testing.assert_array_equal(q.rows[0, :int(want.sum())].cpu().numpy(), np.flatnonzero(want))
    np.testing.assert_array_equal(bits(q.local[0, :int(want.sum())]), pts[want].view(np.int32))


# ------------------------------------------------------------------------------------------------ point major

def check_points_in_boxes(cuda, boxes, b_ids, points, p_ids, batch, n_boxes=None, n_points=None):
    """The public call and the C call into a dirty buffer against refroi over the device's frames; returns the table."""
    from spconv_amd import _lib
    from spconv_amd.pytorch import functional as F
    from spconv_amd.pytorch._rulebook import _ptr, _stream
    fr, host = device_frames(cuda, boxes, n_boxes)
    want = refroi.points_in_boxes(host, b_ids, points, p_ids, batch, n_boxes, n_points)
    d_pts, d_pid, d_bid = dev(cuda, points), dev(cuda, p_ids), dev(cuda, b_ids)
    got = F.points_in_boxes(d_pts, d_pid, fr, d_bid, batch, n_points=count_of(cuda, n_points))
    assert got.dtype == torch.int32 and tuple(got.shape) == (len(points),)
    np.testing.assert_array_equal(got.cpu().numpy(), want)
    from_boxes = F.points_in_boxes(d_pts, d_pid, dev(cuda, boxes), d_bid, batch, n_points=count_of(cuda, n_points),
                                   n_boxes=count_of(cuda, n_boxes))
    np.testing.assert_array_equal(from_boxes.cpu().numpy(), want)
    if len(points):
        out = junk(cuda, (len(points),), torch.int32)
        bg = F.scene_groups(d_bid, len(boxes), batch, count_of(cuda, n_boxes), cuda)
        _lib.check(_lib.load().spx_points_in_boxes(
            d_pts.data_ptr(), int(d_pts.shape[1]), _ptr(d_pid), len(points), _ptr(count_of(cuda, n_points)),
            _ptr(fr.frames), len(boxes), bg.offsets.data_ptr(), _ptr(bg.list), batch, out.data_ptr(), _stream(d_pts)))
        np.testing.assert_array_equal(out.cpu().numpy(), want)
    return want


@pytest.mark.parametrize("n", (0, 1, 255, 256, 257))
def test_points_in_boxes_point_counts(cuda, n):
    boxes, b_ids, points, p_ids = refroi.scene(100 + n, n, 24, batch=2)
    want = check_points_in_boxes(cuda, boxes, b_ids, points, p_ids, 2)
    assert n < 255 or ((want >= 0).sum() > n // 4 and (want < 0).sum() > n // 8)


@pytest.mark.parametrize("m", (0, 1, TILE - 1, TILE, TILE + 1))
def test_points_in_boxes_boxes_per_scene(cuda, m):
    """one scene holds m boxes (the staging tile +- 1), the other three"""
    boxes, b_ids, points, p_ids = refroi.scene(200 + m, 700, m + 3, batch=2, field=60.0)
    b_ids[:], p_ids[:] = 0, 0
    b_ids[-3:] = 1
    p_ids[::5] = 1
    want = check_points_in_boxes(cuda, boxes, b_ids, points, p_ids, 2)
    assert m == 0 or (want[p_ids == 0] >= 0).any()
    assert m < TILE or (want[p_ids == 0] >= TILE - 8).any()          # a hit among the last staged frames


def test_points_in_boxes_across_scenes(cuda):
    """points and boxes shuffled over 3 of 5 scenes, scene 3 with points and no box, scene 4 with boxes and no point,
    foreign batch ids, points and boxes that are not finite, device counts in the middle of a workgroup"""
    boxes, b_ids, points, p_ids = refroi.scene(31, 2000, 300, batch=3)
    p_ids[10:60], b_ids[5:25] = 3, 4
    p_ids[60:70], b_ids[25:30] = [-1, 5, 7, -2, 1 << 30] * 2, [-3, 9, 5, -1, 1 << 20]
    points[70, 0], points[71, 1], points[72, 2] = np.nan, np.inf, -np.inf
    spoil(boxes, range(40, 290, 17))
    want = check_points_in_boxes(cuda, boxes, b_ids, points, p_ids, 5, n_boxes=290, n_points=1900)
    hit, _, _, _ = refroi.incidence(device_frames(cuda, boxes, 290)[1], b_ids, points, p_ids, 5, 290, 1900)
    assert (hit.sum(0) > 1).sum() > 50                               # overlapping boxes: the lowest index wins
    assert (want[:1900] >= 0).sum() > 500 and (want[10:73] == -1).all() and (want[1900:] == -1).all()
    assert not np.isin(want, np.r_[5:30, 290:300]).any()
    # junk beyond the device counts changes nothing
    boxes2, points2, p2, b2 = boxes.copy(), points.copy(), p_ids.copy(), b_ids.copy()
    boxes2[290:], points2[1900:], p2[1900:], b2[290:] = np.nan, np.nan, 1, 0
    np.testing.assert_array_equal(check_points_in_boxes(cuda, boxes2, b2, points2, p2, 5, 290, 1900), want)
    # a permutation of the points permutes the result
    perm = np.random.default_rng(5).permutation(2000)
    again = check_points_in_boxes(cuda, boxes, b_ids, points[perm], p_ids[perm], 5, n_boxes=290)
    full = check_points_in_boxes(cuda, boxes, b_ids, points, p_ids, 5, n_boxes=290)
    np.testing.assert_array_equal(again, full[perm])


# ------------------------------------------------------------------------------------------------ box major

def check_box_query(cuda, boxes, b_ids, points, p_ids, batch, nsample, pad="none", grid=None, n_boxes=None,
                    n_points=None):
    """``box_query_into`` over junk-filled buffers and ``box_query`` against refroi over the device's frames"""
    from spconv_amd.pytorch import _roi
    from spconv_amd.pytorch import functional as F
    fr, host = device_frames(cuda, boxes, n_boxes)
    want = refroi.box_query(host, b_ids, points, p_ids, batch, nsample, PADS[pad], grid, n_boxes, n_points)
    M, N = len(boxes), len(points)
    d_pts, d_pid, d_bid = dev(cuda, points), dev(cuda, p_ids), dev(cuda, b_ids)
    q = F.box_query(fr, d_bid, d_pts, d_pid, batch, nsample, pad=pad, with_local=True, grid=grid,
                    n_points=count_of(cuda, n_points))
    tables = [dict(rows=q.rows, count=q.count, hits=q.hits, local=q.local, cells=q.cells)]
    if M:
        t = dict(rows=junk(cuda, (M, nsample), torch.int32), count=junk(cuda, (M,), torch.int32),
                 hits=junk(cuda, (M,), torch.int32), local=junk(cuda, (M, nsample, 3), torch.float32),
                 cells=None if grid is None else junk(cuda, (M, nsample), torch.int32))
        groups = F.scene_groups(d_pid, N, batch, count_of(cuda, n_points), cuda)
        _roi.box_query_into(fr, d_bid, d_pts, groups, pad, t["rows"], t["count"], t["hits"], t["local"], t["cells"], grid)
        tables.append(t)
    for t in tables:
        for key in ("rows", "count", "hits", "cells"):
            if want[key] is None:
                assert t[key] is None
            else:
                np.testing.assert_array_equal(t[key].cpu().numpy(), want[key], err_msg=key)
        np.testing.assert_array_equal(bits(t["local"]), want["local"].view(np.int32))
    assert (q.nsample, q.num_points, q.grid) == (nsample, N, None if grid is None else tuple(grid))
    return want


@functools.lru_cache(maxsize=None)
def one_scene():
    """700 points and 7 boxes of one scene: boxes 0 .. 4 with some 70 hits each, box 5 far from every point (count 0),
    box 6 around point 0 alone (count 1)"""
    boxes, b_ids, points, p_ids = refroi.scene(43, 700, 7, batch=1, wild=2)
    boxes[5, :3] = [1000.0, 1000.0, 0.0]
    points[0] = [-300.0, 300.0, 1.0]
    boxes[6] = [-300.0, 300.0, 1.0, 0.5, 0.5, 0.5, 0.3]
    return boxes, b_ids, points, p_ids


@pytest.mark.parametrize("n", (0, 1, 63, 64, 65, 129, 511, 512, 513, 1025))
def test_box_query_scene_sizes(cuda, n):
    """(511 .. 513: the eight batches of 64 a wave has in flight; 1025: a third trip, its entries requested ahead)"""
    boxes, b_ids, points, p_ids = refroi.scene(300 + n, n, 6, batch=1, field=4.0)
    want = check_box_query(cuda, boxes, b_ids, points, p_ids, 1, 32, "cycle", (2, 2, 2))
    assert n < 63 or (want["hits"] > 0).sum() >= 3


def test_box_query_nsample_cuts(cuda):
    boxes, b_ids, points, p_ids = one_scene()
    h = int(check_box_query(cuda, boxes, b_ids, points, p_ids, 1, 64)["hits"][0])
    assert 40 < h < 200 and h % 64 != 0                              # the cut falls inside one ballot
    for nsample in (1, 63, 65, h - 1, h, h + 1):
        for pad in ("none", "first", "cycle"):
            want = check_box_query(cuda, boxes, b_ids, points, p_ids, 1, nsample, pad)
            assert want["count"][5] == 0 and want["count"][6] == 1 and (want["rows"][5] == -1).all()
            assert (want["rows"][6] == (0 if pad != "none" else np.r_[0, [-1] * (nsample - 1)])).all()
    want = check_box_query(cuda, boxes, b_ids, points, p_ids, 1, 8, "cycle")
    assert (want["hits"][:5] > 8).all() and (want["count"][:5] == 8).all()        # hits above nsample


def test_box_query_largest_nsample_on_a_small_scene(cuda):
    boxes, b_ids, points, p_ids = one_scene()
    for pad in ("none", "cycle"):
        want = check_box_query(cuda, boxes[4:], b_ids[4:], points, p_ids, 1, 16384, pad, (2, 1, 1))
        assert 0 < want["count"][0] == want["hits"][0] < 200


@pytest.mark.parametrize("m", (0, 1, WAVES - 1, WAVES, WAVES + 1))
def test_box_query_box_counts(cuda, m):
    boxes, b_ids, points, p_ids = one_scene()
    check_box_query(cuda, boxes[:m], b_ids[:m], points, p_ids, 1, 40, "first", (3, 3, 3))


@pytest.mark.parametrize("grid", ((1, 1, 1), (12, 12, 12), (64, 1, 3)))
def test_box_query_cells(cuda, grid):
    boxes, b_ids, points, p_ids = one_scene()
    want = check_box_query(cuda, boxes, b_ids, points, p_ids, 1, 128, "none", grid)
    ncell = grid[0] * grid[1] * grid[2]
    for m in range(7):
        c = want["cells"][m, :want["count"][m]]
        assert ((c >= m * ncell) & (c < (m + 1) * ncell)).all()
    assert ncell == 1 or len(np.unique(want["cells"][0, :want["count"][0]])) > 3


def test_box_query_across_scenes(cuda):
    """3 scenes shuffled, foreign ids, invalid boxes and points, device counts; junk beyond the counts changes nothing;
    a permutation of the boxes permutes the rows"""
    boxes, b_ids, points, p_ids = refroi.scene(57, 3000, 40, batch=3)
    p_ids[60:70], b_ids[5:8] = [-1, 5, 7, -2, 3] * 2, [-3, 9, 3]
    points[70, 0], points[71, 1], points[72, 2] = np.nan, np.inf, -np.inf
    spoil(boxes, (10, 11, 12, 13))
    args = dict(n_boxes=37, n_points=2900)
    want = check_box_query(cuda, boxes, b_ids, points, p_ids, 3, 24, "cycle", (4, 3, 2), **args)
    assert (want["hits"][[5, 6, 7, 10, 11, 12, 13, 37, 38, 39]] == 0).all() and (want["hits"] > 24).sum() > 10
    assert want["rows"].max() < 2900 and not np.isin(want["rows"], np.r_[60:73]).any()
    boxes2, points2, p2, b2 = boxes.copy(), points.copy(), p_ids.copy(), b_ids.copy()
    boxes2[37:], points2[2900:], p2[2900:], b2[37:] = np.inf, np.nan, 1, 0
    again = check_box_query(cuda, boxes2, b2, points2, p2, 3, 24, "cycle", (4, 3, 2), **args)
    for key in ("rows", "count", "hits", "cells"):
        np.testing.assert_array_equal(again[key], want[key])
    np.testing.assert_array_equal(again["local"].view(np.int32), want["local"].view(np.int32))
    perm = np.random.default_rng(9).permutation(40)
    full = check_box_query(cuda, boxes, b_ids, points, p_ids, 3, 24, "first")
    moved = check_box_query(cuda, boxes[perm], b_ids[perm], points, p_ids, 3, 24, "first")
    for key in ("rows", "count", "hits"):
        np.testing.assert_array_equal(moved[key], full[key][perm])


# ------------------------------------------------------------------------------------------------ composites

@functools.lru_cache(maxsize=None)
def pool_scene(C):
    """1500 points and 12 boxes over 2 scenes, box 10 around point 3 alone, box 11 far from every point; features and upstream gradients are small
    integers, so that every sum of a gradient is exact in float32 and in float16 and a max has ties"""
    boxes, b_ids, points, p_ids = refroi.scene(71, 1500, 12, batch=2)
    boxes[11, :3] = [1000.0, 1000.0, 0.0]
    points[3], boxes[10], b_ids[10] = [500.0, 500.0, 0.0], [500.0, 500.0, 0.0, 0.5, 0.5, 0.5, 0.2], p_ids[3]
    rng = np.random.default_rng(72 + C)
    feats = rng.integers(-3, 4, (1500, C)).astype(np.float32)
    return boxes, b_ids, points, p_ids, feats


DTYPES = {"f32": (torch.float32, np.float32, 2.0 ** -24), "f16": (torch.float16, np.float16, 2.0 ** -11)}


@pytest.mark.parametrize("dt", ("f32", "f16"))
@pytest.mark.parametrize("C", (3, 64))
def test_roi_point_pool(cuda, C, dt):
    """Forward: copies (the xyz cast to the feature dtype, round to nearest even on both sides): bit for bit.  Gradient:
    integer upstream gradients, at most 160 slots x a few boxes per point: every sum is an integer below 2048, exact in
    float32 and float16: equal."""
    import spconv_amd.pytorch as sp
    tdt, ndt, _ = DTYPES[dt]
    boxes, b_ids, points, p_ids, feats = pool_scene(C)
    S, extra = (160 if C == 3 else 32), (0.2, 0.1, 0.3)              # (160: wider than the 128 slots group_voxels takes)
    fr, host = device_frames(cuda, boxes, None, extra)
    t = refroi.box_query(host, b_ids, points, p_ids, 2, S, refroi.PAD_CYCLE)
    rows = t["rows"]
    assert (t["count"] == 0).sum() == 1 and ((t["count"] > 0) & (t["count"] < S)).any()
    assert S > 128 or (t["hits"] > S).any()
    want = np.concatenate([points.astype(ndt)[rows], feats.astype(ndt)[rows]], -1)
    want[rows < 0] = 0
    rng = np.random.default_rng(5)
    dout = rng.integers(-2, 3, (12, S, 3 + C)).astype(np.float32)
    dwant = np.zeros((1500, C), np.float64)
    np.add.at(dwant, rows[rows >= 0], dout[..., 3:][rows >= 0].astype(np.float64))
    assert np.abs(dwant).max() < 2048
    runs = []
    for _ in range(2):
        f = dev(cuda, feats).to(tdt).requires_grad_(True)
        pooled, empty = sp.RoIPointPool3d(S, extra)(dev(cuda, points), dev(cuda, p_ids), f, dev(cuda, boxes),
                                                    dev(cuda, b_ids), 2)
        pooled.backward(dev(cuda, dout).to(tdt))
        runs.append((pooled.detach(), empty, f.grad))
    pooled, empty, grad = runs[0]
    assert pooled.dtype == tdt and tuple(pooled.shape) == (12, S, 3 + C) and empty.dtype == torch.int32
    np.testing.assert_array_equal(bits(pooled), want.view(bits(pooled).dtype))
    np.testing.assert_array_equal(empty.cpu().numpy(), (t["count"] == 0).astype(np.int32))
    np.testing.assert_array_equal(grad.cpu().double().numpy(), dwant)
    for a, b in zip(runs[0], runs[1]):                                # identical bits on two runs
        np.testing.assert_array_equal(bits(a), bits(b))


@pytest.mark.parametrize("dt", ("f32", "f16"))
@pytest.mark.parametrize("C", (3, 64))
@pytest.mark.parametrize("reduce", ("max", "mean"))
def test_roi_aware_pool(cuda, reduce, C, dt):
    """Against numpy float64 over refroi's cells.  max: a copy, and its gradient a sum of integers: equal.  mean (eps =
    2^-24 for float32, 2^-11 for float16): the sum of small integers is exact, then one reciprocal or division, one
    product and the rounding of the output: asserted |got - want| <= 4 eps |want|; its gradient is a sum of k <= 4
    such terms of one sign pattern each rounded as above, accumulated in float32 and rounded once: asserted
    |got - want| <= 8 eps sum |terms|."""
    import spconv_amd.pytorch as sp
    tdt, ndt, eps = DTYPES[dt]
    boxes, b_ids, points, p_ids, feats = pool_scene(C)
    grid, S = (3, 2, 2), (192 if C == 3 else 64)                     # (192: no cap bites, wider than 128 slots)
    ncell = 12
    fr, host = device_frames(cuda, boxes)
    t = refroi.box_query(host, b_ids, points, p_ids, 2, S, refroi.PAD_NONE, grid)
    assert (t["hits"] > 64).any() and (t["count"] == 0).sum() == 1
    rows, cells = t["rows"].reshape(-1), t["cells"].reshape(-1)
    live = cells >= 0
    f64 = feats.astype(np.float64)
    rng = np.random.default_rng(6)
    dout = rng.integers(-2, 3, (12 * ncell, C)).astype(np.float64)
    want = np.zeros((12 * ncell, C))
    dwant, dabs = np.zeros((1500, C)), np.zeros((1500, C))
    for cell in np.unique(cells[live]):
        members = rows[live & (cells == cell)]
        x = f64[members]
        if reduce == "max":
            want[cell] = x.max(0)
            np.add.at(dwant, members, (x == x.max(0)) * dout[cell])   # a tie: every point that attains it
        else:
            want[cell] = x.mean(0)
            np.add.at(dwant, members, np.broadcast_to(dout[cell] / len(members), x.shape))
            np.add.at(dabs, members, np.broadcast_to(np.abs(dout[cell]) / len(members), x.shape))
    runs = []
    for _ in range(2):
        f = dev(cuda, feats).to(tdt).requires_grad_(True)
        out = sp.RoIAwarePool3d(grid, S, reduce)(dev(cuda, points), dev(cuda, p_ids), f, dev(cuda, boxes),
                                                  dev(cuda, b_ids), 2)
        out.backward(dev(cuda, dout.reshape(12, 3, 2, 2, C)).to(tdt))
        runs.append((out.detach(), f.grad))
    out, grad = runs[0]
    assert out.dtype == tdt and tuple(out.shape) == (12, 3, 2, 2, C)
    got, dgot = out.cpu().double().numpy().reshape(12 * ncell, C), grad.cpu().double().numpy()
    if reduce == "max":
        np.testing.assert_array_equal(got, want)
        np.testing.assert_array_equal(dgot, dwant)
    else:
        err, derr = np.abs(got - want) - 4.0 * eps * np.abs(want), np.abs(dgot - dwant) - 8.0 * eps * dabs
        print(f"roi_aware_pool mean {dt} C={C}: worst excess {err.max():.3g} / {derr.max():.3g}")
        assert err.max() <= 0.0 and derr.max() <= 0.0
    for a, b in zip(runs[0], runs[1]):                                # identical bits on two runs
        np.testing.assert_array_equal(bits(a), bits(b))


# ------------------------------------------------------------------------------------------------ one graph

def test_one_captured_graph_replayed_on_a_second_input(cuda):
    """frames -> box_query_into -> gather in one captured graph; a replay follows new boxes and points"""
    from spconv_amd.pytorch import _roi
    from spconv_amd.pytorch import functional as F
    M, N, S, grid = 12, 1500, 32, (3, 2, 2)
    sets = [refroi.scene(seed, N, M, batch=2) for seed in (81, 82)]
    feats = dev(cuda, np.random.default_rng(8).integers(-3, 4, (N, 8)).astype(np.float32)).half()
    boxes, points = torch.zeros((M, 7), device=cuda), torch.zeros((N, 3), device=cuda)
    b_ids, p_ids = torch.zeros((M,), dtype=torch.int32, device=cuda), torch.zeros((N,), dtype=torch.int32, device=cuda)
    n_boxes = count_of(cuda, M - 1)
    frames = torch.empty((M, 8), device=cuda)
    rows, cells = (torch.empty((M, S), dtype=torch.int32, device=cuda) for _ in range(2))
    count, hits = (torch.empty((M,), dtype=torch.int32, device=cuda) for _ in range(2))
    local = torch.empty((M, S, 3), device=cuda)

    def load(s):
        bx, bi, pt, pi = sets[s]
        boxes.copy_(dev(cuda, bx)), b_ids.copy_(dev(cuda, bi)), points.copy_(dev(cuda, pt)), p_ids.copy_(dev(cuda, pi))

    def step():
        _roi.frames_into(boxes, n_boxes, (0.1, 0.1, 0.1), frames)
        groups = F.scene_groups(p_ids, N, 2)
        fr = F.BoxFrames(frames, M, n_boxes)
        _roi.box_query_into(fr, b_ids, points, groups, "cycle", rows, count, hits, local, cells, grid)
        nb = F.BoxPoints(rows, count, hits, local, cells, None, S, N, grid, n_boxes, None).neighbors()
        with torch.no_grad():
            return F.group_voxels(feats, nb)

    eager = []
    for s in (0, 1):
        load(s)
        pooled = step()
        bx, bi, pt, pi = sets[s]
        want = refroi.box_query(frames.cpu().numpy(), bi, pt, pi, 2, S, refroi.PAD_CYCLE, grid, n_boxes=M - 1)
        for key, have in (("rows", rows), ("count", count), ("hits", hits), ("cells", cells)):
            np.testing.assert_array_equal(have.cpu().numpy(), want[key], err_msg=key)
        np.testing.assert_array_equal(bits(local), want["local"].view(np.int32))
        ref = feats.cpu().numpy()[want["rows"]]
        ref[want["rows"] < 0] = 0
        np.testing.assert_array_equal(bits(pooled), ref.view(np.int16))
        eager.append([t.clone() for t in (frames, rows, count, hits, local, cells, pooled)])
    assert not torch.equal(eager[0][1], eager[1][1])
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        pooled = step()
    for s in (1, 0, 1):
        load(s)
        graph.replay()
        torch.cuda.synchronize()
        for got, want in zip((frames, rows, count, hits, local, cells, pooled), eager[s]):
            np.testing.assert_array_equal(bits(got), bits(want))
