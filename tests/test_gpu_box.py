"""Rotated boxes on the kernels of csrc/box.hip (spconv_amd/pytorch/_box.py, spatial.RotatedNMS) against the numpy
float32 restatement tests/refbox.py (whose conditions test_refbox.py asserts on the CPU), over the clouds of
tests/boxscenes.py.

The corners are held to float64 numpy within a derived bound (the sine and cosine are the one step a host does not
reproduce).  The device's own corners are then downloaded and handed to refbox, and everything downstream of them --
overlaps, IoUs, keep lists, counts -- is compared bit for bit."""
import functools

import numpy as np
import pytest
import torch

import boxscenes
import refbox

pytestmark = pytest.mark.gpu

SIZES = (0, 1, 63, 64, 65, 257)
MODES = (refbox.OVERLAP_BEV, refbox.IOU_BEV, refbox.IOU_3D)
KEYS = ("box/corners", "box/pairs", "box/aligned", "box/key", "box/mask", "box/reduce")


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32).numpy()


def dev(cuda, a):
    return None if a is None else torch.from_numpy(np.array(a, order="C")).to(cuda)


def count_of(cuda, n):
    return None if n is None else torch.tensor([n], dtype=torch.int32, device=cuda)


def launches():
    from spconv_amd import _lib
    return _lib.launch_counts(KEYS)


def device_table(cuda, boxes, n_boxes=None):
    """(BoxCorners on the device, the refbox Table of the DOWNLOADED corners)"""
    from spconv_amd.pytorch import functional as F
    c = F.boxes_to_corners(dev(cuda, boxes), count_of(cuda, n_boxes))
    return c, refbox.Table(c.bev.cpu().numpy(), c.zrange.cpu().numpy())


def spoil(boxes, rows):
    """NaN, Inf, zero and negative sizes in the given rows, one kind after the other"""
    kinds = [(0, np.nan), (1, np.inf), (6, -np.inf), (3, 0.0), (4, -1.0), (5, 0.0), (2, np.nan), (5, -2.0)]
    for t, r in enumerate(rows):
        col, v = kinds[t % len(kinds)]
        boxes[r, col] = v
    return boxes


# ------------------------------------------------------------------------------------------------ corners

def test_corners_against_float64_numpy(cuda):
    """Bound per coordinate: 8 * 2^-23 * (|centre| + dx / 2 + dy / 2) -- the 4-ulp sine / cosine of OpenCL's full profile
    on a lever of at most dx / 2 + dy / 2, one product and two sums each rounded once: 5.5 * 2^-23 derived, 8 asserted."""
    from spconv_amd.pytorch import _box
    n, live = 1500, 1400
    rng = np.random.default_rng(17)
    b = np.zeros((n, 8), np.float32)
    b[:, :3] = (rng.random((n, 3)) * 200.0 - 100.0)
    b[:, 3:6] = 0.2 + rng.random((n, 3)) * 10.0
    b[:, 6] = rng.random(n) * 16.0 - 8.0
    b[:8, 6] = [0.0, -0.0, 8.0, -8.0, np.pi, -np.pi, np.pi / 2, 1e-30]
    bad = np.arange(20, 1300, 37)
    spoil(b, bad)
    bev = torch.empty((n, 4, 2), dtype=torch.float32, device=cuda)
    z = torch.empty((n, 2), dtype=torch.float32, device=cuda)
    bev.view(torch.int32).fill_(-1), z.view(torch.int32).fill_(-1)
    before = launches()
    _box.corners_into(dev(cuda, b), count_of(cuda, live), bev, z)
    assert launches()["box/corners"] == before["box/corners"] + 1
    got, gz = bev.cpu().numpy(), z.cpu().numpy()
    assert not (bits(bev) == -1).any() and not (bits(z) == -1).any()         # every element written
    dead = np.zeros(n, bool)
    dead[bad], dead[live:] = True, True
    assert np.isnan(got[dead]).all() and np.isnan(gz[dead]).all()
    ok = ~dead
    assert np.isfinite(got[ok]).all()
    b64 = b[ok].astype(np.float64)
    c, s = np.cos(b64[:, 6]), np.sin(b64[:, 6])
    sx, sy = np.array([1.0, -1.0, -1.0, 1.0]), np.array([1.0, 1.0, -1.0, -1.0])
    lx, ly = sx[None] * b64[:, 3:4] * 0.5, sy[None] * b64[:, 4:5] * 0.5
    X = b64[:, 0:1] + (lx * c[:, None] - ly * s[:, None])
    Y = b64[:, 1:2] + (lx * s[:, None] + ly * c[:, None])
    lever = (b64[:, 3] + b64[:, 4]) * 0.5
    bound = 8.0 * 2.0 ** -23
    ex = np.abs(got[ok][:, :, 0] - X) / (np.abs(b64[:, 0]) + lever)[:, None]
    ey = np.abs(got[ok][:, :, 1] - Y) / (np.abs(b64[:, 1]) + lever)[:, None]
    print(f"corners: worst error / (|centre| + dx/2 + dy/2) = {max(ex.max(), ey.max()) / 2.0 ** -23:.2f} x 2^-23")
    assert ex.max() <= bound and ey.max() <= bound
    hz = b[ok, 5] * np.float32(0.5)
    np.testing.assert_array_equal(gz[ok].view(np.int32), np.stack([b[ok, 2] - hz, b[ok, 2] + hz], -1).view(np.int32))
    # counter-clockwise: the signed area is positive
    q = got[ok].astype(np.float64)
    area = sum(q[:, k, 0] * q[:, (k + 1) % 4, 1] - q[:, (k + 1) % 4, 0] * q[:, k, 1] for k in range(4))
    assert (area > 0).all()


# ------------------------------------------------------------------------------------------------ matrix forms

@functools.lru_cache(maxsize=None)
def pools():
    """two pools of 257 boxes over the same field, with NaN, Inf, zero and negative sizes among them"""
    a, _, _ = boxscenes.cloud(41, 257, 1)
    b, _, _ = boxscenes.cloud(42, 257, 1)
    b[5:40:7] = a[5:40:7]                                   # exact duplicates across the pools
    spoil(a, [3, 62, 63, 64, 100, 200, 255, 256])
    spoil(b, [0, 17, 64, 65, 130, 131, 256])
    return a, b


@functools.lru_cache(maxsize=None)
def pool_state():
    cuda = torch.device("cuda:0")
    a, b = pools()
    ca, ta = device_table(cuda, a)
    cb, tb = device_table(cuda, b)
    assert np.isnan(ca.bev.cpu().numpy()[[3, 62, 63, 64, 100, 200, 255, 256]]).all()
    return a, b, ca, cb, ta, tb


@functools.lru_cache(maxsize=None)
def pool_ref(order, mode):
    _, _, _, _, ta, tb = pool_state()
    want = refbox.pairs(ta, tb, mode) if order == "ab" else refbox.pairs(tb, ta, mode)
    want.setflags(write=False)
    return want


def sliced(c, n):
    from spconv_amd.pytorch import functional as F
    return F.BoxCorners(c.bev[:n], c.zrange[:n], n, None)


@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("M", SIZES)
def test_matrix_forms_equal_refbox(cuda, M, N):
    from spconv_amd.pytorch import _box
    from spconv_amd.pytorch import functional as F
    a, b, ca, cb, _, _ = pool_state()
    for order in ("ab", "ba"):
        first, second = (ca, cb) if order == "ab" else (cb, ca)
        raw_first, raw_second = (a, b) if order == "ab" else (b, a)
        for mode, fn in zip(MODES, (F.boxes_overlap_bev, F.boxes_iou_bev, F.boxes_iou3d)):
            want = pool_ref(order, mode)[:M, :N]
            out = torch.empty((M, N), dtype=torch.float32, device=cuda)
            out.view(torch.int32).fill_(-1)
            before = launches()
            if M * N:
                _box.overlap_into(sliced(first, M), sliced(second, N), mode, out)
            assert launches()["box/pairs"] == before["box/pairs"] + (1 if M * N else 0)
            assert not (bits(out) == -1).any()                              # every element written
            np.testing.assert_array_equal(bits(out), want.view(np.int32), err_msg=f"{order} mode {mode}")
            # the boxes form: the corners launch, then the corners form
            boxes_form = fn(dev(cuda, raw_first[:M]), dev(cuda, raw_second[:N]))
            assert tuple(boxes_form.shape) == (M, N) and boxes_form.dtype == torch.float32
            np.testing.assert_array_equal(bits(boxes_form), want.view(np.int32))
            mixed = fn(sliced(first, M), dev(cuda, raw_second[:N]))
            np.testing.assert_array_equal(bits(mixed), want.view(np.int32))
    if M == 257 and N == 257:
        full = pool_ref("ab", refbox.IOU_BEV)
        assert (full > 0).sum() > 300 and (full == 1.0).sum() >= 4 and full.max() <= 1.0
        assert not np.array_equal(full, pool_ref("ba", refbox.IOU_BEV).T)   # the subject is the first argument


def test_device_counts_in_the_middle_of_a_tile(cuda):
    from spconv_amd.pytorch import functional as F
    a, b, ca, cb, _, _ = pool_state()
    for n_a, n_b in ((130, 100), (0, 257), (257, 0), (1, 1), (1000, 1000)):
        for mode, fn in zip(MODES, (F.boxes_overlap_bev, F.boxes_iou_bev, F.boxes_iou3d)):
            want = pool_ref("ab", mode).copy()
            want[n_a:], want[:, n_b:] = 0, 0
            got = fn(ca, cb, n_a=count_of(cuda, n_a), n_b=count_of(cuda, n_b))
            np.testing.assert_array_equal(bits(got), want.view(np.int32))
            got = fn(dev(cuda, a), dev(cuda, b), n_a=count_of(cuda, n_a), n_b=count_of(cuda, n_b))
            np.testing.assert_array_equal(bits(got), want.view(np.int32))


def test_aligned_form_equals_the_matrix_diagonal(cuda):
    from spconv_amd.pytorch import functional as F
    a, b, ca, cb, ta, tb = pool_state()
    want = np.ascontiguousarray(np.diagonal(pool_ref("ab", refbox.IOU_3D)))
    np.testing.assert_array_equal(want.view(np.int32), refbox.aligned(ta, tb, refbox.IOU_3D).view(np.int32))
    before = launches()
    got = F.boxes_iou3d_aligned(ca, cb)
    assert launches()["box/aligned"] == before["box/aligned"] + 1
    np.testing.assert_array_equal(bits(got), want.view(np.int32))
    np.testing.assert_array_equal(bits(F.boxes_iou3d_aligned(dev(cuda, a), dev(cuda, b))), want.view(np.int32))
    assert (want == 1.0).sum() >= 4 and (want > 0).sum() > 4
    cut = want.copy()
    cut[77:] = 0
    np.testing.assert_array_equal(bits(F.boxes_iou3d_aligned(ca, cb, n_b=count_of(cuda, 77))), cut.view(np.int32))
    assert tuple(F.boxes_iou3d_aligned(sliced(ca, 0), sliced(cb, 0)).shape) == (0,)


def test_clockwise_user_corners_equal_counter_clockwise_ones(cuda):
    from spconv_amd.pytorch import functional as F
    _, _, ca, cb, _, _ = pool_state()
    flipped = F.BoxCorners(ca.bev.flip(1).contiguous(), ca.zrange, 257, None)
    for mode, fn in zip(MODES, (F.boxes_overlap_bev, F.boxes_iou_bev, F.boxes_iou3d)):
        np.testing.assert_array_equal(bits(fn(flipped, cb)), pool_ref("ab", mode).view(np.int32))
        np.testing.assert_array_equal(bits(fn(cb, flipped)), pool_ref("ba", mode).view(np.int32))
    plane = F.BoxCorners(ca.bev, None, 257, None)                           # a table for the plane only
    np.testing.assert_array_equal(bits(F.boxes_iou_bev(plane, cb)), pool_ref("ab", refbox.IOU_BEV).view(np.int32))


# ------------------------------------------------------------------------------------------------ NMS

def run_nms(cuda, corners, scores, thresh, bid=None, B=1, cls=None, **kw):
    from spconv_amd.pytorch import functional as F
    n = corners.num_boxes
    before = launches()
    got = F.nms_rotated(corners, dev(cuda, scores), thresh, batch_ids=dev(cuda, bid), batch_size=B, class_ids=dev(cuda, cls),
                        **kw)
    after = launches()
    assert after["box/key"] == before["box/key"] + (1 if n else 0)
    assert after["box/mask"] == before["box/mask"] + (1 if n else 0)
    assert after["box/reduce"] == before["box/reduce"] + 1
    assert after["box/corners"] == before["box/corners"]
    post = kw.get("post_max", 512)
    assert got.keep.dtype == torch.int32 and tuple(got.keep.shape) == (B, post)
    assert got.count.dtype == torch.int32 and tuple(got.count.shape) == (B,)
    return got


def assert_nms(got, want):
    np.testing.assert_array_equal(got.count.cpu().numpy(), want[1])
    np.testing.assert_array_equal(got.keep.cpu().numpy(), want[0])


@functools.lru_cache(maxsize=None)
def cloud_state():
    cuda = torch.device("cuda:0")
    boxes, bid, score = boxscenes.cloud(2025, 768, 3)
    cls = np.random.default_rng(8).integers(0, 3, 768).astype(np.int32)
    c, t = device_table(cuda, boxes)
    return boxes, bid, score, cls, c, t, {}


@pytest.mark.parametrize("pre_post", ((16384, 16384), (100, 100), (256, 10), (64, 1)))
@pytest.mark.parametrize("score_thresh", (None, 0.5))
@pytest.mark.parametrize("with_cls", (False, True))
@pytest.mark.parametrize("thresh", (0.1, 0.3, 0.7, 0.85))
def test_nms_on_the_seeded_cloud_equals_refbox(cuda, thresh, with_cls, score_thresh, pre_post):
    boxes, bid, score, cls, c, t, cache = cloud_state()
    cls = cls if with_cls else None
    pre, post = pre_post
    want = refbox.nms(t, score, thresh, bid, 3, cls, pre, post, score_thresh, cache=cache)
    got = run_nms(cuda, c, score, thresh, bid, 3, cls, pre_max=pre, post_max=post, score_thresh=score_thresh)
    assert_nms(got, want)
    assert want[1].sum() > 0
    if pre == 16384 and not with_cls and score_thresh is None and thresh in (0.3, 0.7, 0.85):
        assert int(want[1].sum()) == {0.3: 473, 0.7: 688, 0.85: 736}[thresh]    # the float64 greedy's counts too
    # the eager convenience: the trimmed 1-D tensor of a scene
    np.testing.assert_array_equal(got.indices(1).cpu().numpy(), want[0][1, :want[1][1]])


def test_module_and_boxes_form(cuda):
    import spconv_amd.pytorch as spconv
    boxes, bid, score, cls, c, t, cache = cloud_state()
    want = refbox.nms(t, score, 0.7, bid, 3, cls, 4096, 512, 0.25, cache=cache)
    before = launches()
    got = spconv.RotatedNMS(0.7, score_thresh=0.25)(dev(cuda, boxes), dev(cuda, score), dev(cuda, bid), 3, dev(cuda, cls))
    assert launches()["box/corners"] == before["box/corners"] + 1
    assert_nms(got, want)


@functools.lru_cache(maxsize=None)
def lattice_state(c):
    """one scene with c candidates on the jittered lattice and three boxes that are none (NaN score, NaN box, another
    scene), its refbox result at 0.3"""
    cuda = torch.device("cuda:0")
    boxes, score = boxscenes.lattice(600 + c, c + 3)
    bid = np.zeros(c + 3, np.int32)
    at = [c // 3, c // 2, c + 2] if c > 2 else [c, c + 1, c + 2]
    score[at[0]], boxes[at[1], 3], bid[at[2]] = np.nan, np.nan, 1
    corners, t = device_table(cuda, boxes)
    want = refbox.nms(t, score, 0.3, bid, 1, None, 16384, 16384)
    return corners, score, bid, want


@pytest.mark.parametrize("c", (1, 63, 64, 65, 128, 129, 4097, 8193))
def test_block_and_tier_edges(cuda, c):
    """64-rank blocks of the mask and the reduce, and the smallest counts that reach the two- and four-word instances of
    the reduce (W = 65 and W = 129 words)"""
    corners, score, bid, want = lattice_state(c)
    kept = int(want[1][0])
    assert max(1, c // 8) <= kept <= c and (want[0][0, kept:] == -1).all()
    assert c < 129 or kept < c                              # (the lattice suppresses)
    got = run_nms(cuda, corners, score, 0.3, bid, 1, pre_max=16384, post_max=16384)
    assert_nms(got, want)
    if c >= 129:                                            # post_max stops a scene in the middle of a block
        stop = kept // 2 + 1
        cut = run_nms(cuda, corners, score, 0.3, bid, 1, pre_max=16384, post_max=stop)
        np.testing.assert_array_equal(cut.keep.cpu().numpy(), want[0][:, :stop])
        assert cut.count.cpu().tolist() == [stop]
        few = run_nms(cuda, corners, score, 0.3, bid, 1, pre_max=100, post_max=100)     # pre_max cuts the ranks
        assert_nms(few, refbox.nms(refbox.Table(corners.bev.cpu().numpy()), score, 0.3, bid, 1, None, 100, 100))


def test_empty_scene_all_invalid_and_no_boxes(cuda):
    from spconv_amd.pytorch import functional as F
    boxes, bid, score, cls, c, t, cache = cloud_state()
    moved = np.where(bid == 1, 3, bid).astype(np.int32)                     # scene 1 of four is empty
    want = refbox.nms(t, score, 0.7, moved, 4, None, 4096, 512, cache=cache)
    got = run_nms(cuda, c, score, 0.7, moved, 4)
    assert_nms(got, want)
    assert want[1][1] == 0 and (want[0][1] == -1).all() and want[1][3] > 0
    nothing = run_nms(cuda, device_table(cuda, np.full((300, 7), np.nan, np.float32))[0], score[:300], 0.7, bid[:300], 3)
    assert nothing.count.cpu().tolist() == [0, 0, 0] and (nothing.keep.cpu().numpy() == -1).all()
    none_live = F.nms_rotated(dev(cuda, boxes), dev(cuda, score), 0.7, batch_ids=dev(cuda, bid), batch_size=3,
                              n_boxes=count_of(cuda, 0))
    assert none_live.count.cpu().tolist() == [0, 0, 0] and (none_live.keep.cpu().numpy() == -1).all()
    empty = run_nms(cuda, device_table(cuda, np.zeros((0, 7), np.float32))[0], np.zeros(0, np.float32), 0.7, None, 2,
                    post_max=5)
    assert empty.count.cpu().tolist() == [0, 0] and (empty.keep.cpu().numpy() == -1).all()
    assert tuple(empty.indices(1).shape) == (0,)


# ------------------------------------------------------------------------------------------------ isolation

def test_dirty_workspace_and_outputs_change_nothing(cuda):
    from spconv_amd.pytorch import functional as F
    boxes, bid, score, cls, c, t, cache = cloud_state()
    want = refbox.nms(t, score, 0.3, bid, 3, cls, 200, 64, cache=cache)
    ws = torch.empty((F.nms_ws_bytes(768, 3, 200) + 256,), dtype=torch.uint8, device=cuda)
    keep = torch.empty((3, 64), dtype=torch.int32, device=cuda)
    count = torch.empty((3,), dtype=torch.int32, device=cuda)
    results = []
    for fill in (0xFF, 0x00, 0xFF):
        ws.fill_(fill), keep.view(torch.uint8).fill_(fill), count.view(torch.uint8).fill_(fill)
        F.nms_rotated_into(c, dev(cuda, score), 0.3, keep, count, ws, batch_ids=dev(cuda, bid), batch_size=3,
                           class_ids=dev(cuda, cls), pre_max=200)
        results.append((keep.cpu().numpy().copy(), count.cpu().numpy().copy()))
        assert (ws[-256:] == fill).all()                                    # nothing beyond spx_nms_ws_bytes is touched
    for keep_h, count_h in results:
        np.testing.assert_array_equal(keep_h, want[0])
        np.testing.assert_array_equal(count_h, want[1])


@pytest.mark.parametrize("junk", ("nan", "huge"))
def test_boxes_beyond_the_device_count_and_foreign_batch_ids_change_nothing(cuda, junk):
    from spconv_amd.pytorch import functional as F
    boxes, bid, score, cls, c, t, cache = cloud_state()
    live = 500
    tail = np.full((268, 7), np.nan if junk == "nan" else 3.0e38, np.float32)
    dirty = np.concatenate([boxes[:live], tail])
    dirty_score = np.concatenate([score[:live], np.full(268, np.nan if junk == "nan" else 3.0e38, np.float32)])
    foreign = bid.copy()
    foreign[live:] = 0                                      # (junk rows claim scene 0 and the best scores)
    out_of_range = np.arange(5, live, 50)
    foreign[out_of_range] = np.array([-1, 3, 1 << 30, -(1 << 31), 7], np.int32)[np.arange(len(out_of_range)) % 5]
    table = refbox.Table(c.bev.cpu().numpy(), c.zrange.cpu().numpy(), n_boxes=live)
    want = refbox.nms(table, score, 0.7, foreign, 3, cls, 4096, 512)
    assert not np.isin(out_of_range, want[0]).any() and want[0].max() < live
    got = F.nms_rotated(dev(cuda, dirty), dev(cuda, dirty_score), 0.7, batch_ids=dev(cuda, foreign), batch_size=3,
                        class_ids=dev(cuda, cls), n_boxes=count_of(cuda, live))
    assert_nms(got, want)
    # the matrix forms: rows and columns beyond the counts are written as 0 whatever lies there
    m = F.boxes_iou3d(dev(cuda, dirty), dev(cuda, boxes), n_a=count_of(cuda, live))
    clean = F.boxes_iou3d(c, c, n_a=count_of(cuda, live))
    np.testing.assert_array_equal(bits(m), bits(clean))
    assert (m[live:] == 0).all() and (m[:live] > 0).any()


# ------------------------------------------------------------------------------------------------ capture

def test_capture_corners_and_nms_in_one_graph(cuda):
    """boxes_to_corners -> nms_rotated_into on ONE stream in one graph, replayed for three inputs and device counts
    copied into the static buffers, without re-capture."""
    from spconv_amd.pytorch import _box
    from spconv_amd.pytorch import functional as F
    n, B, pre, post = 768, 3, 300, 40
    sets = []
    for seed, live in ((2025, 768), (2026, 500), (2027, 701)):
        boxes, bid, score = boxscenes.cloud(seed, n, B)
        cls = np.random.default_rng(seed).integers(0, 2, n).astype(np.int32)
        sets.append((boxes, bid, score, cls, live))
    s_boxes = torch.zeros((n, 7), dtype=torch.float32, device=cuda)
    s_score = torch.zeros((n,), dtype=torch.float32, device=cuda)
    s_bid = torch.zeros((n,), dtype=torch.int32, device=cuda)
    s_cls = torch.zeros((n,), dtype=torch.int32, device=cuda)
    s_live = torch.zeros((1,), dtype=torch.int32, device=cuda)
    bev = torch.empty((n, 4, 2), dtype=torch.float32, device=cuda)
    z = torch.empty((n, 2), dtype=torch.float32, device=cuda)
    keep = torch.empty((B, post), dtype=torch.int32, device=cuda)
    count = torch.empty((B,), dtype=torch.int32, device=cuda)
    ws = torch.empty((F.nms_ws_bytes(n, B, pre),), dtype=torch.uint8, device=cuda)

    def load(k):
        boxes, bid, score, cls, live = sets[k]
        s_boxes.copy_(dev(cuda, boxes)), s_score.copy_(dev(cuda, score)), s_bid.copy_(dev(cuda, bid))
        s_cls.copy_(dev(cuda, cls)), s_live.fill_(live)

    def step():
        _box.corners_into(s_boxes, s_live, bev, z)
        F.nms_rotated_into(F.BoxCorners(bev, z, n, s_live), s_score, 0.7, keep, count, ws, batch_ids=s_bid, batch_size=B,
                           class_ids=s_cls, pre_max=pre)

    wants = []
    for k in range(3):
        load(k)
        step()
        torch.cuda.synchronize()
        boxes, bid, score, cls, live = sets[k]
        table = refbox.Table(bev.cpu().numpy(), z.cpu().numpy())
        assert np.isnan(bev.cpu().numpy()[live:]).all()
        wants.append(refbox.nms(table, score, 0.7, bid, B, cls, pre, post))
        np.testing.assert_array_equal(keep.cpu().numpy(), wants[k][0])
        np.testing.assert_array_equal(count.cpu().numpy(), wants[k][1])
    assert not np.array_equal(wants[0][0], wants[1][0]) and not np.array_equal(wants[1][0], wants[2][0])
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    for k in (1, 0, 2):
        load(k)
        keep.fill_(-7), count.fill_(-7)
        graph.replay()
        torch.cuda.synchronize()
        np.testing.assert_array_equal(keep.cpu().numpy(), wants[k][0])
        np.testing.assert_array_equal(count.cpu().numpy(), wants[k][1])


# ------------------------------------------------------------------------------------------------ order independence

def test_permuting_the_boxes_permutes_the_keep_lists(cuda):
    """The rule sees ranks, not positions: on the permuted input the result is refbox's on that input, and -- where
    scores are distinct, so that the tie rule does not enter -- the kept SET of every scene is the permuted one."""
    boxes, bid, score, cls, c, t, cache = cloud_state()
    perm = np.random.default_rng(12).permutation(768)
    p_corners, p_table = device_table(cuda, boxes[perm])
    np.testing.assert_array_equal(bits(p_corners.bev), bits(c.bev)[perm])               # a box's corners are its own
    want = refbox.nms(p_table, score[perm], 0.7, bid[perm], 3, cls[perm], 4096, 512)
    got = run_nms(cuda, p_corners, score[perm], 0.7, bid[perm], 3, cls[perm])
    assert_nms(got, want)
    base = refbox.nms(t, score, 0.7, bid, 3, cls, 4096, 512, cache=cache)
    tied = np.arange(11, 768, 32)                            # the exact duplicates share a score with their source
    for b in range(3):
        mapped = perm[want[0][b, :want[1][b]]]
        plain = base[0][b, :base[1][b]]
        drop = np.concatenate([tied, tied - 4])
        assert sorted(set(mapped) - set(drop)) == sorted(set(plain) - set(drop))
