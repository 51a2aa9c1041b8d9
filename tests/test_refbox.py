"""CPU: refbox -- the numpy float32 restatement the kernels of csrc/box.hip are held to bit for bit -- against an
INDEPENDENT float64 formulation (the corners of either quad inside the other and the edge crossings, sorted by angle, the
shoelace formula) on the seeded cloud, against closed forms, and its NMS against a plain loop."""
import math

import numpy as np
import pytest

import boxscenes
import refbox

THRESHOLDS = (0.3, 0.7, 0.85)


# ------------------------------------------------------------------------------------------- the float64 formulation
def _inside64(p, q):
    """p inside the counter-clockwise quad q (its edges included)."""
    for e in range(4):
        a, b = q[e], q[(e + 1) % 4]
        if (b[0] - a[0]) * (p[1] - a[1]) - (b[1] - a[1]) * (p[0] - a[0]) < 0:
            return False
    return True


def _ccw64(q):
    a = sum(q[i][0] * q[(i + 1) % 4][1] - q[(i + 1) % 4][0] * q[i][1] for i in range(4))
    return (q if a >= 0 else q[::-1]), abs(a) * 0.5


def iou64(qa, qb):
    qa, area_a = _ccw64(np.asarray(qa, np.float64))
    qb, area_b = _ccw64(np.asarray(qb, np.float64))
    pts = [p for p in qa if _inside64(p, qb)] + [p for p in qb if _inside64(p, qa)]
    for i in range(4):
        p, r = qa[i], qa[(i + 1) % 4] - qa[i]
        for j in range(4):
            q, s = qb[j], qb[(j + 1) % 4] - qb[j]
            den = r[0] * s[1] - r[1] * s[0]
            if den == 0:
                continue
            t = ((q[0] - p[0]) * s[1] - (q[1] - p[1]) * s[0]) / den
            u = ((q[0] - p[0]) * r[1] - (q[1] - p[1]) * r[0]) / den
            if 0 <= t <= 1 and 0 <= u <= 1:
                pts.append(p + t * r)
    if len(pts) < 3:
        return 0.0
    pts = np.asarray(pts)
    c = pts.mean(0)
    pts = pts[np.argsort(np.arctan2(pts[:, 1] - c[1], pts[:, 0] - c[0]), kind="stable")]
    x, y = pts[:, 0], pts[:, 1]
    inter = 0.5 * abs(np.sum(x * np.roll(y, -1) - np.roll(x, -1) * y))
    return inter / max(area_a + area_b - inter, 1e-8)


@pytest.fixture(scope="module")
def scene():
    boxes, bid, score = boxscenes.cloud(2025, 768, 3)
    bev, z = boxscenes.corners64(boxes)
    t = refbox.Table(bev, z)
    i32, i64, pairs = {}, {}, []
    for i in range(t.n):
        js = np.nonzero(bid == bid[i])[0]
        js = js[js != i]
        for j in js[refbox.rect_pass(t, i, t, js)]:
            i32[(i, int(j))] = refbox.value(t, i, t, j, refbox.IOU_BEV)
            i64[(i, int(j))] = iou64(bev[i], bev[j])
    return dict(boxes=boxes, bid=bid, score=score, bev=bev, t=t, i32=i32, i64=i64)


def _greedy64(s, thresh):
    """The float64 greedy over the cloud: (score descending, index ascending) per scene."""
    keep = []
    for b in range(3):
        idx = np.nonzero(s["bid"] == b)[0]
        idx = idx[np.argsort(-s["score"][idx].astype(np.float64), kind="stable")]
        kept = []
        for i in idx:
            if not any(s["i64"].get((k, int(i)), 0.0) > thresh for k in kept):
                kept.append(int(i))
        keep.append(kept)
    return keep


def test_float32_rule_stays_within_the_measured_bound_of_the_float64_formulation(scene):
    """Measured on cloud(2025, 768, 3) over the 7066 ordered same-scene pairs that pass the rectangle test (3533
    unordered, 2433 of them overlapping): the largest |iou32 - iou64| is 1.15e-5 (the two formulations see the same
    fp32 corners; the difference is the rounding of the clip alone, largest where an edge crossing is ill-conditioned).
    The assertion is four times that; the factor covers another libm rounding the corners, not another algorithm."""
    worst = max(abs(float(scene["i32"][k]) - scene["i64"][k]) for k in scene["i32"])
    overlapping = sum(1 for v in scene["i64"].values() if v > 0)
    print(f"pairs past the rectangle test {len(scene['i32'])}, overlapping {overlapping}, worst |iou32 - iou64| {worst:.3e}")
    assert len(scene["i32"]) > 3000 and overlapping > 2000
    assert worst <= 4 * 1.15e-5, worst


def test_duplicates_give_exactly_one(scene):
    d = np.arange(11, 768, 32)
    assert all(scene["i32"][(int(i), int(i) - 4)] == np.float32(1.0) for i in d)
    assert all(scene["i32"][(int(i) - 4, int(i))] == np.float32(1.0) for i in d)
    assert max(float(v) for v in scene["i32"].values()) <= 1.0


@pytest.mark.parametrize("thresh", THRESHOLDS)
def test_keep_sets_equal_the_float64_greedy_at_thresholds_with_a_gap(scene, thresh):
    gap = min(abs(v - thresh) for v in scene["i64"].values())
    assert gap >= 1e-4, (thresh, gap)            # the condition under which the two may be compared
    keep, count = refbox.nms(scene["t"], scene["score"], thresh, scene["bid"], 3, pre_max=16384, post_max=16384,
                             cache=dict(scene["i32"]))
    want = _greedy64(scene, thresh)
    for b in range(3):
        assert keep[b, :count[b]].tolist() == want[b], (thresh, b)
        assert (keep[b, count[b]:] == -1).all()
    print(f"thresh {thresh}: kept {int(count.sum())}, gap {gap:.2e}")


# ------------------------------------------------------------------------------------------- closed forms
def _rect(x0, y0, x1, y1):
    return np.array([[x1, y1], [x0, y1], [x0, y0], [x1, y0]], np.float32)


def _pair(qa, qb, mode=refbox.OVERLAP_BEV, za=None, zb=None):
    ta = refbox.Table(qa[None], None if za is None else np.asarray([za], np.float32))
    tb = refbox.Table(qb[None], None if zb is None else np.asarray([zb], np.float32))
    return float(refbox.pairs(ta, tb, mode)[0, 0])


def test_axis_aligned_boxes_on_an_integer_lattice():
    rng = np.random.default_rng(5)
    for _ in range(200):
        ax0, ay0, bx0, by0 = rng.integers(-8, 8, 4)
        aw, ah, bw, bh = rng.integers(1, 9, 4)
        qa, qb = _rect(ax0, ay0, ax0 + aw, ay0 + ah), _rect(bx0, by0, bx0 + bw, by0 + bh)
        w = max(min(ax0 + aw, bx0 + bw) - max(ax0, bx0), 0)
        h = max(min(ay0 + ah, by0 + bh) - max(ay0, by0), 0)
        got = _pair(qa, qb)
        assert abs(got - w * h) <= 2.0 ** -22 * w * h, (qa, qb, got, w * h)      # (t = d_i / (d_i - d_j) rounds once)
        iou = _pair(qa, qb, refbox.IOU_BEV)
        exact = w * h / (aw * ah + bw * bh - w * h)
        assert abs(iou - exact) <= 2.0 ** -21 * exact
        za, zb = (0.0, 2.0), (1.0, 4.0)
        iou3 = _pair(qa, qb, refbox.IOU_3D, za, zb)
        exact3 = w * h * 1.0 / (aw * ah * 2.0 + bw * bh * 3.0 - w * h)
        assert abs(iou3 - exact3) <= 2.0 ** -21 * exact3


def test_a_box_with_itself_gives_exactly_one():
    boxes, _, _ = boxscenes.cloud(7, 200, 1)
    bev, z = boxscenes.corners64(boxes)
    t = refbox.Table(bev, z)
    assert (refbox.aligned(t, t, refbox.IOU_BEV) == np.float32(1.0)).all()
    assert (refbox.aligned(t, t, refbox.IOU_3D) == np.float32(1.0)).all()
    assert np.array_equal(refbox.aligned(t, t, refbox.OVERLAP_BEV), t.area)


def test_unit_square_against_its_45_degree_turn():
    h = math.sqrt(0.5)
    sq = _rect(-0.5, -0.5, 0.5, 0.5)
    turned = np.array([[h, 0], [0, h], [-h, 0], [0, -h]], np.float32)
    want = 2.0 * math.sqrt(2.0) - 2.0
    assert abs(_pair(sq, turned) - want) <= 4 * 2.0 ** -24
    assert abs(_pair(turned, sq) - want) <= 4 * 2.0 ** -24


def test_disjoint_touching_and_contained_boxes():
    a = _rect(0, 0, 2, 2)
    assert _pair(a, _rect(3, 0, 5, 2)) == 0.0                    # apart: the rectangle test
    assert _pair(a, _rect(2, 0, 4, 2)) == 0.0                    # a shared edge
    assert _pair(a, _rect(2, 2, 4, 4)) == 0.0                    # a shared corner
    diamond = np.array([[4, 1], [3, 2], [2, 1], [3, 0]], np.float32)
    assert _pair(a, diamond) == 0.0                              # a corner on an edge
    inner = _rect(0.5, 0.5, 1.5, 1.25)
    assert _pair(a, inner) == 0.75 and _pair(inner, a) == 0.75   # contained, either way round
    assert _pair(a, inner, refbox.IOU_BEV) == np.float32(0.75) / np.float32(4.0)
    far = np.array([[9, 9], [8, 9.5], [7, 9], [8, 8.5]], np.float32)
    assert _pair(a, far) == 0.0


def test_clockwise_corners_equal_counter_clockwise_corners():
    boxes, _, _ = boxscenes.cloud(11, 64, 1)
    bev, z = boxscenes.corners64(boxes)
    t, r = refbox.Table(bev, z), refbox.Table(bev[:, ::-1], z)
    for mode in (refbox.OVERLAP_BEV, refbox.IOU_BEV, refbox.IOU_3D):
        want = refbox.pairs(t, t, mode)
        assert np.array_equal(refbox.pairs(r, t, mode), want)
        assert np.array_equal(refbox.pairs(t, r, mode), want)
        assert np.array_equal(refbox.pairs(r, r, mode), want)
    assert (want > 0).sum() > 64


def test_invalid_boxes_give_zero():
    boxes, _, _ = boxscenes.cloud(13, 32, 1)
    bev, z = boxscenes.corners64(boxes)
    bev[3, 2, 1] = np.nan
    bev[5] = np.inf
    z[7, 0] = np.nan
    t = refbox.Table(bev, z, n_boxes=20)
    clean = refbox.Table(*boxscenes.corners64(boxes))
    for mode in (refbox.IOU_BEV, refbox.IOU_3D):
        got, want = refbox.pairs(t, clean, mode), refbox.pairs(clean, clean, mode)
        dead = [3, 5] + list(range(20, 32)) + ([7] if mode == refbox.IOU_3D else [])
        assert (got[dead] == 0).all() and (refbox.pairs(clean, t, mode)[:, dead] == 0).all()
        live = [i for i in range(32) if i not in dead]
        assert np.array_equal(got[live], want[live])


# ------------------------------------------------------------------------------------------- NMS against a plain loop
def _plain_nms(iou, valid, score, thresh, bid, B, cls, pre_max, post_max, score_thresh):
    keep, count = np.full((B, post_max), -1, np.int32), np.zeros(B, np.int32)
    for b in range(B):
        cand = [i for i in range(len(score)) if valid[i] and bid[i] == b and not np.isnan(score[i]) and
                (score_thresh is None or score[i] > np.float32(score_thresh))]
        cand.sort(key=lambda i: (-float(score[i]), i))
        kept = []
        for i in cand[:pre_max]:
            if len(kept) < post_max and not any(iou[k, i] > np.float32(thresh) and (cls is None or cls[k] == cls[i])
                                                for k in kept):
                kept.append(i)
        keep[b, :len(kept)], count[b] = kept, len(kept)
    return keep, count


@pytest.mark.parametrize("thresh", (0.1, 0.5))
@pytest.mark.parametrize("with_cls", (False, True))
@pytest.mark.parametrize("score_thresh", (None, 0.4))
@pytest.mark.parametrize("pre_post", ((16384, 16384), (40, 40), (60, 7), (5, 1)))
def test_nms_equals_a_plain_loop(thresh, with_cls, score_thresh, pre_post):
    n, B = 160, 2
    boxes, bid, score = boxscenes.cloud(31, n, B)
    rng = np.random.default_rng(3)
    score = (np.floor(score * 16) / 16).astype(np.float32)       # tied scores
    score[rng.integers(0, n, 6)] = np.nan
    bid[rng.integers(0, n, 6)] = rng.choice([-1, B, 1 << 20], 6)
    bev, z = boxscenes.corners64(boxes)
    bev[rng.integers(0, n, 6)] = np.nan
    cls = rng.integers(0, 3, n).astype(np.int32) if with_cls else None
    t = refbox.Table(bev, z, n_boxes=150)
    iou = refbox.pairs(t, t, refbox.IOU_BEV)
    want = _plain_nms(iou, t.valid, score, thresh, bid, B, cls, *pre_post, score_thresh)
    got = refbox.nms(t, score, thresh, bid, B, cls, *pre_post, score_thresh)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert 0 < got[1].sum() <= B * pre_post[1]


def test_negative_zero_ranks_below_positive_zero_and_ties_go_to_the_lower_index():
    boxes = np.zeros((4, 7), np.float32)
    boxes[:, 0] = np.arange(4) * 10.0
    boxes[:, 3:6] = 1.0
    t = refbox.Table(*boxscenes.corners64(boxes))
    keep, count = refbox.nms(t, np.array([-0.0, 0.0, 0.0, -1.0], np.float32), 0.5, post_max=4)
    assert keep.tolist() == [[1, 2, 0, 3]] and count.tolist() == [4]
