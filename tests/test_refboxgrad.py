"""CPU: refboxgrad -- the restatement ``spx_boxes_iou_aligned_grad`` is held to bit for bit -- against central differences
of an INDEPENDENT float64 value (the points-sorted-by-angle overlap of test_refbox.iou64, extended by the z term and
the DIoU penalty, over the seven numbers of either box), and against closed forms."""
import math

import numpy as np
import pytest

import boxpairs
import boxscenes
import refbox
import refboxgrad as rg
from test_refbox import _ccw64, _inside64

N_PAIRS, STEP = 256, 1e-6
COMBOS = [(rg.IOU_BEV, rg.NONE), (rg.IOU_3D, rg.NONE), (rg.IOU_BEV, rg.DIOU), (rg.IOU_3D, rg.DIOU)]
IDS = ["bev", "3d", "bev-diou", "3d-diou"]
# the worst component error of the float32 restatement against the differences, measured on pairs(2026, 256)
# (no pair is left out by the kink rule there; the float64 rules differ from the differences by 1.6e-8 at the most)
MEASURED_F32 = {(rg.IOU_BEV, rg.NONE): 5.22e-6, (rg.IOU_3D, rg.NONE): 6.14e-6,
                (rg.IOU_BEV, rg.DIOU): 4.41e-6, (rg.IOU_3D, rg.DIOU): 6.13e-6}


# ------------------------------------------------------------------------------------------- the independent value
def _plane64(qa, qb):
    """(inter, area_a, area_b) of two quads in float64: the corners of either inside the other and the edge crossings,
    sorted by angle, the shoelace formula."""
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
        return 0.0, area_a, area_b
    pts = np.asarray(pts)
    c = pts.mean(0)
    pts = pts[np.argsort(np.arctan2(pts[:, 1] - c[1], pts[:, 0] - c[0]), kind="stable")]
    x, y = pts[:, 0], pts[:, 1]
    return 0.5 * abs(np.sum(x * np.roll(y, -1) - np.roll(x, -1) * y)), area_a, area_b


def _corners(box):
    bev, z = rg.corners_f64(box[None])
    return bev[0], z[0]


def _values64(p, penalty, plane=None):
    """{mode: value} of the pair p = (a's seven numbers, b's seven numbers); the box centres are the boxes' own."""
    a, b = p[:7], p[7:]
    (qa, za), (qb, zb) = _corners(a), _corners(b)
    inter, aa, ab = plane if plane is not None else _plane64(qa, qb)
    h = max(min(za[1], zb[1]) - max(za[0], zb[0]), 0.0)
    i3 = inter * h
    out = {rg.IOU_BEV: inter / max(aa + ab - inter, 1e-8), rg.IOU_3D: i3 / max(aa * a[5] + ab * b[5] - i3, 1e-6)}
    if penalty == rg.DIOU:
        both = np.concatenate([qa, qb])
        w, v = both[:, 0].max() - both[:, 0].min(), both[:, 1].max() - both[:, 1].min()
        d = max(za[1], zb[1]) - min(za[0], zb[0])
        r2 = (a[0] - b[0]) ** 2 + (a[1] - b[1]) ** 2
        out[rg.IOU_BEV] -= r2 / max(w * w + v * v, 1e-12)
        out[rg.IOU_3D] -= (r2 + (a[2] - b[2]) ** 2) / max(w * w + v * v + d * d, 1e-12)
    return out


def _differences(a, b, penalty):
    """{mode: [n, 14]} by central differences of the independent value (the plane is not recomputed for z and dz)."""
    n = a.shape[0]
    out = {rg.IOU_BEV: np.zeros((n, 14)), rg.IOU_3D: np.zeros((n, 14))}
    for i in range(n):
        p = np.concatenate([a[i], b[i]]).astype(np.float64)
        base = _plane64(_corners(p[:7])[0], _corners(p[7:])[0])
        for c in range(14):
            plane = base if c % 7 in (2, 5) else None
            hi, lo = p.copy(), p.copy()
            hi[c] += STEP
            lo[c] -= STEP
            vh, vl = _values64(hi, penalty, plane), _values64(lo, penalty, plane)
            for mode in out:
                out[mode][i, c] = (vh[mode] - vl[mode]) / (2 * STEP)
    return out


def _analytic(a, b, mode, penalty, T):
    """[n, 14]: the rules of refboxgrad in T over the corners (float64: unrounded; float32: rounded to fp32), chained to
    the box numbers in float64; and per pair the facts the kink rule looks at."""
    n = a.shape[0]
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    (qa, za), (qb, zb) = (rg.corners_f64(a64), rg.corners_f64(b64)) if T is np.float64 else \
        (boxscenes.corners64(a), boxscenes.corners64(b))
    ga, gza, gb, gzb = np.zeros((n, 4, 2)), np.zeros((n, 2)), np.zeros((n, 4, 2)), np.zeros((n, 2))
    infos = []
    for i in range(n):
        info = {}
        _, ga[i], gza[i], gb[i], gzb[i] = rg.pair_grad(qa[i], za[i], qb[i], zb[i], mode, penalty, 1.0, T, info)
        infos.append(info)
    return np.concatenate([rg.chain64(a64, ga, gza), rg.chain64(b64, gb, gzb)], 1), infos


def _near_kink(a, b, mode, penalty, info):
    """The condition under which a pair is left out: it lies within 1e-4 of a point where the value has no derivative.
    `clip` within 1e-4 of the smaller area counts only when the smaller box is not wholly inside the other: there both
    branches of the min have the same gradient, and leaving those pairs in asks more, not less."""
    eps = 1e-4
    za, zb = (a[2] - a[5] / 2, a[2] + a[5] / 2), (b[2] - b[5] / 2, b[2] + b[5] / 2)
    if mode == rg.IOU_3D and (abs(za[0] - zb[0]) < eps or abs(za[1] - zb[1]) < eps or abs(float(info["h"])) < eps):
        return True
    A, B = info["A"], info["B"]
    S, L = (A, B) if info["aa"] <= info["ab"] else (B, A)
    inside = all(_inside64(p, np.asarray(L.q, np.float64)) for p in np.asarray(S.q, np.float64))
    if abs(float(info["clip"]) - float(info["small"])) < eps and float(info["clip"]) > 0 and not inside:
        return True
    if penalty == rg.DIOU:
        for box in (a, b):
            r = float(box[6]) / (math.pi / 2)
            if abs(r - round(r)) * (math.pi / 2) < 1e-3:
                return True
        both = np.concatenate([np.asarray(A.q, np.float64), np.asarray(B.q, np.float64)])
        for c in (0, 1):
            v = np.sort(both[:, c])
            if v[1] - v[0] < eps or v[-1] - v[-2] < eps:
                return True
    return False


@pytest.fixture(scope="module")
def scene():
    target, pred, far = boxpairs.pairs(2026, N_PAIRS)
    tables = {rg.NONE: (pred, target), rg.DIOU: (far, target)}
    return {"tables": tables, "diff": {pen: _differences(a, b, pen) for pen, (a, b) in tables.items()}}


def _compare(scene, mode, penalty, T):
    a, b = scene["tables"][penalty]
    got, infos = _analytic(a, b, mode, penalty, T)
    want = scene["diff"][penalty][mode]
    if mode == rg.IOU_BEV:                               # the plane knows no z and no dz
        assert not got[:, [2, 5, 9, 12]].any() and np.abs(want[:, [2, 5, 9, 12]]).max() < 1e-9
    keep = np.array([not _near_kink(a[i].astype(np.float64), b[i].astype(np.float64), mode, penalty, infos[i])
                     for i in range(len(a))])
    left_out = int((~keep).sum())
    assert left_out <= 0.02 * len(a), left_out
    err = np.abs(got - want)[keep]
    print(f"mode {mode} penalty {penalty} {T.__name__}: left out {left_out}, worst error {err.max():.3e}, largest "
          f"component {np.abs(want[keep]).max():.3f}")
    return float(err.max())


@pytest.mark.parametrize("mode, penalty", COMBOS, ids=IDS)
def test_float64_rules_equal_the_differences_of_the_independent_value(scene, mode, penalty):
    """The edge integral, the clamp rule, the z rule and the penalty in float64 against central differences (step 1e-6)
    of a value that shares no code with them: within 1e-6 on every one of the fourteen box numbers."""
    assert _compare(scene, mode, penalty, np.float64) <= 1e-6


@pytest.mark.parametrize("mode, penalty", COMBOS, ids=IDS)
def test_float32_restatement_stays_within_the_measured_bound_of_the_differences(scene, mode, penalty):
    """The corner-space part in numpy float32 scalars over fp32 corners, the chain to the box numbers in float64.
    Measured on pairs(2026, 256), worst component error against the differences (MEASURED_F32): 5.22e-6 in the plane,
    6.14e-6 in space, 4.41e-6 / 6.13e-6 with the DIoU penalty (the rounding of the corners to fp32 and of the edge
    cuts; the largest gradient component is 0.77; no pair is left out).  The assertion is four times that; the factor
    covers another libm rounding the corners, not another algorithm."""
    worst = _compare(scene, mode, penalty, np.float32)
    assert worst <= 4 * MEASURED_F32[(mode, penalty)], worst


def test_the_scenario_holds_what_it_promises(scene):
    pred, target = scene["tables"][rg.NONE]
    far = scene["tables"][rg.DIOU][0]
    t = refbox.Table(*boxscenes.corners64(target))
    iou = refbox.aligned(refbox.Table(*boxscenes.corners64(pred)), t, refbox.IOU_3D)
    iou_far = refbox.aligned(refbox.Table(*boxscenes.corners64(far)), t, refbox.IOU_3D)
    assert (iou > 0).sum() >= 0.9 * N_PAIRS and (iou_far[2::4] == 0).all() and (iou[7::8] > 0).all()
    assert np.array_equal(np.delete(iou_far, np.arange(2, N_PAIRS, 4)), np.delete(iou, np.arange(2, N_PAIRS, 4)))


# ------------------------------------------------------------------------------------------- closed forms
def _box(x, y, z, dx, dy, dz, heading=0.0):
    return np.array([[x, y, z, dx, dy, dz, heading]], np.float64)


def _grad7(a, b, mode, penalty=rg.NONE, T=np.float64):
    (qa, za), (qb, zb) = rg.corners_f64(a), rg.corners_f64(b)
    v, ga, gza, gb, gzb = rg.pair_grad(qa[0], za[0], qb[0], zb[0], mode, penalty, 1.0, T)
    return float(v), rg.chain64(a, [ga], [gza])[0], rg.chain64(b, [gb], [gzb])[0]


@pytest.mark.parametrize("T", (np.float32, np.float64))
def test_unit_squares_offset_by_half(T):
    """A = the unit square at (0.5, 0), B = the unit square at the origin: overlap 0.5.  The edge integral by hand (A's
    left edge lies wholly inside B, its top and bottom edges from t = 0.5 on; B's right edge wholly inside A): moving A
    in +x loses area at rate 1."""
    a, b = _box(0.5, 0, 0, 1, 1, 1), _box(0, 0, 0, 1, 1, 1)
    A, B = rg.Rec(rg.corners_f64(a)[0][0], None, T), rg.Rec(rg.corners_f64(b)[0][0], None, T)
    assert refbox.clip_area(A.q, B.q) == 0.5
    gxa, gya, gxb, gyb = [T(0)] * 4, [T(0)] * 4, [T(0)] * 4, [T(0)] * 4
    rg.edge_integral(A, B, gxa, gya, T)
    rg.edge_integral(B, A, gxb, gyb, T)
    assert list(zip(gxa, gya)) == [(0, 0.125), (-0.5, 0.375), (-0.5, -0.375), (0, -0.125)]
    assert list(zip(gxb, gyb)) == [(0.5, 0.375), (0, 0.125), (0, -0.125), (0.5, -0.375)]
    # d overlap / d (x, y, z, dx, dy, dz, heading) of A and of B
    assert rg.chain64(a, [list(zip(gxa, gya))])[0].tolist() == [-1.0, 0, 0, 0.5, 0.5, 0, 0]
    assert rg.chain64(b, [list(zip(gxb, gyb))])[0].tolist() == [1.0, 0, 0, 0.5, 0.5, 0, 0]
    # the IoU in the plane: 0.5 / 1.5, d iou = d inter * 2 / 1.5^2 - d area * 0.5 / 1.5^2
    v, g_a, g_b = _grad7(a, b, rg.IOU_BEV, T=T)
    tol = 1e-6 if T is np.float32 else 1e-14
    assert abs(v - 1 / 3) <= tol
    assert np.abs(g_a - np.array([-8 / 9, 0, 0, 4 / 9 - 2 / 9, 4 / 9 - 2 / 9, 0, 0])).max() <= tol
    assert np.abs(g_b - np.array([8 / 9, 0, 0, 4 / 9 - 2 / 9, 4 / 9 - 2 / 9, 0, 0])).max() <= tol


def test_a_contained_box_has_its_area_gradient():
    a, b = _box(0.25, -0.125, 0, 1, 0.75, 1, 0.5), _box(0, 0, 0, 4, 2, 2, 0.25)
    for T in (np.float32, np.float64):
        A, B = rg.Rec(rg.corners_f64(a)[0][0], None, T), rg.Rec(rg.corners_f64(b)[0][0], None, T)
        gxa, gya, gxb, gyb = [T(0)] * 4, [T(0)] * 4, [T(0)] * 4, [T(0)] * 4
        rg.edge_integral(A, B, gxa, gya, T)
        rg.edge_integral(B, A, gxb, gyb, T)
        wx, wy = rg.area_grad(A, T)
        tol = 4 * float(np.finfo(T).eps)
        assert np.abs(np.array(gxa, np.float64) - np.array(wx, np.float64)).max() <= tol
        assert np.abs(np.array(gya, np.float64) - np.array(wy, np.float64)).max() <= tol
        assert not any(gxb) and not any(gyb)
    # the IoU is area(A) / area(B): it grows with A's sizes and does not move with its centre or heading
    v, g_a, g_b = _grad7(a, b, rg.IOU_BEV)
    assert abs(v - 0.75 / 8) < 1e-14
    assert np.abs(g_a - np.array([0, 0, 0, 0.75 / 8, 1 / 8, 0, 0])).max() < 1e-14
    assert np.abs(g_b - np.array([0, 0, 0, -0.75 / 8 / 4, -0.75 / 8 / 2, 0, 0])).max() < 1e-14


def test_disjoint_boxes_move_only_under_the_penalty():
    a, b = _box(0, 0, 0, 2, 2, 2), _box(10, 0.5, 1, 2, 2, 2)
    for mode in (rg.IOU_BEV, rg.IOU_3D):
        for T in (np.float32, np.float64):
            v, g_a, g_b = _grad7(a, b, mode, T=T)
            assert v == 0 and not g_a.any() and not g_b.any()
    # DIoU in the plane: rho2 = 100.25, the enclosing box is 12 x 2.5.  x_a moves rho2 by 2 * (x_a - x_b) and the lower
    # end of the width; dx_a moves the lower end alone; y_a moves rho2 and the lower end of the height
    v, g_a, g_b = _grad7(a, b, rg.IOU_BEV, rg.DIOU)
    r2, c2 = 100.25, 144 + 6.25
    assert abs(v + r2 / c2) < 1e-14
    assert abs(g_a[0] - (20 / c2 - r2 / c2 ** 2 * 24)) < 1e-14 and abs(g_b[0] - (-20 / c2 + r2 / c2 ** 2 * 24)) < 1e-14
    assert abs(g_a[1] - (1 / c2 - r2 / c2 ** 2 * 5)) < 1e-14 and abs(g_b[1] - (-1 / c2 + r2 / c2 ** 2 * 5)) < 1e-14
    assert abs(g_a[3] - r2 / c2 ** 2 * 12) < 1e-14 and abs(g_b[3] - r2 / c2 ** 2 * 12) < 1e-14
    # in space: the z terms join (dz = -1, the enclosing height 3)
    v, g_a, g_b = _grad7(a, b, rg.IOU_3D, rg.DIOU)
    r3, c3 = r2 + 1, c2 + 9
    assert abs(v + r3 / c3) < 1e-14
    assert abs(g_a[2] - (2 / c3 - r3 / c3 ** 2 * 6)) < 1e-14 and abs(g_a[5] - r3 / c3 ** 2 * 3) < 1e-14
    assert abs(g_b[2] - (-2 / c3 + r3 / c3 ** 2 * 6)) < 1e-14 and abs(g_b[5] - r3 / c3 ** 2 * 3) < 1e-14


@pytest.mark.parametrize("mode, penalty", COMBOS, ids=IDS)
def test_clockwise_corners_get_the_gradient_at_the_reversed_indices(mode, penalty):
    target, pred, far = boxpairs.pairs(5, 24)
    (qa, za), (qb, zb) = boxscenes.corners64(far), boxscenes.corners64(target)
    want = rg.aligned_grad(qa, za, qb, zb, mode, penalty)
    for ra, rb in ((True, False), (False, True), (True, True)):
        got = rg.aligned_grad(qa[:, ::-1] if ra else qa, za, qb[:, ::-1] if rb else qb, zb, mode, penalty)
        assert np.array_equal(got[0], want[0])
        assert np.array_equal(got[1], want[1][:, ::-1] if ra else want[1])
        assert np.array_equal(got[3], want[3][:, ::-1] if rb else want[3])
        assert np.array_equal(got[2], want[2]) and np.array_equal(got[4], want[4])
    assert np.abs(want[1]).max() > 0.01


@pytest.mark.parametrize("mode, penalty", COMBOS, ids=IDS)
def test_an_invalid_box_gives_zeros_and_a_duplicate_is_finite(mode, penalty):
    target, pred, _ = boxpairs.pairs(9, 16)
    pred[4:8] = target[4:8]                              # exact duplicates
    (qa, za), (qb, zb) = boxscenes.corners64(pred), boxscenes.corners64(target)
    qa[1, 2, 0], qb[2], za[3, 1] = np.nan, np.inf, np.nan
    go = np.linspace(-1, 2, 16).astype(np.float32)
    out = rg.aligned_grad(qa, za, qb, zb, mode, penalty, go, n_a=14, n_b=15)
    dead = [1, 2, 14, 15] + ([3] if mode == rg.IOU_3D else [])
    for t in out:
        assert np.isfinite(t).all() and not t[dead].any()
    live = [i for i in range(16) if i not in dead]
    assert all(np.abs(out[1][i]).max() > 0 for i in live if go[i] != 0)
    if penalty == rg.NONE:
        assert (out[0][4:8] == 1).all()
        assert np.array_equal(out[0], refbox.aligned(refbox.Table(qa, za, 14), refbox.Table(qb, zb, 15), mode))
