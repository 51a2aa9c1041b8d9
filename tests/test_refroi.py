"""CPU: tests/refroi.py (the numpy float32 restatement of csrc/roi.hip) against an independent float64 formulation --
the four half-planes of the float64 corners plus the z slab -- and its own tables against each other."""
import functools

import numpy as np

import refroi

U = 2.0 ** -24          # unit round-off of float32


@functools.lru_cache(maxsize=None)
def big():
    """seed 7: 20 000 points, half drawn inside boxes; 64 boxes in +-40 m with sizes x U(0.5, 4), eight headings in +-100"""
    boxes, b_ids, points, p_ids = refroi.scene(7, 20000, 64)
    c, s = refroi.trig32(boxes)
    return boxes, points, refroi.frames_given_trig(boxes, c, s)


def halfplanes64(boxes, points):
    """(inside bool [M, N], distance to the nearest face fp64 [M, N], |sx| + |sy| + |lz| fp64 [M, N]) from the float64
    corners of the float32 boxes: a point is inside when it lies strictly left of the four counter-clockwise edges
    and inside the closed z slab"""
    b, p = boxes.astype(np.float64), points.astype(np.float64)
    c, s = np.cos(b[:, 6]), np.sin(b[:, 6])
    sgx, sgy = np.array([1.0, -1.0, -1.0, 1.0]), np.array([1.0, 1.0, -1.0, -1.0])
    lx, ly = sgx[None] * b[:, 3:4] * 0.5, sgy[None] * b[:, 4:5] * 0.5
    X = b[:, 0:1] + (lx * c[:, None] - ly * s[:, None])                  # [M, 4]
    Y = b[:, 1:2] + (lx * s[:, None] + ly * c[:, None])
    inside = np.ones((len(b), len(p)), bool)
    near = np.full((len(b), len(p)), np.inf)
    for k in range(4):
        ex, ey = X[:, (k + 1) % 4] - X[:, k], Y[:, (k + 1) % 4] - Y[:, k]
        d = (ex[:, None] * (p[None, :, 1] - Y[:, k, None]) - ey[:, None] * (p[None, :, 0] - X[:, k, None])) / np.hypot(ex, ey)[:, None]
        inside &= d > 0.0
        near = np.minimum(near, np.abs(d))
    dz = b[:, 5:6] * 0.5 - np.abs(p[None, :, 2] - b[:, 2:3])
    inside &= dz >= 0.0
    near = np.minimum(near, np.abs(dz))
    mag = np.abs(p[None, :, 0] - b[:, 0:1]) + np.abs(p[None, :, 1] - b[:, 1:2]) + np.abs(p[None, :, 2] - b[:, 2:3])
    return inside, near, mag


def test_float32_test_against_float64_halfplanes():
    """Bound on the distance to the nearest face of a pair the two formulations may disagree on, from the magnitudes:
    with u = 2^-24, sx = fl(px - x) carries a relative error u, the float32 cosine and sine (rounded from float64) u,
    each product u and the sum u: |lx32 - lx| <= (|sx c| + |sy s|) (4 u + O(u^2)) <= 4 u (|sx| + |sy|), the same for
    ly, and |lz32 - lz| <= u |lz|; the half sizes dx * 0.5f are exact.  The float64 side errs by 2^-53 of the same
    magnitudes.  Asserted: 5 u (|sx| + |sy| + |lz|)."""
    boxes, points, frames = big()
    hit32, _, _, _ = refroi.inside(frames, points)
    hit64, near, mag = halfplanes64(boxes, points)
    n64 = int(hit64.sum())
    diff = hit32 != hit64
    per_box = hit64.sum(1)
    multi = int((hit64.sum(0) > 1).sum())
    print(f"{n64} incidences, {int(diff.sum())} disagreements, {per_box.min()}-{per_box.max()} hits per box, "
          f"{multi} points in more than one box")
    assert n64 > 5000 and per_box.min() > 0 and multi > 100            # the scene exercises the test
    assert (near[diff] < 5.0 * U * mag[diff]).all()
    assert diff.sum() <= 0.001 * n64


def test_frames_given_trig_follow_the_validity_rule():
    boxes, _, _, _ = refroi.scene(3, 0, 40)
    kinds = [(0, np.nan), (1, np.inf), (6, -np.inf), (3, 0.0), (4, -1.0), (5, 0.0), (2, np.nan), (5, -2.0)]
    for t, (col, v) in enumerate(kinds):
        boxes[2 + 3 * t, col] = v
    c, s = refroi.trig32(boxes)
    fr = refroi.frames_given_trig(boxes, c, s, (0.25, 0.5, 1.0), n_boxes=35)
    dead = np.zeros(40, bool)
    dead[[2 + 3 * t for t in range(8)]] = True
    dead[35:] = True
    assert np.isnan(fr[dead]).all() and np.isfinite(fr[~dead]).all()
    ok = ~dead
    np.testing.assert_array_equal(fr[ok, 3], boxes[ok, 3] * np.float32(0.5) + np.float32(0.25))
    np.testing.assert_array_equal(fr[ok, 5], boxes[ok, 5] * np.float32(0.5) + np.float32(1.0))
    np.testing.assert_array_equal(fr[ok, :3], boxes[ok, :3])
    assert not refroi.inside(fr[dead], boxes[:, :3]).__getitem__(0).any()     # a NaN frame contains nothing


def test_faces_are_strict_in_the_plane_and_inclusive_in_z():
    box, pts, want = refroi.faces()
    fr = refroi.frames_given_trig(box, [1.0], [0.0])
    np.testing.assert_array_equal(fr[0], np.array([0, 0, 0, 2, 1, 0.5, 1, 0], np.float32))
    assert refroi.inside(fr, pts)[0][0].tolist() == want.tolist()
    assert want.sum() == 7


def test_tables_agree_with_each_other_and_with_the_pads():
    boxes, b_ids, points, p_ids = refroi.scene(11, 3000, 24, batch=3)
    points[5, 0], points[6, 2] = np.nan, np.inf
    p_ids[7], b_ids[3] = 3, -1
    c, s = refroi.trig32(boxes)
    fr = refroi.frames_given_trig(boxes, c, s, n_boxes=22)
    hit, lx, ly, lz = refroi.incidence(fr, b_ids, points, p_ids, 3, n_boxes=22, n_points=2900)
    assert not hit[:, [5, 6, 7]].any() and not hit[3].any() and not hit[22:].any() and not hit[:, 2900:].any()
    assert (b_ids[:, None] == p_ids[None, :])[hit].all()
    pib = refroi.points_in_boxes(fr, b_ids, points, p_ids, 3, n_boxes=22, n_points=2900)
    for i in range(len(points)):
        col = np.flatnonzero(hit[:, i])
        assert pib[i] == (col[0] if len(col) else -1)
    assert (hit.sum(0) > 1).any()                                      # overlapping boxes: the lowest index wins
    ns = 60                                                            # (45 .. 75 hits per box: the cut falls both ways)
    q = {pad: refroi.box_query(fr, b_ids, points, p_ids, 3, ns, pad, (4, 3, 2), 22, 2900) for pad in (0, 2, 4)}
    base = q[0]
    np.testing.assert_array_equal(base["hits"], hit.sum(1))
    np.testing.assert_array_equal(base["count"], np.minimum(base["hits"], ns))
    assert (base["hits"] > ns).any() and (base["count"] == 0).any() and ((base["count"] > 0) & (base["count"] < ns)).any()
    for m in range(24):
        cn = base["count"][m]
        np.testing.assert_array_equal(base["rows"][m, :cn], np.flatnonzero(hit[m])[:cn])
        assert (base["rows"][m, cn:] == -1).all() and (base["cells"][m, cn:] == -1).all() and (base["local"][m, cn:] == 0).all()
        cells = base["cells"][m, :cn]
        assert ((cells >= m * 24) & (cells < (m + 1) * 24)).all()
        # the cell is the one whose float64 bounds hold the local point, up to rounding at a cell face
        ix = (cells - m * 24) // 6
        lo = -fr[m, 3].astype(np.float64) + ix * (2.0 * fr[m, 3] / 4)
        assert (base["local"][m, :cn, 0] >= lo - 1e-4).all() and (base["local"][m, :cn, 0] <= lo + 2.0 * fr[m, 3] / 4 + 1e-4).all()
        for pad in (2, 4):
            for key in ("rows", "cells", "local"):
                np.testing.assert_array_equal(q[pad][key][m, :cn], base[key][m, :cn])
                if cn == 0:
                    np.testing.assert_array_equal(q[pad][key][m], base[key][m])
                for s_ in range(cn, ns if cn else 0):
                    src = s_ % cn if pad == 4 else 0
                    np.testing.assert_array_equal(q[pad][key][m, s_], base[key][m, src])
