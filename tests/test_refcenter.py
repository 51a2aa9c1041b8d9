"""CPU: the numpy float32 restatement of the centre-head targets (tests/refcenter.py, what the GPU tests hold the
kernels to bit for bit) against an independent float64 formulation written the way OpenPCDet's Python loop is
(gaussian_radius with Python floats, gaussian2D arrays sliced into the map box by box, a distance vector per box over
the rows of a scene).  Integer results agree exactly for EVERY box of every fixture -- a condition on the fixtures,
asserted here: a seed that puts a truncation on the fence is changed, no box is excluded.

The heat bound.  u = 2^-24 is the unit roundoff of float32.  A relative error e of the argument a <= 0 of exp moves the
value by |a| exp(a) e <= e / e (t exp(-t) peaks at t = 1 with 1 / e), and the float32 side rounds exp itself once: half
an ulp of a value <= 1, 2^-25.
  * integer distance (dense; sparse anchor="nearest"): the numerator is exact (below 2^24), sigma = (2 r + 1) / 6 is
    rounded once, 2 sigma is exact, (2 sigma) sigma is rounded once over two factors that carry sigma's error, the
    quotient is rounded once: e <= 4 u, so the bound is 4 u / e + 2^-25 = 1.2e-7 (DENSE_BOUND).
  * float distance (sparse anchor="center"): the float32 centre differs from the float64 one by up to eps = 4 u max(W, H)
    (the difference x - x0, two quotients, and float32(0.1) against 0.1), which moves d2 = dx^2 + dy^2 by up to 2 (|dx| +
    |dy|) eps.  With t = |dx| / (sqrt(2) sigma) the change of the value is at most exp(-t^2) sqrt(2) t eps / sigma <=
    eps / (sigma sqrt(e)) per axis (t exp(-t^2) peaks at 1 / sqrt(2 e)); sigma >= (2 min_radius + 1) / 6.  d2 itself is
    three roundings over terms with a relative error of 2 u each: e <= 5 u + the 3 u of the denominator and quotient.
    The bound is 2 eps / (sigma_min sqrt(e)) + 8 u / e + 2^-25 (center_bound())."""
import numpy as np
import pytest

import centerscenes as cs
import refcenter as rc
from spconv_amd import _lib

U = 2.0 ** -24
DENSE_BOUND = 4 * U / np.e + 2.0 ** -25


def center_bound(min_radius=2):
    eps = 4 * U * max(cs.W, cs.H)
    sigma = (2 * min_radius + 1) / 6
    return 2 * eps / (sigma * np.sqrt(np.e)) + 8 * U / np.e + 2.0 ** -25


@pytest.fixture(scope="module")
def tile():
    return int(_lib.load().spx_center_tile())


@pytest.fixture(scope="module", params=cs.STRIDES)
def both(request, tile):
    stride = request.param
    boxes, bid, cls, n = cs.boxes(stride, tile)
    p = cs.params(stride)
    return stride, rc.records(boxes, bid, cls, cs.B, n, **p), rc.records64(boxes, bid, cls, cs.B, n, **p), boxes


def test_the_fixtures_hold_what_they_promise(both, tile):
    stride, r32, r64, boxes = both
    scenes = r32["scenes"]
    assert len(scenes[0]) == tile + 2 > cs.MAX_OBJS and len(scenes[1]) == 0 and len(scenes[2]) == 26
    assert (r32["slot"][scenes[0][cs.MAX_OBJS:]] == -1).all() and (r32["cls"][scenes[0][cs.MAX_OBJS:]] == -1).all()
    part = r32["cls"] >= 0
    cell, rad = r32["cell"][part], r32["radius"][part]
    for corner in ((0, 0), (cs.W - 1, 0), (0, cs.H - 1), (cs.W - 1, cs.H - 1)):
        assert ((cell == corner).all(1)).any(), corner
    assert (r32["center"][part] == (0.0, 0.0)).all(1).any()                       # clamped on both axes
    assert (r32["center"][part][:, 0] == cs.W - 0.5).any() and (r32["center"][part][:, 1] == cs.H - 0.5).any()
    assert rad.min() == 2
    if stride == 1:
        assert rad.max() >= 12
    if stride == 4:
        assert (rad == 2).sum() > 20                                              # the min_radius clamp at work
    same = [i for i in scenes[2] if tuple(r32["cell"][i]) == (12, 33) and r32["cls"][i] >= 0]
    assert sorted(r32["cls"][same]) == [0, 1, 1, 2]
    assert (~part[scenes[2]]).sum() >= 8                                          # the spoiled rows and foreign classes
    assert (r32["slot"][~part] >= 0).sum() >= 8                                   # ... keep their slots
    assert (r32["slot"] == -1).sum() >= tile + 2 - cs.MAX_OBJS + 4 + 9            # no slot: beyond max_objs, foreign, dead


def test_records_agree_with_the_float64_loop(both):
    _, r32, r64, _ = both
    for name in ("slot", "cell", "radius", "cls", "box_index", "mask", "inds"):
        assert np.array_equal(r32[name].astype(np.int64), r64[name]), name
    assert np.abs(r32["center"].astype(np.float64) - r64["center"]).max() <= 4 * U * max(cs.W, cs.H)


def test_dense_heat_agrees_with_sliced_gaussians(both):
    _, r32, r64, _ = both
    arg = rc.dense_args(r32)
    heat32, heat64 = rc.to_heat(arg), rc.dense_heat64(r64)
    assert np.array_equal(np.isnan(arg), heat64 == 0.0)                           # the same cells are reached
    err = np.abs(heat32.astype(np.float64) - heat64).max()
    print(f"dense |float32 - float64| max = {err:.3g} (bound {DENSE_BOUND:.3g})")
    assert err <= DENSE_BOUND
    assert (heat32 == 1.0).sum() >= 40 and heat32.max() == 1.0


@pytest.mark.parametrize("without", [None, 2])
def test_nearest_rows_and_sparse_heat_agree(both, without):
    _, r32, r64, _ = both
    idx, n_live = cs.rows(without=without)
    n32, i32, m32 = rc.nearest_rows(r32, idx, n_live)
    n64, i64, m64 = rc.nearest_rows64(r64, idx, n_live)
    assert np.array_equal(n32, n64) and np.array_equal(i32, i64) and np.array_equal(m32, m64)
    part = r32["cls"] >= 0
    assert (n32[~part] == -1).all()
    if without is None:
        assert (n32[part] >= 0).all() and (n32[part] < n_live).all()
        origin = np.nonzero(part & (r32["center"] == (0.0, 0.0)).all(1))[0]       # the exact tie: the lower row wins
        tied = np.nonzero((idx[:n_live, 0] == 2) & (idx[:n_live, 1] + idx[:n_live, 2] == 1))[0]
        assert len(origin) == 1 and len(tied) == 2 and n32[origin[0]] == tied.min()
    else:
        in2 = r32["bids"][:len(part)] == 2
        assert (n32[part & in2] == -1).all() and (m32[2] == 0).all() and r32["mask"][2].any()
    live = rc.live_rows(idx, cs.B, cs.W, cs.H, n_live)
    for anchor in ("center", "nearest"):
        bound = center_bound() if anchor == "center" else DENSE_BOUND
        for cutoff in ("none", "window"):
            arg = rc.sparse_args(r32, idx, n32, anchor, cutoff, n_live)
            heat32, heat64 = rc.to_heat(arg), rc.sparse_heat64(r64, idx, n64, anchor, cutoff, n_live)
            assert (heat32[~live] == 0).all() and (heat64[~live] == 0).all()
            if cutoff == "window":
                assert np.array_equal(np.isnan(arg), heat64 == 0.0), (anchor, cutoff)
            err = np.abs(heat32.astype(np.float64) - heat64).max()
            print(f"sparse {anchor}/{cutoff} |float32 - float64| max = {err:.3g} (bound {bound:.3g})")
            assert err <= bound, (anchor, cutoff)
            if anchor == "nearest" and without is None:
                assert (heat32 == 1.0).any()                                      # the nearest row itself: arg = 0
