"""Differentiable rotated IoU on the kernels of csrc/boxgrad.hip (spconv_amd/pytorch/_boxgrad.py,
spatial.RotatedIoU3DLoss) against the numpy float32 restatement tests/refboxgrad.py (whose rules test_refboxgrad.py
holds to central differences of an independent float64 value on the CPU), over the pairs of tests/boxpairs.py.

The device's own corners are downloaded and handed to refboxgrad; the value and the four gradient tables of the pair
entry are compared bit for bit.  The corners backward is held to float64 numpy within a derived bound (the sine and
cosine are the one step a host does not reproduce), and the whole chain to the differences under the CPU's bound."""
import functools

import numpy as np
import pytest
import torch

import boxpairs
import refboxgrad as rg

pytestmark = pytest.mark.gpu

SIZES = (0, 1, 63, 64, 65, 257)
COMBOS = [(rg.IOU_BEV, "none"), (rg.IOU_3D, "none"), (rg.IOU_BEV, "diou"), (rg.IOU_3D, "diou")]
IDS = ["bev", "3d", "bev-diou", "3d-diou"]
PEN = {"none": rg.NONE, "diou": rg.DIOU}
NAMES = ("value", "gbev_a", "gz_a", "gbev_b", "gz_b")


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32).numpy()


def fbits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def dev(cuda, a):
    return None if a is None else torch.from_numpy(np.array(a, order="C")).to(cuda)


def count_of(cuda, n):
    return None if n is None else torch.tensor([n], dtype=torch.int32, device=cuda)


def dirty(cuda, shape):
    """an output table in the state a caller may hand it over in: every byte 0xFF"""
    return torch.full(shape, 0xFF, dtype=torch.uint8, device=cuda).repeat_interleave(4, dim=-1).view(torch.float32)


def outputs(cuda, n, names=NAMES):
    shapes = {"value": (n,), "gbev_a": (n, 4, 2), "gz_a": (n, 2), "gbev_b": (n, 4, 2), "gz_b": (n, 2)}
    return {k: dirty(cuda, shapes[k]).reshape(shapes[k]) for k in names}


def run(cuda, ca, cb, mode, penalty, go=None, names=NAMES):
    """the pair entry over dirty outputs -> {name: tensor}"""
    from spconv_amd.pytorch import functional as F
    out = outputs(cuda, ca.num_boxes, names)                 # (in the plane the z tables are written too: zeros)
    F.boxes_iou_aligned_grad_into(ca, cb, mode, penalty=penalty, grad_out=go, **out)
    torch.cuda.synchronize()
    return out


def reference(ca, cb, mode, penalty, go=None, n_a=None, n_b=None):
    """refboxgrad over the DOWNLOADED corners -> {name: array}"""
    z = lambda c: None if c.zrange is None else c.zrange.cpu().numpy()
    got = rg.aligned_grad(ca.bev.cpu().numpy(), z(ca), cb.bev.cpu().numpy(), z(cb), mode, PEN[penalty],
                          None if go is None else go.cpu().numpy(), n_a, n_b)
    return dict(zip(NAMES, got))


def assert_bits(out, want):
    for k, t in out.items():
        np.testing.assert_array_equal(bits(t), fbits(want[k]).reshape(bits(t).shape), err_msg=k)


@functools.lru_cache(maxsize=None)
def pair_state(n):
    """(BoxCorners of the predictions, of the targets, a random grad_out), on the device; every fourth pair disjoint,
    every eighth prediction contained"""
    from spconv_amd.pytorch import functional as F
    cuda = torch.device("cuda:0")
    target, _, far = boxpairs.pairs(2026 + n, n)
    go = np.random.default_rng(n).standard_normal(n).astype(np.float32)
    return F.boxes_to_corners(dev(cuda, far)), F.boxes_to_corners(dev(cuda, target)), dev(cuda, go)


@functools.lru_cache(maxsize=None)
def pair_reference(n, mode, penalty, with_go):
    ca, cb, go = pair_state(n)
    return reference(ca, cb, mode, penalty, go if with_go else None)


# ------------------------------------------------------------------------------------------------ the pair entry

@pytest.mark.parametrize("mode, penalty", COMBOS, ids=IDS)
@pytest.mark.parametrize("N", SIZES)
def test_pair_entry_equals_refboxgrad_bit_for_bit(cuda, N, mode, penalty):
    ca, cb, go = pair_state(N)
    for with_go in (False, True):
        out = run(cuda, ca, cb, mode, penalty, go if with_go else None)
        want = pair_reference(N, mode, penalty, with_go)
        assert_bits(out, want)
        if N >= 63:
            assert np.abs(want["gbev_a"]).max() > 0.01 and (want["value"] > 0.3).any()
            if penalty == "diou":
                assert (want["value"] < 0).any()        # and every disjoint pair moves
                assert np.abs(want["gbev_a"][2::4]).reshape(-1, 8).max(1).min() > 0


def test_without_a_penalty_the_value_has_the_bits_of_the_forward(cuda):
    from spconv_amd.pytorch import functional as F
    ca, cb, _ = pair_state(257)
    v3 = run(cuda, ca, cb, rg.IOU_3D, "none", names=("value",))["value"]
    np.testing.assert_array_equal(bits(v3), bits(F.boxes_iou3d_aligned(ca, cb)))
    np.testing.assert_array_equal(bits(v3), bits(F.boxes_iou3d_diff(ca, cb)))
    vb = run(cuda, ca, cb, rg.IOU_BEV, "none", names=("value",))["value"]
    np.testing.assert_array_equal(bits(vb), bits(torch.diagonal(F.boxes_iou_bev(ca, cb))))
    np.testing.assert_array_equal(bits(vb), bits(F.boxes_iou_bev_diff(ca, cb)))
    assert (v3 > 0).sum() > 150 and (vb > v3).any()
    assert F.boxes_iou3d_diff(dev(cuda, np.zeros((0, 7), np.float32)), dev(cuda, np.zeros((0, 7), np.float32))).shape == (0,)


@pytest.mark.parametrize("mode, penalty", COMBOS, ids=IDS)
def test_device_counts_in_the_middle_of_a_block(cuda, mode, penalty):
    from spconv_amd.pytorch import functional as F
    ca, cb, go = pair_state(257)
    a = F.BoxCorners(ca.bev, ca.zrange, 257, count_of(cuda, 100))
    b = F.BoxCorners(cb.bev, cb.zrange, 257, count_of(cuda, 130))
    out = run(cuda, a, b, mode, penalty, go)
    assert_bits(out, reference(ca, cb, mode, penalty, go, 100, 130))
    full = pair_reference(257, mode, penalty, True)
    for k, t in out.items():
        assert not bits(t)[100:].any(), k
        np.testing.assert_array_equal(bits(t)[:100], fbits(full[k])[:100], err_msg=k)


@pytest.mark.parametrize("mode, penalty", COMBOS, ids=IDS)
def test_spoiled_rows_give_zero_value_and_zero_rows(cuda, mode, penalty):
    from spconv_amd.pytorch import functional as F
    target, _, far = boxpairs.pairs(77, 130)
    kinds = [(0, np.nan), (1, np.inf), (6, -np.inf), (3, 0.0), (4, -1.0), (5, 0.0), (2, np.nan), (5, -2.0)]
    rows_a, rows_b = list(range(3, 130, 9)), list(range(5, 130, 11))
    for t, r in enumerate(rows_a):
        far[r, kinds[t % 8][0]] = kinds[t % 8][1]
    for t, r in enumerate(rows_b):
        target[r, kinds[(t + 3) % 8][0]] = kinds[(t + 3) % 8][1]
    ca, cb = F.boxes_to_corners(dev(cuda, far)), F.boxes_to_corners(dev(cuda, target))
    za = ca.zrange.clone()
    za[64, 1], za[65, 0] = float("inf"), float("nan")                     # a z range spoiled in the caller's own table
    ca = F.BoxCorners(ca.bev, za, 130)
    out = run(cuda, ca, cb, mode, penalty)
    assert_bits(out, reference(ca, cb, mode, penalty))
    dead = sorted(set(rows_a) | set(rows_b) | ({64, 65} if mode == rg.IOU_3D else set()))
    live = [i for i in range(130) if i not in dead]
    for k, t in out.items():
        assert not bits(t)[dead].any(), k
        assert torch.isfinite(t).all(), k
    assert all(bits(out["gbev_a"])[i].any() for i in live if penalty == "diou" or i % 4 != 2)


@pytest.mark.parametrize("mode, penalty", COMBOS, ids=IDS)
def test_clockwise_caller_corners_get_their_gradient_at_their_own_indices(cuda, mode, penalty):
    from spconv_amd.pytorch import functional as F
    ca, cb, go = pair_state(65)
    ra = F.BoxCorners(ca.bev.flip(1).contiguous(), ca.zrange, 65)
    rb = F.BoxCorners(cb.bev.flip(1).contiguous(), cb.zrange, 65)
    want = pair_reference(65, mode, penalty, True)
    for a, b, fa, fb in ((ra, cb, True, False), (ca, rb, False, True), (ra, rb, True, True)):
        out = run(cuda, a, b, mode, penalty, go)
        assert_bits(out, reference(a, b, mode, penalty, go))
        np.testing.assert_array_equal(bits(out["value"]), fbits(want["value"]))
        np.testing.assert_array_equal(bits(out["gbev_a"].flip(1) if fa else out["gbev_a"]), fbits(want["gbev_a"]))
        np.testing.assert_array_equal(bits(out["gbev_b"].flip(1) if fb else out["gbev_b"]), fbits(want["gbev_b"]))


@pytest.mark.parametrize("mode, penalty", COMBOS, ids=IDS)
def test_each_output_may_be_left_out(cuda, mode, penalty):
    ca, cb, go = pair_state(65)
    full = run(cuda, ca, cb, mode, penalty, go)
    for gone in NAMES:
        out = run(cuda, ca, cb, mode, penalty, go, tuple(k for k in NAMES if k != gone))
        assert gone not in out
        for k, t in out.items():
            np.testing.assert_array_equal(bits(t), bits(full[k]), err_msg=f"{k} without {gone}")


def test_two_runs_give_identical_bits(cuda):
    from spconv_amd.pytorch import functional as F
    ca, cb, go = pair_state(257)
    first, second = run(cuda, ca, cb, rg.IOU_3D, "diou", go), run(cuda, ca, cb, rg.IOU_3D, "diou", go)
    for k in NAMES:
        np.testing.assert_array_equal(bits(first[k]), bits(second[k]))
    target, _, far = boxpairs.pairs(2026, 257)
    grads = []
    for _ in range(2):
        p, t = dev(cuda, far).requires_grad_(), dev(cuda, target).requires_grad_()
        F.boxes_iou3d_diff(p, t, penalty="diou").backward(go)
        grads.append((bits(p.grad), bits(t.grad)))
    np.testing.assert_array_equal(grads[0][0], grads[1][0])
    np.testing.assert_array_equal(grads[0][1], grads[1][1])


# ------------------------------------------------------------------------------------------------ the corners backward

def test_corners_backward_against_float64_numpy(cuda):
    """Bound per box number: 8 * 2^-23 * (the sum of the absolute values of its terms, refboxgrad.chain_terms: a term is
    one corner gradient times its factors).  A term's factors are exact (0.5, a sign), rounded once (lx * c), or the
    device's sine / cosine, 4 ulp at the most (OpenCL's full profile, as in the corners forward): 4 * 2^-23 of the term.
    On top: one rounding for lx * c, one for the sum or difference of the two products, one for the product with the
    corner gradient and one per partial sum of the four corners, each at most 2^-24 of the sum of the absolute terms:
    7 * 2^-24.  Together 7.5 * 2^-23 <= 8 * 2^-23.  x, y, z and dz have no trigonometry and stay far inside.
    Measured: the largest error is 0.13 of the bound (the sine and cosine are far better than 4 ulp)."""
    from spconv_amd.pytorch import functional as F
    n, nfeat = 300, 9
    rng = np.random.default_rng(4)
    boxes = np.zeros((n, nfeat), np.float32)
    boxes[:, :7] = boxpairs.pairs(12, n)[1]
    boxes[:, 7:] = rng.standard_normal((n, 2))
    dead = list(range(4, n, 13))
    kinds = [(0, np.nan), (1, np.inf), (6, -np.inf), (3, 0.0), (4, -1.0), (5, 0.0), (2, np.nan), (5, -2.0)]
    for t, r in enumerate(dead):
        boxes[r, kinds[t % 8][0]] = kinds[t % 8][1]
    gbev = rng.standard_normal((n, 4, 2)).astype(np.float32)
    gz = rng.standard_normal((n, 2)).astype(np.float32)
    live = 280
    worst = 0.0
    for with_z in (True, False):
        out = dirty(cuda, (n, nfeat))
        F.boxes_to_corners_bwd_into(dev(cuda, boxes), count_of(cuda, live), dev(cuda, gbev),
                                    dev(cuda, gz) if with_z else None, out)
        got = out.cpu().numpy()
        gone = sorted(set(dead) | set(range(live, n)))
        assert not fbits(got)[gone].any() and not fbits(got)[:, 7:].any()
        keep = np.array([i for i in range(n) if i not in gone])
        terms = rg.chain_terms(boxes[keep].astype(np.float64), gbev[keep], gz[keep] if with_z else None)
        err = np.abs(got[keep, :7] - terms.sum(-1))
        bound = 8 * 2.0 ** -23 * np.abs(terms).sum(-1)
        assert (err <= bound).all(), (err / np.maximum(bound, 1e-30)).max()
        worst = max(worst, float((err / np.maximum(bound, 1e-30)).max()))
        assert (np.abs(got[keep, :7]).max(0)[[0, 1, 3, 4, 6]] > 0.1).all() and (with_z or not got[:, [2, 5]].any())
    print(f"corners backward: the largest error is {worst:.3f} of the bound")


# ------------------------------------------------------------------------------------------------ end to end

@functools.lru_cache(maxsize=None)
def difference_state():
    """the first 64 pairs of the CPU scenario: the float64 differences and the pairs the kink rule leaves out"""
    import test_refboxgrad as cpu
    target, pred, far = (t[:64] for t in boxpairs.pairs(2026, cpu.N_PAIRS))
    state = {}
    for penalty, a in (("none", pred), ("diou", far)):
        diff = cpu._differences(a, target, PEN[penalty])
        for mode in (rg.IOU_BEV, rg.IOU_3D):
            _, infos = cpu._analytic(a, target, mode, PEN[penalty], np.float64)
            keep = np.array([not cpu._near_kink(a[i].astype(np.float64), target[i].astype(np.float64), mode, PEN[penalty],
                                                infos[i]) for i in range(64)])
            state[(mode, penalty)] = (a, target, diff[mode], keep, 4 * cpu.MEASURED_F32[(mode, PEN[penalty])])
    return state


@pytest.mark.parametrize("mode, penalty", COMBOS, ids=IDS)
def test_end_to_end_gradient_against_the_float64_differences(cuda, mode, penalty):
    """boxes -> corners -> value -> backward(g) with |g| <= 1, against g times the central differences of the independent
    float64 value, under the bound the CPU test asserts for the restatement (four times its measured error: the
    factor is there for the device's sine and cosine in place of the host's)."""
    from spconv_amd.pytorch import functional as F
    a, b, diff, keep, bound = difference_state()[(mode, penalty)]
    assert keep.sum() >= 0.98 * 64
    fn = F.boxes_iou3d_diff if mode == rg.IOU_3D else F.boxes_iou_bev_diff
    g = np.random.default_rng(3).uniform(-1, 1, 64).astype(np.float32)
    want = g[:, None].astype(np.float64) * diff
    p, t = dev(cuda, a).requires_grad_(), dev(cuda, b).requires_grad_()
    fn(p, t, penalty=penalty).backward(dev(cuda, g))
    got = np.concatenate([p.grad.cpu().numpy(), t.grad.cpu().numpy()], 1).astype(np.float64)
    err = np.abs(got - want)[keep].max()
    print(f"mode {mode} penalty {penalty}: worst error {err:.3e}, bound {bound:.3e}")
    assert err <= bound
    # one side alone: the same bits, and nothing for the other
    p1, t1 = dev(cuda, a).requires_grad_(), dev(cuda, b)
    fn(p1, t1, penalty=penalty).backward(dev(cuda, g))
    np.testing.assert_array_equal(bits(p1.grad), bits(p.grad))
    assert t1.grad is None
    p2, t2 = dev(cuda, a), dev(cuda, b).requires_grad_()
    fn(p2, t2, penalty=penalty).backward(dev(cuda, g))
    np.testing.assert_array_equal(bits(t2.grad), bits(t.grad))
    assert not fn(dev(cuda, a), dev(cuda, b), penalty=penalty).requires_grad


@pytest.mark.parametrize("mode, penalty", COMBOS, ids=IDS)
def test_corners_that_require_grad_receive_the_tables_of_the_pair_entry(cuda, mode, penalty):
    from spconv_amd.pytorch import functional as F
    ca, cb, go = pair_state(65)
    fn = F.boxes_iou3d_diff if mode == rg.IOU_3D else F.boxes_iou_bev_diff
    want = pair_reference(65, mode, penalty, True)
    bev_a, z_a = ca.bev.clone().requires_grad_(), ca.zrange.clone().requires_grad_()
    bev_b = cb.bev.clone().requires_grad_()
    v = fn(F.BoxCorners(bev_a, z_a, 65), F.BoxCorners(bev_b, cb.zrange, 65), penalty=penalty)
    np.testing.assert_array_equal(bits(v), fbits(want["value"]))
    v.backward(go)
    np.testing.assert_array_equal(bits(bev_a.grad), fbits(want["gbev_a"]))
    np.testing.assert_array_equal(bits(bev_b.grad), fbits(want["gbev_b"]))
    if mode == rg.IOU_3D:
        np.testing.assert_array_equal(bits(z_a.grad), fbits(want["gz_a"]))
    else:
        assert z_a.grad is None
    assert cb.zrange.grad is None


@pytest.mark.parametrize("reduction, with_weight, avg_factor", [("mean", False, None), ("mean", True, None),
                                                                ("mean", True, 37.5), ("sum", True, None),
                                                                ("none", True, 5.0), ("none", False, None)])
@pytest.mark.parametrize("mode, plane", [("iou", False), ("diou", False), ("diou", True)])
def test_loss_module_against_the_same_arithmetic_in_float64(cuda, mode, plane, reduction, with_weight, avg_factor):
    """The module's reduction against torch float64 over the SAME per-pair values and the same backward kernels.  Value:
    a float32 sum of n terms differs from the float64 one by at most (n + 2) * 2^-24 of the sum of their absolute
    values.  Gradient: the two differ in grad_out alone (rounded products in float32, one rounding of the float64
    coefficient), at most 2^-22 of it; the gradient is linear in grad_out and the sum of the absolute values of its
    terms stays below 16 per unit of it in this scenario (components below 1, boxes of a few metres)."""
    import spconv_amd.pytorch as sp
    from spconv_amd.pytorch import functional as F
    n = 64
    target, _, far = boxpairs.pairs(31, n)
    w = np.random.default_rng(8).uniform(0, 2, n).astype(np.float32) if with_weight else None
    m = sp.RotatedIoU3DLoss(mode, plane=plane, reduction=reduction, loss_weight=1.5)
    p = dev(cuda, far).requires_grad_()
    loss = m(p, dev(cuda, target), dev(cuda, w), avg_factor)
    gout = torch.ones_like(loss) if reduction != "none" else dev(cuda, np.linspace(-1, 1, n).astype(np.float32))
    loss.backward(gout)
    q = dev(cuda, far).requires_grad_()
    fn = F.boxes_iou_bev_diff if plane else F.boxes_iou3d_diff
    each = 1.0 - fn(q, dev(cuda, target), penalty="none" if mode == "iou" else "diou").double()
    if with_weight:
        each = each * dev(cuda, w).double()
    if reduction == "sum":
        want = each.sum()
    elif reduction == "mean":
        want = each.mean() if avg_factor is None else each.sum() / (avg_factor + float(np.finfo(np.float32).eps))
    else:
        want = each
    want = 1.5 * want
    want.backward(gout.double())
    scale = 1.5 * (1.0 if reduction != "mean" else 1.0 / (n if avg_factor is None else avg_factor))
    size = each.detach().abs()
    tol = (n + 2) * 2.0 ** -24 * float(size.sum() if reduction != "none" else size.max()) * scale
    assert loss.shape == want.shape and float((loss.detach().double() - want.detach()).abs().max()) <= tol
    coef = scale * (2.0 if with_weight else 1.0)
    assert float((p.grad.double() - q.grad.double()).abs().max()) <= 2.0 ** -22 * 16 * coef
    assert float(p.grad.abs().max()) > 0


# ------------------------------------------------------------------------------------------------ capture

def test_capture_corners_value_gradient_and_corners_backward_in_one_graph(cuda):
    """corners of both tables -> value and the four gradient tables -> the corners backward of both, through the `_into`
    forms on one stream in one graph, replayed for three inputs and device counts without re-capture: the eager bits."""
    from spconv_amd.pytorch import _box
    from spconv_amd.pytorch import functional as F
    n = 200
    sets = []
    for seed, live in ((1, 200), (2, 130), (3, 77)):
        target, _, far = boxpairs.pairs(seed, n)
        sets.append((far, target, np.random.default_rng(seed).standard_normal(n).astype(np.float32), live))
    s_a, s_b = torch.zeros((n, 7), device=cuda), torch.zeros((n, 7), device=cuda)
    s_go, s_live = torch.zeros((n,), device=cuda), torch.zeros((1,), dtype=torch.int32, device=cuda)
    bev_a, z_a, bev_b, z_b = (torch.empty(s, device=cuda) for s in ((n, 4, 2), (n, 2), (n, 4, 2), (n, 2)))
    out = outputs(cuda, n)
    g_a, g_b = dirty(cuda, (n, 7)), dirty(cuda, (n, 7))
    results = (out["value"], out["gbev_a"], out["gz_a"], out["gbev_b"], out["gz_b"], g_a, g_b)

    def load(k):
        far, target, go, live = sets[k]
        s_a.copy_(dev(cuda, far)), s_b.copy_(dev(cuda, target)), s_go.copy_(dev(cuda, go)), s_live.fill_(live)

    def step():
        _box.corners_into(s_a, s_live, bev_a, z_a)
        _box.corners_into(s_b, None, bev_b, z_b)
        F.boxes_iou_aligned_grad_into(F.BoxCorners(bev_a, z_a, n, s_live), F.BoxCorners(bev_b, z_b, n), rg.IOU_3D,
                                      penalty="diou", grad_out=s_go, **out)
        F.boxes_to_corners_bwd_into(s_a, s_live, out["gbev_a"], out["gz_a"], g_a)
        F.boxes_to_corners_bwd_into(s_b, None, out["gbev_b"], out["gz_b"], g_b)

    wants = []
    for k in range(3):
        load(k)
        step()
        torch.cuda.synchronize()
        wants.append([bits(t).copy() for t in results])
        far, target, go, live = sets[k]
        p, t = dev(cuda, far).requires_grad_(), dev(cuda, target).requires_grad_()
        F.boxes_iou3d_diff(p, t, penalty="diou", n_a=s_live).backward(dev(cuda, go))
        np.testing.assert_array_equal(bits(p.grad), wants[k][5])           # the autograd path is these launches
        np.testing.assert_array_equal(bits(t.grad), wants[k][6])
        assert not wants[k][5][live:].any() and wants[k][5][:live].any(axis=1).all()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    for k in (1, 0, 2):
        load(k)
        for t in results:
            t.view(torch.int32).fill_(-1)
        graph.replay()
        torch.cuda.synchronize()
        for t, want in zip(results, wants[k]):
            np.testing.assert_array_equal(bits(t), want)
