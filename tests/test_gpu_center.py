"""GPU: the centre-head targets of csrc/center.hip against tests/refcenter.py.  Every call goes through its ``_into``
form into junk-filled buffers.  The tables of ``box_centers``, the nearest rows and the sparse inds / mask equal the
numpy float32 loop bit for bit; heat is exactly 0 where no box reaches, exactly 1.0 where the argument is 0 and elsewhere
within 3 ulp of float32(exp(float64(arg))) with the reference's float32 argument -- OpenCL's full-profile bound for
exp, the source of the 4-ulp sine / cosine bound of test_gpu_roi.py; where that value is subnormal (or underflows) the
device value only has to be below 2^-125.  Worst seen on an MI355X: 1 ulp (printed by every heat test)."""
import numpy as np
import pytest
import torch

import centerscenes as cs
import refcenter as rc

pytestmark = pytest.mark.gpu

ULP_BOUND = 3
JUNK_I, JUNK_F = -1234567, float("nan")


def dev(cuda, a):
    return None if a is None else torch.from_numpy(np.array(a, order="C")).to(cuda)


def count_of(cuda, n):
    return None if n is None else torch.tensor([n], dtype=torch.int32, device=cuda)


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32).numpy()


def junk(t):
    return t.fill_(JUNK_F if t.dtype.is_floating_point else JUNK_I)


def check_heat(got, arg, what):
    """got: device heat; arg: the reference's float32 arguments (NaN: no box reaches).  Returns the worst ulp."""
    got = got.detach().cpu().numpy()
    assert got.shape == arg.shape and got.dtype == np.float32
    none, zero = np.isnan(arg), arg == 0
    assert (got.view(np.int32)[none] == 0).all(), what                            # +0, bit for bit
    assert (got[zero] == 1.0).all(), what
    rest = ~none & ~zero
    want, have = rc.heat_of(arg[rest]), got[rest]
    tiny = want < 2.0 ** -126
    assert (have[tiny] >= 0).all() and (have[tiny] < 2.0 ** -125).all(), what
    ulp = np.abs(have[~tiny].view(np.int32).astype(np.int64) - want[~tiny].view(np.int32).astype(np.int64))
    worst = int(ulp.max()) if ulp.size else 0
    print(f"{what}: {int(rest.sum())} values, {int(tiny.sum())} below 2^-126, worst {worst} ulp")
    assert worst <= ULP_BOUND, what
    return worst


@pytest.fixture(scope="module")
def tile():
    from spconv_amd.pytorch import functional as F
    return F.center_tile()


@pytest.fixture(scope="module")
def scenes(tile):
    """per stride: the numpy fixture and its float32 reference, computed once and left unchanged"""
    out = {}
    for stride in cs.STRIDES:
        boxes, bid, cls, n = cs.boxes(stride, tile)
        out[stride] = (boxes, bid, cls, n, rc.records(boxes, bid, cls, cs.B, n, **cs.params(stride)))
    return out


def records_into(cuda, boxes, bid, cls, n, p, B=cs.B):
    """box_centers through its _into form over junk-filled buffers, the scene list included"""
    from spconv_amd.pytorch import _center
    from spconv_amd.pytorch import functional as F
    params = _center.check_params("test", B, p["grid_size"], p["voxel_size"], p["range_min"], p["stride"],
                                  p["num_classes"], p["max_objs"], p["min_overlap"], p["min_radius"])
    M = len(boxes)
    buf = F.center_buffers(M, params, cuda)
    for t in (buf.center, buf.cell, buf.radius, buf.cls, buf.slot, buf.box_index, buf.mask, buf.inds, buf.groups.rows,
              buf.groups.offsets, buf.groups.list):
        junk(t)
    ws = F.center_groups_ws(M, B, cuda).fill_(0xA5)
    return F.box_centers_into(dev(cuda, boxes), dev(cuda, bid), dev(cuda, cls), count_of(cuda, n), buf, ws)


def assert_records(got, want):
    for name in ("center", "cell", "radius", "cls", "slot", "box_index", "mask", "inds"):
        g = getattr(got, name)
        np.testing.assert_array_equal(bits(g), want[name].view(np.int32), err_msg=name)


@pytest.mark.parametrize("stride", cs.STRIDES)
def test_records_bit_for_bit(cuda, scenes, stride):
    boxes, bid, cls, n, want = scenes[stride]
    got = records_into(cuda, boxes, bid, cls, n, cs.params(stride))
    assert_records(got, want)
    assert int((got.cls >= 0).sum()) > 100 and int((got.slot < 0).sum()) > 30


def test_records_of_the_public_call_int32_classes_and_no_ids(cuda, scenes):
    """F.box_centers itself; int32 class ids; batch ids None (all scene 0), classes None (all class 0), no device count"""
    from spconv_amd.pytorch import functional as F
    boxes, bid, cls, n, want = scenes[2]
    p = cs.params(2)
    got = F.box_centers(dev(cuda, boxes), dev(cuda, bid), dev(cuda, cls.astype(np.int32)), cs.B, n_boxes=count_of(cuda, n), **p)
    assert_records(got, want)
    got = F.box_centers(dev(cuda, boxes), None, None, 1, **p)
    assert_records(got, rc.records(boxes, None, None, 1, None, **p))
    empty = F.box_centers(dev(cuda, boxes[:0]), None, None, cs.B, **p)             # no boxes: the tables only
    assert (bits(empty.box_index) == -1).all() and (bits(empty.mask) == 0).all() and (bits(empty.inds) == 0).all()
    heat = F.center_heatmap(empty, junk(torch.empty((cs.B, cs.C, cs.H, cs.W), device=cuda)))
    assert (bits(heat) == 0).all()
    empty = records_into(cuda, boxes[:0], bid[:0], cls[:0], None, p)               # ... and through the _into form
    assert (bits(empty.groups.offsets) == 0).all() and (bits(empty.box_index) == -1).all() and (bits(empty.mask) == 0).all()
    assert (bits(F.center_heatmap(empty)) == 0).all()


@pytest.mark.parametrize("stride", cs.STRIDES)
def test_dense_heat(cuda, scenes, stride):
    from spconv_amd.pytorch import functional as F
    boxes, bid, cls, n, want = scenes[stride]
    got = records_into(cuda, boxes, bid, cls, n, cs.params(stride))
    heat = junk(torch.empty((cs.B, cs.C, cs.H, cs.W), dtype=torch.float32, device=cuda))
    F.center_heatmap_into(got, heat)
    arg = rc.dense_args(want)
    check_heat(heat, arg, f"dense stride {stride}")
    assert (bits(heat[1]) == 0).all()                                              # the scene without a box
    again = junk(torch.empty_like(heat))
    F.center_heatmap_into(got, again)
    np.testing.assert_array_equal(bits(again), bits(heat))                         # run to run


def test_dense_heat_does_not_depend_on_the_order_of_the_boxes(cuda, scenes):
    """two permutations that keep every slot's box set: the scenes sorted apart (the interleaving changes), and the
    boxes that have a slot reversed inside every scene"""
    from spconv_amd.pytorch import functional as F
    boxes, bid, cls, n, want = scenes[1]
    base = F.center_heatmap(records_into(cuda, boxes, bid, cls, n, cs.params(1)))
    apart = np.argsort(bid[:n], kind="stable")
    rev = np.arange(n)
    for b in range(cs.B):
        mine = np.asarray(want["scenes"][b][:cs.MAX_OBJS], dtype=np.int64)
        rev[mine] = mine[::-1]
    for order in (apart, rev):
        full = np.concatenate([order, np.arange(n, len(boxes))])
        heat = F.center_heatmap(records_into(cuda, boxes[full], bid[full], cls[full], n, cs.params(1)))
        np.testing.assert_array_equal(bits(heat), bits(base))


def sparse_into(cuda, centers, idx, n_live, anchor, cutoff):
    """the three sparse calls through their _into forms over junk-filled buffers"""
    from spconv_amd.pytorch import functional as F
    from spconv_amd.pytorch._pointvoxel import PointGroups, point_groups_into
    N, B = len(idx), centers.params.batch_size
    indices, live = dev(cuda, idx), count_of(cuda, n_live)
    i32 = dict(dtype=torch.int32, device=cuda)
    rows, offs, lst = junk(torch.empty(N, **i32)), junk(torch.empty(B + 1, **i32)), junk(torch.empty(N, **i32))
    point_groups_into(indices[:, 0].contiguous(), B, live, rows, offs, lst, F.center_groups_ws(N, B, cuda))
    nearest = junk(torch.empty(len(centers.cls), **i32))
    inds, mask = junk(torch.empty_like(centers.inds)), junk(torch.empty_like(centers.mask))
    heat = junk(torch.empty((N, centers.params.num_classes), dtype=torch.float32, device=cuda))
    F.center_nearest_into(centers, indices, PointGroups(rows, offs, lst, B, live), live, nearest, inds, mask)
    F.center_heatmap_sparse_into(centers, indices, live, nearest, anchor, cutoff, heat)
    return nearest, inds, mask, heat


@pytest.mark.parametrize("without", [None, 2])
@pytest.mark.parametrize("stride", cs.STRIDES)
def test_sparse_heat_and_nearest_rows(cuda, scenes, stride, without):
    boxes, bid, cls, n, want = scenes[stride]
    centers = records_into(cuda, boxes, bid, cls, n, cs.params(stride))
    idx, n_live = cs.rows(without=without)
    ref_nearest, ref_inds, ref_mask = rc.nearest_rows(want, idx, n_live)
    for anchor in ("center", "nearest"):
        for cutoff in ("none", "window"):
            nearest, inds, mask, heat = sparse_into(cuda, centers, idx, n_live, anchor, cutoff)
            np.testing.assert_array_equal(bits(nearest), ref_nearest)
            np.testing.assert_array_equal(bits(inds), ref_inds)
            np.testing.assert_array_equal(bits(mask), ref_mask)
            arg = rc.sparse_args(want, idx, ref_nearest, anchor, cutoff, n_live)
            check_heat(heat, arg, f"sparse {anchor}/{cutoff} stride {stride} without {without}")
    assert int(ref_mask.sum()) < int(want["mask"].sum()) or without is None


def test_sparse_public_call_more_than_eight_classes_and_no_rows(cuda, scenes):
    """F.center_heatmap_sparse itself over indices and over a SparseConvTensor; 11 classes: the sparse kernel keeps eight
    maxima per pass and walks twice; a level without a row"""
    import spconv_amd.pytorch as spconv
    from spconv_amd.pytorch import functional as F
    boxes, bid, cls, n, _ = scenes[2]
    many = np.where((cls >= 0) & (cls < cs.C), cls * 4 + np.arange(len(cls)) % 3, np.where(cls < 0, cls, 11))  # 0 .. 10
    p = cs.params(2, num_classes=11)
    want = rc.records(boxes, bid, many, cs.B, n, **p)
    assert len(set(want["cls"][want["cls"] >= 0])) == 9 and want["cls"].max() == 10
    centers = F.box_centers(dev(cuda, boxes), dev(cuda, bid), dev(cuda, many), cs.B, n_boxes=count_of(cuda, n), **p)
    assert_records(centers, want)
    check_heat(F.center_heatmap(centers), rc.dense_args(want), "dense, 11 classes")
    idx, n_live = cs.rows()
    ref_nearest, ref_inds, ref_mask = rc.nearest_rows(want, idx, n_live)
    got = F.center_heatmap_sparse(centers, dev(cuda, idx), anchor="nearest", cutoff="window", n_live=count_of(cuda, n_live))
    np.testing.assert_array_equal(bits(got.nearest), ref_nearest)
    np.testing.assert_array_equal(bits(got.inds), ref_inds)
    np.testing.assert_array_equal(bits(got.mask), ref_mask)
    check_heat(got.heat, rc.sparse_args(want, idx, ref_nearest, "nearest", "window", n_live), "sparse, 11 classes")
    x = spconv.SparseConvTensor(torch.zeros((len(idx), 4), device=cuda), dev(cuda, idx), [cs.H, cs.W], cs.B)
    x.n_live_dev = count_of(cuda, n_live)
    via = F.center_heatmap_sparse(centers, x)                                      # VoxelNeXt's: centre anchor, no cutoff
    check_heat(via.heat, rc.sparse_args(want, idx, ref_nearest, "center", "none", n_live), "sparse tensor, 11 classes")
    np.testing.assert_array_equal(bits(via.nearest), ref_nearest)
    with pytest.raises(ValueError, match="2-D"):
        F.center_heatmap_sparse(centers, spconv.SparseConvTensor(torch.zeros((4, 4), device=cuda),
                                                                 torch.zeros((4, 4), dtype=torch.int32, device=cuda),
                                                                 [4, cs.H, cs.W], cs.B))
    none = F.center_heatmap_sparse(centers, dev(cuda, idx[:0]))
    assert tuple(none.heat.shape) == (0, 11) and (bits(none.nearest) == -1).all() and (bits(none.mask) == 0).all()


def test_replay_from_a_captured_graph_with_other_boxes_and_counts(cuda, scenes, tile):
    """groups -> records -> row groups -> nearest -> dense and sparse heat on one stream in one graph, replayed with a
    second box set, other rows and smaller device counts copied into the static buffers"""
    from spconv_amd.pytorch import _center
    from spconv_amd.pytorch import functional as F
    from spconv_amd.pytorch._pointvoxel import PointGroups, point_groups_into
    stride = 2
    p = cs.params(stride)
    rows_a, live_a = cs.rows()
    rows_b, live_b = cs.rows(seed=3)
    N = min(len(rows_a), len(rows_b))
    sets = [scenes[stride][:4] + (rows_a[:N], min(live_a, N)), cs.second_boxes(stride, tile) + (rows_b[:N], min(live_b, N) - 55)]
    M = len(sets[0][0])
    assert len(sets[1][0]) == M and sets[1][3] < sets[0][3]
    params = _center.check_params("test", cs.B, p["grid_size"], p["voxel_size"], p["range_min"], p["stride"],
                                  p["num_classes"], p["max_objs"], p["min_overlap"], p["min_radius"])
    i32 = dict(dtype=torch.int32, device=cuda)
    boxes = torch.empty((M, sets[0][0].shape[1]), dtype=torch.float32, device=cuda)
    bid, cls = torch.empty(M, **i32), torch.empty(M, dtype=torch.int64, device=cuda)
    indices, row_ids = torch.empty((N, 3), **i32), torch.empty(N, **i32)
    n_boxes, n_live = torch.empty(1, **i32), torch.empty(1, **i32)
    buf = F.center_buffers(M, params, cuda)
    ws, ws_rows = F.center_groups_ws(M, cs.B, cuda), F.center_groups_ws(N, cs.B, cuda)
    rows, offs, lst = torch.empty(N, **i32), torch.empty(cs.B + 1, **i32), torch.empty(N, **i32)
    nearest, inds, mask = torch.empty(M, **i32), torch.empty_like(buf.inds), torch.empty_like(buf.mask)
    dense = torch.empty((cs.B, cs.C, cs.H, cs.W), dtype=torch.float32, device=cuda)
    heat_c, heat_n = (torch.empty((N, cs.C), dtype=torch.float32, device=cuda) for _ in range(2))
    outs = [buf.center, buf.cell, buf.radius, buf.cls, buf.slot, buf.box_index, buf.mask, buf.inds, nearest, inds, mask,
            dense, heat_c, heat_n]

    def step():
        centers = F.box_centers_into(boxes, bid, cls, n_boxes, buf, ws)
        row_ids.copy_(indices[:, 0])
        point_groups_into(row_ids, cs.B, n_live, rows, offs, lst, ws_rows)
        F.center_heatmap_into(centers, dense)
        F.center_nearest_into(centers, indices, PointGroups(rows, offs, lst, cs.B, n_live), n_live, nearest, inds, mask)
        F.center_heatmap_sparse_into(centers, indices, n_live, None, "center", "none", heat_c)
        F.center_heatmap_sparse_into(centers, indices, n_live, nearest, "nearest", "window", heat_n)

    def load(k):
        b, i, c, n, r, live = sets[k]
        boxes.copy_(dev(cuda, b)), bid.copy_(dev(cuda, i)), cls.copy_(dev(cuda, c)), indices.copy_(dev(cuda, r))
        n_boxes.fill_(n), n_live.fill_(live)
    eager = []
    for k in (0, 1):
        load(k)
        for t in outs:
            junk(t)
        step()
        eager.append([t.clone() for t in outs])
        b, i, c, n, r, live = sets[k]
        want = rc.records(b, i, c, cs.B, n, **p)
        np.testing.assert_array_equal(bits(buf.inds), want["inds"])
        np.testing.assert_array_equal(bits(nearest), rc.nearest_rows(want, r, live)[0])
    assert not torch.equal(eager[0][5], eager[1][5]) and not torch.equal(eager[0][11], eager[1][11])
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    for k in (1, 0, 1):
        load(k)
        for t in outs:
            junk(t)
        graph.replay()
        torch.cuda.synchronize()
        for got, want in zip(outs, eager[k]):
            np.testing.assert_array_equal(bits(got), bits(want))


def target_rows(boxes, want, cell):
    """the numpy gather of the regression rows over box_index"""
    B, K = want["box_index"].shape
    out = np.zeros((B, K, boxes.shape[1] + 1), np.float32)
    for b in range(B):
        for k in range(K):
            i = want["box_index"][b, k]
            if i >= 0 and want["mask_used"][b, k]:
                v = boxes[i]
                out[b, k] = np.concatenate([want["center"][i] - cell[i].astype(np.float32), v[2:3], np.log(v[3:6]),
                                            np.cos(v[6:7]), np.sin(v[6:7]), v[7:]])
    return out


@pytest.mark.parametrize("sparse", [False, "tensor", "indices"])
def test_module_targets(cuda, scenes, sparse):
    """target_boxes equal a numpy gather over box_index: the offsets, z and the extra columns bit for bit, log / cos /
    sin within torch's own (1e-6 relative, 1e-6 absolute: a few ulp of values up to 2).  The sparse level is given as a
    SparseConvTensor (with its device row count) and as a plain int32 [N, 3] index tensor (every row live); the
    module's parameters arrive as the numpy arrays of a data config"""
    import spconv_amd.pytorch as spconv
    stride = 2
    boxes, bid, cls, n, want = scenes[stride]
    p = cs.params(stride)
    head = spconv.CenterHeadTargets(cs.C, np.array(p["grid_size"] + (1,)), np.array(p["voxel_size"] + (0.2,)),
                                    np.array(p["range_min"] + (-3.0, 1.0, 1.0, 1.0)), stride, max_objs=cs.MAX_OBJS,
                                    anchor="nearest", cutoff="window")
    assert (head.grid_size, head.voxel_size, head.range_min) == (p["grid_size"], p["voxel_size"], p["range_min"])
    idx, n_live = cs.rows()
    want = dict(want)
    if sparse:
        if sparse == "indices":
            idx, n_live = np.ascontiguousarray(idx[:n_live]), None
            x = dev(cuda, idx)
        else:
            x = spconv.SparseConvTensor(torch.zeros((len(idx), 4), device=cuda), dev(cuda, idx), [cs.H, cs.W], cs.B)
            x.n_live_dev = count_of(cuda, n_live)
        out = head(dev(cuda, boxes), dev(cuda, bid), dev(cuda, cls), cs.B, x=x, n_boxes=count_of(cuda, n))
        nearest, inds, mask = rc.nearest_rows(want, idx, n_live)
        check_heat(out.heatmap, rc.sparse_args(want, idx, nearest, "nearest", "window", n_live), "module, sparse")
        cell = idx[np.clip(nearest, 0, None)][:, [2, 1]]
    else:
        out = head(dev(cuda, boxes), dev(cuda, bid), dev(cuda, cls), cs.B, n_boxes=count_of(cuda, n))
        inds, mask, cell = want["inds"], want["mask"], want["cell"]
        check_heat(out.heatmap, rc.dense_args(want), "module, dense")
    np.testing.assert_array_equal(bits(out.inds), inds)
    np.testing.assert_array_equal(bits(out.mask), mask)
    want["mask_used"] = mask
    ref = target_rows(boxes, want, cell)
    got = out.target_boxes.cpu().numpy()
    assert got.shape == (cs.B, cs.MAX_OBJS, 8 + boxes.shape[1] - 7) and int(mask.sum()) > 100
    for cols in ([0, 1, 2], list(range(8, got.shape[2]))):
        np.testing.assert_array_equal(got[:, :, cols].view(np.int32), ref[:, :, cols].view(np.int32))
    np.testing.assert_allclose(got[:, :, 3:8], ref[:, :, 3:8], rtol=1e-6, atol=1e-6)
    assert (got[mask == 0] == 0).all() and np.isfinite(got).all()
