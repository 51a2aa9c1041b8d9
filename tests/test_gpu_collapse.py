"""Axis collapse on the kernels of csrc/collapse.hip (spconv_amd/pytorch/_collapse.py, functional.sparse_collapse,
spatial.SparseCollapse) against the numpy reference of tests/refcollapse.py.

The builder's four tables, sum, max and their gradients are compared bit for bit: the reference walks a group's rows in
the contract's order (ascending input row) with the same IEEE float32 (float64) additions.  mean carries the bound of
the global pools: half an ulp of the output + (len + 2) 2^-24 of the mean of magnitudes, len the group's own length (a
sequential fp32 sum of len terms errs by at most about len 2^-24 of the magnitude sum, the division adds one fp32
rounding, the output half an ulp).  Its gradient: half an ulp of the dtype + 2^-23 |ref| (one fp32 division before the
rounding)."""
import numpy as np
import pytest
import torch

import refcollapse as rc
from util import HALF_ULP, assert_close_abs_sum

pytestmark = pytest.mark.gpu

KEYS = ("collapse/mark", "collapse/prefix", "collapse/rank", "collapse/list", "collapse/fwd", "collapse/bwd")
OPS = ("sum", "mean", "max")
# half the spacing of the dtype's smallest numbers: what "half an ulp" is for a result in the subnormal range
HALF_MIN_STEP = {"float16": 2.0 ** -25, "bfloat16": 2.0 ** -134, "float32": 2.0 ** -150, "float64": 0.0}


def counts():
    from spconv_amd import _lib
    return _lib.launch_counts(KEYS)


def bits(t):
    t = t.detach().cpu().contiguous()
    return t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def native_build(cuda, idx, bs, shape, axes, n_live=None, cap=None):
    from spconv_amd.pytorch import _collapse
    dev = torch.from_numpy(np.ascontiguousarray(idx)).to(cuda)
    nl = None if n_live is None else torch.tensor([n_live], dtype=torch.int32, device=cuda)
    return _collapse.sparse_collapse_build(dev, bs, shape, axes, n_live=nl, static_num_out=cap)


def check_build(c, ref, n):
    """the four tables of an eager build against the reference, bit for bit"""
    assert c.n_out == ref.live == ref.found and c.live_rows == ref.live_rows and c.spatial_shape == ref.kept_shape
    np.testing.assert_array_equal(c.out_indices.cpu().numpy(), ref.out_indices)
    np.testing.assert_array_equal(c.rows.cpu().numpy(), ref.rows)
    np.testing.assert_array_equal(c.offsets.cpu().numpy(), ref.offsets)
    assert tuple(c.list.shape) == (n,)
    np.testing.assert_array_equal(c.list.cpu().numpy()[:ref.offsets[-1]], ref.list)


BUILDS = {
    # name: (batch, shape, axes, rows, duplicated rows)
    "1d": (3, [97], (), 150, 20),
    "2d_first": (2, [33, 70], (0,), 300, 10),
    "2d_last": (2, [33, 70], (1,), 300, 10),
    "3d_z": (2, [5, 14, 16], (0,), 600, 30),
    "3d_middle": (2, [5, 14, 16], (1,), 600, 30),           # a middle axis: the key arithmetic skips a factor
    "3d_two": (2, [5, 14, 16], (0, 2), 600, 30),
    "3d_none": (2, [5, 14, 16], (), 600, 200),              # axes = (): duplicates of a full coordinate merge
    "4d": (1, [5, 6, 7, 9], (0, 3), 500, 30),
    "4d_one": (2, [3, 6, 7, 9], (2,), 500, 30),
    "empty": (2, [5, 14, 16], (0,), 0, 0),
    "blocks": (2, [4, 300, 300], (0,), 3000, 100),          # 180 000 projected cells: the prefix pass spans blocks
    "rows_20k": (2, [8, 100, 100], (0,), 20000, 500),       # 41 sort blocks, two radix passes
    "long_groups": (1, [64, 3, 3], (0,), 900, 100),         # 9 cells: ~110 rows per group
}


@pytest.mark.parametrize("name", sorted(BUILDS))
def test_builder(cuda, name):
    from spconv_amd.pytorch import ops
    bs, shape, axes, n, dups = BUILDS[name]
    idx = rc.scene(bs, shape, n, 21, dups, dead=n > 0)
    ref = rc.build(idx, bs, shape, axes)
    if name == "long_groups":
        assert int(np.diff(ref.offsets).max()) > 64
    if name == "blocks":
        assert bs * int(np.prod(ref.kept_shape)) > 65536 and ref.out_indices[-1, 0] == 1
    c0 = counts()
    c = native_build(cuda, idx, bs, shape, axes)
    c1 = counts()
    check_build(c, ref, idx.shape[0])
    rows_passes = 1 if idx.shape[0] else 0
    assert [c1[k] - c0[k] for k in KEYS] == [rows_passes, 1, rows_passes, 1, 0, 0]
    if ref.live:
        assert ops._rankmap_of(c.out_indices, bs, ref.kept_shape, ref.live, 3 ** len(ref.kept_shape)) is not None
    again = native_build(cuda, idx, bs, shape, axes)                       # the same tables on every call
    for a, b in ((c.rows, again.rows), (c.offsets, again.offsets), (c.out_indices, again.out_indices)):
        assert torch.equal(a, b)
    assert torch.equal(c.list[:ref.offsets[-1]], again.list[:ref.offsets[-1]])


def test_every_row_dead(cuda):
    bs, shape = 2, [5, 14, 16]
    idx = np.array([[-1, 0, 0, 0], [2, 1, 1, 1], [0, 5, 0, 0], [0, 0, -1, 0], [1, 0, 0, 16]] * 40, np.int32)
    ref = rc.build(idx, bs, shape, (0,))
    assert ref.live == 0
    c = native_build(cuda, idx, bs, shape, (0,))
    check_build(c, ref, idx.shape[0])
    assert tuple(c.out_indices.shape) == (0, 3)
    st = native_build(cuda, idx, bs, shape, (0,), cap=8)
    assert st.n_out_dev.cpu().tolist() == [0, 0, 0] and bool((st.out_indices == -1).all())
    assert bool((st.rows == -1).all()) and not bool(st.offsets.any())


def test_key_space_that_does_not_fit_raises(cuda):
    idx = torch.zeros((4, 4), dtype=torch.int32, device=cuda)
    from spconv_amd.pytorch import _collapse
    with pytest.raises(NotImplementedError, match="does not fit"):
        _collapse.sparse_collapse_build(idx, 1, [2, 65536, 32768], (0,))
    c = _collapse.sparse_collapse_build(idx, 1, [2048, 1024, 1024], (0,))  # fits once the long axis is gone
    assert c.n_out == 1 and c.offsets.cpu().tolist() == [0, 4]


# ---------------------------------------------------------------------------------------- static form
def check_static(c, ref, n, cap):
    """a static build against the reference built with the same cap"""
    live = ref.live
    assert c.n_out == cap and c.n_out_dev.cpu().tolist() == [ref.found, 0, live]
    np.testing.assert_array_equal(c.out_indices[:live].cpu().numpy(), ref.out_indices)
    assert bool((c.out_indices[live:] == -1).all())
    np.testing.assert_array_equal(c.rows.cpu().numpy(), ref.rows)
    off = c.offsets.cpu().numpy()
    assert off.shape == (cap + 1,)
    np.testing.assert_array_equal(off[:live + 1], ref.offsets)
    assert bool((off[live:] == ref.offsets[-1]).all())                      # flat behind the live count
    np.testing.assert_array_equal(c.list.cpu().numpy()[:ref.offsets[-1]], ref.list)


@pytest.mark.parametrize("case", ["n_live", "cap_above", "cap_below", "cap_above_rows"])
def test_static_form(cuda, case):
    from spconv_amd.pytorch import _collapse
    bs, shape, axes = 2, [5, 14, 16], (0,)
    idx = rc.scene(bs, shape, 500, 31, 30)
    n = idx.shape[0]
    found = rc.build(idx, bs, shape, axes).found
    n_live = 300 if case == "n_live" else None
    cap = {"n_live": None, "cap_above": found + 37, "cap_below": found - 50, "cap_above_rows": n + 100}[case]
    ref = rc.build(idx, bs, shape, axes, n_live, cap)
    if case == "cap_below":
        assert (ref.found, ref.live) == (found, cap) and int((ref.rows < 0).sum()) > n - ref.live_rows
    c = native_build(cuda, idx, bs, shape, axes, n_live, cap)
    room = cap if cap is not None else n                                    # None: room for the input's rows
    check_static(c, ref, n, room)
    # the reduction behind it: rows past the live count are zeros, the live ones the reference's
    feat = rc.features(n, 8, torch.float16, 32)
    for op in OPS:
        out = _collapse.fwd(feat.to(cuda), c, op, c.n_out_dev[2:3])
        assert tuple(out.shape) == (room, 8) and not bool(out[ref.live:].any())
        if op != "mean":
            assert torch.equal(bits(out[:ref.live]), bits(rc.reduce(feat, ref, op))), op


# ---------------------------------------------------------------------------------------- forward
_CACHE = {}


def fwd_case():
    """the forward / backward scene, its reference and its native build: made once"""
    if "ref" not in _CACHE:
        s = rc.FWD_SCENE
        idx = rc.fwd_scene()
        _CACHE["idx"], _CACHE["ref"] = idx, rc.build(idx, s["bs"], s["shape"], s["axes"])
    return _CACHE["idx"], _CACHE["ref"]


def fwd_build(cuda):
    if "build" not in _CACHE:
        s = rc.FWD_SCENE
        _CACHE["build"] = native_build(cuda, _CACHE["idx"], s["bs"], s["shape"], s["axes"])
    return _CACHE["build"]


FWD = [(dt, C) for dt in (torch.float16, torch.bfloat16, torch.float32) for C in (1, 8, 20, 64, 136, 264)] + \
      [(torch.float64, 1), (torch.float64, 8)]


@pytest.mark.parametrize("dtype,C", FWD, ids=lambda v: str(v).replace("torch.", ""))
def test_forward(cuda, dtype, C):
    from spconv_amd.pytorch import _collapse
    idx, ref = fwd_case()
    c = fwd_build(cuda)
    feat = rc.features(idx.shape[0], C, dtype, 100 + C)
    one = int(np.nonzero(np.diff(ref.offsets) == 1)[0][0])                 # a one-row group holding -0.0
    feat[int(ref.list[ref.offsets[one]])] = -0.0
    dev = feat.to(cuda)
    c0 = counts()
    got = {op: _collapse.fwd(dev, c, op) for op in OPS}
    assert counts()["collapse/fwd"] == c0["collapse/fwd"] + 3
    for op in ("sum", "max"):
        assert got[op].dtype == dtype and torch.equal(bits(got[op]), bits(rc.reduce(feat, ref, op))), op
    assert bool(torch.signbit(got["sum"][one].cpu()).all())                 # copied, not added to a zero
    mean, A, lens = rc.mean_f64(feat, ref)
    assert_close_abs_sum(got["mean"].double().cpu().numpy(), mean, A * (lens[:, None] + 2), dtype, 2.0 ** -24,
                         name=f"mean {dtype} C={C}")
    for op in OPS:                                                          # identical run to run
        assert torch.equal(bits(_collapse.fwd(dev, c, op)), bits(got[op])), op


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
def test_forward_long_groups(cuda, dtype):
    """groups of more than 64 rows: many rounds of the walk, the additions still in list order"""
    from spconv_amd.pytorch import _collapse
    bs, shape, axes, n, dups = BUILDS["long_groups"]
    idx = rc.scene(bs, shape, n, 21, dups)
    ref = rc.build(idx, bs, shape, axes)
    feat = rc.features(idx.shape[0], 8, dtype, 41)
    c = native_build(cuda, idx, bs, shape, axes)
    for op in ("sum", "max"):
        assert torch.equal(bits(_collapse.fwd(feat.to(cuda), c, op)), bits(rc.reduce(feat, ref, op))), op
    mean, A, lens = rc.mean_f64(feat, ref)
    assert_close_abs_sum(_collapse.fwd(feat.to(cuda), c, "mean").double().cpu().numpy(), mean, A * (lens[:, None] + 2),
                         dtype, 2.0 ** -24, name="mean")


def group_lengths_scene():
    """columns of 1 to 9 rows on a 10 x 4 x 4 grid collapsed along its first axis, the rows in a shuffled order; with
    room for 12 output rows the static form adds three groups of length 0"""
    shape, cap = [10, 4, 4], 12
    rows = [(0, z, k // 4, k % 4) for k in range(9) for z in range(k + 1)]
    idx = np.array(rows, np.int32)[np.random.default_rng(5).permutation(len(rows))]
    ref = rc.build(idx, 1, shape, (0,), None, cap)
    assert sorted(np.diff(ref.offsets).tolist()) == list(range(1, 10)) and ref.live == 9
    return idx, shape, cap, ref


@pytest.mark.parametrize("C", [3, 8])
@pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=lambda v: str(v).replace("torch.", ""))
def test_forward_every_group_length_0_to_9(cuda, dtype, C):
    """the walk fetches four list entries at a time: every group length from 0 to 9 crosses each of its boundaries
    (an empty group, a partial first round, exactly one and two rounds, a partial last round)"""
    from spconv_amd.pytorch import _collapse
    idx, shape, cap, ref = group_lengths_scene()
    c = native_build(cuda, idx, 1, shape, (0,), cap=cap)
    check_static(c, ref, idx.shape[0], cap)
    feat = rc.features(idx.shape[0], C, dtype, 70 + C)
    dev = feat.to(cuda)
    mean, A, lens = rc.mean_f64(feat, ref)
    # with the live count the tail rows are skipped; without it they are walked as groups of length 0 (flat offsets)
    for n_live in (c.n_out_dev[2:3], None):
        for op in OPS:
            out = _collapse.fwd(dev, c, op, n_live)
            assert tuple(out.shape) == (cap, C) and not bool(out[ref.live:].any()), op
            if op != "mean":
                assert torch.equal(bits(out[:ref.live]), bits(rc.reduce(feat, ref, op))), op
            else:
                assert_close_abs_sum(out[:ref.live].double().cpu().numpy(), mean, A * (lens[:, None] + 2), dtype,
                                     2.0 ** -24, name=f"mean {dtype} C={C}")


# ---------------------------------------------------------------------------------------- backward
def mean_bwd_bound(ref_din, dtype):
    name = str(dtype).replace("torch.", "")
    return (HALF_ULP[name] * (1 + 1e-6) + 2.0 ** -23) * np.abs(ref_din) + HALF_MIN_STEP[name]


@pytest.mark.parametrize("C", [8, 20])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, torch.float32], ids=lambda v: str(v).replace("torch.", ""))
def test_backward(cuda, dtype, C):
    from spconv_amd.pytorch import functional as Fsp
    idx, ref = fwd_case()
    c = fwd_build(cuda)
    feat = rc.features(idx.shape[0], C, dtype, 200 + C)
    dout = rc.features(ref.live, C, dtype, 300 + C)
    dead = torch.from_numpy(ref.rows < 0)
    assert int(dead.sum()) > 0
    for op in OPS:
        x = feat.to(cuda).requires_grad_(True)
        c0 = counts()
        out = Fsp.SparseCollapseFunction.apply(x, c, op, None)
        out.backward(dout.to(cuda))
        c1 = counts()
        assert c1["collapse/bwd"] - c0["collapse/bwd"] == (0 if op == "sum" else 1)      # sum: the union's gather
        grad = x.grad.cpu()
        assert grad.dtype == dtype and not bool(grad[dead].any()), op
        want = rc.backward(feat, rc.reduce(feat, ref, op), dout, ref, op)
        if op == "mean":
            err = np.abs(grad.double().numpy() - want)
            assert bool((err <= mean_bwd_bound(want, dtype)).all()), float((err - mean_bwd_bound(want, dtype)).max())
        else:
            assert torch.equal(bits(grad), bits(torch.from_numpy(want).to(dtype))), op


def test_backward_max_ties_all_receive_and_dropped_rows_get_zeros(cuda):
    from spconv_amd.pytorch import _collapse
    from spconv_amd.pytorch import functional as Fsp
    bs, shape, axes = 1, [6, 4, 5], (0,)
    idx = rc.scene(bs, shape, 100, 51, 10)
    n = idx.shape[0]
    full = rc.build(idx, bs, shape, axes)
    cap = full.found - 4                                                    # the last four cells are dropped
    ref = rc.build(idx, bs, shape, axes, cap=cap)
    g = torch.Generator().manual_seed(52)
    feat = torch.randint(0, 3, (n, 6), generator=g).to(torch.float32)       # three values: ties in nearly every group
    c = native_build(cuda, idx, bs, shape, axes, cap=cap)
    dout = rc.features(cap, 6, torch.float32, 53)
    for op in OPS:
        x = feat.to(cuda).requires_grad_(True)
        out = Fsp.SparseCollapseFunction.apply(x, c, op, c.n_out_dev[2:3])
        out.backward(dout.to(cuda))
        want = rc.backward(feat, rc.reduce(feat, ref, op), dout, ref, op)
        grad = x.grad.cpu()
        dropped = torch.from_numpy((full.rows >= 0) & (ref.rows < 0))
        assert int(dropped.sum()) > 0 and not bool(grad[dropped].any()) and not bool(grad[torch.from_numpy(full.rows < 0)].any())
        if op == "mean":
            assert bool((np.abs(grad.double().numpy() - want) <= mean_bwd_bound(want, torch.float32)).all())
        else:
            assert torch.equal(bits(grad), bits(torch.from_numpy(want).float())), op
        if op == "max":
            outs = rc.reduce(feat, ref, "max")
            held = np.nonzero(ref.rows >= 0)[0]
            hit = (feat[held] == outs[ref.rows[held]])
            per_group = np.zeros((cap, 6))
            np.add.at(per_group, ref.rows[held], hit.numpy())
            assert int(per_group.max()) >= 2                                # several rows of a group share its maximum
            assert torch.equal(grad[held][hit], dout[ref.rows[held]][hit])  # and every one of them receives


@pytest.mark.parametrize("op", OPS)
def test_gradcheck_f64(cuda, op):
    from spconv_amd.pytorch import functional as Fsp
    bs, shape, axes = 1, [4, 3, 3], (0,)
    idx = rc.scene(bs, shape, 24, 61, 0)
    assert idx.shape[0] == 32                                               # 24 + the 8 rows no scene owns: ~30 rows
    c = native_build(cuda, idx, bs, shape, axes)
    g = torch.Generator().manual_seed(62)
    feat = (torch.randperm(idx.shape[0] * 3, generator=g).double().reshape(-1, 3) * 0.01).to(cuda).requires_grad_(True)
    fn = lambda x: Fsp.SparseCollapseFunction.apply(x, c, op, None)         # (distinct values: max is differentiable)
    assert torch.autograd.gradcheck(fn, (feat,), eps=1e-6, atol=1e-9, rtol=1e-7)


# ---------------------------------------------------------------------------------------- module
def test_module_and_subm2d_over_the_rank_map(cuda):
    import spconv_amd.pytorch as spconv
    from spconv_amd.pytorch import ops
    bs, shape, C = 2, [6, 20, 24], 16
    idx = rc.scene(bs, shape, 800, 71, 20)
    ref = rc.build(idx, bs, shape, (0,))
    feat = rc.features(idx.shape[0], C, torch.float16, 72)
    x = spconv.SparseConvTensor(feat.to(cuda), torch.from_numpy(idx).to(cuda), shape, bs, benchmark=True)
    x.indice_dict["k"] = object()
    mod = spconv.SparseCollapse((0,), name="bev")
    out = mod(x)
    assert isinstance(out, spconv.SparseConvTensor) and out is not x
    assert out.spatial_shape == [20, 24] and out.batch_size == bs and out.indice_dict == {} and out.benchmark
    assert out.n_live_dev is None and mod._static_n_out_dev is None and out.grid.numel() == 0
    np.testing.assert_array_equal(out.indices.cpu().numpy(), ref.out_indices)
    assert torch.equal(bits(out.features), bits(rc.reduce(feat, ref, "sum")))
    assert ops._rankmap_of(out.indices, bs, [20, 24], ref.live, 9) is not None
    out.benchmark = False                                                   # (carried over, checked above; a benchmarked layer needs a name)
    torch.manual_seed(0)
    conv = spconv.SubMConv2d(C, C, 3, bias=False).to(cuda).half().eval()
    plain = spconv.SparseConvTensor(out.features, out.indices.clone(), [20, 24], bs)
    assert ops._rankmap_of(plain.indices, bs, [20, 24], ref.live, 9) is None        # the hash build
    with torch.no_grad():
        got, want = conv(out), conv(plain)
    assert torch.equal(bits(got.features), bits(want.features))
    for op in ("mean", "max"):
        o = spconv.SparseCollapse((0,), reduce=op)(x)
        if op == "max":
            assert torch.equal(bits(o.features), bits(rc.reduce(feat, ref, op)))
    with pytest.raises(NotImplementedError, match="float16"):
        spconv.SparseCollapse((0,))(spconv.SparseConvTensor(torch.zeros((idx.shape[0], 4), dtype=torch.int8, device=cuda),
                                                            x.indices, shape, bs))


def test_install_as_spconv_exposes_the_module(cuda):
    import spconv_amd
    spconv_amd.install_as_spconv()
    import spconv.pytorch as sp
    from spconv.pytorch.spatial import SparseCollapse
    assert sp.SparseCollapse is SparseCollapse


def test_module_is_captured_in_one_graph(cuda):
    import spconv_amd.pytorch as spconv
    bs, shape, C, cap = 2, [6, 14, 16], 16, 512
    scenes = []
    for s in range(2):
        idx = rc.scene(bs, shape, 300 + 120 * s, 80 + s, 10, dead=False)
        scenes.append((idx, rc.features(idx.shape[0], C, torch.float16, 82 + s) * 0.25))
    idx_buf = torch.full((cap, 4), -1, dtype=torch.int32, device=cuda)
    feat_buf = torch.zeros((cap, C), dtype=torch.float16, device=cuda)
    live = torch.zeros((1,), dtype=torch.int32, device=cuda)
    torch.manual_seed(1)
    collapse = spconv.SparseCollapse((0,))
    conv = spconv.SubMConv2d(C, C, 3, bias=False).to(cuda).half().eval()

    def load(idx, feat):
        n = idx.shape[0]
        idx_buf.fill_(-1)
        feat_buf.zero_()
        idx_buf[:n].copy_(torch.from_numpy(idx))
        feat_buf[:n].copy_(feat)
        live.fill_(n)

    def forward():
        x = spconv.SparseConvTensor(feat_buf, idx_buf, shape, bs)
        x.n_live_dev = live
        mid = collapse(x)
        return mid, conv(mid)

    eager = []
    with torch.no_grad():
        for idx, feat in scenes:
            m = collapse(spconv.SparseConvTensor(feat.to(cuda), torch.from_numpy(idx).to(cuda), shape, bs))
            eager.append((m.indices.clone(), m.features.clone(), conv(m).features.clone()))
    load(*scenes[0])
    side = torch.cuda.Stream(device=cuda)
    side.wait_stream(torch.cuda.current_stream(cuda))
    with torch.cuda.stream(side), torch.no_grad():
        forward()
    torch.cuda.current_stream(cuda).wait_stream(side)
    torch.cuda.synchronize(cuda)
    graph = torch.cuda.CUDAGraph()
    with torch.no_grad(), torch.cuda.graph(graph):              # one stream, no forked branches
        mid, out = forward()
    for s in (1, 0, 1):
        load(*scenes[s])
        graph.replay()
        e_idx, e_mid, e_out = eager[s]
        n = int(mid.n_live_dev.item())
        assert n == e_idx.shape[0] and collapse._static_n_out_dev.cpu().tolist() == [n, 0, n]
        assert torch.equal(mid.indices[:n], e_idx) and bool((mid.indices[n:] == -1).all())
        assert torch.equal(bits(mid.features[:n]), bits(e_mid)) and not bool(mid.features[n:].any())
        assert torch.equal(bits(out.features[:n]), bits(e_out))


class Bev(torch.nn.Module):
    """a 3-D SubM layer, the collapse, a 2-D SubM layer"""

    def __init__(self, C, static_num_out=None):
        super().__init__()
        import spconv_amd.pytorch as spconv
        self.conv0 = spconv.SubMConv3d(C, C, 3, bias=False, indice_key="s0")
        self.bev = spconv.SparseCollapse((0,), static_num_out=static_num_out)
        self.head = spconv.SubMConv2d(C, C, 3, bias=False, indice_key="h0")

    def forward(self, x):
        return self.head(self.bev(self.conv0(x)))


def test_bounded_module_under_static_inference(cuda):
    import spconv_amd.pytorch as spconv
    from spconv_amd.pytorch.static import StaticInference
    bs, shape, C = 2, [6, 14, 16], 16
    idx = np.unique(rc.scene(bs, shape, 400, 91, dead=False), axis=0)       # distinct, in key order: the entry sort moves nothing
    ref = rc.build(idx, bs, shape, (0,))
    feat = (rc.features(idx.shape[0], C, torch.float16, 92) * 0.25).to(cuda)
    dev_idx = torch.from_numpy(idx).to(cuda)
    torch.manual_seed(2)
    net = Bev(C).to(cuda).half().eval()
    with torch.no_grad():
        eager = net(spconv.SparseConvTensor(feat, dev_idx, shape, bs))
    np.testing.assert_array_equal(eager.indices.cpu().numpy(), ref.out_indices)
    for bound, over in ((ref.found + 20, {}), (ref.found - 7, {"bev": ref.found})):
        net.bev.static_num_out = bound
        runner = StaticInference(net, max_voxels=idx.shape[0] + 50, in_channels=C, spatial_shape=shape, batch_size=bs,
                                 dtype=torch.float16)
        try:
            out = runner(feat, dev_idx)
            live = min(ref.found, bound)
            assert int(out.n_live_dev.item()) == live and out.spatial_shape == [14, 16]
            assert runner.counts()["bev"][0] == ref.found and runner.bounds["bev"] == bound
            assert runner.overflowed() == over
            np.testing.assert_array_equal(out.indices[:live].cpu().numpy(), ref.out_indices[:live])
            if not over:
                assert torch.equal(bits(out.features[:live]), bits(eager.features))
        finally:
            runner.release_bounds()
