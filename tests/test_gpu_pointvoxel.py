"""Point <-> voxel features on the kernels of csrc/pointvoxel.hip and csrc/collapse.hip (spconv_amd/pytorch/_pointvoxel.py,
vfe.DynamicVFE, StaticPointToVoxel.point_groups, StaticInference(point_encoder=...)) against numpy references written
from the contracts of include/spconv_amd.h.

Bit for bit: the groups (a stable argsort of the keys + searchsorted), sum and max (a sequential float32 loop in list
order: tests/refcollapse.py walks a group's rows one by one), the gather and its fill, the gather's gradient (the same
sequential sum), the decoration (numpy float32 arithmetic rounds every multiply, add and subtract on its own, which is
the contract; torch's CPU cast is the one round-to-nearest-even into float16 / bfloat16).
mean carries the bound tests/test_gpu_collapse.py derives: a sequential fp32 sum of len terms errs by at most about
len 2^-24 of the magnitude sum, the division adds one fp32 rounding, the output half an ulp -- half an ulp of the output
+ (len + 2) 2^-24 of the mean of magnitudes, len the group's own length."""
import copy

import numpy as np
import pytest
import torch

import refcollapse as rc
from util import assert_close_abs_sum

pytestmark = pytest.mark.gpu

DTYPES = {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32, "f64": torch.float64}
N, NV, LONG = 5000, 700, 300            # the main case: points, voxels, the voxel with 600 points


def bits(t):
    t = t.detach().cpu().contiguous()
    return t.view({1: torch.int8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()]).numpy()


def main_ids(id_dtype=np.int64):
    """5000 ids over 700 voxels: voxels 0..19 and 680..699 empty (and a few in between by chance), ~10 % dropped (-1),
    ids >= num_voxels and < -1 sprinkled in, voxel 300 with 600 points: 400 in a run across the 2048 boundary (longer
    than a 256-entry tile), 200 scattered."""
    rng = np.random.default_rng(5)
    ids = rng.integers(20, 680, N).astype(np.int64)
    ids[ids == LONG] = LONG + 1
    ids[rng.random(N) < 0.1] = -1
    big = np.iinfo(id_dtype).max
    ids[rng.choice(N, 30, replace=False)] = rng.choice([NV, NV + 1, 4 * NV, big], 30)
    ids[rng.choice(N, 30, replace=False)] = rng.choice([-2, -NV, -big], 30)
    ids[1850:2250] = LONG
    ids[rng.choice(np.r_[0:1850, 2250:N], 200, replace=False)] = LONG
    assert (ids == LONG).sum() == 600
    return ids.astype(id_dtype)


def ref_groups(ids, nv, n_points=None):
    """rows, offsets [nv + 1], list [offsets[-1]]: a stable argsort of the keys (a point without a voxel: key nv)"""
    ids = np.asarray(ids).astype(np.int64)
    ok = (ids >= 0) & (ids < nv)
    if n_points is not None:
        ok[n_points:] = False
    key = np.where(ok, ids, nv)
    order = np.argsort(key, kind="stable")
    offsets = np.searchsorted(key[order], np.arange(nv + 1), side="left")
    return np.where(ok, ids, -1), offsets, order[:offsets[-1]]


def as_ref(rows, offsets, lst, nv) -> rc.Ref:
    """the groups in the form tests/refcollapse.py reduces"""
    return rc.Ref(None, rows.astype(np.int64), offsets.astype(np.int64), lst.astype(np.int64), nv, nv, [], int((rows >= 0).sum()))


def check_groups(g, ids, nv, n_points=None):
    rows, offsets, lst = ref_groups(ids, nv, n_points)
    assert g.num_voxels == nv and g.rows.dtype == g.offsets.dtype == g.list.dtype == torch.int32
    assert tuple(g.rows.shape) == tuple(g.list.shape) == (len(ids),) and tuple(g.offsets.shape) == (nv + 1,)
    np.testing.assert_array_equal(g.rows.cpu().numpy(), rows)
    np.testing.assert_array_equal(g.offsets.cpu().numpy(), offsets)
    np.testing.assert_array_equal(g.list.cpu().numpy()[:offsets[-1]], lst)
    return rows, offsets, lst


@pytest.fixture(scope="module")
def main(cuda):
    """the main case's groups on the device and as the numpy reference (shared, never modified)"""
    from spconv_amd.pytorch import functional as F
    ids = main_ids()
    g = F.point_groups(torch.from_numpy(ids).to(cuda), NV)
    rows, offsets, lst = ref_groups(ids, NV)
    return g, as_ref(rows, offsets, lst, NV)


# ------------------------------------------------------------------------------------------------ groups
@pytest.mark.parametrize("id_dtype", [np.int64, np.int32])
def test_groups_main_case(cuda, id_dtype):
    from spconv_amd import _lib
    from spconv_amd.pytorch import functional as F
    ids = main_ids(id_dtype)
    before = _lib.load().spx_launch_count(b"pointvoxel/groups")
    g = F.point_groups(torch.from_numpy(ids).to(cuda), NV)
    assert _lib.load().spx_launch_count(b"pointvoxel/groups") == before + 1
    rows, offsets, _ = check_groups(g, ids, NV)
    lens = np.diff(offsets)
    assert lens[LONG] == 600 and (lens[:20] == 0).all() and (lens[680:] == 0).all() and (rows < 0).sum() > 400


def test_groups_behind_the_point_count_are_no_points(cuda):
    from spconv_amd.pytorch import functional as F
    ids = main_ids()
    ids[4321:] = np.random.default_rng(2).integers(0, NV, N - 4321)          # stale rows with valid-looking ids
    n_points = torch.tensor([4321], dtype=torch.int32, device=cuda)
    g = F.point_groups(torch.from_numpy(ids).to(cuda), NV, n_points=n_points)
    rows, offsets, lst = check_groups(g, ids, NV, 4321)
    assert g.n_points is n_points and (rows[4321:] == -1).all()
    feat = torch.rand((N, 8), dtype=torch.float32)
    feat[4321:] = float("nan")                                               # whatever the stale rows hold
    for op in ("sum", "max"):
        got = F.points_to_voxels(feat.to(cuda), g, op)
        np.testing.assert_array_equal(bits(got), bits(rc.reduce(feat, as_ref(rows, offsets, lst, NV), op)), err_msg=op)


@pytest.mark.parametrize("name", ["one_voxel", "no_points", "all_dropped", "nv255", "nv256", "nv257", "nv511", "nv512"])
def test_groups_edges(cuda, name):
    from spconv_amd.pytorch import functional as F
    rng = np.random.default_rng(9)
    if name == "one_voxel":
        nv, ids = 1, rng.integers(-1, 2, 1300)
    elif name == "no_points":
        nv, ids = 7, np.zeros((0,), np.int64)
    elif name == "all_dropped":
        nv, ids = 40, np.where(rng.random(1300) < 0.5, -1, 40 + rng.integers(0, 5, 1300))
    else:       # the key width ceil(log2(nv + 1)) goes 8 -> 9 bits at 256, 9 -> 10 at 512; the last voxel is occupied
        nv = int(name[2:])
        ids = rng.integers(-1, nv, 1300)
        ids[-1] = nv - 1
    g = F.point_groups(torch.from_numpy(ids.astype(np.int64)).to(cuda), nv)
    _, offsets, _ = check_groups(g, ids, nv)
    if name in ("no_points", "all_dropped"):
        assert (offsets == 0).all()
        feat = torch.ones((len(ids), 3), device=cuda)
        assert bool((F.points_to_voxels(feat, g, "sum") == 0).all())        # empty groups: zeros


# ------------------------------------------------------------------------------------------------ reduce
@pytest.mark.parametrize("C", [1, 3, 8, 20, 64])
@pytest.mark.parametrize("dt", ["f16", "bf16", "f32"])
def test_reduce(cuda, main, dt, C):
    from spconv_amd.pytorch import functional as F
    g, ref = main
    dtype = DTYPES[dt]
    feat = rc.features(N, C, dtype, 100 + C)
    dev = feat.to(cuda)
    lens = np.diff(ref.offsets)
    empty = torch.from_numpy(np.nonzero(lens == 0)[0])
    for op in ("sum", "max"):
        got = F.points_to_voxels(dev, g, op)
        assert got.dtype == dtype and tuple(got.shape) == (NV, C)
        np.testing.assert_array_equal(bits(got), bits(rc.reduce(feat, ref, op)), err_msg=f"{op} {dt} C={C}")
        assert len(empty) >= 40 and bool((got.cpu()[empty] == 0).all())
    mean, A, _ = rc.mean_f64(feat, ref)
    got = F.points_to_voxels(dev, g, "mean")
    assert_close_abs_sum(got.double().cpu().numpy(), mean, A * (lens[:, None] + 2), dtype, 2.0 ** -24, name=f"mean {dt} C={C}")
    assert bool((got.cpu()[empty] == 0).all())
    # voxel rows at or beyond *n_live are dead: zeros, the rows in front unchanged
    n_live = torch.tensor([500], dtype=torch.int32, device=cuda)
    part = F.points_to_voxels(dev, g._replace(n_live=n_live), "max")
    np.testing.assert_array_equal(bits(part[:500]), bits(rc.reduce(feat, ref, "max")[:500]))
    assert bool((part[500:] == 0).all()) and lens[500:].sum() > 0


# ------------------------------------------------------------------------------------------------ gather
@pytest.mark.parametrize("C", [1, 3, 8, 64])
@pytest.mark.parametrize("dt", ["f16", "bf16", "f32", "f64", "i8"])
def test_gather_forward(cuda, main, dt, C):
    from spconv_amd.pytorch import functional as F
    g, ref = main
    if dt == "i8":
        vfeat = torch.randint(-128, 128, (NV, C), dtype=torch.int8, generator=torch.Generator().manual_seed(C))
    else:
        vfeat = rc.features(NV, C, DTYPES[dt], 7 + C)
        vfeat[3, 0] = -0.0
    for fill in (0, -1):
        got = F.voxels_to_points(vfeat.to(cuda), g, invalid_value=fill)
        want = torch.full((N, C), fill, dtype=vfeat.dtype)
        held = torch.from_numpy(np.nonzero(ref.rows >= 0)[0])
        want[held] = vfeat[torch.from_numpy(ref.rows[ref.rows >= 0])]
        assert got.dtype == vfeat.dtype
        np.testing.assert_array_equal(bits(got), bits(want), err_msg=f"{dt} C={C} fill={fill}")


def seq_sum_over_groups(dout: torch.Tensor, ref: rc.Ref) -> torch.Tensor:
    """dvfeat[v] = the rows of dout of voxel v's points added one by one in list order in fp32 (fp64), rounded once"""
    return rc.reduce(dout, ref, "sum")


@pytest.mark.parametrize("C", [1, 3, 8, 64])
@pytest.mark.parametrize("dt", ["f16", "bf16", "f32", "f64"])
def test_gather_backward_is_the_sequential_sum_and_reproducible(cuda, main, dt, C):
    from spconv_amd.pytorch import functional as F
    g, ref = main
    dtype = DTYPES[dt]
    dout = rc.features(N, C, dtype, 31 + C)
    want = seq_sum_over_groups(dout, ref)
    grads = []
    for _ in range(2):
        vfeat = rc.features(NV, C, dtype, 3).to(cuda).requires_grad_(True)
        F.voxels_to_points(vfeat, g, invalid_value=-1).backward(dout.to(cuda))
        grads.append(vfeat.grad)
    np.testing.assert_array_equal(bits(grads[0]), bits(want), err_msg=f"{dt} C={C}")
    np.testing.assert_array_equal(bits(grads[0]), bits(grads[1]))


def composite_gather(seg_res_features, pc_voxel_id, invalid_value=0):
    """gather_features_by_pc_voxel_id as it was before it went through voxels_to_points"""
    ids = pc_voxel_id.to(seg_res_features.device)
    inside = ids >= 0
    rows = seg_res_features.index_select(0, ids.clamp_min(0))
    shape = [-1] + [1] * (seg_res_features.ndim - 1)
    fill = torch.full_like(rows, invalid_value)
    return torch.where(inside.view(shape), rows, fill)


def test_gather_features_by_pc_voxel_id_returns_what_the_composite_returns(cuda):
    from spconv_amd.pytorch.utils import gather_features_by_pc_voxel_id
    ids = torch.from_numpy(np.where(np.random.default_rng(4).random(N) < 0.1, -1, np.random.default_rng(3).integers(0, NV, N)))
    for dtype, C, fill in ((torch.float16, 64, 0), (torch.float16, 5, -1), (torch.float32, 3, 0.5), (torch.bfloat16, 8, 2),
                           (torch.float64, 2, -1), (torch.int64, 4, -1), (torch.int32, 1, 7), (torch.uint8, 16, 255)):
        seg = torch.rand((NV, C), generator=torch.Generator().manual_seed(C)) * 200 - 100
        seg = (seg.abs() if dtype == torch.uint8 else seg).to(dtype).to(cuda)
        for pid in (ids.to(cuda), ids):                                       # (ids on the host are moved over)
            got = gather_features_by_pc_voxel_id(seg, pid, fill)
            want = composite_gather(seg, pid, fill)
            assert got.dtype == want.dtype and got.shape == want.shape
            np.testing.assert_array_equal(bits(got), bits(want), err_msg=f"{dtype} C={C}")
    # with a gradient: the composite's index_add_ sums the same rows in some order; in float64 the two agree closely
    seg = torch.rand((NV, 6), dtype=torch.float64, device=cuda, requires_grad=True)
    dout = torch.rand((N, 6), dtype=torch.float64, device=cuda)
    (g_new,) = torch.autograd.grad(gather_features_by_pc_voxel_id(seg, ids.to(cuda)), seg, dout)
    (g_old,) = torch.autograd.grad(composite_gather(seg, ids.to(cuda)), seg, dout)
    assert float((g_new - g_old).abs().max()) <= 2.0 ** -45 * float(g_old.abs().max())
    # inputs the kernel does not take keep the composite: 3-d rows
    seg3 = torch.rand((NV, 2, 3), device=cuda)
    assert torch.equal(gather_features_by_pc_voxel_id(seg3, ids.to(cuda), -1), composite_gather(seg3, ids.to(cuda), -1))


# ------------------------------------------------------------------------------------------------ decorate
def deco_scene(ndim, nfeat, seed=0, n=1500):
    """points in a grid with a non-zero lower bound and a voxel size of 0.3 (no power of two: where an FMA would show),
    the voxels they fall into numbered in key order, ~8 % of the points dropped.  -> points, ids, indices (batch, zyx),
    vsize_xyz, coors_range_xyz"""
    rng = np.random.default_rng(seed)
    vsize = [0.3, 0.3, 0.4][:ndim]
    lo = [-3.1, 2.0, -1.0][:ndim]
    cells = [11, 9, 5][:ndim]
    hi = [l + v * c for l, v, c in zip(lo, vsize, cells)]
    pts = np.concatenate([rng.uniform(lo, hi, (n, ndim)), rng.uniform(0, 1, (n, nfeat - ndim))], axis=1).astype(np.float32)
    c = np.floor((pts[:, :ndim] - np.float32(lo)) / np.float32(vsize)).astype(np.int64)
    c = np.clip(c, 0, np.asarray(cells) - 1)
    zyx = c[:, ::-1]
    uniq, ids = np.unique(zyx, axis=0, return_inverse=True)
    ids = ids.reshape(-1).astype(np.int64)
    ids[rng.random(n) < 0.08] = -1
    indices = np.concatenate([np.zeros((len(uniq), 1), np.int64), uniq], axis=1).astype(np.int32)
    return pts, ids, indices, vsize, lo + hi


def ref_decorate(pts, rows, indices, vsize_xyz, range_xyz, mean, flags, ndim, C_out):
    """the header's formula in numpy float32: every operation rounds on its own"""
    from spconv_amd.pytorch.utils import calc_point2voxel_meta_data
    vs, _, _, cr = calc_point2voxel_meta_data(list(vsize_xyz), list(range_xyz))          # zyx, as the C call takes them
    vs_xyz, lo_xyz = np.float32(vs[::-1]), np.float32(cr[:ndim][::-1])
    out = np.zeros((pts.shape[0], C_out), np.float32)
    ok = rows >= 0
    r = rows[ok]
    cols = [pts[ok]]
    if flags & 1:
        cols.append(pts[ok, :ndim] - mean[r, :ndim])
    if flags & 2:
        cell = indices[r, 1:][:, ::-1].astype(np.float32)
        centre = (cell + np.float32(0.5)) * vs_xyz + lo_xyz
        cols.append(pts[ok, :ndim] - centre)
    row = np.concatenate(cols, axis=1)
    assert row.dtype == np.float32
    out[ok, :row.shape[1]] = row
    return out


@pytest.mark.parametrize("ndim,nfeat", [(3, 4), (3, 5), (2, 4)])
def test_decorate(cuda, ndim, nfeat):
    from spconv_amd.pytorch import functional as F
    pts, ids, indices, vsize, crange = deco_scene(ndim, nfeat, seed=ndim * 10 + nfeat)
    nv = indices.shape[0]
    g = F.point_groups(torch.from_numpy(ids).to(cuda), nv)
    rows = g.rows.cpu().numpy()
    assert (rows < 0).sum() > 50
    dpts, didx = torch.from_numpy(pts).to(cuda), torch.from_numpy(indices).to(cuda)
    mean = F.points_to_voxels(dpts, g, "mean").cpu().numpy()                  # what the decoration subtracts
    for flags in (0, 1, 2, 3):
        width = nfeat + ndim * bin(flags).count("1")
        for dt in ("f32", "f16", "bf16"):
            for pad_to in (None, 16):
                got = F.decorate_points(dpts, g, didx, vsize, crange, cluster=bool(flags & 1), center=bool(flags & 2),
                                        dtype=DTYPES[dt], pad_to=pad_to)
                C_out = pad_to or width
                want = torch.from_numpy(ref_decorate(pts, rows, indices, vsize, crange, mean, flags, ndim, C_out)).to(DTYPES[dt])
                assert got.dtype == DTYPES[dt] and tuple(got.shape) == (len(ids), C_out)
                np.testing.assert_array_equal(bits(got), bits(want), err_msg=f"flags={flags} {dt} pad_to={pad_to}")
                assert bool((got.cpu()[torch.from_numpy(rows < 0)] == 0).all())
    with pytest.raises(ValueError, match="pad_to"):
        F.decorate_points(dpts, g, didx, vsize, crange, pad_to=nfeat)


# ------------------------------------------------------------------------------------------------ autograd
def small_groups(cuda):
    from spconv_amd.pytorch import functional as F
    rng = np.random.default_rng(1)
    ids = rng.integers(-1, 7, 40)
    ids[ids == 5] = 4                                  # an empty voxel in the middle
    return F.point_groups(torch.from_numpy(ids.astype(np.int64)).to(cuda), 7)


def distinct(n, C, cuda, seed):
    """distinct values, far enough apart for gradcheck's finite differences not to reorder a maximum"""
    perm = torch.randperm(n * C, generator=torch.Generator().manual_seed(seed)).double().reshape(n, C)
    return (perm / (n * C) - 0.5).to(cuda).requires_grad_(True)


@pytest.mark.parametrize("op", ["sum", "mean", "max"])
def test_gradcheck_points_to_voxels(cuda, op):
    from spconv_amd.pytorch import functional as F
    g = small_groups(cuda)
    assert torch.autograd.gradcheck(lambda f: F.points_to_voxels(f, g, op), (distinct(40, 3, cuda, 1),), eps=1e-6, atol=1e-7)


def test_gradcheck_voxels_to_points(cuda):
    from spconv_amd.pytorch import functional as F
    g = small_groups(cuda)
    assert torch.autograd.gradcheck(lambda v: F.voxels_to_points(v, g, -1), (distinct(7, 3, cuda, 2),), eps=1e-6, atol=1e-7)


def test_gradcheck_dynamic_vfe(cuda):
    import spconv_amd.pytorch as spconv
    pts, ids, indices, vsize, crange = deco_scene(3, 4, seed=3, n=40)
    g = spconv.point_groups(torch.from_numpy(ids).to(cuda), indices.shape[0])
    torch.manual_seed(0)
    vfe = spconv.DynamicVFE(4, (3, 3), norm=False, reduce="max").to(cuda).double()
    dpts, didx = torch.from_numpy(pts).to(cuda), torch.from_numpy(indices).to(cuda)
    names = [n for n, _ in vfe.named_parameters()]
    ps = [p.detach().clone().requires_grad_(True) for _, p in vfe.named_parameters()]
    assert [tuple(p.shape) for p in ps] == [(3, 10), (3,), (3, 6), (3,)]

    def f(*values):        # the module as a function of its parameters
        return torch.func.functional_call(vfe, dict(zip(names, values)), (dpts, g, didx, vsize, crange))
    assert tuple(f(*ps).shape) == (indices.shape[0], 3)
    assert torch.autograd.gradcheck(f, ps, eps=1e-6, atol=1e-6)


def test_training_statistics_see_real_points_only(cuda):
    import spconv_amd.pytorch as spconv
    pts, ids, indices, vsize, crange = deco_scene(3, 4, seed=8, n=600)
    g = spconv.point_groups(torch.from_numpy(ids).to(cuda), indices.shape[0])
    torch.manual_seed(1)
    vfe = spconv.DynamicVFE(4, (8,)).to(cuda).train()
    vfe.norms[0].momentum = 1.0
    dpts, didx = torch.from_numpy(pts).to(cuda), torch.from_numpy(indices).to(cuda)
    out = vfe(dpts, g, didx, vsize, crange)
    out.sum().backward()
    real = torch.from_numpy(ids >= 0).to(cuda)
    x = spconv.functional.decorate_points(dpts, g, didx, vsize, crange)[real]
    y = vfe.linears[0](x)
    assert torch.allclose(vfe.norms[0].running_mean, y.mean(0), rtol=1e-4, atol=1e-6)
    assert vfe.linears[0].weight.grad is not None and bool(torch.isfinite(vfe.linears[0].weight.grad).all())


# ------------------------------------------------------------------------------------------------ capture, runner
VSIZE, RANGE, GRID = [0.5, 0.5, 0.5], [0.0, 0.0, 0.0, 16.0, 16.0, 8.0], [16, 32, 32]


def cloud(n, seed):
    rng = np.random.default_rng(seed)
    xyz = rng.uniform([-0.5, 0, 0], [16.5, 16, 8], (n, 3))                   # (a few points outside the range: dropped)
    return torch.from_numpy(np.concatenate([xyz, rng.uniform(0, 1, (n, 1))], axis=1).astype(np.float32))


def make_gen(cuda, max_voxels=4000, max_points=3000):
    from spconv_amd.pytorch.utils import StaticPointToVoxel
    return StaticPointToVoxel(VSIZE, RANGE, 4, max_voxels, 5, max_points, key_order=True, keep_voxels=False, device=cuda)


def make_vfe(cuda, channels=(16, 32)):
    import spconv_amd.pytorch as spconv
    torch.manual_seed(0)
    vfe = spconv.DynamicVFE(4, channels).to(cuda)
    for bn in vfe.norms:                               # (statistics a training run would have left)
        bn.running_mean.uniform_(-0.5, 0.5)
        bn.running_var.uniform_(0.5, 2.0)
    return vfe.half().eval()


def test_capture_voxeliser_groups_and_vfe_in_one_graph(cuda):
    gen, vfe = make_gen(cuda), make_vfe(cuda)
    scenes = [cloud(3000, 1).to(cuda), cloud(1200, 2).to(cuda)]

    def head():
        gen.run()
        return vfe(gen.points, gen.point_groups(), gen.indices, VSIZE, RANGE)
    eager = []
    with torch.no_grad():
        for pc in scenes:
            gen.load(pc)
            out = head()
            nv = int(gen.n_voxels[0])
            ids = gen.pc_voxel_id.cpu().numpy()
            check_groups(gen.point_groups(), ids, gen.max_num_voxels, pc.shape[0])
            eager.append((out[:nv].clone(), nv))
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = head()
    assert eager[0][1] > eager[1][1] > 500
    for k in (0, 1, 0):               # the 1200-point scene finds the 3000-point scene's rows behind its count
        gen.load(scenes[k])
        graph.replay()
        torch.cuda.synchronize()
        want, nv = eager[k]
        assert int(gen.n_voxels[0]) == nv
        np.testing.assert_array_equal(bits(out[:nv]), bits(want))
        assert bool((out[nv:] == 0).all())


def test_runner_with_a_point_encoder(cuda):
    import spconv_amd.pytorch as spconv
    from spconv_amd.pytorch.static import StaticInference
    torch.manual_seed(0)
    net = spconv.SparseSequential(spconv.SubMConv3d(32, 32, 3, indice_key="a"),
                                  spconv.SubMConv3d(32, 16, 3, indice_key="a")).to(cuda).half().eval()
    eager = copy.deepcopy(net)
    gen, vfe = make_gen(cuda), make_vfe(cuda)
    with pytest.raises(ValueError, match="in_channels"):
        StaticInference(net, 4000, 4, GRID, 1, torch.float16, voxelizer=gen, point_encoder=vfe)
    with pytest.raises(ValueError, match="voxelizer"):
        StaticInference(net, 4000, 32, GRID, 1, torch.float16, point_encoder=vfe)
    runner = StaticInference(net, 4000, 32, GRID, 1, torch.float16, voxelizer=gen, point_encoder=vfe)
    assert runner.point_encoder is vfe and not vfe.training
    for n, seed in ((3000, 1), (1200, 2)):
        pc = cloud(n, seed).to(cuda)
        got = runner.run_points(pc)
        live = got.indices[:, 0] >= 0
        n_live = int(live.sum())
        with torch.no_grad():
            gen(pc)
            nv = int(gen.n_voxels[0])
            feats = vfe(gen.points, gen.point_groups(), gen.indices, VSIZE, RANGE)
            want = eager(spconv.SparseConvTensor(feats[:nv].clone(), gen.indices[:nv].clone(), GRID, 1))
        assert n_live == nv > 500 and bool(live[:nv].all())
        assert torch.equal(got.indices[:nv], want.indices)
        np.testing.assert_array_equal(bits(got.features[:nv]), bits(want.features))
    runner.release_bounds()
