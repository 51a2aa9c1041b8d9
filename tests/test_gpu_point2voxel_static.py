"""GPU: the static-shape voxeliser (spx_point2voxel_static, utils.StaticPointToVoxel) and the runner that starts from
points (StaticInference(voxelizer=...)) against oracle.point2voxel, the sequential CPU restatement of the reference's
Point2VoxelCPU: live rows bit-exact, every row behind them dead, counts on the device, key order = the first-seen
result renumbered, the rank map left behind equal in effect to the hash build, mean feature rows bit-exact against a
float32 numpy loop, the call recordable in a graph, and a captured backbone fed from points bit-identical to the eager
pass over the oracle's voxels."""
import copy
import functools

import numpy as np
import pytest
import torch

import oracle

pytestmark = pytest.mark.gpu

VSIZE, RANGE = [0.1, 0.1, 0.2], [0, -4, -2, 8, 4, 2]          # an 80 x 80 x 20 grid (xyz)
GRID = [20, 80, 80]                                            # zyx


def _cloud(n, seed, lo=(-1.0, -5.0, -3.0), hi=(9.0, 5.0, 3.0), nfeat=4):
    """(the cloud of tests/test_gpu_point2voxel.py: clusters -> several points per voxel, points outside the range)"""
    rng = np.random.default_rng(seed)
    pts = rng.uniform(lo + (0.0,) * (nfeat - 3), hi + (1.0,) * (nfeat - 3), (n, nfeat)).astype(np.float32)
    pts[: n // 2, :3] = pts[: n // 2, :3] * 0.05 + np.array([4.0, 0.0, 0.0], dtype=np.float32)
    return pts


def _gen(cuda, max_voxels, max_points, max_num_points=20000, **kw):
    from spconv_amd.pytorch.utils import StaticPointToVoxel
    return StaticPointToVoxel(VSIZE, RANGE, 4, max_voxels, max_points, max_num_points, device=cuda, **kw)


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def _meta():
    from spconv_amd.pytorch.utils import calc_point2voxel_meta_data
    vsize, grid, _, coors_range = calc_point2voxel_meta_data(VSIZE, RANGE)
    assert grid == GRID
    return vsize, coors_range


@functools.lru_cache(maxsize=None)
def _oracle(n, seed, max_voxels, max_points, empty_mean=False):
    """One scene, first-seen: (voxels, indices with the batch column, num, pc_voxel_id, voxels found).  Computed once
    per case, shared, read-only."""
    vsize, coors_range = _meta()
    pts = _cloud(n, seed)
    v, i, c, pid = oracle.point2voxel(pts, vsize, coors_range, GRID, max_voxels, max_points, empty_mean)
    found = oracle.point2voxel(pts, vsize, coors_range, GRID, max(n, 1), 1, False)[1].shape[0]
    i = np.concatenate([np.zeros((i.shape[0], 1), np.int32), i], axis=1)
    return _frozen(pts, v, i, c, pid) + (found,)


def _keys(idx):
    k = idx[:, 0].astype(np.int64)
    for d, g in enumerate(GRID):
        k = k * g + idx[:, 1 + d]
    return k


def _key_ordered(v, i, c, pid):
    """The first-seen result renumbered by ascending key."""
    order = np.argsort(_keys(i), kind="stable")
    rank = np.empty_like(order)
    rank[order] = np.arange(order.shape[0])
    return v[order], i[order], c[order], np.where(pid >= 0, rank[np.maximum(pid, 0)], -1)


def _check(gen, want, n_points, found):
    """Live rows equal `want` bit for bit, every row behind them is dead in all outputs, the counts are {kept, found}."""
    v, i, c, pid = want
    kept = i.shape[0]
    assert gen.n_voxels.tolist() == [kept, found]
    assert gen.overflowed() == (found > kept)
    gi, gc, gp = gen.indices.cpu().numpy(), gen.num_per_voxel.cpu().numpy(), gen.pc_voxel_id.cpu().numpy()
    np.testing.assert_array_equal(gi[:kept], i)
    np.testing.assert_array_equal(gc[:kept], c)
    np.testing.assert_array_equal(gp[:n_points], pid)
    assert (gi[kept:] == -1).all() and (gc[kept:] == 0).all() and (gp[n_points:] == -1).all()
    if gen.voxels is not None:
        gv = gen.voxels.cpu().numpy()
        np.testing.assert_array_equal(gv[:kept].view(np.int32), v.view(np.int32))
        assert (gv[kept:].view(np.int32) == 0).all()
    if gen.mean is not None:
        assert (gen.mean[kept:].cpu().view(torch.int32 if gen.mean.dtype == torch.float32 else torch.int16) == 0).all()


# ---------------------------------------------------------------------------------------------- 1: first-seen, one scene
@pytest.mark.parametrize("n,max_voxels,max_points,empty_mean",
                         [(20000, 40000, 5, False), (20000, 40000, 5, True), (20000, 300, 3, False),
                          (20000, 300, 3, True), (50, 100, 1, False)])
def test_first_seen_is_the_oracle_and_the_rest_is_dead(cuda, n, max_voxels, max_points, empty_mean):
    pts, v, i, c, pid, found = _oracle(n, 1, max_voxels, max_points, empty_mean)
    gen = _gen(cuda, max_voxels, max_points, key_order=False)
    out = gen(torch.tensor(pts, device=cuda), empty_mean=empty_mean)
    assert out[0] is gen.voxels and out[1] is gen.indices and out[2] is gen.num_per_voxel and out[3] is gen.pc_voxel_id
    assert out[1].shape == (max_voxels, 4) and out[3].shape == (20000,)
    _check(gen, (v, i, c, pid), n, found)
    if n == 20000:
        assert (pid == -1).any() and c.max() == max_points and (found > max_voxels) == (max_voxels == 300)


# ---------------------------------------------------------------------------------------------- 2: live count on the device
@pytest.mark.parametrize("key_order", [False, True])
def test_rows_behind_the_device_side_count_are_no_points(cuda, key_order):
    pts, v, i, c, pid, found = _oracle(12000, 4, 40000, 5)
    gen = _gen(cuda, 40000, 5, key_order=key_order)
    gen.points.fill_(float("nan"))                      # whatever lies behind the 12 000 points
    gen.batch_ids[12000:].fill_(7)
    gen(torch.tensor(pts, device=cuda))
    _check(gen, _key_ordered(v, i, c, pid) if key_order else (v, i, c, pid), 12000, found)
    assert bool(torch.isnan(gen.points[12000:]).all())  # (and they were there during the call)


def test_too_many_points_raise(cuda):
    gen = _gen(cuda, 100, 2, max_num_points=64)
    with pytest.raises(ValueError, match="64"):
        gen.load(torch.zeros((65, 4)))
    with pytest.raises(ValueError, match="64"):
        gen(torch.zeros((65, 4), device=cuda))


# ---------------------------------------------------------------------------------------------- 3: reuse
@pytest.mark.parametrize("key_order", [False, True])
def test_a_smaller_scene_leaves_nothing_of_the_one_before(cuda, key_order):
    gen = _gen(cuda, 40000, 5, key_order=key_order, mean_dtype=torch.float32)
    form = _key_ordered if key_order else (lambda *a: a)
    for n, seed in ((20000, 1), (3000, 6)):
        pts, v, i, c, pid, found = _oracle(n, seed, 40000, 5, True)
        gen(torch.tensor(pts, device=cuda), empty_mean=True)
        _check(gen, form(v, i, c, pid), n, found)         # (rows kept .. max_voxels dead: none of the first scene's)


# ---------------------------------------------------------------------------------------------- 4: key order
@pytest.mark.parametrize("n,max_voxels,max_points", [(20000, 40000, 5), (20000, 300, 3)])
def test_key_order_is_the_first_seen_result_renumbered(cuda, n, max_voxels, max_points):
    pts, v, i, c, pid, found = _oracle(n, 1, max_voxels, max_points)
    gen = _gen(cuda, max_voxels, max_points, key_order=True)
    gen(torch.tensor(pts, device=cuda))
    _check(gen, _key_ordered(v, i, c, pid), n, found)
    keys = _keys(gen.indices[: i.shape[0]].cpu().numpy())
    assert (np.diff(keys) > 0).all()                     # strictly ascending over the live rows
    assert (found > max_voxels) == (max_voxels == 300)   # the capped case keeps the first 300 in first-seen order


# ---------------------------------------------------------------------------------------------- 5: two scenes
def _two_scenes(ids):
    """8000 points of seed 2 and 8000 of seed 3 interleaved point by point; ids[p] = scene of point p (anything outside
    {0, 1} drops it).  Per scene the oracle's result over the points that carry its id; returns the points, the
    first-seen and the key-ordered expectation (voxels by the index of their first point / per scene by key,
    batch-major), and the voxels found."""
    vsize, coors_range = _meta()
    pts = np.empty((16000, 4), np.float32)
    pts[0::2], pts[1::2] = _cloud(8000, 2), _cloud(8000, 3)
    parts, first_point, pid, base = [], [], np.full((16000,), -1, np.int64), 0
    for b in (0, 1):
        sel = np.flatnonzero(ids == b)
        v, i, c, p = oracle.point2voxel(pts[sel], vsize, coors_range, GRID, 40000, 5, False)
        inside = np.flatnonzero(p >= 0)
        vox, first = np.unique(p[inside], return_index=True)
        assert np.array_equal(vox, np.arange(i.shape[0]))
        first_point.append(sel[inside[first]])
        pid[sel] = np.where(p >= 0, p + base, -1)
        parts.append((v, np.concatenate([np.full((i.shape[0], 1), b, np.int32), i], axis=1), c))
        base += i.shape[0]
    v, i, c = (np.concatenate([q[k] for q in parts]) for k in range(3))       # batch-major, first-seen inside a scene
    order = np.argsort(np.concatenate(first_point), kind="stable")            # -> first-seen over the whole array
    rank = np.empty_like(order)
    rank[order] = np.arange(order.shape[0])
    first_seen = (v[order], i[order], c[order], np.where(pid >= 0, rank[np.maximum(pid, 0)], -1))
    return pts, first_seen, _key_ordered(v, i, c, pid), base


@pytest.mark.parametrize("key_order", [True, False])
@pytest.mark.parametrize("strays", [False, True])
def test_two_interleaved_scenes(cuda, key_order, strays):
    ids = np.tile(np.array([0, 1], np.int32), 8000)
    if strays:
        ids[100:140], ids[5000:5031] = 2, -1             # a batch index outside [0, batch_size) drops the point
    pts, first_seen, keyed, found = _two_scenes(ids)
    gen = _gen(cuda, 40000, 5, batch_size=2, key_order=key_order)
    gen(torch.tensor(pts, device=cuda), torch.from_numpy(ids).to(cuda))
    _check(gen, keyed if key_order else first_seen, 16000, found)
    if strays:
        got = gen.pc_voxel_id.cpu().numpy()
        assert (got[100:140] == -1).all() and (got[5000:5031] == -1).all()
    if key_order:
        idx = gen.indices[:found].cpu().numpy()
        assert (np.diff(_keys(idx)) > 0).all() and set(idx[:, 0]) == {0, 1}


# ---------------------------------------------------------------------------------------------- 6: rank map
def test_the_rank_map_left_behind_builds_the_hash_builds_rulebook(cuda):
    from spconv_amd.pytorch import _rulebook, ops
    ids = np.tile(np.array([0, 1], np.int32), 8000)
    pts, _, _, found = _two_scenes(ids)
    gen = _gen(cuda, 40000, 5, batch_size=2, key_order=True)
    gen(torch.tensor(pts, device=cuda), torch.from_numpy(ids).to(cuda))
    assert getattr(gen.indices, "_spx_rankmap", None) is not None
    assert _rulebook._rankmap_of(gen.indices, 2, GRID, 40000, 27) is not None       # (the SubM build will take it)
    plain = gen.indices.clone()
    assert getattr(plain, "_spx_rankmap", None) is None
    rb_hash, _ = ops.build_rulebook(plain, 2, GRID, [3] * 3, [1] * 3, [1] * 3, [1] * 3, [0] * 3, True)
    rb_rank, _ = ops.build_rulebook(gen.indices, 2, GRID, [3] * 3, [1] * 3, [1] * 3, [1] * 3, [0] * 3, True)
    assert torch.equal(rb_rank.pair_fwd, rb_hash.pair_fwd) and torch.equal(rb_rank.mask_fwd, rb_hash.mask_fwd)
    assert int((rb_hash.pair_fwd >= 0).sum()) > found        # (neighbours, not only centres)


# ---------------------------------------------------------------------------------------------- 7: mean features
def _mean_rows(v, c, dtype):
    """Slots 0 .. num - 1 added in that order in float32, divided in float32, converted by torch on the CPU."""
    acc = np.zeros((v.shape[0], v.shape[2]), np.float32)
    for j in range(v.shape[1]):
        acc = np.where((c > j)[:, None], acc + v[:, j], acc).astype(np.float32)
    mean = acc / np.maximum(c, 1).astype(np.float32)[:, None]
    assert mean.dtype == np.float32
    return torch.from_numpy(mean).to(dtype)


def _bits(t):
    return t.cpu().contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16).numpy()


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16])
def test_mean_rows_are_bit_exact(cuda, dtype):
    pts, v, i, c, pid, found = _oracle(20000, 1, 40000, 5)
    v, i, c, pid = _key_ordered(v, i, c, pid)
    want = _bits(_mean_rows(v, c, dtype))
    assert c.min() == 1 and c.max() == 5
    kept = i.shape[0]
    pc = torch.tensor(pts, device=cuda)
    filled = _gen(cuda, 40000, 5, mean_dtype=dtype)
    filled(pc, empty_mean=True)                               # (the fill of the empty slots is not part of the mean)
    bare = _gen(cuda, 40000, 5, mean_dtype=dtype, keep_voxels=False)
    out = bare(pc)
    assert out[0] is None and bare.voxels is None
    with pytest.raises(ValueError, match="keep_voxels"):
        bare.run(empty_mean=True)
    for gen in (filled, bare):
        assert gen.mean.dtype == dtype and gen.mean.shape == (40000, 4)
        got = _bits(gen.mean)
        np.testing.assert_array_equal(got[:kept], want)
        assert (got[kept:] == 0).all()
    np.testing.assert_array_equal(bare.indices.cpu().numpy()[:kept], i)
    np.testing.assert_array_equal(bare.num_per_voxel.cpu().numpy()[:kept], c)
    np.testing.assert_array_equal(bare.pc_voxel_id.cpu().numpy(), pid)


# ---------------------------------------------------------------------------------------------- 8: capture
def test_run_replays_from_a_graph(cuda):
    """A call that synchronised or read anything back would fail the capture."""
    gen = _gen(cuda, 40000, 5, key_order=True, mean_dtype=torch.float16)
    scenes = [torch.tensor(_oracle(20000, 1, 40000, 5)[0], device=cuda),
              torch.tensor(_oracle(3000, 6, 40000, 5, True)[0], device=cuda)]
    outputs = lambda: [t.clone() for t in (gen.voxels, gen.indices, gen.num_per_voxel, gen.pc_voxel_id, gen.mean,
                                           gen.n_voxels, gen._rankmap)]
    plain = []
    for pc in scenes:
        gen(pc)
        plain.append(outputs())
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        gen.run()
    for pc, want in list(zip(scenes, plain)) + [(scenes[0], plain[0])]:
        gen.load(pc)
        graph.replay()
        for got, ref in zip(outputs(), want):
            assert torch.equal(got, ref)
    assert gen.n_voxels.tolist()[0] == _oracle(20000, 1, 40000, 5)[2].shape[0]


# ---------------------------------------------------------------------------------------------- 9: runner
def test_a_captured_backbone_runs_from_points(cuda):
    import spconv_amd.pytorch as spconv
    from spconv_amd.pytorch.static import StaticInference
    torch.manual_seed(0)
    net = spconv.SparseSequential(spconv.SubMConv3d(4, 16, 3), spconv.SparseConv3d(16, 32, 3, stride=2),
                                  spconv.SubMConv3d(32, 32, 3)).to(cuda).half().eval()
    eager = copy.deepcopy(net)                                  # (the runner freezes bounds on `net`)
    gen = _gen(cuda, 40000, 5, key_order=True, mean_dtype=torch.float16, keep_voxels=False)
    with pytest.raises(ValueError, match="in_channels"):
        StaticInference(net, 40000, 8, GRID, 1, torch.float16, bounds={"1": 40000}, voxelizer=gen)
    with pytest.raises(ValueError, match="dtype"):
        StaticInference(net, 40000, 4, GRID, 1, torch.float32, bounds={"1": 40000}, voxelizer=gen)
    with pytest.raises(ValueError, match="spatial_shape"):
        StaticInference(net, 40000, 4, [80, 80, 20], 1, torch.float16, bounds={"1": 40000}, voxelizer=gen)
    with pytest.raises(ValueError, match="max_voxels"):
        StaticInference(net, 30000, 4, GRID, 1, torch.float16, bounds={"1": 40000}, voxelizer=gen)
    with pytest.raises(ValueError, match="batch_size"):
        StaticInference(net, 40000, 4, GRID, 2, torch.float16, bounds={"1": 40000}, voxelizer=gen)
    runner = StaticInference(net, 40000, 4, GRID, 1, torch.float16, bounds={"1": 40000}, voxelizer=gen)
    assert runner.voxelizer is gen and runner.key_ordered_input
    for n, seed in ((20000, 1), (3000, 6)):
        pts, v, i, c, pid, found = _oracle(n, seed, 40000, 5)
        v, i, c, pid = _key_ordered(v, i, c, pid)
        feats = _mean_rows(v, c, torch.float16).to(cuda)
        with torch.no_grad():
            want = eager(spconv.SparseConvTensor(feats, torch.from_numpy(i).to(cuda), GRID, 1))
        got = runner.run_points(torch.tensor(pts, device=cuda))
        assert runner.overflowed() == {}, runner.counts()
        live = got.indices[:, 0] >= 0
        n_live = int(live.sum())
        assert n_live == want.indices.shape[0] > 0 and bool(live[:n_live].all())
        assert torch.equal(got.indices[:n_live], want.indices)
        assert np.array_equal(_bits(got.features[:n_live]), _bits(want.features))
        np.testing.assert_array_equal(runner.voxelizer.pc_voxel_id.cpu().numpy()[:n], pid)   # results back to points
    with pytest.raises(ValueError, match="run_points"):
        runner(feats, torch.from_numpy(i).to(cuda))
    runner.release_bounds()


# ---------------------------------------------------------------------------------------------- 10: edges
@pytest.mark.parametrize("key_order", [False, True])
def test_no_points_leave_every_row_dead(cuda, key_order):
    gen = _gen(cuda, 1000, 3, key_order=key_order, mean_dtype=torch.float32)
    pts, v, i, c, pid, found = _oracle(50, 1, 1000, 3)
    gen(torch.tensor(pts, device=cuda))
    assert gen.n_voxels.tolist()[0] > 0
    gen(torch.zeros((0, 4), device=cuda))
    empty = (np.zeros((0, 3, 4), np.float32), np.zeros((0, 4), np.int32), np.zeros((0,), np.int32),
             np.zeros((0,), np.int64))
    _check(gen, empty, 0, 0)
    assert gen.n_voxels.tolist() == [0, 0]


def test_grid_beyond_32_bits(cuda):
    """2667 x 2000 x 1000 cells: first-seen numbering takes the 64-bit-key form of the hash table; key order, which
    numbers through a rank map, refuses the grid at construction."""
    from spconv_amd.pytorch.utils import StaticPointToVoxel
    vsize_xyz = [0.003, 0.004, 0.004]
    gen = StaticPointToVoxel(vsize_xyz, RANGE, 4, 30000, 4, 20000, key_order=False, device=cuda)
    assert int(np.prod(np.asarray(gen.grid_size, dtype=np.int64))) > 2 ** 32
    pts = _cloud(20000, 5)
    pts[:10000, :3] = pts[10000:, :3] + 1e-4                          # several points per voxel
    rv, ri, rc, rpid = oracle.point2voxel(pts, gen.vsize, gen.coors_range, gen.grid_size, 30000, 4, True)
    found = oracle.point2voxel(pts, gen.vsize, gen.coors_range, gen.grid_size, 20000, 1, False)[1].shape[0]
    gen(torch.tensor(pts, device=cuda), empty_mean=True)
    ri = np.concatenate([np.zeros((ri.shape[0], 1), np.int32), ri], axis=1)
    _check(gen, (rv, ri, rc, rpid), 20000, found)
    with pytest.raises(ValueError, match="key_order"):
        StaticPointToVoxel(vsize_xyz, RANGE, 4, 30000, 4, 20000, key_order=True, device=cuda)
