"""GPU: voxel serialisation (csrc/serialize.hip) against the plain-Python restatement of tests/refserial.py.  Every
output is an integer or a moved row, so every comparison is exact (torch.equal, bit patterns for the feature rows)."""
import functools

import numpy as np
import pytest
import torch

import refserial as R

pytestmark = pytest.mark.gpu

ORDERS = ("z", "z-trans", "hilbert", "hilbert-trans")
# (ndim, depth, batch_size): keys within 32 bits (the existing sort), 36 bits (the LiDAR case), the full 63 bits, ...
GEOMETRIES = [(3, 4, 2), (3, 11, 4), (3, 16, 32767), (2, 16, 3), (1, 16, 3), (4, 15, 7)]
SIZES = [0, 1, 511, 512, 513, 5000]                 # the sort block is 512 entries


def F():
    import spconv_amd.pytorch.functional as fn
    return fn


def lib():
    from spconv_amd import _lib
    return _lib.load()


def unique_rows(ndim, depth, batch_size, n, seed, batches=None):
    """n index rows [batch, spatial...] without a repeated coordinate, in random order."""
    rng = np.random.default_rng(seed)
    batches = np.arange(batch_size) if batches is None else np.asarray(batches)
    side = 1 << depth
    cells = len(batches) * side ** ndim
    if cells < 1 << 20:
        flat = rng.choice(cells, n, replace=False)
    else:
        flat = np.unique(rng.integers(0, cells, 2 * n + 16, dtype=np.int64))
        rng.shuffle(flat)
        flat = flat[:n]
    assert len(flat) == n
    cols = []
    for _ in range(ndim):
        cols.append(flat % side)
        flat = flat // side
    return np.stack([batches[flat]] + cols[::-1], axis=1).astype(np.int32)


def kill(idx, depth, batch_size):
    """Rows 1, 2, 3 die by batch -1, a coordinate at 2^depth and batch = batch_size."""
    if idx.shape[0] >= 4:
        idx[1, 0] = -1
        idx[2, -1] = 1 << depth
        idx[3, 0] = batch_size
    return idx


@functools.lru_cache(maxsize=None)
def case(ndim, depth, batch_size, n, orders=ORDERS, axes=None, n_live=None, repeat=False, batches=None):
    """(index rows, the restatement's code / order / inverse / offsets): computed once, shared, left unchanged."""
    if repeat:          # coordinates drawn WITH repetition from a small corner of the grid
        rng = np.random.default_rng(7)
        idx = np.concatenate([rng.integers(0, batch_size, (n, 1)), rng.integers(0, 3, (n, ndim))], axis=1).astype(np.int32)
    else:
        idx = unique_rows(ndim, depth, batch_size, n, 1000 * ndim + depth, batches)
    idx = kill(idx, depth, batch_size)
    idx.setflags(write=False)
    return idx, R.serialize(idx, batch_size, depth, orders, axes, n_live)


def run(cuda, idx, batch_size, depth, orders=ORDERS, axes=None, n_live=None):
    nl = None if n_live is None else torch.tensor([n_live], dtype=torch.int32, device=cuda)
    return F().serialize(torch.from_numpy(np.array(idx)).to(cuda), None, batch_size, orders, depth=depth, axes=axes, n_live=nl)


def assert_serialization(ser, want, n):
    code, order, inverse, offsets = want
    assert ser.code.dtype == torch.int64 and ser.order.dtype == torch.int32 and ser.inverse.dtype == torch.int32
    assert torch.equal(ser.code.cpu(), torch.from_numpy(code))
    assert torch.equal(ser.order.cpu(), torch.from_numpy(order))
    assert torch.equal(ser.inverse.cpu(), torch.from_numpy(inverse))
    assert torch.equal(ser.offsets.cpu(), torch.from_numpy(offsets))
    for k in range(order.shape[0]):          # a full permutation whatever the restatement says
        assert sorted(ser.inverse[k].tolist()) == list(range(n))


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("ndim,depth,batch_size", GEOMETRIES)
def test_keys_and_orders(cuda, ndim, depth, batch_size, n):
    idx, want = case(ndim, depth, batch_size, n)
    ser = run(cuda, idx, batch_size, depth)
    assert ser.depth == depth and ser.orders == ORDERS
    assert_serialization(ser, want, n)
    if n >= 4:                               # the three killed rows come last, in ascending row
        assert (want[0][:, 1:4] == -1).all() and (want[1][:, -3:] == np.array([1, 2, 3])).all()


@pytest.mark.parametrize("ndim,depth,batch_size", [(3, 4, 2), (3, 11, 4)])
def test_repeated_coordinates_stay_in_ascending_row(cuda, ndim, depth, batch_size):
    idx, want = case(ndim, depth, batch_size, 1500, repeat=True)
    code, order = want[0], want[1]
    assert len(set(code[0].tolist())) < 120                      # (the case holds what it claims: long runs of equal keys)
    for k in range(4):
        for t in range(1, 1500):
            a, b = order[k][t - 1], order[k][t]
            assert code[k][a] != code[k][b] or a < b or code[k][a] == -1
    assert_serialization(run(cuda, idx, batch_size, depth), want, 1500)


@pytest.mark.parametrize("n", [513, 5000])
@pytest.mark.parametrize("ndim,depth,batch_size", [(3, 12, 1), (3, 12, 3), (2, 16, 20000)])
def test_key_widths_that_take_eight_bit_digits(cuda, ndim, depth, batch_size, n):
    """37, 38 and 47 key bits: five or six 8-bit digits where 9-bit ones save no pass, so a 512-entry block is two rounds
    of the 64-bit passes' 256 threads."""
    bits = R.key_bits(ndim, depth, batch_size)
    assert bits > 32 and (bits + 8) // 9 == (bits + 7) // 8
    idx, want = case(ndim, depth, batch_size, n)
    assert_serialization(run(cuda, idx, batch_size, depth), want, n)


def test_repeated_coordinates_with_eight_bit_digits(cuda):
    idx, want = case(3, 12, 3, 1500, repeat=True)
    assert len(set(want[0][0].tolist())) < 120
    assert_serialization(run(cuda, idx, 3, 12), want, 1500)


def test_axes_override(cuda):
    idx, want = case(3, 11, 4, 513, orders=("z", "hilbert-trans"), axes=(0, 2, 1))
    assert not np.array_equal(want[0], case(3, 11, 4, 513, orders=("z", "hilbert-trans"))[1][0])
    assert_serialization(run(cuda, idx, 4, 11, ("z", "hilbert-trans"), (0, 2, 1)), want, 513)


@pytest.mark.parametrize("ndim,depth,batch_size", [(3, 4, 4), (3, 11, 4)])
def test_dead_rows_live_count_and_an_empty_scene(cuda, ndim, depth, batch_size):
    n, n_live = 1000, 700
    idx, want = case(ndim, depth, batch_size, n, n_live=n_live, batches=(0, 2, 3))
    code, order, inverse, offsets = want
    dead = [i for i in range(n) if i >= n_live or i in (1, 2, 3)]
    assert offsets[2] == offsets[1] and offsets[-1] == n - len(dead)          # scene 1 is empty
    for k in range(4):
        assert order[k][n - len(dead):].tolist() == dead
    assert_serialization(run(cuda, idx, batch_size, depth, n_live=n_live), want, n)


def test_a_sparse_tensor_supplies_geometry_and_live_count(cuda):
    import spconv_amd.pytorch as spconv
    idx, want = case(3, 4, 4, 1000, n_live=700, batches=(0, 2, 3))
    x = spconv.SparseConvTensor(torch.zeros((1000, 4), device=cuda), torch.from_numpy(np.array(idx)).to(cuda), [16, 16, 16], 4)
    x.n_live_dev = torch.tensor([700], dtype=torch.int32, device=cuda)
    ser = F().serialize(x)
    assert ser.depth == 4
    assert_serialization(ser, want, 1000)


def test_launch_counters(cuda):
    idx, _ = case(3, 11, 4, 513)
    count = lambda key: lib().spx_launch_count(f"serialize/{key}".encode())
    before = {k: count(k) for k in ("keys", "sort", "offsets", "plan", "bwd")}
    assert min(before.values()) >= 0
    ser = run(cuda, idx, 4, 11)
    assert count("keys") == before["keys"] + 1 and count("sort") == before["sort"] + 4
    assert count("offsets") == before["offsets"] + 1
    F().patch_plan(ser, 8)
    assert count("plan") == before["plan"] + 1 and count("bwd") == before["bwd"]


# ------------------------------------------------------------------------------------------------ plan

def scenes_of(K):
    return [0, 1, K - 1, K, K + 1, 2 * K + 3]


@functools.lru_cache(maxsize=None)
def plan_case(K):
    """One batch with scenes of 0, 1, K - 1, K, K + 1 and 2 K + 3 rows, rows shuffled, three of them dead."""
    counts = scenes_of(K)
    rng = np.random.default_rng(K)
    rows = [unique_rows(3, 6, 1, c + (3 if b == 5 else 0), 50 + b) for b, c in enumerate(counts)]
    for b, r in enumerate(rows):
        r[:, 0] = b
    idx = np.concatenate(rows)
    idx[-3:, 0] = (-1, 6, 9)                                                    # dead rows
    idx = idx[rng.permutation(idx.shape[0])]
    idx.setflags(write=False)
    want = R.serialize(idx, 6, 6, ("hilbert", "z"))
    assert np.diff(want[3]).tolist() == counts
    return idx, want


@pytest.mark.parametrize("pad", ["mask", "borrow"])
@pytest.mark.parametrize("K", [1, 4, 48])
def test_patch_plan(cuda, K, pad):
    idx, want = plan_case(K)
    n = idx.shape[0]
    ser = run(cuda, idx, 6, 6, ("hilbert", "z"))
    assert_serialization(ser, want, n)
    for which in (0, 1):
        plan = F().patch_plan(ser, K, which=which, pad=pad)
        ref = R.patch_plan(want[1][which], want[3], K, pad)
        P_cap = n // K + 6
        assert plan.patch_rows.shape == (P_cap, K) and plan.patch_size == K and plan.pad == pad
        for name in ("patch_rows", "patch_rows_canon", "row_slot", "row_slot2", "patch_scene"):
            assert torch.equal(getattr(plan, name).cpu(), torch.from_numpy(ref[name])), name
        used = ref["n_patches"]
        assert used == sum((c + K - 1) // K for c in scenes_of(K)) and plan.n_patches_dev.tolist() == [used]
        assert bool((plan.patch_rows[used:] == -1).all()) and bool((plan.patch_scene[used:] == -1).all())
        if pad == "borrow" and K > 1:
            assert int((plan.row_slot2 >= 0).sum()) == sum((-c) % K for c in scenes_of(K) if c >= K) > 0
        else:
            assert bool((plan.row_slot2 == -1).all()) and torch.equal(plan.patch_rows, plan.patch_rows_canon)


def test_patch_plan_of_no_rows(cuda):
    ser = run(cuda, np.zeros((0, 4), dtype=np.int32), 3, 5, ("z",))
    assert ser.offsets.tolist() == [0, 0, 0, 0]
    plan = F().patch_plan(ser, 4)
    assert plan.patch_rows.shape == (3, 4) and bool((plan.patch_rows == -1).all()) and plan.n_patches_dev.tolist() == [0]
    assert plan.row_slot.shape == (0,) and bool((plan.patch_scene == -1).all())


# ------------------------------------------------------------------------------------------------ row moves

DTYPES = {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32}


def bits(t):
    return t.contiguous().view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()]).cpu()


@pytest.fixture(scope="module")
def moved(cuda):
    idx, _ = plan_case(4)
    ser = run(cuda, idx, 6, 6, ("hilbert",))
    plan = F().patch_plan(ser, 4, pad="borrow")
    assert int((plan.row_slot2 >= 0).sum()) > 0 and int((plan.row_slot < 0).sum()) == 3
    return plan


def take(src, rows):
    """src[rows] with zeros where rows < 0: index arithmetic on the host."""
    src, rows = src.cpu(), rows.cpu().long()
    out = src[rows.clamp(min=0)]
    out[rows < 0] = 0
    return out


@pytest.mark.parametrize("name", sorted(DTYPES))
@pytest.mark.parametrize("C", [1, 3, 16, 64])
def test_rows_to_patches_and_back(cuda, moved, C, name):
    plan, dtype = moved, DTYPES[name]
    n, (P_cap, K) = plan.row_slot.shape[0], plan.patch_rows.shape
    torch.manual_seed(C)
    feat = torch.randn((n, C), device=cuda).to(dtype).requires_grad_(True)
    before = lib().spx_launch_count(b"serialize/bwd")
    patches = F().rows_to_patches(feat, plan)
    assert patches.shape == (P_cap, K, C) and patches.dtype == dtype
    assert torch.equal(bits(patches), bits(take(feat.detach(), plan.patch_rows.reshape(-1)).reshape(P_cap, K, C)))
    g = torch.randn((P_cap, K, C), device=cuda).to(dtype)
    patches.backward(g)
    assert lib().spx_launch_count(b"serialize/bwd") == before + 1
    flat = g.reshape(P_cap * K, C)
    a, b = take(flat, plan.row_slot), take(flat, plan.row_slot2)
    two = (plan.row_slot2 >= 0).cpu()
    want = torch.where(two[:, None], (a.float() + b.float()).to(dtype), a)      # rounded once; one term keeps its bits
    assert torch.equal(bits(feat.grad), bits(want))
    # and back: every live row reads its canonical slot, the gradient goes to canonical slots only
    src = torch.randn((P_cap, K, C), device=cuda).to(dtype).requires_grad_(True)
    rows = F().patches_to_rows(src, plan)
    assert rows.shape == (n, C) and torch.equal(bits(rows), bits(take(src.detach().reshape(P_cap * K, C), plan.row_slot)))
    g_rows = torch.randn((n, C), device=cuda).to(dtype)
    rows.backward(g_rows)
    assert torch.equal(bits(src.grad), bits(take(g_rows, plan.patch_rows_canon.reshape(-1)).reshape(P_cap, K, C)))
    # the round trip gives every live row back and zeros for the dead ones
    own = torch.where(plan.row_slot >= 0, torch.arange(n, device=cuda), torch.full((n,), -1, device=cuda))
    assert torch.equal(bits(F().patches_to_rows(patches.detach(), plan)), bits(take(feat.detach(), own)))


@pytest.mark.parametrize("name", sorted(DTYPES))
@pytest.mark.parametrize("amp", [torch.float16, torch.bfloat16])
def test_row_moves_under_autocast_keep_dtype_and_bits(cuda, moved, amp, name):
    """Mixed-precision training: inside torch.autocast both moves run forward and backward, cast nothing and give the
    bits they give outside it."""
    plan, dtype, C = moved, DTYPES[name], 16
    n, (P_cap, K) = plan.row_slot.shape[0], plan.patch_rows.shape
    torch.manual_seed(5)
    feat0 = torch.randn((n, C), device=cuda).to(dtype)
    g_rows = torch.randn((n, C), device=cuda).to(dtype)

    def both(f):
        patches = F().rows_to_patches(f, plan)
        rows = F().patches_to_rows(patches, plan)
        rows.backward(g_rows)
        return patches.detach(), rows.detach(), f.grad

    plain = both(feat0.clone().requires_grad_(True))
    with torch.autocast("cuda", dtype=amp):
        cast = both(feat0.clone().requires_grad_(True))
    for a, b in zip(cast, plain):
        assert a.dtype == dtype and a.shape == b.shape and torch.equal(bits(a), bits(b))
    assert cast[0].shape == (P_cap, K, C) and int((cast[2] != 0).any(dim=1).sum()) == n - 3


def test_gradcheck_float64(cuda):
    idx = unique_rows(3, 5, 3, 40, 3)
    idx[5, 0] = -1
    ser = run(cuda, idx, 3, 5, ("hilbert-trans",))
    plan = F().patch_plan(ser, 6, pad="borrow")
    assert int((plan.row_slot2 >= 0).sum()) > 0
    torch.manual_seed(1)
    feat = torch.randn((40, 3), dtype=torch.float64, device=cuda, requires_grad=True)
    assert torch.autograd.gradcheck(lambda f: F().rows_to_patches(f, plan), (feat,), eps=1e-6, atol=1e-9, rtol=1e-7)
    patches = torch.randn((plan.patch_rows.shape[0], 6, 3), dtype=torch.float64, device=cuda, requires_grad=True)
    assert torch.autograd.gradcheck(lambda p: F().patches_to_rows(p, plan), (patches,), eps=1e-6, atol=1e-9, rtol=1e-7)
    assert torch.autograd.gradcheck(lambda f: F().patches_to_rows(F().rows_to_patches(f, plan) * 2.0, plan), (feat,),
                                    eps=1e-6, atol=1e-9, rtol=1e-7)


# ------------------------------------------------------------------------------------------------ capture

@pytest.mark.parametrize("depth", [7, 11, 12])      # keys of 23 bits (the 32-bit sort), 35 (9-bit digits) and 38 (8-bit)
def test_capture_serialize_plan_attention_and_back_in_one_graph(cuda, depth):
    """serialize -> plan -> rows_to_patches -> softmax(Q K^T) V with a mask from patch_rows >= 0 -> patches_to_rows in one
    graph, replayed on a scene of another live count in the same padded buffers."""
    cap, B, C, K = 3000, 3, 16, 32
    scenes = []
    for seed, live in ((11, 3000), (12, 1100)):
        torch.manual_seed(seed)
        scenes.append((torch.from_numpy(unique_rows(3, 7, B, cap, seed)).to(cuda), torch.randn((cap, C), device=cuda).half(),
                       live))
    idx_buf = torch.empty((cap, 4), dtype=torch.int32, device=cuda)
    feat_buf = torch.empty((cap, C), dtype=torch.float16, device=cuda)
    n_live = torch.zeros((1,), dtype=torch.int32, device=cuda)

    def load(k):
        idx_buf.copy_(scenes[k][0])
        feat_buf.copy_(scenes[k][1])
        n_live.fill_(scenes[k][2])

    def block():
        ser = F().serialize(idx_buf, [100, 128, 128], B, orders=("hilbert", "z"), depth=depth, n_live=n_live)
        plan = F().patch_plan(ser, K, which=0, pad="borrow")
        x = F().rows_to_patches(feat_buf, plan).float()
        score = torch.bmm(x, x.transpose(1, 2)) / C ** 0.5
        score = score.masked_fill((plan.patch_rows < 0)[:, None, :], -1e30)
        y = torch.bmm(torch.softmax(score, dim=-1), x).half()
        return ser, plan, F().patches_to_rows(y, plan)

    eager = []
    with torch.no_grad():
        for k in (0, 1):
            load(k)
            ser, plan, out = block()
            eager.append((ser.order.clone(), plan.patch_rows.clone(), plan.n_patches_dev.clone(), out.clone()))
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            ser, plan, out = block()
    assert ser.depth == depth and eager[0][2].item() > eager[1][2].item() > 30
    assert bool((eager[1][3][1100:] == 0).all()) and int((eager[1][3][:1100] != 0).any(dim=1).sum()) > 1000
    for k in (1, 0, 1):
        load(k)
        graph.replay()
        torch.cuda.synchronize()
        order, patch_rows, n_patches, want = eager[k]
        assert torch.equal(ser.order, order) and torch.equal(plan.patch_rows, patch_rows)
        assert torch.equal(plan.n_patches_dev, n_patches) and torch.equal(bits(out), bits(want))
