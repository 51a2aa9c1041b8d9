"""GPU: the sparse-class hint of the 16-bit gather-GEMM launches (SPX_SPARSE_ROWS_HINT, include/spconv_amd.h).

Once the host has READ {class 1, M} of a rows layout, forward, dgrad and the fused backward launch exactly the appendix
workgroups that receive rows under the dealing rule, and those workgroups take M from their arguments.  The hint is a
launch shape only:

* hinted and unhinted launches over the same rulebook are bit-identical (and equal the oracle within the bars of util),
  at every edge of the dealing rule -- an empty appendix, an M that is no multiple of a block, M on either side of the
  fused backward's budget of kAppBudget = 64 whole tiles;
* the hint is given when, and only when, the header of this very blob has been read and says class 1: never for a
  class-0 rulebook, a rulebook built inside a capture, or an M beyond the bits of the word;
* the BatchNorm statistics out of the forward's epilogue are the same records, in a shorter list.

M of every scene is counted on the CPU from the coordinates and compared with the blob's header before it is relied on.
The unhinted launch of a test is the same call over a clone of the blob: the knowledge lives on the tensor object.
"""
import numpy as np
import pytest
import torch

import oracle
from util import assert_close_abs_sum, gpu_rulebook, oracle_rulebook, rel_err, scene

pytestmark = pytest.mark.gpu

K3, ONE = [3] * 3, [1] * 3
K_APP_BUDGET = 64                     # csrc/igemm_defs.h: kAppBudget
TOL = {torch.float16: 2e-3, torch.bfloat16: 1.2e-2}      # the norm-wise bars of test_gpu_conv


def rows_with_neighbour(idx: np.ndarray, shape) -> int:
    """M on the CPU: voxels with at least one of their 26 neighbours in the scene (distinct coordinates)."""
    pad = [s + 2 for s in shape]
    c = idx[:, 1:].astype(np.int64) + 1
    key = idx[:, 0].astype(np.int64) * int(np.prod(pad)) + np.ravel_multi_index((c[:, 0], c[:, 1], c[:, 2]), pad)
    srt = np.sort(key)
    has = np.zeros(idx.shape[0], dtype=bool)
    for dz in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                if dz == dy == dx == 0:
                    continue
                q = key + (dz * pad[1] + dy) * pad[2] + dx
                p = np.searchsorted(srt, q)
                p[p >= srt.shape[0]] = 0
                has |= srt[p] == q
    return int(has.sum())


def lattice_scene(shape, n, seed):
    """n distinct voxels on the stride-2 lattice of `shape`: nobody has a neighbour."""
    return scene([s // 2 for s in shape], n, 1, seed) * np.array([1, 2, 2, 2], dtype=np.int32)


def _counts():
    from spconv_amd import _lib
    return tuple(_lib.launch_counts(("sparse_hint/v4", "sparse_hint/bwd", "igemm_v4", "igemm_bwd")).values())


def _delta(before):
    return tuple(a - b for a, b in zip(_counts(), before))


def _operands(rb, C, K, dtype, seed, cuda):
    g = torch.Generator(device="cpu").manual_seed(seed)
    f = (torch.rand((rb.n_in, C), generator=g) * 2 - 1).to(dtype)
    w = (torch.rand((K, 3, 3, 3, C), generator=g) * 2 - 1).to(dtype)
    d = ((torch.rand((rb.n_out, K), generator=g) * 2 - 1) * 0.2).to(dtype)
    return f, w, d, f.to(cuda), w.to(cuda), d.to(cuda)


def _read_rulebook(idx, shape, m_cpu):
    """A rulebook with a rows layout whose header the host has read: (rb, pair, mask, blob, tile_order)."""
    from spconv_amd.pytorch import ops
    rb, _ = gpu_rulebook(idx, 1, shape, K3, ONE, ONE, ONE, True, do_sort="layout")
    assert rb.layout is not None
    head = rb.layout[:2].cpu().tolist()
    assert head[1] == m_cpu, f"the blob counts {head[1]} rows with a neighbour, the coordinates give {m_cpu}"
    pair, mask, blob, to = ops.tables_of(rb, "fwd", 64)       # (polls the class word: the build has been waited for)
    assert to == 2 and blob is rb.layout
    return rb, pair, mask, blob, to, head[0]


def _three(ops, fg, wg, dg, rb, pair, mask, blob, to, fused=True):
    """forward, dgrad and (where the width has one) the fused backward of one layer over `blob`"""
    out = ops.igemm_fwd(fg, wg, pair, mask, blob, rb.n_out, 13, tile_order=to)
    din = ops.igemm_dgrad(dg, wg, pair, mask, blob, rb.n_in, True, tile_order=to)
    bw = ops.igemm_bwd(fg, dg, wg, pair, mask, blob, rb.pair_native, rb.num_per_loc, True, ops._plan_of(rb),
                       tile_order=to) if fused else None
    torch.cuda.synchronize()
    return out, din, bw


@pytest.fixture(scope="module")
def sparse_rulebook(cuda):
    shape = [40, 1280, 1600]
    idx = scene(shape, 40_000, 1, 3)
    m = rows_with_neighbour(idx, shape)
    assert m == 561 and m % 16 and m % 32 and m % 64
    return _read_rulebook(idx, shape, m) + (m,)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("width", [64, 16, 128])
def test_hinted_launches_are_bit_identical(cuda, sparse_rulebook, width, dtype):
    """(a) C = K = 64, a narrow width (offset packing) and a wide one (64-row tiles, two waves per SIMD)."""
    from spconv_amd.pytorch import ops
    rb, pair, mask, blob, to, cls, m = sparse_rulebook
    assert cls == 1 and blob._spx_class == 1 and blob._spx_heavy == m
    _, _, _, fg, wg, dg = _operands(rb, width, width, dtype, 5, cuda)
    before = _counts()
    out_h, din_h, bw_h = _three(ops, fg, wg, dg, rb, pair, mask, blob, to)
    hv4, hbwd, v4, bwd = _delta(before)
    assert (hv4, hbwd) == (2, 1) and v4 == 2 and bwd == 1, "forward, dgrad and the fused backward take the hint"
    plain = blob.clone()
    before = _counts()
    out_p, din_p, bw_p = _three(ops, fg, wg, dg, rb, pair, mask, plain, to)
    hv4, hbwd, v4, bwd = _delta(before)
    assert (hv4, hbwd) == (0, 0) and v4 == 2 and bwd == 1, "a blob nobody has read gets today's launches"
    assert torch.equal(out_h, out_p) and torch.equal(din_h, din_p)
    assert torch.equal(bw_h[0], bw_p[0]) and torch.equal(bw_h[1], bw_p[1]) and torch.equal(bw_h[0], din_h)


def _check_oracle(got, idx, shape, f, w, d, dtype):
    ref = oracle_rulebook(idx, 1, shape, K3, ONE, ONE, ONE, True)
    f32, w32, d32 = f.float(), w.float(), d.float()
    out_ref = oracle.indice_conv(f32, w32, ref["pair"], ref["num"], ref["n_out"], subm=True)
    din_ref, dw_ref = oracle.indice_conv_backward(f32, w32, d32, ref["pair"], ref["num"], subm=True)
    oa = oracle.indice_conv(f32.abs(), w32.abs(), ref["pair"], ref["num"], ref["n_out"], subm=True)
    dia, dwa = oracle.indice_conv_backward(f32.abs(), w32.abs(), d32.abs(), ref["pair"], ref["num"], subm=True)
    for name, g, r, a in zip(("out", "din", "dw"), got, (out_ref, din_ref, dw_ref), (oa, dia, dwa)):
        g = g.float().cpu().numpy()
        e = rel_err(g, r.numpy())
        assert e <= TOL[dtype], f"{name}: rel err {e:.3e}"
        assert_close_abs_sum(g, r.numpy(), a.numpy(), dtype, 1e-6, name=name)


@pytest.mark.parametrize("n,shape,seed,m_want,note", [
    (33_000, [40, 1280, 1600], 3, 299, "a few 16-row blocks, ragged: no multiple of 16, 32 or 64"),
    (48_000, [40, 402, 404], 5, 8173, "just below kAppBudget whole tiles"),
    (48_000, [40, 404, 404], 5, 8200, "just above: more than kAppBudget workgroups have rows in the fused backward"),
    (48_000, [40, 364, 364], 5, 10030, "well above, still below n / 4"),
])
def test_edges_of_the_dealing_rule(cuda, n, shape, seed, m_want, note):
    """(b) hinted == unhinted == oracle on either side of every threshold of the rule."""
    from spconv_amd.pytorch import ops
    idx = scene(shape, n, 1, seed)
    m = rows_with_neighbour(idx, shape)
    assert m == m_want and 4 * m < n and m % 16 and m % 32 and m % 64, (m, note)
    assert (m > K_APP_BUDGET * 128) == (m_want > 8192)
    rb, pair, mask, blob, to, cls = _read_rulebook(idx, shape, m)
    assert cls == 1 and blob._spx_class == 1 and blob._spx_heavy == m
    f, w, d, fg, wg, dg = _operands(rb, 64, 64, torch.float16, 6, cuda)
    before = _counts()
    out_h, din_h, bw_h = _three(ops, fg, wg, dg, rb, pair, mask, blob, to)
    assert _delta(before)[:2] == (2, 1)
    out_p, din_p, bw_p = _three(ops, fg, wg, dg, rb, pair, mask, blob.clone(), to)
    assert torch.equal(out_h, out_p) and torch.equal(din_h, din_p)
    assert torch.equal(bw_h[0], bw_p[0]) and torch.equal(bw_h[1], bw_p[1]) and torch.equal(bw_h[0], din_h)
    _check_oracle((out_h, bw_h[0], bw_h[1]), idx, shape, f, w, d, torch.float16)


def test_empty_appendix(cuda):
    """(b) M = 0.  The builder gives a rulebook nobody of whose rows has a neighbour class 0 (rowsort.hip: class 1 needs
    0 < 4 M < n), so it never hints it; the class-1 blob with an empty appendix that the ABI allows is that blob with its
    class word set -- word for word (no main mask word is zeroed when no row moves).  Its header is then read like any
    other, and the hinted launch holds no appendix workgroup at all."""
    from spconv_amd.pytorch import ops
    shape = [40, 800, 800]
    idx = lattice_scene(shape, 33_000, 4)
    assert rows_with_neighbour(idx, shape) == 0
    rb, pair, mask, blob, to, cls = _read_rulebook(idx, shape, 0)
    assert cls == 0 and blob._spx_class == 0
    f, w, d, fg, wg, dg = _operands(rb, 64, 64, torch.float16, 7, cuda)
    before = _counts()
    out_0, din_0, bw_0 = _three(ops, fg, wg, dg, rb, pair, mask, blob, to)
    assert _delta(before)[:2] == (0, 0), "the builder's class-0 blob takes no sparse hint"
    empty = blob.clone()
    empty[0] = 1
    head = empty[:2].cpu().tolist()
    assert head == [1, 0]
    empty._spx_class, empty._spx_heavy = head                   # what _set_class leaves after a read
    before = _counts()
    out_h, din_h, bw_h = _three(ops, fg, wg, dg, rb, pair, mask, empty, to)
    assert _delta(before)[:2] == (2, 1)
    unread = empty.clone()
    out_p, din_p, bw_p = _three(ops, fg, wg, dg, rb, pair, mask, unread, to)
    for a, b, c in ((out_h, out_p, out_0), (din_h, din_p, din_0), (bw_h[0], bw_p[0], bw_0[0]), (bw_h[1], bw_p[1], bw_0[1])):
        assert torch.equal(a, b) and torch.equal(a, c)
    _check_oracle((out_h, bw_h[0], bw_h[1]), idx, shape, f, w, d, torch.float16)


def test_no_hint_for_a_class_0_rulebook(cuda):
    """(c) a LiDAR-like rulebook: class 0 has been read, no sparse hint reaches the driver, results as over row order."""
    from spconv_amd.pytorch import ops
    from spconv_amd.utils import synthetic
    shape = [40, 1280, 1600]
    idx = synthetic.lidar_like_scene(shape, 40_000, 1, 2)
    m = rows_with_neighbour(idx, shape)
    assert 4 * m >= idx.shape[0]
    rb, pair, mask, blob, to, cls = _read_rulebook(idx, shape, m)
    assert cls == 0 and blob._spx_class == 0 and ops.split_tile_order(ops._with_hints(to, blob))[2] is None
    _, _, _, fg, wg, dg = _operands(rb, 64, 64, torch.float16, 8, cuda)
    before = _counts()
    out, din, bw = _three(ops, fg, wg, dg, rb, pair, mask, blob, to)
    assert _delta(before)[:2] == (0, 0)
    assert torch.equal(out, ops.igemm_fwd(fg, wg, rb.pair_fwd, rb.mask_fwd, None, rb.n_out, 13))
    assert torch.equal(din, ops.igemm_dgrad(dg, wg, rb.pair_fwd, rb.mask_fwd, None, rb.n_in, True))
    assert torch.equal(bw[0], din)


def test_no_hint_for_an_m_beyond_the_bits(cuda, sparse_rulebook):
    """(c) an M that does not fit the word travels as no hint: the launch is today's, whatever the tensor claims."""
    from spconv_amd.pytorch import _rulebook, ops
    rb, pair, mask, blob, to, cls, m = sparse_rulebook
    big = _rulebook._SPARSE_ROWS_MAX + 1
    assert ops.sparse_rows_hint(to, big) == to and ops.sparse_rows_hint(to, -1) == to and ops.sparse_rows_hint(to, None) == to
    claim = blob.clone()
    claim._spx_class, claim._spx_heavy = 1, big
    assert ops._with_sparse_hint(to, claim) == to and ops._with_hints(to, claim) == to
    _, _, _, fg, wg, dg = _operands(rb, 64, 64, torch.float16, 9, cuda)
    before = _counts()
    out, din, bw = _three(ops, fg, wg, dg, rb, pair, mask, claim, to)
    assert _delta(before)[:2] == (0, 0)
    out_h, din_h, bw_h = _three(ops, fg, wg, dg, rb, pair, mask, blob, to)
    assert torch.equal(out, out_h) and torch.equal(din, din_h) and torch.equal(bw[1], bw_h[1])


def test_no_hint_for_a_rulebook_built_inside_a_capture(cuda):
    """(c) nothing is polled inside a capture: a rulebook built there carries no class, and neither its captured launches
    nor their replays take the hint; the values are those of an eager pass."""
    import spconv_amd.pytorch as spconv
    shape = [40, 1280, 1600]
    idx = scene(shape, 40_000, 1, 3)
    net = spconv.SubMConv3d(64, 64, 3, bias=False, indice_key="g").to(cuda).half()
    g = torch.Generator(device="cpu").manual_seed(3)
    feats = (torch.rand((idx.shape[0], 64), generator=g) * 2 - 1).to(cuda).half()
    ind = torch.from_numpy(idx).to(cuda)

    def run():
        with torch.no_grad():
            return net(spconv.SparseConvTensor(feats, ind, shape, 1))

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    before = _counts()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y = run()
    graph.replay()
    torch.cuda.synchronize()
    hv4, hbwd, v4, _ = _delta(before)
    assert (hv4, hbwd) == (0, 0) and v4 == 1
    blob = y.indice_dict["g"].rulebook.layout
    assert blob is not None and getattr(blob, "_spx_class", None) is None
    assert int(blob[0].item()) == 1
    ref = run()
    assert torch.equal(y.features, ref.features)


def test_hint_known_before_a_capture_shapes_the_captured_launch(cuda, sparse_rulebook):
    """What was read before the capture is what the captured launch is shaped by: the benchmark's and a training loop's
    reuse of a rulebook through indice_key."""
    from spconv_amd.pytorch import ops
    rb, pair, mask, blob, to, cls, m = sparse_rulebook
    _, _, _, fg, wg, dg = _operands(rb, 64, 64, torch.float16, 10, cuda)
    want = ops.igemm_fwd(fg, wg, pair, mask, blob.clone(), rb.n_out, 13, tile_order=to)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.igemm_fwd(fg, wg, pair, mask, blob, rb.n_out, 13, tile_order=to)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    before = _counts()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = ops.igemm_fwd(fg, wg, pair, mask, blob, rb.n_out, 13, tile_order=to)
    assert _delta(before)[:3] == (1, 0, 1)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(got, want)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_bn_statistics_are_the_same_records(cuda, sparse_rulebook, dtype):
    """(d) spx_igemm_fwd_stats: every tile leaves the same {rows, mean, M2} record, bit for bit; the hinted launch reports
    fewer workgroups (the appendix workgroups without rows are gone) and, with fewer workgroups ahead of them, hands the
    main tiles to its workgroups in another order -- the records are compared as a set."""
    from spconv_amd.pytorch import ops
    rb, pair, mask, blob, to, cls, m = sparse_rulebook
    K = 64
    _, _, _, fg, wg, _ = _operands(rb, 64, K, dtype, 11, cuda)

    def stats(b):
        with ops.collect_bn_stats() as sink:
            out = ops.igemm_fwd(fg, wg, pair, mask, b, rb.n_out, 13, tile_order=to)
        torch.cuda.synchronize()
        assert sink.records is not None and sink.count > 0 and sink.channels == K and sink.rows == rb.n_out
        return out, sink.count, sink.records[:3 * K * sink.count].view(3, K, sink.count).cpu().numpy()

    before = _counts()
    out_h, cnt_h, rec_h = stats(blob)
    assert _delta(before)[:3] == (1, 0, 1)
    out_p, cnt_p, rec_p = stats(blob.clone())
    assert torch.equal(out_h, out_p)
    tiles = -(-rb.n_out // 128)
    h = min(128, (-(-m // (-(-(rb.n_out // 4) // 128))) + 15) // 16 * 16)      # the dealing rule: rows per appendix workgroup
    assert cnt_p == tiles + -(-(rb.n_out // 4) // 128) and cnt_h == tiles + -(-m // h) and cnt_h < cnt_p
    live_h, live_p = rec_h[0, 0] > 0, rec_p[0, 0] > 0
    assert live_h.sum() == live_p.sum() and int(rec_h[0, 0].sum()) == rb.n_out == int(rec_p[0, 0].sum())
    assert not rec_h[:, :, ~live_h].any() and not rec_p[:, :, ~live_p].any()

    def as_set(rec, live):          # one row per workgroup, in an order that does not depend on the workgroup's number
        rows = rec[:, :, live].reshape(3 * K, -1).T
        return rows[np.lexsort(rows.T[::-1])]
    np.testing.assert_array_equal(as_set(rec_h, live_h), as_set(rec_p, live_p))
