"""GPU: no rulebook build writes outside the bytes its workspace size query asked for.

Every builder carves its scratch arrays out of one caller buffer whose size comes from a `_ws_bytes` query (csrc/
rulebook_subm.hip, rulebook_conv.hip, rulebook_sorted.hip, rulebook_lists.hip: one carve function per workspace serves
the query and the build).  Here the buffer the build receives is the head of a larger tensor full of 0xA5: an array the
query forgot, or sized too small, lands in the tail the test owns -- nothing faults -- and the tail is no longer 0xA5.
The tables are compared with refrulebook.py as well (bit for bit, as in test_gpu_rulebook_matrix.py), so a carve whose
arrays overlap each other shows too.

One scene: 2500 rows of one batch item (dense_box) -- more than one 2048-entry block of the list passes, ten 256-row
groups, both with a ragged tail -- and one run at a single row."""
import contextlib
import functools
import types

import numpy as np
import pytest
import torch

import refrulebook
from test_gpu_rulebook_matrix import SUBM_KERNELS, counters, dense_box, ran
from test_gpu_sorted import _check_renumbered, _keys
from util import assert_rulebook_equal, gpu_rulebook, to_np

pytestmark = pytest.mark.gpu

N = 2500
DEFAULTS = {"SPX_SUBM_PROBE": 5, "SPX_SUBM_MASK_PASS": -1, "SPX_CONV_V": 3, "SPX_SUBM_RANK_ROWS": -1}
K3S2 = ([3] * 3, [2] * 3, [1] * 3, [1] * 3)          # ksize, stride, padding, dilation


@contextlib.contextmanager
def options(**values):
    from spconv_amd import _lib
    L = _lib.load()
    assert set(values) <= set(DEFAULTS)
    try:
        for name, v in values.items():
            _lib.check(L.spx_set_option(name.encode(), int(v)))
        yield
    finally:
        for name in values:
            _lib.check(L.spx_set_option(name.encode(), DEFAULTS[name]))


@pytest.fixture
def guard(monkeypatch):
    """Every workspace of the test is the first max(nbytes, 16) bytes of a tensor of 2 * that + 4096 bytes of 0xA5; the
    returned check synchronises and asserts that the bytes behind every view handed out are untouched, and returns how
    many workspaces were asked for."""
    from spconv_amd.pytorch import _rulebook
    held = []

    def ws(nbytes, device):
        size = max(int(nbytes), 16)
        whole = torch.full((2 * size + 4096,), 0xA5, dtype=torch.uint8, device=device)
        held.append((whole, size))
        return whole[:size]

    def check():
        torch.cuda.synchronize()
        for whole, size in held:
            tail = whole[size:]
            assert tail.numel() == size + 4096
            bad = int((tail != 0xA5).sum())
            assert bad == 0, f"{bad} bytes written behind a workspace of {size} bytes"
        n = len(held)
        held.clear()
        return n

    monkeypatch.setattr(_rulebook, "_ws", ws)
    return check


@functools.lru_cache(maxsize=None)
def the_scene(n=N):
    idx, bs, shape = dense_box(3, N, seed=N % 97)
    return np.ascontiguousarray(idx[:n]), bs, shape          # (nobody writes to it)


def frozen(ref):
    for a in ref.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return ref


@functools.lru_cache(maxsize=None)
def subm_ref(kernel, n=N):
    idx, bs, shape = the_scene(n)
    ksize, dil = SUBM_KERNELS[kernel]
    pad = [(k // 2) * d for k, d in zip(ksize, dil)]
    return frozen(refrulebook.rulebook(idx, bs, shape, ksize, [1] * 3, pad, dil, True))


@functools.lru_cache(maxsize=None)
def conv_ref(transposed=False, n=N):
    idx, bs, shape = the_scene(n)
    return frozen(refrulebook.rulebook(idx, bs, shape, *K3S2, False, transposed, [1] * 3 if transposed else None))


def build_subm(kernel, native, n=N):
    idx, bs, shape = the_scene(n)
    ksize, dil = SUBM_KERNELS[kernel]
    pad = [(k // 2) * d for k, d in zip(ksize, dil)]
    rb, _ = gpu_rulebook(idx, bs, shape, ksize, [1] * 3, pad, dil, True, need_bwd_table=True, need_native=native)
    return rb


def test_the_guard_sees_a_byte_behind_the_view(cuda, guard):
    """The fixture itself: the last byte of the tail, written through the whole tensor, fails the check."""
    from spconv_amd.pytorch import _rulebook
    ws = _rulebook._ws(1000, torch.device("cuda:0"))
    assert ws.numel() == 1000 and guard() == 1
    ws = _rulebook._ws(1000, torch.device("cuda:0"))
    ws._base[2 * 1000 + 4096 - 1] = 0
    with pytest.raises(AssertionError, match="1 bytes written behind"):
        guard()


# -------------------------------------------------------------------------------------------------------------- SubM
@pytest.mark.parametrize("probe", [5, 4])
@pytest.mark.parametrize("native", [True, False], ids=["native", "tables"])
def test_subm_hash_build_stays_inside_its_workspace(cuda, guard, probe, native):
    with options(SPX_SUBM_PROBE=probe):
        before = counters()
        rb = build_subm("k27", native)
        ran(before, **{f"subm_probe{probe}": 1, "subm_lists": int(native)})
    assert guard() == 1
    assert_rulebook_equal(rb, subm_ref("k27"), True)


@pytest.mark.parametrize("kernel", ["k1", "k175"])
def test_subm_first_form_stays_inside_its_workspace(cuda, guard, kernel):
    """One offset, and more than 128: the first form, lists by count -> scan -> scatter (launch_native_lists)."""
    before = counters()
    rb = build_subm(kernel, True)
    ran(before, subm_probe3=1, native_lists_v1=int(kernel != "k1"))
    assert guard() == 1
    assert_rulebook_equal(rb, subm_ref(kernel), True)


def test_one_row_stays_inside_its_workspace(cuda, guard):
    """A single row: every array of the carves at its smallest (a table of 512 slots takes the fourth probe form)."""
    idx, bs, shape = the_scene(1)
    before = counters()
    rb = build_subm("k27", True, n=1)
    ran(before, subm_probe4=1, subm_lists=1)
    assert guard() == 1
    assert_rulebook_equal(rb, subm_ref("k27", 1), True)
    before = counters()
    rb, _ = gpu_rulebook(idx, bs, shape, *K3S2, False)
    ran(before, sized_by_history=True, conv3__8=2, conv3_shares__8=2)
    assert guard() == 1
    assert_rulebook_equal(rb, conv_ref(False, 1), False)


def ranked_subm(ind, bs, shape, rows, form):
    """SubM k27 with lists over the rank map `ind` carries; no pass of the hash build may run."""
    from spconv_amd.pytorch import ops
    assert ops._rankmap_of(ind, bs, shape, ind.shape[0], 27) is not None
    with options(SPX_SUBM_RANK_ROWS=form):
        before = counters()
        rb = ops.build_rulebook(ind, bs, list(shape), [3] * 3, [1] * 3, [1] * 3, [1] * 3, [0] * 3, True,
                                need_bwd_table=True)[0]
        ran(before)
    ref = refrulebook.rulebook(rows, bs, shape, [3] * 3, [1] * 3, [1] * 3, [1] * 3, True)
    assert ref["num"].sum() > rows.shape[0]
    return rb, ref


@pytest.mark.parametrize("form", [1, 0], ids=["rows", "probe"])
def test_subm_behind_a_sorted_build_stays_inside_its_workspace(cuda, guard, form):
    idx, bs, shape = the_scene()
    rs, out_shape = gpu_rulebook(idx, bs, shape, *K3S2, False, out_order="sorted")
    assert guard() == 1
    rb, ref = ranked_subm(rs.out_indices, bs, out_shape, to_np(rs.out_indices), form)
    assert guard() == 1
    assert_rulebook_equal(rb, ref, True)


@pytest.mark.parametrize("form", [1, 0], ids=["rows", "probe"])
def test_subm_over_a_level_in_key_order_stays_inside_its_workspace(cuda, guard, form):
    """The scene's own 2500 rows in key order with their rank map attached (the level a sorted build leaves behind has
    fewer than 2048 rows): the ranked build across more than one block of the list pass."""
    from spconv_amd.pytorch import ops
    idx, bs, shape = the_scene()
    rows = np.ascontiguousarray(idx[np.argsort(_keys(idx, shape), kind="stable")])
    ind = torch.from_numpy(rows).to("cuda:0")
    ops.attach_rank_map(ind, bs, shape)
    rb, ref = ranked_subm(ind, bs, shape, rows, form)
    assert guard() == 1
    assert_rulebook_equal(rb, ref, True)


# ------------------------------------------------------------------------------------------------------- convolution
@pytest.mark.parametrize("gen", [3, 2])
@pytest.mark.parametrize("static", [False, True], ids=["two_call", "static"])
def test_first_seen_build_stays_inside_its_workspace(cuda, guard, static, gen):
    idx, bs, shape = the_scene()
    ref = conv_ref()
    kw = dict(static_num_out=ref["n_out"]) if static else {}          # (a bound equal to the count: every row is live)
    with options(SPX_CONV_V=gen):
        before = counters()
        rb, _ = gpu_rulebook(idx, bs, shape, *K3S2, False, **kw)
        ran(before, sized_by_history=True, **({"conv3__8": 2, "conv3_shares__8": 2} if gen == 3 else {"conv_generic": 2}))
    assert guard() == 1
    if static:
        assert to_np(rb.n_out_dev).tolist() == [ref["n_out"], 0]
    assert_rulebook_equal(rb, ref, False)


def test_transposed_build_stays_inside_its_workspace(cuda, guard):
    idx, bs, shape = the_scene()
    before = counters()
    rb, out_shape = gpu_rulebook(idx, bs, shape, *K3S2, False, True, [1] * 3)
    ran(before, sized_by_history=True, conv_generic=2)
    assert guard() == 1
    ref = conv_ref(True)
    assert list(out_shape) == list(ref["out_shape"])
    assert_rulebook_equal(rb, ref, False)


@pytest.mark.parametrize("static", [False, True], ids=["two_call", "static"])
def test_sorted_build_stays_inside_its_workspace(cuda, guard, static):
    """Against refrulebook's first-seen build with the outputs renumbered by ascending key (test_gpu_sorted.py)."""
    idx, bs, shape = the_scene()
    ref = conv_ref()
    kw = dict(static_num_out=ref["n_out"]) if static else {}
    before = counters()
    rs, out_shape = gpu_rulebook(idx, bs, shape, *K3S2, False, out_order="sorted", **kw)
    ran(before)                                                       # (no pass of the hash builders)
    assert guard() == 1 and rs.rankmap is not None
    if static:
        assert to_np(rs.n_out_dev).tolist() == [ref["n_out"], 0]
    as_i32 = lambda a: torch.from_numpy(np.array(a).view(np.int32))
    rf = types.SimpleNamespace(out_indices=as_i32(ref["out_inds"]), pair_fwd=as_i32(ref["fwd"]), pair_bwd=as_i32(ref["bwd"]),
                               mask_fwd=as_i32(ref["mfwd"]), mask_bwd=as_i32(ref["mbwd"]), num_per_loc=as_i32(ref["num"]))
    _check_renumbered(rs, rf, out_shape)


# ------------------------------------------------------------------------------------------------------------- lists
def test_lists_from_a_table_stay_inside_their_workspace(cuda, guard):
    from spconv_amd.pytorch import ops
    rb = build_subm("k27", False)
    idx, bs, shape = the_scene()
    rc, _ = gpu_rulebook(idx, bs, shape, *K3S2, False, need_native=False)
    assert guard() == 2
    for table, subm, ref in ((rb.pair_fwd, True, subm_ref("k27")), (rc.pair_bwd, False, conv_ref())):
        native, num = ops._native_from_table(table, subm)
        assert guard() == 1
        np.testing.assert_array_equal(to_np(num), ref["num"])
        np.testing.assert_array_equal(to_np(native), ref["pair"])
