"""The row operators between the layers -- union, collapse, point groups, score / top-k / select, corner lookup and
interpolation, neighbour grouping -- on the inputs their own suites do not use: dirty memory on entry, rows that nothing
names, and NaN / Inf in rows that are named (include/spconv_amd.h, "What the row operators may be handed").

Scenes and references are the existing ones (refcollapse, refselect, refinterp, the fixtures of test_gpu_union /
test_gpu_interp / test_gpu_pointvoxel), the poisoned rows those of tests/rowopscenes.py, which tests/test_refrowops.py holds
to their conditions on the CPU.  Every case names the launch keys it moves and asserts through spx_launch_count that they
moved (the `moves` decorator); test_cases_claim_every_key holds the claims against the list of keys.  Three groups:

  dirty    the C entries through ctypes on caller-owned buffers: every output, workspace, counter record and rank map
           starts as 0x00 in one run and as 0xFF (-1 = "absent" in every index, NaN in every float) in the other.  Inputs
           are valid.  The two runs agree bit for bit and the second meets the numpy reference bit for bit (the mean of
           a collapse: within the bound test_gpu_collapse.py holds it to -- its reference is a bound, not a bit pattern).
           Regions the header calls unspecified (list from offsets[n_out] on) are left out of both comparisons.
  unnamed  the rows of (b) hold zeros in one run and NaN (or +Inf) in the other: no output bit differs.  Once per unit
           through the Python static path (static_num_out, n_live_dev), where such rows arise.
  named    NaN, +Inf and -Inf in rows that ARE named: the output is NaN / +Inf / -Inf exactly where the reference is,
           bits equal everywhere else; a NaN that is moved (max, gathers) keeps its bits.

The neighbour table of the grouping cases is the corner table of the interpolation scene read as [N, nsample = 8]: rows of
the level and -1, which is all spx_group_fwd / _bwd see of a query."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import nonfinite as nf
import refcollapse as rc
import refinterp as ri
import refselect as rs
import rowopscenes as S
from util import assert_close_abs_sum

# (the numpy references add Inf to -Inf and multiply 0 by Inf on purpose)
pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:invalid value encountered:RuntimeWarning")]

REQUIRED = {f"union/{k}" for k in ("mark", "prefix", "claim", "fill", "add_fwd", "add_bwd")} | \
           {f"collapse/{k}" for k in ("mark", "prefix", "rank", "list", "fwd", "bwd")} | \
           {f"select/{k}" for k in ("score", "hist", "pick", "ties", "flags", "count", "scan", "scatter", "map")} | \
           {"pointvoxel/groups", "interp/corners_ranked", "interp/corners_hash", "interp/fwd", "interp/bwd",
            "query/group_fwd", "query/group_bwd"}
CLAIMS = {}
DT = S.DTYPES
INT = {1: torch.int8, 2: torch.int16, 4: torch.int32, 8: torch.int64}
FILLS = (0x00, 0xFF)
COLLAPSE_OPS = {"sum": 0, "mean": 1, "max": 2}
SCORE_OPS = {"absmean": 0, "absmax": 1}


def lib():
    from spconv_amd import _lib
    return _lib.load()


def check(status):
    from spconv_amd import _lib
    _lib.check(status)


def moves(*keys, **only):
    """the launch keys a case claims: each must have moved when the case ends.  key = (argument, value): claimed by the
    cases with that value of that argument alone"""
    def deco(fn):
        CLAIMS[fn.__name__] = keys + tuple(only)

        @functools.wraps(fn)
        def run(*a, **kw):
            L = lib()
            mine = keys + tuple(k for k, (arg, value) in only.items() if kw.get(arg) == value)
            before = {k: L.spx_launch_count(k.encode()) for k in mine}
            fn(*a, **kw)
            for k in mine:
                assert L.spx_launch_count(k.encode()) > before[k], f"launch key {k} did not move"
        return run
    return deco


@pytest.fixture(autouse=True)
def _end_the_run_at_a_gpu_fault(request):
    """A mismatch is one failed test.  A faulted device fails every later launch as well: the run ends at the first."""
    yield
    if torch.cuda.is_available():
        try:
            torch.cuda.synchronize()
        except RuntimeError as e:
            pytest.exit(f"the GPU faulted in {request.node.nodeid}: {e}", returncode=3)


# ---------------------------------------------------------------------------------------- small tools
def buf(shape, dtype, fill, dev):
    """a caller-owned buffer whose every byte is `fill`"""
    n = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
    raw = torch.full((max(n, 16),), fill, dtype=torch.uint8, device=dev)
    return raw[:n].view(dtype).reshape(shape) if n else torch.empty(shape, dtype=dtype, device=dev)


def ibits(t):
    t = torch.as_tensor(t).detach().cpu().contiguous()
    return t.view(INT[t.element_size()]).numpy()


def same_bits(a, b, what=""):
    np.testing.assert_array_equal(ibits(a), ibits(b), err_msg=what)


def same_outputs(a, b, what=""):
    assert a.keys() == b.keys()
    for k in a:
        same_bits(a[k], b[k], f"{what}: {k} differs between the two runs")


def same_but_nan_payload(got, want, what=""):
    """NaN exactly where the reference is (a computed NaN's payload is not part of the contract), bits equal elsewhere"""
    g, w = torch.as_tensor(got).detach().cpu(), torch.as_tensor(want).cpu()
    assert g.dtype == w.dtype and g.shape == w.shape, (what, g.dtype, w.dtype, g.shape, w.shape)
    gn, wn = torch.isnan(g).numpy(), torch.isnan(w).numpy()
    np.testing.assert_array_equal(gn, wn, err_msg=f"{what}: NaN placement")
    np.testing.assert_array_equal(ibits(g)[~gn], ibits(w)[~wn], err_msg=f"{what}: bits outside the NaNs")


def i32(dev, a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a), dtype=np.int32)).to(dev)


def code(t):
    from spconv_amd.pytorch._rulebook import _float_code
    return _float_code(t, "test")


def stream(t):
    from spconv_amd.pytorch._rulebook import _stream
    return _stream(t)


def ptr(t):
    return None if t is None else t.data_ptr()


def ints(v):
    from spconv_amd import _lib
    return _lib.ints(v)


def ptrs(v):
    from spconv_amd import _lib
    return _lib.ptrs(v)


def poison_value(kind):
    return float("nan") if kind == "nan" else float("inf")


# ---------------------------------------------------------------------------------------- the C entries, once each
def c_collapse_build(dev, idx, bs, shape, axes, fill, form, cap=None, n_live=None):
    L = lib()
    didx = i32(dev, idx)
    n, ndim = idx.shape[0], len(shape)
    kept = [s for d, s in enumerate(shape) if d not in axes]
    mask = sum(1 << a for a in axes)
    sp = ints(shape)
    nbytes = int(L.spx_rankmap_bytes(len(kept), bs, ints(kept)))
    wsb = int(L.spx_collapse_ws_bytes(ndim, bs, sp, mask, n))
    cells, ws = buf((nbytes // 4,), torch.int32, fill, dev), buf((max(wsb, 16),), torch.uint8, fill, dev)
    rows, lst = buf((n,), torch.int32, fill, dev), buf((n,), torch.int32, fill, dev)
    nl = None if n_live is None else i32(dev, [n_live])
    head = (didx.data_ptr(), n, ptr(nl), ndim, bs, sp, mask)
    tail = (cells.data_ptr(), nbytes, ws.data_ptr(), ws.numel())
    if form == "static":
        out_indices = buf((cap, len(kept) + 1), torch.int32, fill, dev)
        offsets, n_out_dev = buf((cap + 1,), torch.int32, fill, dev), buf((3,), torch.int32, fill, dev)
        check(L.spx_collapse_static(*head, cap, out_indices.data_ptr(), rows.data_ptr(), offsets.data_ptr(), lst.data_ptr(),
                                    n_out_dev.data_ptr(), *tail, stream(didx)))
        return dict(out_indices=out_indices, rows=rows, offsets=offsets, list=lst, n_out_dev=n_out_dev)
    result = (ctypes.c_int * 2)()
    check(L.spx_collapse_count(*head, *tail, result, stream(didx)))
    n_out = int(result[0])
    out_indices = buf((n_out, len(kept) + 1), torch.int32, fill, dev)
    offsets = buf((n_out + 1,), torch.int32, fill, dev)
    check(L.spx_collapse_fill(*head, n_out, out_indices.data_ptr(), rows.data_ptr(), offsets.data_ptr(), lst.data_ptr(),
                              *tail, stream(didx)))
    return dict(out_indices=out_indices, rows=rows, offsets=offsets, list=lst,
                result=torch.tensor([result[0], result[1]], dtype=torch.int32))


def c_collapse_fwd(feat, offsets, lst, n_out, op, fill, n_live=None):
    out = buf((n_out, feat.shape[1]), feat.dtype, fill, feat.device)
    check(lib().spx_collapse_fwd(feat.data_ptr(), feat.shape[0], offsets.data_ptr(), lst.data_ptr(), n_out, feat.shape[1],
                                 code(feat), COLLAPSE_OPS[op], out.data_ptr(), ptr(n_live), stream(feat)))
    return out


def c_collapse_bwd(feat, out, dout, rows, offsets, n_out, op, fill):
    din = buf((rows.shape[0], dout.shape[1]), dout.dtype, fill, dout.device)
    check(lib().spx_collapse_bwd(ptr(feat), ptr(out), dout.data_ptr(), rows.data_ptr(), offsets.data_ptr(), rows.shape[0],
                                 n_out, dout.shape[1], code(dout), COLLAPSE_OPS[op], din.data_ptr(), stream(dout)))
    return din


def c_point_groups(ids, nv, fill, n_points=None):
    dev, n = ids.device, ids.shape[0]
    L = lib()
    rows, lst = buf((n,), torch.int32, fill, dev), buf((n,), torch.int32, fill, dev)
    offsets = buf((nv + 1,), torch.int32, fill, dev)
    ws = buf((max(int(L.spx_point_groups_ws_bytes(n, nv)), 16),), torch.uint8, fill, dev)
    check(L.spx_point_groups(ids.data_ptr(), ids.element_size(), n, ptr(n_points), nv, rows.data_ptr(), offsets.data_ptr(),
                             lst.data_ptr(), ws.data_ptr(), ws.numel(), stream(ids)))
    return dict(rows=rows, offsets=offsets, list=lst)


def c_row_score(feat, op, fill, n_live=None):
    score = buf((feat.shape[0],), torch.float32, fill, feat.device)
    check(lib().spx_row_score(feat.data_ptr(), feat.shape[0], feat.shape[1], code(feat), SCORE_OPS[op], ptr(n_live),
                              score.data_ptr(), stream(feat)))
    return score


def c_topk(score, idx, batch, n_live, k, ratio, fill):
    L, dev, n = lib(), score.device, score.shape[0]
    keep, sel = buf((n,), torch.uint8, fill, dev), buf((4,), torch.int32, fill, dev)
    ws = buf((max(int(L.spx_topk_ws_bytes(n)), 16),), torch.uint8, fill, dev)
    ndim = 0 if idx is None else idx.shape[1] - 1
    check(L.spx_topk_flags(score.data_ptr(), ptr(idx), n, ptr(n_live), ndim, batch if idx is not None else 0,
                           -1 if k is None else int(k), 0.0 if ratio is None else float(ratio), keep.data_ptr(),
                           sel.data_ptr(), ws.data_ptr(), ws.numel(), stream(score)))
    return dict(keep=keep, sel=sel)


def c_select(dev, idx, bs, shape, keep, invert, fill, form, cap=None, n_live=None, rank_map=False):
    L = lib()
    didx, dkeep = i32(dev, idx), torch.from_numpy(keep).to(dev)
    n, ndim = idx.shape[0], len(shape)
    sp = ints(shape)
    cells, nbytes, bad = None, 0, None
    if rank_map:
        nbytes = int(L.spx_rankmap_bytes(ndim, bs, sp))
        cells, bad = buf((nbytes // 4,), torch.int32, fill, dev), torch.zeros((1,), dtype=torch.int32, device=dev)
    ws = buf((max(int(L.spx_select_ws_bytes(ndim, n)), 16),), torch.uint8, fill, dev)
    rows = buf((n,), torch.int32, fill, dev)
    nl = None if n_live is None else i32(dev, [n_live])
    head = (didx.data_ptr(), n, ptr(nl), ndim, bs, sp, dkeep.data_ptr(), int(invert))
    tail = (ptr(cells), nbytes, ptr(bad), ws.data_ptr(), ws.numel())
    if form == "static":
        out_indices, src = buf((cap, ndim + 1), torch.int32, fill, dev), buf((cap,), torch.int32, fill, dev)
        n_out_dev = buf((3,), torch.int32, fill, dev)
        check(L.spx_select_static(*head, cap, out_indices.data_ptr(), rows.data_ptr(), src.data_ptr(), n_out_dev.data_ptr(),
                                  *tail, stream(didx)))
        out = dict(out_indices=out_indices, rows=rows, src=src, n_out_dev=n_out_dev)
    else:
        result = (ctypes.c_int * 2)()
        check(L.spx_select_count(*head, ws.data_ptr(), ws.numel(), result, stream(didx)))
        n_out = int(result[0])
        out_indices, src = buf((n_out, ndim + 1), torch.int32, fill, dev), buf((n_out,), torch.int32, fill, dev)
        check(L.spx_select_fill(*head, n_out, out_indices.data_ptr(), rows.data_ptr(), src.data_ptr(), *tail, stream(didx)))
        out = dict(out_indices=out_indices, rows=rows, src=src, result=torch.tensor([result[0], result[1]], dtype=torch.int32))
    if rank_map:                                                             # (spx_rankmap_from_sorted stores every byte of the map)
        out["violation"], out["map"] = bad, cells
    return out


def c_union(dev, idxs, bs, shape, fill, form, cap=None, n_live=None):
    L = lib()
    didx = [i32(dev, i) for i in idxs]
    T, ndim = len(idxs), len(shape)
    ns = [int(i.shape[0]) for i in idxs]
    sp = ints(shape)
    nbytes = int(L.spx_rankmap_bytes(ndim, bs, sp))
    wsb = int(L.spx_union_ws_bytes(ndim, bs, sp, T, sum(ns)))
    cells, ws = buf((nbytes // 4,), torch.int32, fill, dev), buf((max(wsb, 16),), torch.uint8, fill, dev)
    rows = [buf((n,), torch.int32, fill, dev) for n in ns]
    lives = [None] * T if n_live is None else [i32(dev, [v]) for v in n_live]
    head = (ptrs([t.data_ptr() for t in didx]), ints(ns), ptrs([ptr(v) for v in lives]), T, ndim, bs, sp)
    tail = (cells.data_ptr(), nbytes, ws.data_ptr(), ws.numel())
    row_ptrs = ptrs([r.data_ptr() for r in rows])
    if form == "static":
        out_indices, src = buf((cap, ndim + 1), torch.int32, fill, dev), buf((T, cap), torch.int32, fill, dev)
        n_out_dev = buf((3,), torch.int32, fill, dev)
        check(L.spx_union_static(*head, cap, out_indices.data_ptr(), row_ptrs, src.data_ptr(), n_out_dev.data_ptr(), *tail,
                                 stream(didx[0])))
        out = dict(out_indices=out_indices, src=src, n_out_dev=n_out_dev)
    else:
        result = (ctypes.c_int * (2 + T))()
        check(L.spx_union_count(*head, *tail, result, stream(didx[0])))
        n_out = int(result[0])
        out_indices, src = buf((n_out, ndim + 1), torch.int32, fill, dev), buf((T, n_out), torch.int32, fill, dev)
        check(L.spx_union_fill(*head, n_out, -1, out_indices.data_ptr(), row_ptrs, src.data_ptr(), *tail, stream(didx[0])))
        out = dict(out_indices=out_indices, src=src, result=torch.tensor(list(result), dtype=torch.int32))
    out.update({f"rows{t}": r for t, r in enumerate(rows)})
    return out


def c_union_add_fwd(feats, src, n_out, fill, n_live=None):
    out = buf((n_out, feats[0].shape[1]), feats[0].dtype, fill, feats[0].device)
    check(lib().spx_union_add_fwd(ptrs([f.data_ptr() for f in feats]), ints([f.shape[0] for f in feats]), len(feats),
                                  src.data_ptr(), n_out, feats[0].shape[1], code(feats[0]), out.data_ptr(), ptr(n_live),
                                  stream(out)))
    return out


def c_union_add_bwd(dout, rows, fill):
    dins = [buf((r.shape[0], dout.shape[1]), dout.dtype, fill, dout.device) for r in rows]
    check(lib().spx_union_add_bwd(dout.data_ptr(), dout.shape[0], ptrs([d.data_ptr() for d in dins]),
                                  ptrs([r.data_ptr() for r in rows]), ints([d.shape[0] for d in dins]), len(rows),
                                  dout.shape[1], dout.element_size(), stream(dout)))
    return dins


def c_corners(dev, sc, idx, n_live, rankmap, fill, n_points="scene"):
    """spx_point_corners over the interpolation scene `sc` (test_gpu_interp.Scene), normalised weights"""
    import test_gpu_interp as TI
    from spconv_amd.pytorch._level import _floats, _geometry
    L = lib()
    ndim, K = sc.ndim, 1 << sc.ndim
    _, vsize, coors_range = _geometry(sc.vs, sc.range)
    pts, bid = torch.from_numpy(sc.pts).to(dev), torch.from_numpy(sc.bid).to(dev)
    didx = i32(dev, idx)
    N, n = pts.shape[0], idx.shape[0]
    npt = sc.n_points if n_points == "scene" else n_points
    dn, dl = (None if npt is None else i32(dev, [npt])), (None if n_live is None else i32(dev, [n_live]))
    rows, w = buf((N, K), torch.int32, fill, dev), buf((N, K), torch.float32, fill, dev)
    ws = None
    if rankmap is None:
        ws = buf((max(int(L.spx_point_corners_ws_bytes(N, ndim, n)), 16),), torch.uint8, fill, dev)
    check(L.spx_point_corners(pts.data_ptr(), int(pts.shape[1]), bid.data_ptr(), N, ptr(dn), ndim, _floats(vsize),
                              _floats(coors_range), didx.data_ptr(), n, ptr(dl), TI.B, ints(sc.shape), ptr(rankmap),
                              0 if rankmap is None else rankmap.numel() * rankmap.element_size(), 1, rows.data_ptr(),
                              w.data_ptr(), ptr(ws), 0 if ws is None else ws.numel(), stream(pts)))
    return dict(rows=rows, weights=w)


def c_rankmap_from_sorted(dev, idx, count, bs, shape, fill):
    L = lib()
    didx = i32(dev, idx)
    nbytes = int(L.spx_rankmap_bytes(len(shape), bs, ints(shape)))
    cells, bad = buf((nbytes // 4,), torch.int32, fill, dev), torch.zeros((1,), dtype=torch.int32, device=dev)
    check(L.spx_rankmap_from_sorted(didx.data_ptr(), count, len(shape), bs, ints(shape), cells.data_ptr(), nbytes,
                                    bad.data_ptr(), stream(didx)))
    assert int(bad.item()) == 0
    return cells


def c_interp_fwd(vfeat, rows, w, fill):
    N, K = rows.shape
    out = buf((N, vfeat.shape[1]), vfeat.dtype, fill, vfeat.device)
    check(lib().spx_interp_fwd(vfeat.data_ptr(), vfeat.shape[0], rows.data_ptr(), w.data_ptr(), N, K.bit_length() - 1,
                               vfeat.shape[1], code(vfeat), out.data_ptr(), stream(vfeat)))
    return out


def c_interp_bwd(dout, K, w, offsets, lst, n, n_live, fill):
    dv = buf((n, dout.shape[1]), dout.dtype, fill, dout.device)
    check(lib().spx_interp_bwd(dout.data_ptr(), dout.shape[0], K.bit_length() - 1, w.data_ptr(), offsets.data_ptr(),
                               lst.data_ptr(), n, ptr(n_live), dout.shape[1], code(dout), dv.data_ptr(), stream(dout)))
    return dv


def c_group_fwd(vfeat, rows, fill):
    M, Sn = rows.shape
    out = buf((M, Sn, vfeat.shape[1]), vfeat.dtype, fill, vfeat.device)
    check(lib().spx_group_fwd(vfeat.data_ptr(), vfeat.shape[0], rows.data_ptr(), M, Sn, vfeat.shape[1], code(vfeat),
                              out.data_ptr(), stream(vfeat)))
    return out


def c_group_bwd(dout, offsets, lst, n, n_live, fill):
    M, Sn, C = dout.shape
    dv = buf((n, C), dout.dtype, fill, dout.device)
    check(lib().spx_group_bwd(dout.data_ptr(), M, Sn, offsets.data_ptr(), lst.data_ptr(), n, ptr(n_live), C, code(dout),
                              dv.data_ptr(), stream(dout)))
    return dv


def both(fn, what=""):
    """fn(fill) -> {name: tensor}: run on 0x00 and on 0xFF buffers, the two agree bit for bit; the 0xFF run's outputs"""
    a, b = fn(FILLS[0]), fn(FILLS[1])
    if not isinstance(a, dict):
        a, b = {"out": a}, {"out": b}
    same_outputs(a, b, what)
    return b


# ========================================================================================= collapse
def ref_tables(dev, ref):
    return i32(dev, ref.rows), i32(dev, ref.offsets), i32(dev, ref.list)


def mean_close(got, feat, ref, what):
    """the finite elements of a mean against test_gpu_collapse's bound; the others where the reference has them"""
    want = rc.reduce(feat, ref, "mean").double().numpy()
    g = got.detach().cpu().double().numpy()
    for a, b in zip(nf.masks_np(g), nf.masks_np(want)):
        np.testing.assert_array_equal(a, b, err_msg=f"{what}: non-finite placement")
    ok = np.isfinite(want)
    clean = torch.where(torch.isfinite(feat), feat, torch.zeros_like(feat))
    mean, A, lens = rc.mean_f64(clean, ref)
    fin = np.isfinite(mean_of_finite_groups(feat, ref))
    sel = ok & fin
    assert_close_abs_sum(np.where(sel, g, 0.0), np.where(sel, mean, 0.0), np.where(sel, A * (lens[:, None] + 2), 0.0),
                         feat.dtype, 2.0 ** -24, name=what)


def mean_of_finite_groups(feat, ref):
    """[live, C]: NaN where a group holds a non-finite entry (those elements are compared by placement alone), else 0"""
    grp = nf.group_of_entries(ref.offsets)
    bad = nf._any_by_group(ref.live, grp, ~np.isfinite(feat.double().numpy()[ref.list]))
    return np.where(bad, np.nan, 0.0)


@pytest.mark.parametrize("form", ["static", "two_call"])
@pytest.mark.parametrize("case", ["one", "rows255", "rows256", "rows257", "fwd", "rows3000"])
@moves("collapse/mark", "collapse/prefix", "collapse/rank", "collapse/list")
def test_dirty_collapse_build(cuda, case, form):
    idx, bs, shape, axes, full = S.collapse_case(case)
    n = idx.shape[0]
    n_live = n - n // 6 if n > 1 else None
    variants = [(full.found + 5, n_live), (max(full.found - 3, 1), n_live)] if form == "static" else [(None, n_live), (None, None)]
    for cap, nl in variants:
        ref = rc.build(idx, bs, shape, axes, nl, cap)
        out = both(lambda fill: spec_of_build(c_collapse_build(cuda, idx, bs, shape, axes, fill, form, cap, nl), ref),
                   f"collapse {case} {form}")
        np.testing.assert_array_equal(out["out_indices"].cpu().numpy()[:ref.live], ref.out_indices)
        np.testing.assert_array_equal(out["rows"].cpu().numpy(), ref.rows)
        np.testing.assert_array_equal(out["offsets"].cpu().numpy()[:ref.live + 1], ref.offsets)
        np.testing.assert_array_equal(out["list"].cpu().numpy(), ref.list)
        if form == "static":
            assert out["n_out_dev"].cpu().tolist() == [ref.found, 0, ref.live]
            assert bool((out["out_indices"][ref.live:] == -1).all())
            assert bool((out["offsets"][ref.live:] == int(ref.offsets[-1])).all())
        else:
            assert out["result"].tolist() == [ref.found, ref.live_rows]


def spec_of_build(out, ref):
    """the specified part: list entries from offsets[n_out] on are unspecified (the dead and dropped rows in whatever
    order the sort left them), so the list is cut at the kept rows"""
    out["list"] = out["list"][:int(ref.offsets[-1])]
    return out


@pytest.mark.parametrize("dt,C", [("f16", 8), ("f16", 520), ("f32", 3), ("f64", 3)])
@moves("collapse/fwd", "collapse/bwd")
def test_dirty_collapse_reduce(cuda, dt, C):
    idx, bs, shape, axes, ref = S.collapse_case("fwd")
    feat = rc.features(idx.shape[0], C, DT[dt], 100 + C)
    dout = rc.features(ref.live + 4, C, DT[dt], 300 + C)
    rows, offsets, lst = ref_tables(cuda, ref)
    offsets = torch.cat([offsets, offsets[-1:].expand(4)]).contiguous()      # four rows of room behind the live count
    n_out = ref.live + 4
    nl = i32(cuda, [ref.live])
    dfeat, ddout = feat.to(cuda), dout.to(cuda)
    for op in COLLAPSE_OPS:
        out = both(lambda fill: c_collapse_fwd(dfeat, offsets, lst, n_out, op, fill, nl), f"fwd {op}")["out"]
        assert not bool(out[ref.live:].any())
        if op == "mean":
            mean_close(out[:ref.live], feat, ref, f"mean {dt} C={C}")
        else:
            same_bits(out[:ref.live], rc.reduce(feat, ref, op), op)
        if op == "sum":
            continue
        fo = out if op == "max" else None
        din = both(lambda fill: c_collapse_bwd(dfeat if op == "max" else None, fo, ddout, rows, offsets, n_out, op, fill),
                   f"bwd {op}")["out"]
        want = rc.backward(feat, rc.reduce(feat, ref, op), dout[:ref.live], ref, op)
        if op == "max":
            same_bits(din, torch.from_numpy(want).to(DT[dt]), "max backward")
        else:
            from test_gpu_collapse import mean_bwd_bound
            assert bool((np.abs(din.double().cpu().numpy() - want) <= mean_bwd_bound(want, DT[dt])).all())


@pytest.mark.parametrize("kind", ["nan", "inf"])
@moves("collapse/mark", "collapse/prefix", "collapse/rank", "collapse/list", "collapse/fwd", "collapse/bwd")
def test_unnamed_collapse_through_the_static_path(cuda, kind):
    """feature rows behind n_live, rows whose index row is dead and rows of groups that the cap drops; dout rows behind
    the live output count"""
    from spconv_amd.pytorch import _collapse
    idx, bs, shape, axes, full = S.collapse_case("fwd")
    n, C = idx.shape[0], 8
    n_live = n - 60
    cap = rc.build(idx, bs, shape, axes, n_live).found - 20
    ref = rc.build(idx, bs, shape, axes, n_live, cap)
    unnamed = torch.from_numpy(ref.rows < 0)
    assert int(unnamed.sum()) > 60 + 8 and ref.found > cap
    c = _collapse.sparse_collapse_build(i32(cuda, idx), bs, shape, axes, n_live=i32(cuda, [n_live]), static_num_out=cap)
    assert c.n_out_dev.cpu().tolist() == [ref.found, 0, ref.live]
    outs = []
    for value in (0.0, poison_value(kind)):
        feat = rc.features(n, C, torch.float16, 5)
        feat[unnamed] = value
        dout = rc.features(cap, C, torch.float16, 6)
        dout[ref.live:] = value
        run = {}
        for op in COLLAPSE_OPS:
            out = _collapse.fwd(feat.to(cuda), c, op, c.n_out_dev[2:3])
            run[f"fwd_{op}"] = out
            run[f"bwd_{op}"] = _collapse.bwd(dout.to(cuda), c, op, feat.to(cuda), out)
        outs.append(run)
    same_outputs(outs[0], outs[1], f"collapse unnamed {kind}")
    for op in ("sum", "max"):
        feat = rc.features(n, C, torch.float16, 5)
        same_bits(outs[1][f"fwd_{op}"][:ref.live], rc.reduce(feat, ref, op), op)
        assert not bool(outs[1][f"fwd_{op}"][ref.live:].any())


NAMED_COLLAPSE = [("fwd", dt, C) for dt, C in S.WIDTHS] + [("lengths", "f16", 3), ("lengths", "f16", 8), ("lengths", "f32", 40),
                                                         ("rows3000", "bf16", 40), ("rows3000", "f16", 8)]


@pytest.mark.parametrize("case,dt,C", NAMED_COLLAPSE)
@moves("collapse/fwd", "collapse/bwd")
def test_named_collapse(cuda, case, dt, C):
    idx, bs, shape, axes, ref = S.collapse_case(case)
    feat, plan = S.collapse_named(case, dt, C)
    rows, offsets, lst = ref_tables(cuda, ref)
    dfeat = feat.to(cuda)
    dout = rc.features(ref.live, C, DT[dt], 11)
    dout[plan.roles["pinf"], int(plan.channels[0])] = float("inf")           # the gradient holds non-finite values too
    dout[plan.roles["nan_first"], int(plan.channels[-1])] = float("nan")
    ddout = dout.to(cuda)
    got = {op: c_collapse_fwd(dfeat, offsets, lst, ref.live, op, 0xFF) for op in COLLAPSE_OPS}
    same_but_nan_payload(got["sum"], rc.reduce(feat, ref, "sum"), "sum")
    same_bits(got["max"], rc.reduce(feat, ref, "max"), "max: a copy of an input element, the first NaN included")
    mean_close(got["mean"], feat, ref, f"mean {case} {dt} C={C}")
    if dt == "f16":
        assert bool(torch.isposinf(got["sum"][plan.roles["big"], torch.from_numpy(plan.channels).to(cuda)]).all())
    # backward: max bit for bit (every element is a copy of dout or zero), mean by placement and bound
    din = c_collapse_bwd(dfeat, got["max"], ddout, rows, offsets, ref.live, "max", 0xFF)
    want = rc.backward(feat, rc.reduce(feat, ref, "max"), dout, ref, "max")
    same_but_nan_payload(din, torch.from_numpy(want).to(DT[dt]), "max backward")
    g, c0 = plan.roles["nan_two"], int(plan.channels[0])
    members = ref.list[ref.offsets[g]:ref.offsets[g + 1]]
    assert int((din[torch.from_numpy(members).to(cuda), c0] != 0).sum()) == 2          # both NaN rows receive
    din = c_collapse_bwd(None, None, ddout, rows, offsets, ref.live, "mean", 0xFF)
    want = rc.backward(feat, None, dout, ref, "mean")
    gd = din.double().cpu().numpy()
    for a, b in zip(nf.masks_np(gd), nf.masks_np(want)):
        np.testing.assert_array_equal(a, b, err_msg="mean backward: non-finite placement")
    from test_gpu_collapse import mean_bwd_bound
    ok = np.isfinite(want)
    assert bool((np.abs(gd - want)[ok] <= mean_bwd_bound(want[ok], DT[dt])).all())


# ========================================================================================= point groups (DynamicVFE)
@pytest.mark.parametrize("id_dtype", [np.int64, np.int32])
@moves("pointvoxel/groups")
def test_dirty_point_groups(cuda, id_dtype):
    import test_gpu_pointvoxel as TP
    ids = TP.main_ids(id_dtype)
    dids = torch.from_numpy(ids).to(cuda)
    for n_points in (None, 4321):
        rows, offsets, lst = TP.ref_groups(ids, TP.NV, n_points)
        npd = None if n_points is None else i32(cuda, [n_points])

        def run(fill):
            out = c_point_groups(dids, TP.NV, fill, npd)
            out["list"] = out["list"][:int(offsets[-1])]                   # (entries from offsets[num_voxels] on: unspecified)
            return out
        out = both(run, "point groups")
        np.testing.assert_array_equal(out["rows"].cpu().numpy(), rows)
        np.testing.assert_array_equal(out["offsets"].cpu().numpy(), offsets)
        np.testing.assert_array_equal(out["list"].cpu().numpy(), lst)


@pytest.mark.parametrize("kind", ["nan", "inf"])
@moves("pointvoxel/groups", "collapse/fwd", "collapse/bwd")
def test_unnamed_points_through_the_static_path(cuda, kind):
    """rows behind *n_points and points without a voxel hold anything; voxel rows behind *n_live are zeros"""
    import test_gpu_pointvoxel as TP
    from spconv_amd.pytorch import functional as F
    ids = TP.main_ids()
    n_points, n_live = 4321, 690                                             # (ids end at 679: no point names a dead voxel)
    rows, offsets, lst = TP.ref_groups(ids, TP.NV, n_points)
    g = F.point_groups(torch.from_numpy(ids).to(cuda), TP.NV, n_points=i32(cuda, [n_points]), n_live=i32(cuda, [n_live]))
    outs = []
    for value in (0.0, poison_value(kind)):
        feat = rc.features(TP.N, 8, torch.float16, 8)
        feat[torch.from_numpy(rows < 0)] = value
        dvox = rc.features(TP.NV, 8, torch.float16, 9)
        dvox[n_live:] = value
        run = {}
        for op in COLLAPSE_OPS:
            x = feat.to(cuda).requires_grad_(True)
            out = F.points_to_voxels(x, g, op)
            (run[f"bwd_{op}"],) = torch.autograd.grad(out, x, dvox.to(cuda))
            run[f"fwd_{op}"] = out.detach()
        outs.append(run)
    same_outputs(outs[0], outs[1], f"points unnamed {kind}")
    assert not bool(outs[1]["fwd_max"][n_live:].any())


@pytest.mark.parametrize("dt,C", [("f16", 8), ("f32", 3), ("bf16", 40)])
@moves("collapse/fwd", "collapse/bwd")
def test_named_points_to_voxels(cuda, dt, C):
    """the DynamicVFE reductions: groups of up to 600 points (many rounds of the four-entry walk)"""
    import test_gpu_pointvoxel as TP
    ids = TP.main_ids()
    rows, offsets, lst = TP.ref_groups(ids, TP.NV)
    ref = TP.as_ref(rows, offsets, lst, TP.NV)
    plan = nf.poison_groups(ref.offsets, ref.list, C, 3)
    long_rows = ref.list[ref.offsets[TP.LONG]:ref.offsets[TP.LONG + 1]]
    plan.cells.append((int(long_rows[411]), "nan_a"))                         # a NaN deep inside the 600-point voxel
    feat = nf.poisoned_groups(rc.features(TP.N, C, DT[dt], 21), plan)
    drows, doff, dlst = ref_tables(cuda, ref)
    dfeat = feat.to(cuda)
    got = {op: c_collapse_fwd(dfeat, doff, dlst, TP.NV, op, 0xFF) for op in ("sum", "max")}
    same_but_nan_payload(got["sum"], rc.reduce(feat, ref, "sum"), "sum")
    same_bits(got["max"], rc.reduce(feat, ref, "max"), "max")
    assert bool(torch.isnan(got["max"][TP.LONG, int(plan.channels[0])]))
    dout = rc.features(TP.NV, C, DT[dt], 22)
    din = c_collapse_bwd(dfeat, got["max"], dout.to(cuda), drows, doff, TP.NV, "max", 0xFF)
    same_bits(din, torch.from_numpy(rc.backward(feat, rc.reduce(feat, ref, "max"), dout, ref, "max")).to(DT[dt]), "max backward")


# ========================================================================================= score, top-k, select
@pytest.mark.parametrize("n", [1, 255, 256, 257, 3000])
@moves("select/score", "select/hist", "select/pick", "select/ties", "select/flags")
def test_dirty_score_and_flags(cuda, n):
    feat = rc.features(n, 40, torch.float16, n)
    n_live = n - n // 5
    nl = i32(cuda, [n_live])
    for op in SCORE_OPS:
        score = both(lambda fill: c_row_score(feat.to(cuda), op, fill, nl), f"score {op}")["out"]
        same_bits(score, torch.from_numpy(rs.score(feat, op, n_live)), op)
    s = rs.scores("normal", n, 11 + n)
    idx = np.zeros((n, 4), dtype=np.int32)
    idx[np.random.default_rng(n).random(n) < 0.1, 0] = -1
    live = int(rs.live_rows(n, idx, 2, n_live).sum())
    for k, ratio in ((max(live // 3, 0), None), (None, 0.5), (0, None), (live, None)):
        ref = rs.topk(s, k, ratio, idx, 2, n_live)
        out = both(lambda fill: c_topk(torch.from_numpy(s).to(cuda), i32(cuda, idx), 2, nl, k, ratio, fill), "top-k")
        np.testing.assert_array_equal(out["keep"].cpu().numpy(), ref.keep)
        assert out["sel"].cpu().tolist() == ref.sel


@pytest.mark.parametrize("form", ["static", "two_call"])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 3000])
@moves("select/count", "select/scan", "select/scatter", "select/map")
def test_dirty_select_build(cuda, n, form):
    bs, shape = 2, [5, 14, 16]
    idx = rs.sorted_scene(bs, shape, n, 5 * n)                                # key order: a rank map may be asked for
    rows = idx.shape[0]
    keep = (np.random.default_rng(n).random(rows) < 0.5).astype(np.uint8)
    keep[0] = 1
    n_live = rows - rows // 9
    found = rs.select(idx, bs, shape, keep, False, n_live).found
    variants = [(found + 3, n_live), (max(found - 2, 1), n_live)] if form == "static" else [(None, n_live), (None, None)]
    for cap, nl in variants:
        for invert in (False, True):
            ref = rs.select(idx, bs, shape, keep, invert, nl, cap)
            out = both(lambda fill: c_select(cuda, idx, bs, shape, keep, invert, fill, form, cap, nl, rank_map=True),
                       f"select n={n} {form}")
            np.testing.assert_array_equal(out["rows"].cpu().numpy(), ref.rows)
            np.testing.assert_array_equal(out["out_indices"].cpu().numpy()[:ref.live], ref.out_indices)
            np.testing.assert_array_equal(out["src"].cpu().numpy()[:ref.live], ref.src)
            assert int(out["violation"].item()) == 0
            if form == "static":
                assert out["n_out_dev"].cpu().tolist() == [ref.found, 0, ref.live]
                assert bool((out["out_indices"][ref.live:] == -1).all()) and bool((out["src"][ref.live:] == -1).all())
            else:
                assert out["result"].tolist() == [ref.found, ref.live_rows]


@pytest.mark.parametrize("kind", ["nan", "inf"])
@moves("select/score", "select/hist", "select/pick", "select/ties", "select/flags", "select/count", "select/scan",
       "select/scatter")
def test_unnamed_rows_of_a_prune_through_the_static_path(cuda, kind):
    """feature rows behind n_live_dev (and their index rows, whatever they hold) change nothing of a static prune; a
    score behind n_live or of a row with a dead batch index changes no flag"""
    import spconv_amd.pytorch as spconv
    F = spconv.functional
    bs, shape, C = 2, [6, 14, 16], 16
    idx = rs.sorted_scene(bs, shape, 700, 61)
    n, cap = idx.shape[0], 900
    outs = []
    for value in (0.0, poison_value(kind)):
        feat = torch.full((cap, C), value, dtype=torch.float16)
        feat[:n] = rc.features(n, C, torch.float16, 62)
        full = np.full((cap, 4), -1, dtype=np.int32)
        full[:n] = idx
        full[n:n + 50] = idx[:50]                                             # stale rows that look alive
        x = spconv.SparseConvTensor(feat.to(cuda), torch.from_numpy(full).to(cuda), shape, bs)
        x.n_live_dev = i32(cuda, [n])
        kept = F.sparse_prune(x, ratio=0.5, static_num_out=500)
        score = F.row_score(feat.to(cuda), "absmax", x.n_live_dev)
        s = rs.scores("normal", cap, 63).copy()
        dead = np.zeros((cap,), dtype=bool)
        dead[n:] = True
        dead[::13] = True
        flag_idx = full.copy()
        flag_idx[dead, 0] = -1
        s[dead] = value
        keep, sel = c_topk(torch.from_numpy(s).to(cuda), i32(cuda, flag_idx), bs, None, 200, None, 0xFF).values()
        outs.append(dict(features=kept.features, indices=kept.indices, live=kept.n_live_dev, score=score, keep=keep, sel=sel))
    same_outputs(outs[0], outs[1], f"prune unnamed {kind}")
    live = int(outs[1]["live"].item())
    assert live == n // 2 and not bool(outs[1]["features"][live:].any()) and bool((outs[1]["indices"][live:] == -1).all())
    ref = rs.topk(rs.score(rc.features(n, C, torch.float16, 62), "absmean"), None, 0.5)
    np.testing.assert_array_equal(outs[1]["indices"][:live].cpu().numpy(), idx[ref.keep != 0])


@pytest.mark.parametrize("dt,C", S.WIDTHS)
@moves("select/score")
def test_named_score(cuda, dt, C):
    feat, sets = S.score_named(dt, C)
    for op in SCORE_OPS:
        got = c_row_score(feat.to(cuda), op, 0xFF)
        same_but_nan_payload(got, torch.from_numpy(rs.score(feat, op)), f"{op} {dt} C={C}")
        nan = torch.isnan(got)
        assert int(nan.sum()) == len(sets["nan"]) and not bool(torch.signbit(got[nan]).any())      # a POSITIVE NaN
        assert bool(torch.isposinf(got[torch.tensor(sets["pinf"] + sets["ninf"]).to(cuda)]).all())


@pytest.mark.parametrize("n", [257, 3000])
@moves("select/hist", "select/pick", "select/ties", "select/flags")
def test_named_flags_on_nan_scores(cuda, n):
    """the key order over all bit patterns: NaNs of both signs and two payloads, at the variants of test_gpu_select.test_flags"""
    from spconv_amd.pytorch import _select
    s = rs.scores("nan", n, 11 + n)
    rng = np.random.default_rng(n + 1)
    idx = np.zeros((n, 4), dtype=np.int32)
    idx[:, 0] = rng.integers(0, 2, n)
    idx[rng.random(n) < 0.1, 0] = -1
    n_live = n - n // 7
    dev_s, dev_idx, dev_live = torch.from_numpy(s).to(cuda), torch.from_numpy(idx).to(cuda), i32(cuda, [n_live])
    same_bits(dev_s, torch.from_numpy(s), "the payloads reach the device")
    live = int(rs.live_rows(n, idx, 2, n_live).sum())
    b = s.view(np.uint32)
    ok = rs.live_rows(n, idx, 2, n_live)
    top_nan = int((ok & (b == 0x7fc12345)).sum())
    variants = [(k, None) for k in (0, 1, top_nan, top_nan + 1, live - 1, live, live + 5)] + [(None, r) for r in (0.0, 0.3, 0.5, 1.0)]
    for k, ratio in variants:
        ref = rs.topk(s, k, ratio, idx, 2, n_live)
        keep, sel = _select.topk_flags(dev_s, k, ratio, dev_idx, 2, dev_live)
        assert sel.cpu().tolist() == ref.sel
        np.testing.assert_array_equal(keep.cpu().numpy(), ref.keep)
    keep, _ = _select.topk_flags(dev_s, top_nan, None, dev_idx, 2, dev_live)
    np.testing.assert_array_equal(keep.cpu().numpy() != 0, ok & (b == 0x7fc12345))      # the larger payload first


@pytest.mark.parametrize("score", ["absmean", "absmax"])
@moves("select/score", "select/hist", "select/pick", "select/ties", "select/flags", "select/count", "select/scan",
       "select/scatter")
def test_named_prune_keeps_the_nan_rows_first(cuda, score):
    """k = the NaN-scored rows + 100, the threshold between two distinct finite scores: the selection does not depend on
    the payload of a computed NaN"""
    import spconv_amd.pytorch as spconv
    bs, shape = 2, [6, 14, 16]
    feat, sets = S.score_named("f16", 40, 600)
    idx = rs.sorted_scene(bs, shape, 600, 71)
    s = S.keep_of_nan_scores(rs.score(feat, score))
    order = np.sort(s[~np.isnan(s)])[::-1]
    m = next(m for m in range(100, 200) if order[m - 1] > order[m])           # the first cut behind 100 rows between two
    assert np.isfinite(order[m - 1]) and np.isfinite(order[m])                # distinct finite scores
    k = len(sets["nan"]) + m
    ref = rs.topk(s, k)
    x = spconv.SparseConvTensor(feat.to(cuda), torch.from_numpy(idx).to(cuda), shape, bs)
    kept = spconv.functional.sparse_prune(x, k=k, score=score)
    np.testing.assert_array_equal(kept.indices.cpu().numpy(), idx[ref.keep != 0])
    same_bits(kept.features, feat[torch.from_numpy(ref.keep != 0)], "the kept rows keep their bits")
    assert bool(ref.keep[np.array(sets["nan"])].all())


# ========================================================================================= union
@pytest.mark.parametrize("form", ["static", "two_call"])
@moves("union/mark", "union/prefix", "union/claim", "union/add_fwd", "union/add_bwd", **{"union/fill": ("form", "two_call")})
def test_dirty_union(cuda, form):
    import test_gpu_union as TU
    bs, shape = TU.SMALL
    idxs = [TU.operand(bs, shape, 260 + 30 * t, 120 + t) for t in range(3)]
    C = 8
    feats = [TU.features(i.shape[0], C, torch.float16, 123 + t) for t, i in enumerate(idxs)]
    uniq, want, rows_ref = TU.expect(idxs, feats, bs, shape)
    n = uniq.shape[0]
    for cap in ((n + 6, n - 9) if form == "static" else (None,)):
        out = both(lambda fill: c_union(cuda, idxs, bs, shape, fill, form, cap), f"union {form}")
        live = n if cap is None else min(n, cap)
        np.testing.assert_array_equal(out["out_indices"].cpu().numpy()[:live], TU.decode(uniq[:live], shape))
        src = out["src"].cpu().numpy()
        for t, r in enumerate(rows_ref):
            rows = out[f"rows{t}"].cpu().numpy()
            np.testing.assert_array_equal(rows, np.where(r < live, r, -1))
            held = np.nonzero(rows >= 0)[0]
            np.testing.assert_array_equal(src[t][rows[held]], held)
            assert int((src[t] >= 0).sum()) == held.shape[0]
        if form == "static":
            assert out["n_out_dev"].cpu().tolist() == [n, 0, live]
            assert bool((out["out_indices"][live:] == -1).all()) and bool((out["src"][:, live:] == -1).all())
        else:
            assert out["result"].tolist() == [n, 0] + [i.shape[0] for i in idxs]
        room = src.shape[1]
        nl = i32(cuda, [live])
        dfeats = [f.to(cuda) for f in feats]
        merged = both(lambda fill: c_union_add_fwd(dfeats, out["src"], room, fill, nl), "add_fwd")["out"]
        same_bits(merged[:live], want[:live], "merge")
        assert not bool(merged[live:].any())
        dout = TU.features(room, C, torch.float16, 130).to(cuda)
        rows_dev = [out[f"rows{t}"] for t in range(3)]
        dins = both(lambda fill: {str(t): d for t, d in enumerate(c_union_add_bwd(dout, rows_dev, fill))}, "add_bwd")
        for t in range(3):
            r = rows_dev[t].long()
            want_din = torch.where((r >= 0)[:, None], dout[r.clamp_min(0)], torch.zeros_like(dout[:1]))
            same_bits(dins[str(t)], want_din, f"din {t}")


@pytest.mark.parametrize("kind", ["nan", "inf"])
@moves("union/mark", "union/prefix", "union/claim", "union/add_fwd", "union/add_bwd")      # (the static form: no fill pass)
def test_unnamed_union_through_the_static_path(cuda, kind):
    """the operands' rows behind their live counts, rows with a dead index row, and the rows of cells the cap drops"""
    import test_gpu_union as TU
    from spconv_amd.pytorch import _union, ops
    bs, shape = TU.SMALL
    idxs = [TU.operand(bs, shape, 260 + 30 * t, 120 + t) for t in range(3)]
    fulls = []
    for i in idxs:
        full = np.full((i.shape[0] + 7, 4), -1, np.int32)
        full[:i.shape[0]] = i
        full[i.shape[0]:, :] = i[:7]                                          # stale rows behind the live count
        full[5, 0] = bs                                                       # a dead index row in the middle
        fulls.append(full)
    uniq, _, rows_ref = TU.expect(fulls, [torch.zeros((f.shape[0], 1)) for f in fulls], bs, shape,
                                  n_live=[i.shape[0] for i in idxs])
    cap = uniq.shape[0] - 12
    outs = []
    for value in (0.0, poison_value(kind)):
        dev_idx, dev_feat, lives = [], [], []
        for t, full in enumerate(fulls):
            named = torch.from_numpy((rows_ref[t] >= 0) & (rows_ref[t] < cap))
            f = torch.full((full.shape[0], 8), value, dtype=torch.float16)
            f[named] = TU.features(full.shape[0], 8, torch.float16, 123 + t)[named]
            dev_idx.append(torch.from_numpy(full).to(cuda))
            dev_feat.append(f.to(cuda))
            lives.append(i32(cuda, [idxs[t].shape[0]]))
        u = ops.sparse_union(dev_idx, bs, shape, n_live=lives, static_num_out=cap)
        out = _union.add_fwd(dev_feat, u.src, u.n_out, u.n_out_dev[2:3])
        dout = TU.features(cap, 8, torch.float16, 131)
        dins = _union.add_bwd(dout.to(cuda), u.rows, [True] * 3)
        outs.append(dict(out=out, n_out_dev=u.n_out_dev, src=u.src, **{f"din{t}": d for t, d in enumerate(dins)}))
    same_outputs(outs[0], outs[1], f"union unnamed {kind}")
    found, _, live = outs[1]["n_out_dev"].cpu().tolist()
    assert found > cap == live and bool(torch.isfinite(outs[1]["out"]).all())


@pytest.mark.parametrize("dt,C", [("f16", 8), ("f16", 3), ("bf16", 40), ("f32", 3), ("f64", 3)])
@moves("union/add_fwd", "union/add_bwd")
def test_named_union(cuda, dt, C):
    """rows held by one, two and three operands; a single holder's row keeps its bits, NaN payload included"""
    idxs, feats, uniq, want, rows_ref, _, present = S.union_case(dt, C)
    n = uniq.shape[0]
    src = np.full((3, n), -1, dtype=np.int64)
    for t, r in enumerate(rows_ref):
        src[t, r[r >= 0]] = np.nonzero(r >= 0)[0]
    got = c_union_add_fwd([f.to(cuda) for f in feats], i32(cuda, src), n, 0xFF)
    same_but_nan_payload(got, want, f"union {dt} C={C}")
    for t, r in enumerate(rows_ref):                                          # a row of one operand is a copy of it
        mine = np.nonzero((r >= 0) & (present[np.maximum(r, 0)] == 1))[0]
        same_bits(got[torch.from_numpy(r[mine]).to(cuda)], feats[t][torch.from_numpy(mine)], "a single holder's bits")
    dout = nf.poisoned(rc.features(n, C, DT[dt], 5), nf.Poison(torch.tensor([3]), torch.tensor([n // 2]), torch.tensor([n - 1]),
                                                              torch.tensor([0])))
    dins = c_union_add_bwd(dout.to(cuda), [i32(cuda, r) for r in rows_ref], 0xFF)
    for t, r in enumerate(rows_ref):
        rr = torch.from_numpy(r)
        same_bits(dins[t], torch.where((rr >= 0)[:, None], dout[rr.clamp_min(0)], torch.zeros_like(dout[:1])), f"din {t}")


# ========================================================================================= corners, interpolation, grouping
@functools.lru_cache(maxsize=None)
def interp_tables():
    """the reference corner table of the 3-d scene (hash form) and its transposed list"""
    import test_gpu_interp as TI
    sc = TI.scene(3)
    rows, w = sc.ref(True)
    offsets, lst = ri.transposed(rows, len(sc.full))
    return sc, rows, w, offsets, lst


def dev_tables(dev):
    sc, rows, w, offsets, lst = interp_tables()
    full = np.zeros((rows.size,), dtype=np.int32)
    full[:lst.shape[0]] = lst
    return i32(dev, rows), torch.from_numpy(w).to(dev), i32(dev, offsets), i32(dev, full)


def rounded(acc, dt):
    return torch.from_numpy(acc).to(DT[dt])


def raised(host, dt):
    return host.double().numpy() if dt == "f64" else host.float().numpy()


@moves("interp/corners_ranked", "interp/corners_hash")
def test_dirty_corners(cuda):
    import test_gpu_interp as TI
    sc = TI.scene(3)
    rows, w = sc.ref(True)
    out = both(lambda fill: c_corners(cuda, sc, sc.full, sc.n_live, None, fill), "corners, hash form")
    np.testing.assert_array_equal(out["rows"].cpu().numpy(), rows)
    same_bits(out["weights"], torch.from_numpy(w), "weights")
    rows, w = sc.ref(True, False)
    out = both(lambda fill: c_corners(cuda, sc, sc.ordered, sc.n_live_ordered,
                                      c_rankmap_from_sorted(cuda, sc.ordered, TI.NV, TI.B, sc.shape, fill), fill),
               "corners, rank form over a map built in a dirty buffer")
    np.testing.assert_array_equal(out["rows"].cpu().numpy(), rows)
    same_bits(out["weights"], torch.from_numpy(w), "weights")


@pytest.mark.parametrize("dt,C", [("f16", 8), ("f16", 520), ("f32", 3), ("f64", 3)])
@moves("interp/fwd", "interp/bwd", "query/group_fwd", "query/group_bwd")
def test_dirty_interp_and_group(cuda, dt, C):
    sc, rows, w, offsets, lst = interp_tables()
    drows, dw, doff, dlst = dev_tables(cuda)
    n, N, K = len(sc.full), rows.shape[0], rows.shape[1]
    acc = np.float64 if dt == "f64" else np.float32
    g = torch.Generator().manual_seed(C)
    vfeat = torch.randn((n, C), generator=g, dtype=torch.float64).to(DT[dt])
    dout = torch.randn((N, C), generator=g, dtype=torch.float64).to(DT[dt])
    nl = i32(cuda, [sc.n_live])
    out = both(lambda fill: c_interp_fwd(vfeat.to(cuda), drows, dw, fill), "interp fwd")["out"]
    same_bits(out, rounded(ri.forward(raised(vfeat, dt), rows, w, acc), dt), "interp forward")
    dv = both(lambda fill: c_interp_bwd(dout.to(cuda), K, dw, doff, dlst, n, nl, fill), "interp bwd")["out"]
    same_bits(dv, rounded(ri.backward(raised(dout, dt), rows, w, n, sc.n_live, acc), dt), "interp backward")
    grouped = both(lambda fill: c_group_fwd(vfeat.to(cuda), drows, fill), "group fwd")["out"]
    want = torch.where(torch.from_numpy(rows >= 0)[:, :, None], vfeat[torch.from_numpy(np.maximum(rows, 0)).long()],
                       torch.zeros((), dtype=DT[dt]))
    same_bits(grouped, want, "group forward")
    gout = torch.randn((N, K, C), generator=g, dtype=torch.float64).to(DT[dt])
    dv = both(lambda fill: c_group_bwd(gout.to(cuda), doff, dlst, n, nl, fill), "group bwd")["out"]
    want = ri.backward(raised(gout, dt).reshape(N * K, C), rows.reshape(-1, 1), np.ones((N * K, 1), dtype=np.float32), n,
                       sc.n_live, acc)                                         # (the table as N * K points of one slot)
    same_bits(dv, rounded(want, dt), "group backward")


@pytest.mark.parametrize("kind", ["nan", "inf"])
@moves("interp/corners_hash", "interp/fwd", "interp/bwd", "pointvoxel/groups")
def test_unnamed_interp_through_the_static_path(cuda, kind):
    """voxel rows behind n_live_dev, rows with a dead index row and rows no corner names; dout rows of points that are
    invalid or lie behind *n_points"""
    import test_gpu_interp as TI
    from spconv_amd.pytorch import functional as F
    sc, rows, w, _, _ = interp_tables()
    n, N, C = len(sc.full), rows.shape[0], 8
    named = np.zeros((n,), dtype=bool)
    named[rows[rows >= 0]] = True
    no_corner = ~(rows >= 0).any(axis=1)
    assert (~named[:sc.n_live]).sum() > 5 and (~named[sc.n_live:]).all() and no_corner.sum() > N - sc.n_points
    outs = []
    for value in (0.0, poison_value(kind)):
        x = TI.tensor_of(cuda, sc.full, sc.shape, C=C, dtype=torch.float16, n_live=sc.n_live, seed=3)
        feat = x.features.detach().clone()
        feat[torch.from_numpy(~named).to(cuda)] = value
        feat.requires_grad_(True)
        c = TI.run_corners(cuda, sc, x, True, with_groups=True)
        out = F.voxels_to_points_trilinear(feat, c)
        dout = torch.randn((N, C), generator=torch.Generator().manual_seed(4), dtype=torch.float64).half()
        dout[torch.from_numpy(no_corner)] = value
        (grad,) = torch.autograd.grad(out, feat, dout.to(cuda))
        outs.append(dict(out=out.detach(), grad=grad))
    same_outputs(outs[0], outs[1], f"interp unnamed {kind}")
    assert bool(torch.isfinite(outs[1]["out"]).all()) and not bool(outs[1]["grad"][sc.n_live:].any())


@pytest.mark.parametrize("kind", ["nan", "inf"])
@moves("interp/fwd", "interp/bwd", "query/group_fwd", "query/group_bwd")
def test_unnamed_table_entries(cuda, kind):
    """corner_w entries whose corner_rows entry is -1, and dout entries of neighbour slots with rows == -1"""
    sc, rows, w, offsets, lst = interp_tables()
    drows, dw, doff, dlst = dev_tables(cuda)
    n, N, K, C = len(sc.full), rows.shape[0], rows.shape[1], 8
    g = torch.Generator().manual_seed(9)
    vfeat = torch.randn((n, C), generator=g).half().to(cuda)
    dout = torch.randn((N, C), generator=g).half().to(cuda)
    gout = torch.randn((N, K, C), generator=g).half()
    nl = i32(cuda, [sc.n_live])
    absent = torch.from_numpy(rows < 0)
    named = np.zeros((n,), dtype=bool)
    named[rows[rows >= 0]] = True
    outs = []
    for value in (0.0, poison_value(kind)):
        w2 = torch.from_numpy(w).clone()
        w2[absent] = value
        g2 = gout.clone()
        g2[absent] = value
        v2 = vfeat.clone()
        v2[torch.from_numpy(~named).to(cuda)] = value
        outs.append(dict(fwd=c_interp_fwd(vfeat, drows, w2.to(cuda), 0xFF),
                         bwd=c_interp_bwd(dout, K, w2.to(cuda), doff, dlst, n, nl, 0xFF),
                         group_fwd=c_group_fwd(v2, drows, 0xFF),
                         group_bwd=c_group_bwd(g2.to(cuda), doff, dlst, n, nl, 0xFF)))
    same_outputs(outs[0], outs[1], f"table entries {kind}")


@pytest.mark.parametrize("kind", ["nan", "inf"])
@moves("query/group_fwd", "query/group_bwd", "pointvoxel/groups")
def test_unnamed_group_through_the_static_path(cuda, kind):
    """a query's neighbour table over a level with n_live_dev (scene A of test_gpu_query): voxel rows that no slot names
    -- those behind the live count among them -- and dout entries of empty slots"""
    import queryscenes as qs
    import test_gpu_query as TQ
    from spconv_amd.pytorch import functional as F
    sc = qs.scene("A")
    C = 8
    x = TQ.tensor_of(cuda, sc.level, sc.shape, C=C, dtype=torch.float16, n_live=sc.n_live, seed=2)
    nb = TQ.run_query(cuda, sc, x, None, "none", with_groups=True)
    rows = nb.rows.cpu().numpy()
    named = np.zeros((sc.n,), dtype=bool)
    named[rows[rows >= 0]] = True
    assert not named[sc.n_live:].any() and (~named[:sc.n_live]).sum() >= 2 and (rows < 0).sum() > 1000
    outs = []
    for value in (0.0, poison_value(kind)):
        feat = x.features.detach().clone()
        feat[torch.from_numpy(~named).to(cuda)] = value
        feat.requires_grad_(True)
        out = F.group_voxels(feat, nb)
        dout = torch.randn(tuple(out.shape), generator=torch.Generator().manual_seed(5), dtype=torch.float64).half()
        dout[torch.from_numpy(rows < 0)] = value
        (grad,) = torch.autograd.grad(out, feat, dout.to(cuda))
        outs.append(dict(out=out.detach(), grad=grad))
    same_outputs(outs[0], outs[1], f"group unnamed {kind}")
    assert bool(torch.isfinite(outs[1]["out"]).all()) and not bool(outs[1]["grad"][sc.n_live:].any())


@pytest.mark.parametrize("dt,C", [("f16", 3), ("f16", 8), ("bf16", 8), ("f32", 3), ("f64", 3)])
@moves("interp/fwd", "interp/bwd", "query/group_fwd", "query/group_bwd")
def test_named_interp_and_group(cuda, dt, C):
    """IEEE as written: a live corner of weight exactly 0 on an Inf row gives NaN (it spreads; the header says so)"""
    sc, rows, w, p, zero_rows = S.interp_case(C)
    _, _, _, offsets, lst = interp_tables()
    drows, dw, doff, dlst = dev_tables(cuda)
    n, N, K = len(sc.full), rows.shape[0], rows.shape[1]
    acc = np.float64 if dt == "f64" else np.float32
    g = torch.Generator().manual_seed(C)
    vfeat = S.interp_poisoned(torch.randn((n, C), generator=g, dtype=torch.float64).to(DT[dt]), p, zero_rows)
    with np.errstate(invalid="ignore", over="ignore"):
        want = rounded(ri.forward(raised(vfeat, dt), rows, w, acc), dt)
    got = c_interp_fwd(vfeat.to(cuda), drows, dw, 0xFF)
    same_but_nan_payload(got, want, f"interp forward {dt} C={C}")
    assert int(torch.isnan(want).sum()) > 20 and int(torch.isinf(want).sum()) > 0
    grouped = c_group_fwd(vfeat.to(cuda), drows, 0xFF)
    same_bits(grouped, torch.where(torch.from_numpy(rows >= 0)[:, :, None], vfeat[torch.from_numpy(np.maximum(rows, 0)).long()],
                                   torch.zeros((), dtype=DT[dt])), "group forward moves the bits")
    # backward: poisoned dout rows of points whose corners are live rows below the live count
    grp = nf.group_of_entries(offsets)
    keep = grp < sc.n_live
    pb = nf.poison_rows_flat(grp[keep], lst[keep] // K, N, C, 43)
    dout = nf.poisoned(torch.randn((N, C), generator=g, dtype=torch.float64).to(DT[dt]), pb)
    nl = i32(cuda, [sc.n_live])
    with np.errstate(invalid="ignore", over="ignore"):
        want = rounded(ri.backward(raised(dout, dt), rows, w, n, sc.n_live, acc), dt)
    same_but_nan_payload(c_interp_bwd(dout.to(cuda), K, dw, doff, dlst, n, nl, 0xFF), want, f"interp backward {dt} C={C}")
    assert int(torch.isnan(want).sum()) > 0 and int(torch.isinf(want).sum()) > 0
    gout = dout[:, None, :].expand(N, K, C).contiguous()                      # every slot of a point carries its row
    with np.errstate(invalid="ignore", over="ignore"):
        want = rounded(ri.backward(raised(gout, dt).reshape(N * K, C), rows.reshape(-1, 1), np.ones((N * K, 1), np.float32), n,
                                   sc.n_live, acc), dt)
    same_but_nan_payload(c_group_bwd(gout.to(cuda), doff, dlst, n, nl, 0xFF), want, f"group backward {dt} C={C}")
    assert int(torch.isnan(want).sum()) > 0


# ========================================================================================= the claims
def test_cases_claim_every_key():
    claimed = {k for keys in CLAIMS.values() for k in keys}
    assert claimed >= REQUIRED, sorted(REQUIRED - claimed)
