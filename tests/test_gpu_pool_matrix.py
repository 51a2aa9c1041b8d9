"""Every reachable pooling kernel INSTANCE (csrc/pool.hip) against the fp64 reference of refpool.py, element by element.

Each case names the op, the dtype, the row width C, a scene, a window geometry, the table form and the instance key
(include/spconv_amd.h: pool/<op>/<dt>/<piece>) the dispatcher must reach.  A case snapshots that key's counter, calls the
ops.indice_*pool* entry eagerly, asserts that the counter moved, maps the output rows to the reference's rows with
util.match_rows and compares every element: the max forward, the counts and everything int8 bit for bit, the three summing
ops with util.assert_close_abs_sum under c = (kv + 4) eps_acc -- the worst-case bound of a sum of kv terms with one extra
multiply and one reciprocal; eps_acc = 2^-24 where the kernel accumulates in fp32 (f16, bf16, f32), 2^-53 for f64.  At
kv = 27 that is 1.8e-6 A, and a missing pair costs about A / kv.  Operands are rounded to the case's dtype before the
reference sees them.

Table forms: `attached` carries the rulebook's masks (for_each_pair walks the set bits), `bare` is the same pair table
without an attached rulebook (mask == nullptr: every offset is visited, holes are idx < 0); `native` / `native_bare` go
through the ConvAlgo.Native entries (zero-initialised output).  The backward of a SubM pool walks without a mask in either
form.  No case hands a kernel a table that indexes out of range (asserted before every launch).

The module and global-pool cases at the end run the nn.Modules of pytorch/pool.py under the same bounds.
The CPU test test_cases_claim_every_pool_instance holds the table to all 34 instances."""
import functools
import zlib

import numpy as np
import pytest
import torch

import refpool
from refconv import out_spatial_shape, pairs
from util import assert_close_abs_sum, match_rows

F16, BF16, F32, F64, I8 = torch.float16, torch.bfloat16, torch.float32, torch.float64, torch.int8
DTN = {F16: "f16", BF16: "bf16", F32: "f32", F64: "f64", I8: "i8"}
OPS = ("max_fwd", "max_bwd", "avg_fwd", "avg_bwd")
BITS = {F16: torch.int16, BF16: torch.int16, F32: torch.int32, F64: torch.int64, I8: torch.int8}


# ---------------------------------------------------------------- dispatch model (launch_pool / dispatch_pool)
def pool_key(op, dtype, C):
    """launch_pool: 16-byte pieces (V = 4 / 2 / 8 / 8 / 16 elements) when C is a multiple of V, one element otherwise"""
    v = 16 // torch.empty((), dtype=dtype).element_size()
    return f"pool/{op}/{DTN[dtype]}/{'v' if C % v == 0 else 's'}"


def reachable():
    """dispatch_pool: four ops x {f32, f64, f16, bf16} x two pieces, and int8 for the max forward only"""
    keys = {f"pool/{op}/{dt}/{p}" for op in OPS for dt in ("f16", "bf16", "f32", "f64") for p in "vs"}
    return keys | {"pool/max_fwd/i8/v", "pool/max_fwd/i8/s"}


def eps_acc(dtype):
    return 2.0 ** -53 if dtype == F64 else 2.0 ** -24


# ---------------------------------------------------------------- scenes and geometries
GEOMS = {
    # ksize, stride, padding, dilation, subm
    "k2s2": ([2, 2, 2], [2] * 3, [0] * 3, [1] * 3, False),         # kv 8
    "s2": ([3, 3, 3], [2] * 3, [1] * 3, [1] * 3, False),           # kv 27
    "subm3": ([3, 3, 3], [1] * 3, [1] * 3, [1] * 3, True),
    "subm3d2": ([3, 3, 3], [1] * 3, [2] * 3, [2] * 3, True),
    "k32": ([2, 4, 4], [2] * 3, [0, 1, 1], [1] * 3, False),        # one untrimmed mask word
    "k45": ([5, 3, 3], [1] * 3, [2, 1, 1], [1] * 3, True),         # two words, 13-bit tail
    "k64": ([4, 4, 4], [2] * 3, [1] * 3, [1] * 3, False),          # two untrimmed words
    "k125": ([5, 5, 5], [1] * 3, [2] * 3, [1] * 3, True),          # four words, 29-bit tail
}

SCENES = {
    # kind, shape, voxels per scene, batch, seed (the small scenes of test_gpu_kernel_matrix.py)
    "small": ("u", [16, 16, 16], 1500, 2, 1),
    "mid": ("u", [20, 20, 20], 2500, 1, 2),
    "n1": ("u", [4, 4, 4], 1, 1, 3),
    "n63": ("u", [6, 6, 6], 63, 1, 4),
    "n65": ("u", [6, 6, 6], 65, 1, 5),
    "empty1": ("gap", [16, 16, 16], 800, 3, 10),         # batch 1 of 3 holds nothing
    "n64": ("u", [6, 6, 6], 64, 1, 14),                  # at C = 16 fp32: 64 x 4 pieces fill one 256-thread block exactly
}
STATIC_EXTRA = 37                                        # dead rows of a static-shape table


@functools.lru_cache(maxsize=None)
def scene_indices(name):
    from spconv_amd.utils import synthetic
    kind, shape, n, bs, seed = SCENES[name]
    idx = synthetic.uniform_scene(shape, n, bs, seed)
    if kind == "gap":
        idx = idx[idx[:, 0] != 1]
    else:
        assert idx.shape[0] == n * bs
    return np.ascontiguousarray(idx.astype(np.int32)), shape, bs


@functools.lru_cache(maxsize=None)
def ref_pairs(scene, geom, dev):
    idx, shape, bs = scene_indices(scene)
    ks, st, pd, dl, subm = GEOMS[geom]
    return pairs(idx, bs, shape, ks, st, pd, dl, subm, device=dev)


@functools.lru_cache(maxsize=32)
def rulebook(scene, geom, static):
    from util import gpu_rulebook
    idx, shape, bs = scene_indices(scene)
    ks, st, pd, dl, subm = GEOMS[geom]
    kw = {}
    if static:
        kw["static_num_out"] = ref_pairs(scene, geom, "cuda:0")[0].shape[0] + STATIC_EXTRA
    return gpu_rulebook(idx, bs, shape, ks, st, pd, dl, subm, need_bwd_table=True, **kw)[0]


# ---------------------------------------------------------------- the case table
def case(op, dtype, C, scene, geom, table="attached", content="uniform", name=None, init_zero=False, quirks=False,
         lowered=False):
    return dict(op=op, dtype=dtype, C=C, scene=scene, geom=geom, table=table, content=content, name=name,
                init_zero=init_zero or table.startswith("native"), quirks=quirks, lowered=lowered,
                key=pool_key(op, dtype, C))


WIDTHS = {F32: (1, 6, 4, 20), F64: (3, 2, 6), F16: (20, 1, 8, 64), BF16: (12, 16), I8: (24, 16, 32)}


def _instance_cases():
    sites = [("small", "s2"), ("mid", "k2s2"), ("n63", "subm3"), ("empty1", "s2"), ("n65", "subm3"), ("n1", "s2"),
             ("small", "subm3d2"), ("empty1", "k2s2"), ("mid", "subm3"), ("n1", "subm3"), ("n65", "s2"), ("n63", "k2s2")]
    out, i = [], 0
    for op in OPS:
        for dtype in (F16, BF16, F32, F64, I8):
            if dtype == I8 and op != "max_fwd":
                continue
            for C in WIDTHS[dtype]:
                i += 1
                scene, geom = sites[i % len(sites)]
                content = "uniform" if op.startswith("avg") or (op == "max_fwd" and i % 2) else "ties"
                out.append(case(op, dtype, C, scene, geom, ["attached", "bare"][(i // 2) % 2], content))
    return out


def _other_cases():
    out = []
    # kernel volumes beyond one mask word: the two-word walk, the untrimmed last word, four words
    for i, op in enumerate(OPS):
        content = "uniform" if op.startswith("avg") else "ties"
        for j, (dtype, C) in enumerate((([F16, BF16][i % 2], 16), (F32, 6))):
            out.append(case(op, dtype, C, ["mid", "small"][j], "k45", ["attached", "bare"][(i + j) % 2], content))
            out.append(case(op, dtype, C, ["small", "mid"][j], "k64", ["bare", "attached"][(i + j) % 2], content))
        out.append(case(op, [BF16, F16][i % 2], 8, "mid", "k32", ["bare", "attached"][i % 2], content))
        out.append(case(op, F32, 4, "n65", "k32", ["attached", "bare"][i % 2], content))
        out.append(case(op, [F16, BF16, F32, F64][i], 8, "mid", "k125", ["attached", "bare"][i % 2], content))
        # both table forms of every backward op over one regular and one SubM table
        if op.endswith("bwd"):
            for table in ("attached", "bare"):
                out.append(case(op, F16, 8, "small", "s2", table, content))
                out.append(case(op, F32, 5, "n65", "subm3", table, content))
        # one SubM scene of exactly 64 voxels at C = 16 fp32: the grid ends on a block edge
        out.append(case(op, F32, 16, "n64", "subm3", "attached", content, name="full-block"))
    # the zero-initialised (ConvAlgo.Native) flavour on features that are all negative
    out.append(case("max_fwd", F16, 8, "small", "s2", "native", "negative", name="init-zero"))
    out.append(case("max_fwd", F32, 6, "mid", "k2s2", "native_bare", "negative", name="init-zero"))
    out.append(case("max_fwd", BF16, 16, "n65", "subm3", "bare", "negative", name="init-zero", init_zero=True))
    out.append(case("max_bwd", F32, 4, "small", "s2", "native", "ties", name="init-zero"))
    out.append(case("max_bwd", BF16, 12, "mid", "k2s2", "native_bare", "ties", name="init-zero"))
    # the reference kernel's arithmetic of the average backward (it multiplies by the count)
    out.append(case("avg_bwd", F32, 4, "small", "s2", "attached", "uniform", name="quirks", quirks=True))
    out.append(case("avg_bwd", F16, 20, "n65", "subm3", "bare", "uniform", name="quirks", quirks=True))
    # content edges of the max pool
    for dtype, C, scene, geom in ((F16, 8, "small", "s2"), (BF16, 12, "n65", "subm3"), (F32, 6, "mid", "k2s2")):
        for op in ("max_fwd", "max_bwd"):
            for content in ("nan", "neginf", "lowest"):
                out.append(case(op, dtype, C, scene, geom, "attached", content, name=content))
    # the backward is a function of (features, out, dout): an `out` lowered below the window's maximum at some elements
    # (a stale or edited forward result) makes `feat > out` pairs, which must receive nothing, like `feat < out` ones
    for dtype, C, scene, geom, table in ((F16, 8, "small", "s2", "attached"), (BF16, 12, "n65", "subm3", "bare"),
                                         (F32, 6, "mid", "k2s2", "bare")):
        out.append(case("max_bwd", dtype, C, scene, geom, table, "ties", name="out-below-max", lowered=True))
    for dtype, C, scene, geom in ((F16, 20, "small", "s2"), (BF16, 16, "n65", "k2s2"), (F32, 4, "mid", "k64")):
        for op in ("max_fwd", "max_bwd"):
            out.append(case(op, dtype, C, scene, geom, "static", "ties", name="dead-rows"))
    return out


CASES = _instance_cases() + _other_cases()


def _seed_id(c):
    return (f"{c['name'] + '-' if c['name'] else ''}{c['op']}-{DTN[c['dtype']]}-C{c['C']}-{c['scene']}-{c['geom']}-"
            f"{c['table']}-{c['content']}")


def _case_id(c):
    return c["key"].replace("/", ".") + "-" + _seed_id(c)


# ---------------------------------------------------------------- running a case
def _rounded(t, dtype):
    return t.to(dtype).to(torch.float64)


def _window_rows(cand, n_out):
    """the input rows of a few whole windows (every input of the chosen output rows)"""
    chosen = torch.arange(min(2, n_out - 1), n_out, max(5, n_out // 12))
    rows = [i.cpu()[torch.isin(o.cpu(), chosen)] for _, i, o in cand if i.numel()]
    return torch.unique(torch.cat(rows)) if rows else torch.zeros(0, dtype=torch.int64)


def _operands(c, n_in, n_rows_out, cand, n_out):
    """(f [n_in, C], dout [n_rows_out, C] in the GPU's row order): float64 holding values of the case's dtype"""
    g = torch.Generator(device="cpu").manual_seed(zlib.crc32(_seed_id(c).encode()))
    C, dtype, content = c["C"], c["dtype"], c["content"]
    if dtype == I8:
        f = torch.randint(-3 if content == "ties" else -128, 4 if content == "ties" else 128, (n_in, C),
                          generator=g).to(torch.float64)
    elif content == "uniform":
        f = torch.rand((n_in, C), generator=g, dtype=torch.float64) * 2 - 1
    elif content == "negative":
        f = -(torch.rand((n_in, C), generator=g, dtype=torch.float64) * 2 + 2.0 ** -6)
    else:           # few distinct values: windows tie
        f = torch.randint(-8, 9, (n_in, C), generator=g).to(torch.float64) / 4
    d = (torch.rand((n_rows_out, C), generator=g, dtype=torch.float64) * 2 - 1) * 0.2
    if content in ("nan", "neginf", "lowest"):
        value = {"nan": float("nan"), "neginf": float("-inf"), "lowest": refpool.lowest(dtype)}[content]
        f[_window_rows(cand, n_out)] = value                                  # whole windows of it
        if content != "neginf":
            f[torch.rand((n_in, C), generator=g) < 0.1] = value               # and scattered elements
    return _rounded(f, dtype), _rounded(d, dtype)


def _check(got, want, A, dtype, kv, name):
    assert got.is_contiguous() and tuple(got.shape) == tuple(want.shape), (name, tuple(got.shape), tuple(want.shape))
    c = (kv + 4) * eps_acc(dtype)
    a, r, A = got.double().cpu().numpy(), want.cpu().numpy(), A.cpu().numpy()
    if dtype == F16:
        # below 2^-14 fp16 is subnormal: half an ulp of the output is the fixed 2^-25 there, which u |ref| does not express
        tiny = np.abs(r) < 2.0 ** -14
        bad = tiny & (np.abs(a - r) > 2.0 ** -25 + c * A)
        assert not bad.any(), f"{name}: {int(bad.sum())} subnormal-range elements outside 2^-25 + {c:g} A"
        a = np.where(tiny, r, a)
    assert_close_abs_sum(a, r, A, dtype, c, name=name)


def _assert_bits(got, want, dtype, name):
    """bit for bit: `want` is float64 holding values of `dtype`"""
    assert got.dtype == dtype and got.is_contiguous() and tuple(got.shape) == tuple(want.shape), name
    np.testing.assert_array_equal(got.view(BITS[dtype]).cpu().numpy(), want.to(dtype).view(BITS[dtype]).cpu().numpy(),
                                  err_msg=name)


def _in_bounds(table, n_src):
    assert table.dtype == torch.int32 and table.is_contiguous()
    if table.numel():
        assert int(table.min()) >= -1 and int(table.max()) < n_src, "table indexes out of range"


def _run(c, dev):
    from spconv_amd import _lib, constants
    from spconv_amd.pytorch import ops
    L = _lib.load()
    idx, shape, bs = scene_indices(c["scene"])
    ks, st, pd, dl, subm = GEOMS[c["geom"]]
    kv = int(np.prod(ks))
    op, dtype, C, table = c["op"], c["dtype"], c["C"], c["table"]
    static = table == "static"
    rb = rulebook(c["scene"], c["geom"], static)
    out_idx, cand = ref_pairs(c["scene"], c["geom"], str(dev))
    n_in, n_out = idx.shape[0], out_idx.shape[0]
    rows = rb.n_out                                 # rows of the GPU's output tensor (dead rows included)
    assert rb.n_in == n_in and rows == n_out + (STATIC_EXTRA if static else 0)
    if static:
        assert int(rb.n_out_dev[0]) == n_out
        assert bool((rb.out_indices[n_out:] == -1).all())
    out_shape = out_spatial_shape(shape, ks, st, pd, dl, subm)
    perm = torch.from_numpy(match_rows(rb.out_indices[:n_out].cpu().numpy(), out_idx.cpu().numpy(), out_shape)).to(dev)

    def gpu_order(t, fill=0.0):                     # reference rows -> the GPU's rows, dead rows `fill`
        res = torch.full((rows,) + tuple(t.shape[1:]), fill, dtype=t.dtype, device=dev)
        res[:n_out] = t[perm]
        return res

    f, d_gpu = _operands(c, n_in, rows, cand, n_out)
    f, d_gpu = f.to(dev), d_gpu.to(dev)
    if static:
        d_gpu[n_out:] = 1000.0                      # a dead row's gradient must reach no input
    d = torch.empty((n_out, C), dtype=torch.float64, device=dev)
    d[perm] = d_gpu[:n_out]                         # dout in the reference's row order
    fg, dg = f.to(dtype), d_gpu.to(dtype)

    fwd = op.endswith("fwd")
    if table in ("native", "native_bare"):
        assert not subm
        native = ops.attach_rulebook(rb.pair_native, rb) if table == "native" else rb.pair_native.clone()
        _in_bounds(native[0], n_in)
        _in_bounds(native[1], rows)
    else:
        tab = rb.pair_fwd if fwd else rb.pair_bwd
        _in_bounds(tab, n_in if fwd else rows)
        assert tuple(tab.shape) == (kv, rows if fwd else n_in)
        tab = tab.clone() if table == "bare" else ops.attach_rulebook(tab, rb)
        assert (ops.rulebook_of(tab) is None) == (table == "bare")

    key = c["key"].encode()
    before = L.spx_launch_count(key)
    assert before >= 0, f"unknown instance key {c['key']}"
    want = A = cnt_got = None
    if op == "max_fwd":
        want = gpu_order(refpool.max_fwd(cand, f, n_out, dtype, init_zero=c["init_zero"]))
        if table in ("native", "native_bare"):
            got = ops.indice_maxpool(fg, native, rb.num_per_loc, rows)
        else:
            got = ops.indice_maxpool_implicit_gemm(fg, tab, rows, init_zero=c["init_zero"])
    elif op == "max_bwd":
        out = refpool.max_fwd(cand, f, n_out, dtype, init_zero=c["init_zero"])
        if c["lowered"]:                            # (multiples of 1/4 stay exact in every dtype)
            gen = torch.Generator().manual_seed(zlib.crc32(_seed_id(c).encode()) ^ 1)
            out = out - 0.5 * (torch.rand(out.shape, generator=gen) < 0.25).to(dev, torch.float64)
        ref = refpool.max_bwd(cand, f, out, d)
        want, A = ref.value, ref.abs_sum
        og = gpu_order(out).to(dtype)
        if table in ("native", "native_bare"):
            got = ops.indice_maxpool_backward(fg, og, dg, native, rb.num_per_loc)
        else:
            got = ops.indice_maxpool_implicit_gemm_backward(fg, og, dg, tab)
    elif op == "avg_fwd":
        ref = refpool.avg_fwd(cand, f, n_out)
        want, A = gpu_order(ref.value), gpu_order(ref.abs_sum)
        got, cnt_got = ops.indice_avgpool_implicit_gemm(fg, tab, rows, True)
        cnt_want = gpu_order(ref.count)
    else:
        cnt = refpool.counts(cand, n_out, dev)
        ref = refpool.avg_bwd(cand, d, cnt, n_in, reference_quirks=c["quirks"])
        want, A = ref.value, ref.abs_sum
        saved = constants.REFERENCE_QUIRKS
        try:
            constants.REFERENCE_QUIRKS = c["quirks"]
            got = ops.indice_avgpool_implicit_gemm_backward(dg, tab, gpu_order(cnt))
        finally:
            constants.REFERENCE_QUIRKS = saved
    torch.cuda.synchronize()
    after = L.spx_launch_count(key)
    assert after > before, f"{c['key']} was not launched (counter {before} -> {after})"
    if dtype == F64:
        assert L.spx_launch_count(b"pool/f64") > 0

    name = f"{op} {_seed_id(c)}"
    if op == "max_fwd" or dtype == I8:
        _assert_bits(got, want, dtype, name)
    else:
        assert got.dtype == dtype
        _check(got, want, A, dtype, kv, name)
    if cnt_got is not None:
        assert cnt_got.dtype == torch.int32
        np.testing.assert_array_equal(cnt_got.cpu().numpy(), cnt_want.cpu().numpy(), err_msg=name)
    if static and fwd:
        assert bool((got[n_out:] == 0).all()), "dead rows are not zero"


@pytest.mark.gpu
@pytest.mark.parametrize("c", CASES, ids=[_case_id(c) for c in CASES])
def test_pool_instance_against_fp64(cuda, c):
    _run(c, cuda)


# ---------------------------------------------------------------- modules
def _mod(kind, ndim, ks, st, pd, dl, dtype, C, shape, n, bs, subm=False, native=False):
    return dict(kind=kind, ndim=ndim, ks=ks, st=st, pd=pd, dl=dl, dtype=dtype, C=C, shape=shape, n=n, bs=bs, subm=subm,
                native=native)


MODULE_CASES = []
for _dt in (0, 1):
    _h = [F16, BF16]
    MODULE_CASES += [
        _mod("max", 1, [3], [2], [1], [1], [F32, _h[0]][_dt], 5 + 3 * _dt, [60], 25, 2),
        _mod("max", 2, [3, 3], [2, 2], [1, 1], [2, 2], [F32, _h[1]][_dt], 4 + 4 * _dt, [20, 20], 150, 2),     # dilated
        _mod("max", 3, [3] * 3, [2] * 3, [1] * 3, [1] * 3, [F32, _h[0]][_dt], 6 + 2 * _dt, [12] * 3, 400, 2),
        _mod("max", 4, [2] * 4, [2] * 4, [0] * 4, [1] * 4, [F32, _h[1]][_dt], 4 + 4 * _dt, [6] * 4, 300, 1),
        _mod("avg", 1, [3], [2], [1], [1], [F32, _h[1]][_dt], 4 + 4 * _dt, [60], 25, 2),
        _mod("avg", 2, [3, 3], [2, 2], [1, 1], [2, 2], [F32, _h[0]][_dt], 5 + 3 * _dt, [20, 20], 150, 2),     # dilated
        _mod("avg", 3, [3] * 3, [2] * 3, [1] * 3, [1] * 3, [F32, _h[1]][_dt], 6 + 10 * _dt, [12] * 3, 400, 2),
        _mod("max", 3, [3] * 3, [1] * 3, [1] * 3, [1] * 3, [F32, _h[0]][_dt], 4 + 4 * _dt, [12] * 3, 400, 2, subm=True),
        _mod("avg", 3, [3] * 3, [1] * 3, [1] * 3, [1] * 3, [F32, _h[1]][_dt], 4 + 4 * _dt, [12] * 3, 400, 1, subm=True),
        # kv 216: ConvAlgo.Native by default, the zero-initialised output
        _mod("max", 3, [6] * 3, [2] * 3, [2] * 3, [1] * 3, [F32, _h[0]][_dt], 4 + 4 * _dt, [16] * 3, 900, 1, native=True),
    ]


def _mod_id(m):
    return (f"{m['kind']}{m['ndim']}d-{DTN[m['dtype']]}-C{m['C']}-k{m['ks'][0]}s{m['st'][0]}p{m['pd'][0]}d{m['dl'][0]}"
            f"{'-subm' if m['subm'] else ''}{'-native' if m['native'] else ''}")


def _make_module(m):
    import spconv_amd.pytorch as spconv
    from spconv_amd.pytorch import pool
    if m["subm"]:
        base = pool.SparseMaxPool if m["kind"] == "max" else pool.SparseAvgPool
        return base(m["ndim"], m["ks"], m["st"], m["pd"], m["dl"], subm=True)
    cls = getattr(spconv, f"Sparse{'Max' if m['kind'] == 'max' else 'Avg'}Pool{m['ndim']}d")
    return cls(m["ks"], m["st"], m["pd"], m["dl"])


def _module_scene(m, seed):
    from spconv_amd.utils import synthetic
    return np.ascontiguousarray(synthetic.uniform_scene(m["shape"], m["n"], m["bs"], seed).astype(np.int32))


def _module_reference(m, idx, f, y_indices, g_gpu, dev, init_zero):
    """(out, A_out or None, din, A_din, n_out, perm) of refpool for the module's geometry; g_gpu is in the GPU's rows"""
    out_idx, cand = pairs(idx, m["bs"], m["shape"], m["ks"], m["st"], m["pd"], m["dl"], m["subm"], device=str(dev))
    n_out = out_idx.shape[0]
    out_shape = out_spatial_shape(m["shape"], m["ks"], m["st"], m["pd"], m["dl"], m["subm"])
    perm = torch.from_numpy(match_rows(y_indices[:n_out].cpu().numpy(), out_idx.cpu().numpy(), out_shape)).to(dev)
    d = torch.empty((n_out, f.shape[1]), dtype=torch.float64, device=dev)
    d[perm] = g_gpu[:n_out]
    if m["kind"] == "max":
        out = refpool.max_fwd(cand, f, n_out, m["dtype"], init_zero=init_zero)
        back = refpool.max_bwd(cand, f, out, d)
        return out[perm], None, back.value, back.abs_sum, n_out, out_shape
    fw = refpool.avg_fwd(cand, f, n_out)
    back = refpool.avg_bwd(cand, d, fw.count, f.shape[0])
    return fw.value[perm], fw.abs_sum[perm], back.value, back.abs_sum, n_out, out_shape


@pytest.mark.gpu
@pytest.mark.parametrize("m", MODULE_CASES, ids=[_mod_id(m) for m in MODULE_CASES])
def test_pool_module_against_fp64(cuda, m):
    import spconv_amd.pytorch as spconv
    from spconv_amd.pytorch.core import ConvAlgo
    dtype, C = m["dtype"], m["C"]
    kv = int(np.prod(m["ks"]))
    idx = _module_scene(m, 21)
    g = torch.Generator().manual_seed(zlib.crc32(_mod_id(m).encode()))
    f = _rounded(torch.rand((idx.shape[0], C), generator=g, dtype=torch.float64) * 2 - 1, dtype).to(cuda)
    net = _make_module(m)
    assert (net.algo == ConvAlgo.Native) == m["native"]
    feats = f.to(dtype).requires_grad_(True)
    y = net(spconv.SparseConvTensor(feats, torch.from_numpy(idx).to(cuda), m["shape"], m["bs"]))
    n_rows = y.features.shape[0]
    gg = _rounded((torch.rand((n_rows, C), generator=g, dtype=torch.float64) * 2 - 1) * 0.2, dtype).to(cuda)
    (y.features * gg.to(dtype)).sum().backward()
    torch.cuda.synchronize()
    out, A_out, din, A_din, n_out, out_shape = _module_reference(m, idx, f, y.indices, gg, cuda, m["native"])
    assert n_rows == n_out and list(y.spatial_shape) == out_shape
    name = _mod_id(m)
    if m["kind"] == "max":
        _assert_bits(y.features.detach(), out, dtype, name + " out")
    else:
        _check(y.features.detach(), out, A_out, dtype, kv, name + " out")
    assert feats.grad is not None and feats.grad.dtype == dtype
    _check(feats.grad, din, A_din, dtype, kv, name + " din")


@pytest.mark.gpu
def test_quantised_max_pool_module_is_bit_exact_and_keeps_the_scale(cuda):
    import spconv_amd.pytorch as spconv
    m = _mod("max", 3, [2] * 3, [2] * 3, [0] * 3, [1] * 3, I8, 32, [12] * 3, 400, 2)
    idx = _module_scene(m, 22)
    g = torch.Generator().manual_seed(5)
    q = torch.randint(-128, 128, (idx.shape[0], m["C"]), generator=g).to(torch.int8)
    feats = torch._make_per_tensor_quantized_tensor(q.to(cuda), 0.037, 3)
    x = spconv.SparseConvTensor(feats, torch.from_numpy(idx).to(cuda), m["shape"], m["bs"])
    assert x.is_quantized
    y = _make_module(m)(x)
    torch.cuda.synchronize()
    assert y.features.dtype == torch.qint8 and y.features.q_scale() == 0.037 and y.features.q_zero_point() == 3
    out_idx, cand = pairs(idx, m["bs"], m["shape"], m["ks"], m["st"], m["pd"], m["dl"], False, device=str(cuda))
    out_shape = out_spatial_shape(m["shape"], m["ks"], m["st"], m["pd"], m["dl"], False)
    perm = torch.from_numpy(match_rows(y.indices.cpu().numpy(), out_idx.cpu().numpy(), out_shape)).to(cuda)
    want = refpool.max_fwd(cand, q.to(cuda).to(torch.float64), out_idx.shape[0], I8)[perm]
    _assert_bits(y.features.int_repr(), want, I8, "quantised max pool")


@pytest.mark.gpu
@pytest.mark.parametrize("kind,dtype", [("max", F32), ("max", F16), ("avg", F32), ("avg", BF16)])
def test_static_pool_module_equals_the_dynamic_one(cuda, kind, dtype):
    """static_num_out above the true output count: the live rows are the dynamic module's (and the reference's), the dead
    rows are zero, and the input gradient is the dynamic module's although the dead rows carry a gradient"""
    import spconv_amd.pytorch as spconv
    m = _mod(kind, 3, [3] * 3, [2] * 3, [1] * 3, [1] * 3, dtype, 8, [12] * 3, 400, 2)
    idx = _module_scene(m, 23)
    g = torch.Generator().manual_seed(9)
    f = _rounded(torch.randint(-8, 9, (idx.shape[0], m["C"]), generator=g).to(torch.float64) / 4, dtype).to(cuda)
    it = torch.from_numpy(idx).to(cuda)
    dyn_in = f.to(dtype).requires_grad_(True)
    y = _make_module(m)(spconv.SparseConvTensor(dyn_in, it, m["shape"], m["bs"]))
    n_out = y.features.shape[0]
    cap = n_out + 50
    gs = _rounded((torch.rand((cap, m["C"]), generator=g, dtype=torch.float64) * 2 - 1) * 0.2, dtype).to(cuda)
    gs[n_out:] = 1000.0
    net = _make_module(m)
    net.static_num_out = cap
    st_in = f.to(dtype).requires_grad_(True)
    ys = net(spconv.SparseConvTensor(st_in, it, m["shape"], m["bs"]))
    assert ys.features.shape[0] == cap
    assert bool((ys.indices[n_out:] == -1).all()) and bool((ys.indices[:n_out, 0] >= 0).all())
    perm = torch.from_numpy(match_rows(ys.indices[:n_out].cpu().numpy(), y.indices.cpu().numpy(),
                                       list(y.spatial_shape))).to(cuda)
    gd = torch.empty((n_out, m["C"]), dtype=torch.float64, device=cuda)
    gd[perm] = gs[:n_out]
    (y.features * gd.to(dtype)).sum().backward()
    (ys.features * gs.to(dtype)).sum().backward()
    torch.cuda.synchronize()
    assert torch.equal(ys.features.detach()[:n_out], y.features.detach()[perm])
    assert bool((ys.features.detach()[n_out:] == 0).all())
    assert torch.equal(st_in.grad, dyn_in.grad)
    # and both are the reference's
    out, A_out, din, A_din, n_ref, _ = _module_reference(m, idx, f, ys.indices, gs, cuda, False)
    assert n_ref == n_out
    if kind == "max":
        _assert_bits(ys.features.detach()[:n_out].contiguous(), out, dtype, "static out")
    else:
        _check(ys.features.detach()[:n_out].contiguous(), out, A_out, dtype, 27, "static out")
    _check(st_in.grad, din, A_din, dtype, 27, "static din")


# ---------------------------------------------------------------- global pools
GLOBAL_CASES = {
    # dtype, rows per scene, batch size, which scene is emptied (or None), rows given batch index -1
    "f16-5000-rows": (F16, 5000, 1, None, 0),            # beyond an fp16 count (2048)
    "bf16-5000-rows": (BF16, 5000, 1, None, 0),          # beyond a bf16 count (256)
    "f32": (F32, 700, 2, None, 0),
    "f32-empty-scene": (F32, 500, 3, 1, 0),
    "f16-empty-scene": (F16, 500, 3, 0, 0),
    "f32-batch-minus-one": (F32, 600, 2, None, 150),
    "bf16-batch-minus-one": (BF16, 600, 2, None, 150),
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(GLOBAL_CASES))
def test_global_pools_against_fp64(cuda, name):
    import spconv_amd.pytorch as spconv
    from spconv_amd.utils import synthetic
    dtype, n, bs, empty, minus = GLOBAL_CASES[name]
    C, shape = 8, [20, 20, 20]
    idx = np.ascontiguousarray(synthetic.uniform_scene(shape, n, bs, 31).astype(np.int32))
    if empty is not None:
        idx = idx[idx[:, 0] != empty]
    g = torch.Generator().manual_seed(zlib.crc32(name.encode()))
    if minus:
        idx[torch.randperm(idx.shape[0], generator=g)[:minus].numpy(), 0] = -1
    f = _rounded(torch.rand((idx.shape[0], C), generator=g, dtype=torch.float64) * 2 - 1, dtype)
    if minus:       # rows of no scene must not count: make them loud
        f[torch.from_numpy(idx[:, 0] == -1)] = 100.0
    f = f.to(cuda)
    x = spconv.SparseConvTensor(f.to(dtype), torch.from_numpy(idx).to(cuda), shape, bs)
    b = torch.from_numpy(idx[:, 0].copy()).to(cuda)
    got_max, got_mean = spconv.SparseGlobalMaxPool()(x), spconv.SparseGlobalAvgPool()(x)
    torch.cuda.synchronize()
    want_max = refpool.global_pool(b, f, bs, dtype, False)
    _assert_bits(got_max, want_max.value, dtype, name + " max")
    want = refpool.global_pool(b, f, bs, dtype, True)
    assert got_mean.dtype == dtype and tuple(got_mean.shape) == (bs, C)
    nan = torch.isnan(want.value)
    assert torch.equal(torch.isnan(got_mean), nan), "NaN exactly for the scenes without rows"
    if empty is not None:
        assert bool(nan[empty].all()) and int(nan.sum()) == C
        assert bool((got_max[empty].double() == refpool.lowest(dtype)).all())
    # half an ulp of the output + (n_rows + 2) 2^-24 mean|f|, n_rows the scene's own (folded into A: c is one number)
    rows = torch.stack([(b == s).sum() for s in range(bs)]).to(torch.float64).unsqueeze(1)
    keep = ~nan
    assert_close_abs_sum(got_mean.double()[keep].cpu().numpy(), want.value[keep].cpu().numpy(),
                         (want.abs_sum * (rows + 2))[keep].cpu().numpy(), dtype, 2.0 ** -24, name=name + " mean")


# ---------------------------------------------------------------- CPU: the table and the key grammar
def test_cases_claim_every_pool_instance():
    reach = reachable()
    assert len(reach) == 34
    claimed = {c["key"] for c in CASES}
    assert claimed <= reach, sorted(claimed - reach)
    assert not (reach - claimed), f"instances without a case: {sorted(reach - claimed)}"


def test_cases_cover_the_walks_and_forms_the_kernels_have():
    """the coverage the instance keys do not express: mask-word walks, table forms, flavours, content edges"""
    def has(**kw):
        return any(all(c[k] == v for k, v in kw.items()) for c in CASES)
    for op in OPS:
        for geom in ("k45", "k64"):
            assert has(op=op, geom=geom, dtype=F32) and (has(op=op, geom=geom, dtype=F16) or has(op=op, geom=geom, dtype=BF16))
        assert has(op=op, geom="k32") and has(op=op, geom="k125") and has(op=op, scene="n64", C=16, dtype=F32)
        for geom in ("k2s2", "s2", "subm3", "subm3d2"):
            assert has(geom=geom)
        if op.endswith("bwd"):
            assert has(op=op, table="bare") and has(op=op, table="attached")
    assert has(op="max_fwd", content="negative", init_zero=True) and has(op="avg_bwd", quirks=True)
    assert has(op="max_bwd", lowered=True)
    for dtype in (F16, BF16, F32):
        for op in ("max_fwd", "max_bwd"):
            for content in ("nan", "neginf", "lowest"):
                assert has(op=op, dtype=dtype, content=content)
            assert has(op=op, dtype=dtype, table="static")
    for scene in SCENES:
        assert has(scene=scene)
    want = {F32: {1, 6, 4, 20}, F64: {3, 2, 6}, F16: {20, 8, 64}, BF16: {12, 16}, I8: {24, 16, 32}}
    for dtype, widths in want.items():
        assert widths <= {c["C"] for c in CASES if c["dtype"] == dtype}


def test_pool_keys_parse():
    """spx_launch_count knows every pooling key and rejects malformed ones (host only: nothing launches)"""
    from spconv_amd import _lib
    L = _lib.load()
    for k in sorted(reachable()) + ["pool/f64", "pool/avg_bwd/i8/v"]:       # (int8 average: well formed, never built)
        assert L.spx_launch_count(k.encode()) >= 0, k
    for bad in ("pool", "pool/", "pool/max_fwd", "pool/max_fwd/f16", "pool/max_fwd/f16/", "pool/max_fwd/f16/x",
                "pool/max_fwd/f16/v/", "pool/max/f16/v", "pool/max_fwd/f8/v", "pool/max_fwd//v", "pool/f32",
                "pool/max_fwd/f16/vs"):
        assert L.spx_launch_count(bad.encode()) == -1, bad


@pytest.mark.parametrize("dtype", [F16, BF16, F32, F64])
def test_checker_rejects_a_missing_pair_and_a_wrong_divisor(dtype):
    """the bound itself, on the CPU: the reference rounded to the output dtype passes; one pair less, or the mean over kv
    instead of the pair count, does not"""
    from util import scene
    shape = [10, 10, 10]
    idx = scene(shape, 300, 1, 3)
    ks, kv = [3] * 3, 27
    out_idx, cand = pairs(idx, 1, shape, ks, [2] * 3, [1] * 3, [1] * 3, False)
    n_out = out_idx.shape[0]
    g = torch.Generator().manual_seed(1)
    f = _rounded(torch.rand((idx.shape[0], 4), generator=g, dtype=torch.float64) * 2 - 1, dtype)
    ref = refpool.avg_fwd(cand, f, n_out)
    _check(ref.value.to(dtype), ref.value, ref.abs_sum, dtype, kv, "exact")
    k, i, o = next(t for t in cand if t[1].numel() > 1)
    cut = [(kk, ii[1:], oo[1:]) if kk == k else (kk, ii, oo) for kk, ii, oo in cand]
    with pytest.raises(AssertionError):
        _check(refpool.avg_fwd(cut, f, n_out).value.to(dtype), ref.value, ref.abs_sum, dtype, kv, "cut")
    with pytest.raises(AssertionError):
        wrong = ref.value * ref.count.unsqueeze(1) / kv
        _check(wrong.to(dtype), ref.value, ref.abs_sum, dtype, kv, "kv divisor")
