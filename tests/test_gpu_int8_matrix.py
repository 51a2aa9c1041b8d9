"""Every int8 gather-GEMM INSTANCE and every edge of the quantised epilogue, bit for bit against refint8.py.

The float kernels have test_gpu_kernel_matrix.py; this is the same treatment of ops.igemm_fwd_int8 (spx_igemm_fwd_int8:
csrc/igemm_i8.hip, the streaming kernel of csrc/igemm_v4.h, the column-blocked instances of csrc/igemm_wide.hip).  A case
names its entry conditions -- scene, geometry, widths, table form, hint -- and the instance key (spx_launch_count) it must
reach; it snapshots that counter, calls the entry eagerly, asserts that the counter moved and compares EVERY output element
with the reference: the accumulator from coordinate-derived pairs (refconv.pairs, float64, exact) and the epilogue in numpy
float32, one rounding per operation.  int8, f32, f16 and bf16 outputs are compared for equality; only Sigmoid (the kernel
uses __expf) is held to the bound the float matrix applies to its fp32 sigmoid epilogue, assert_close_abs_sum with c = 1e-5.

Dispatch rules the keys are read off (expected_key below restates them; a host test holds every case to it):
  NKS 1 for padded C <= 64, else 2;  COUT 16 / 32 / 64: 128-row tiles (MB 2);  256 and the wide launch: 64-row tiles;
  COUT 128: MB 2 with row-order tables (a rows layout without the hint included), MB 1 with tables in tile order or a rows
  layout plus the sparse hint;  the streaming launch: a rows layout whose class word the host has read + the hint,
  identity_k >= 0, kv <= 32, COUT 64 / 128, C <= 128.

Content cases carry a host-side assertion that the reference data holds the edge they are about (rounding ties, both clip
ends, accumulators fp32 cannot hold, rows without a neighbour, the defaults); the host tests at the end pin the coverage
and show that the reference tells rounding half away, floor(v + 0.5), a +-127 clamp, a fused multiply-add, a dropped pair,
swapped channels and shifted per-channel vectors from the formula on that very data."""
import fnmatch
import functools
import zlib

import numpy as np
import pytest
import torch

import refint8
from refconv import out_spatial_shape, pairs
from test_gpu_kernel_matrix import GEOMS as _KM_GEOMS, SCENES, reachable, scene_indices
from util import assert_close_abs_sum, match_rows

GEOMS = dict(_KM_GEOMS)
GEOMS["k32"] = ([4, 4, 2], [2] * 3, [1] * 3, [1] * 3, False)      # kv 32: the largest the int8 entry accepts

STREAM = "igemm_i8_stream"
OUT_DTYPES = {"i8": torch.int8, "f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32}
TIE_SCALES, TIE_BIASES = (0.5, 0.25, 1.5), (0.0, 0.5, -0.5)


# ---------------------------------------------------------------- dispatch model
def pad16(c):
    return -(-c // 16) * 16


def round_cout(k):
    for v in (16, 32, 64, 128, 256):
        if k <= v:
            return v
    return -(-k // 128) * 128


def expected_key(c):
    """The counter a case must move (csrc/igemm.hip spx_igemm_fwd_int8, csrc/igemm_i8.hip, launch_v4 / launch_v4w)."""
    ks, _, _, _, subm = GEOMS[c["geom"]]
    kv = int(np.prod(ks))
    C, K = pad16(c["C"]), round_cout(c["K"])
    nks = 1 if C <= 64 else 2
    hinted = c["table"] == "layout" and bool(c["hint"])
    if hinted and subm and kv <= 32 and K in (64, 128) and C <= 128:
        return STREAM
    if K > 256:
        return f"igemm_v4w/128/i8/fwd/{nks}/1"
    mb = 1 if (K == 256 or (K == 128 and (c["table"] == "sort" or hinted))) else 2
    return f"igemm_v4/{K}/{mb}/i8/fwd/{nks}/1"


def _key(abbr):
    if abbr == "stream":
        return STREAM
    if abbr in ("w1", "w2"):
        return f"igemm_v4w/128/i8/fwd/{abbr[1]}/1"
    cout, mb, nks = abbr.split(".")
    return f"igemm_v4/{cout}/{mb}/i8/fwd/{nks}/1"


# ---------------------------------------------------------------- the case table
def case(key, scene, geom, C, K, table="row", hint=False, out="i8", act=None, alpha=0.0, add=False, add_scale=0.37,
         content="uniform", wipe=False, name=None):
    """table: row | argsort (mask order over row-order tables) | sort (tile order) | layout | null (kv 1: no tables);
    hint: False | True (the class word read: sparse_hint + heavy_rows) | "stale" (a dense layout behind a hint)."""
    return dict(key=_key(key), scene=scene, geom=geom, C=C, K=K, table=table, hint=hint, out=out, act=act, alpha=alpha,
                add=add, add_scale=add_scale, content=content, wipe=wipe, name=name)


def _instance_cases():
    c = case
    return [
        # COUT 16
        c("16.2.1", "n1", "subm3", 16, 16, act="relu", add=True),
        c("16.2.1", "small", "subm3", 4, 5, "sort"),
        c("16.2.1", "n32769", "line", 16, 16, "layout", out="f32"),
        c("16.2.2", "mid", "s2", 128, 5, "argsort", add=True),
        c("16.2.2", "n65", "subm3d2", 72, 16, act="relu"),
        # COUT 32
        c("32.2.1", "n65", "subm3", 40, 32, add=True),
        c("32.2.1", "empty1", "s2", 32, 24, "sort", act="relu"),
        c("32.2.2", "mid", "k2s2", 96, 32, "argsort", add=True),
        c("32.2.2", "n33025", "line", 72, 32, "layout", act="relu"),
        # COUT 64
        c("64.2.1", "small", "subm3", 64, 64, act="relu", add=True),
        c("64.2.1", "mid", "k32", 40, 40),
        c("64.2.1", "n32769", "line", 64, 64, "layout", add=True),
        c("64.2.2", "n63", "subm3", 128, 64, "sort"),
        c("64.2.2", "empty1", "k2s2", 72, 40, act="relu"),
        c("64.2.2", "n33025", "line", 144, 64, "layout", hint=True, name="hint-C144-no-stream"),
        # COUT 128
        c("128.2.1", "small", "subm3", 64, 128),
        c("128.2.1", "n32769", "line", 32, 128, "layout", act="relu"),
        c("128.2.2", "mid", "s2", 128, 96, act="relu", add=True),
        c("128.2.2", "n63", "subm3", 128, 128, "argsort"),
        c("128.1.1", "small", "subm3", 64, 128, "sort", add=True),
        c("128.1.1", "n1", "subm3", 16, 96, "sort"),
        c("128.1.2", "mid", "subm3", 128, 128, "sort", act="relu"),
        c("128.1.2", "n33025", "line", 144, 128, "layout", hint=True, name="hint-C144-no-stream"),
        # COUT 256
        c("256.1.1", "small", "subm3", 64, 256),
        c("256.1.1", "n65", "subm3", 16, 200, "sort", add=True),
        c("256.1.1", "n32769", "line", 64, 256, "layout", act="relu"),
        c("256.1.2", "mid", "s2", 144, 256, act="relu", add=True),
        # beyond 256 columns
        c("w1", "small", "subm3", 64, 320, add=True),
        c("w1", "n65", "subm3", 40, 512, "sort", out="f16"),
        c("w1", "n33025", "line", 64, 320, "layout", hint=True, act="relu"),
        c("w2", "mid", "s2", 144, 320, act="relu", add=True),
        c("w2", "n33025", "line", 72, 320, "layout"),
        c("w2", "n63", "subm3", 128, 384, "argsort", out="f32"),
        # the streaming launch: COUT 64 / 128, each with one and with two reduction pieces; a dense layout behind a hint
        c("stream", "n33025", "line", 64, 64, "layout", hint=True, act="relu", add=True),
        c("stream", "n33025", "line", 72, 96, "layout", hint=True, add=True),
        c("stream", "n33025", "line", 40, 40, "layout", hint=True, out="f32"),
        c("stream", "n33025", "line", 128, 128, "layout", hint=True),
        c("stream", "n33025", "line", 64, 128, "layout", hint=True, out="bf16", act="relu"),
        c("stream", "n32769", "line", 64, 64, "layout", hint="stale", add=True, name="stale-hint"),
        c("stream", "n32769", "line", 128, 128, "layout", hint="stale", out="f16", act="relu", name="stale-hint"),
        # kernel volumes 1 (with and without tables), 3, 32
        c("32.2.1", "small", "k1", 32, 32, "null", add=True, name="kv1-null-tables"),
        c("32.2.1", "small", "k1", 32, 32, "row", add=True, name="kv1"),
        c("128.2.2", "n65", "k1", 128, 128, "null", act="relu", name="kv1-null-tables"),
        c("64.2.1", "small", "line", 16, 64, name="kv3"),
        c("32.2.1", "mid", "k32", 64, 32, "sort", name="kv32"),
        c("128.2.2", "mid", "k32", 144, 128, act="relu", add=True, name="kv32"),
        c("w1", "mid", "k32", 16, 320, name="kv32"),
    ]


def _content_cases():
    c = case
    out = []
    # rounding ties and both clip ends: a narrow, a tile-order, a 256-wide, a column-blocked and a streaming launch
    for content in ("ties", "clip"):
        out += [c("16.2.1", "small", "subm3", 16, 16, content=content, name=content),
                c("128.1.1", "mid", "subm3", 16, 128, "sort", content=content, name=content),
                c("256.1.1", "small", "subm3d2", 16, 200, content=content, name=content),
                c("w1", "small", "subm3", 16, 320, content=content, name=content),
                c("stream", "n33025", "line", 16, 64, "layout", hint=True, content=content, name=content)]
    # accumulators beyond 2^24 that fp32 cannot hold
    for o in ("i8", "f32"):
        out += [c("128.2.2", "small", "subm3", 144, 128, out=o, content="bigacc", name="big-acc"),
                c("w2", "small", "subm3", 144, 320, out=o, content="bigacc", name="big-acc")]
    # output rows without a neighbour: the epilogue of acc = 0
    out += [c("64.2.1", "mid", "s2", 32, 64, act="leaky", alpha=0.1, add=True, wipe=True, name="no-neighbour-rows"),
            c("256.1.2", "mid", "s2", 72, 256, out="f16", wipe=True, name="no-neighbour-rows"),
            c("w1", "mid", "k2s2", 64, 320, out="bf16", act="leaky", alpha=0.01, add=True, wipe=True,
              name="no-neighbour-rows")]
    # scale = None and bias = None; residuals without activation, with a negative add_scale
    out += [c("16.2.1", "small", "subm3", 16, 16, content="defaults", name="defaults"),
            c("128.2.1", "mid", "s2", 64, 128, add=True, content="defaults", name="defaults"),
            c("stream", "n33025", "line", 64, 64, "layout", hint=True, content="defaults", name="defaults"),
            c("64.2.2", "small", "subm3", 128, 64, add=True, add_scale=-0.37, name="negative-add-scale"),
            c("256.1.1", "mid", "k2s2", 64, 256, "sort", add=True, add_scale=-0.37, out="f16", name="negative-add-scale")]
    # LeakyReLU: both slopes, int8 and f16 output, a narrow, a column-blocked and a streaming launch
    out += [c("32.2.1", "small", "subm3", 64, 32, act="leaky", alpha=0.1, name="leaky"),
            c("64.2.2", "mid", "s2", 128, 64, out="f16", act="leaky", alpha=0.01, add=True, name="leaky"),
            c("w1", "small", "subm3", 64, 320, act="leaky", alpha=0.01, add=True, name="leaky"),
            c("stream", "n33025", "line", 128, 128, "layout", hint=True, act="leaky", alpha=0.1, add=True, name="leaky"),
            c("stream", "n33025", "line", 64, 64, "layout", hint=True, out="f16", act="leaky", alpha=0.01, name="leaky")]
    # Sigmoid (f32 output, bounded)
    out += [c("64.2.1", "small", "subm3", 64, 64, out="f32", act="sigmoid", name="sigmoid"),
            c("256.1.2", "mid", "s2", 144, 256, out="f32", act="sigmoid", add=True, name="sigmoid")]
    # float outputs equal the fp32 value of the formula rounded once
    sites = [("16.2.1", "n63", "subm3", 16, 16, "row", False), ("64.2.2", "small", "s2", 72, 40, "row", False),
             ("128.1.1", "n65", "subm3", 64, 128, "sort", False), ("256.1.2", "mid", "k2s2", 128, 200, "argsort", False),
             ("stream", "n33025", "line", 128, 64, "layout", True)]
    for i, (key, scene, geom, C, K, table, hint) in enumerate(sites):
        for j, o in enumerate(("f16", "bf16", "f32")):
            out.append(c(key, scene, geom, C, K, table, hint=hint, out=o, act=(None, "relu", "leaky")[(i + j) % 3], alpha=0.1,
                         add=(i + j) % 2 == 0, name="out-" + o))
    return out


CASES = _instance_cases() + _content_cases()


def _seed_id(c):
    opts = "".join(["-" + c["act"] + (f"{c['alpha']:g}" if c["act"] == "leaky" else "") if c["act"] else "",
                    f"-add{c['add_scale']:g}" if c["add"] else "", "-wipe" if c["wipe"] else "",
                    {False: "", True: "-hint", "stale": "-stale"}[c["hint"]]])
    return (f"{c['name'] + '-' if c['name'] else ''}{c['content']}-C{c['C']}-K{c['K']}-{c['scene']}-{c['geom']}-{c['table']}-"
            f"{c['out']}{opts}")


def _case_id(c):
    return c["key"].replace("/", ".") + "-" + _seed_id(c)


# ---------------------------------------------------------------- operands and their host-side content assertions
def _operands(c, n_in, n_out, kv, centre):
    """int8 features [n_in, C] and weights [K, kv, C], fp32 scale / bias [K] (None for the defaults), int8 add [n_out, K]
    (rows in the order the launch writes them) or None."""
    rng = np.random.default_rng(zlib.crc32(_seed_id(c).encode()))
    C, K, content = c["C"], c["K"], c["content"]
    scale = bias = None
    if content in ("ties", "clip"):
        # dyadic scales and half-integer biases over an integer accumulator: exact .5 fractions occur by themselves
        lo, hi = (-3, 4) if content == "ties" else (-127, 128)
        f = rng.integers(lo, hi, (n_in, C), dtype=np.int8)
        w = rng.integers(lo, hi, (K, kv, C), dtype=np.int8)
        scale = rng.choice(np.array(TIE_SCALES, np.float32), K)
        bias = rng.choice(np.array(TIE_BIASES, np.float32), K)
        if content == "clip":
            # at full-range operands nearly every sum saturates; three weight columns that read ONE channel of the row
            # itself (the centre offset of a SubM layer) put values at and between the clip ends:
            #   column 0: v = f / 2 (ties inside the range);  1: v = 1.5 f (127.5 at f = 85);  2: v = 2 f - 0.5 (-128.5 at -64)
            assert centre >= 0 and n_in >= 3 and K >= 3
            w[:3] = 0
            w[0, centre, 0], w[1, centre, 0], w[2, centre, 0] = 1, 3, 4
            scale[:3], bias[:3] = 0.5, (0.0, 0.0, -0.5)
            f[:3, 0] = (85, -64, 64)
    elif content == "bigacc":
        # sums of one sign near the operand range: 144 * 127 * 127 per neighbour, beyond 2^24 from eight neighbours on
        f = rng.integers(120, 128, (n_in, C), dtype=np.int8)
        sign = np.where(rng.integers(0, 2, K) == 0, -1, 1).astype(np.int8)
        w = (rng.integers(120, 128, (K, kv, C), dtype=np.int8) * sign[:, None, None]).astype(np.int8)
        scale = (rng.uniform(0.8, 1.2, K) * 2.0 ** -19).astype(np.float32)
        bias = rng.uniform(-5, 5, K).astype(np.float32)
    elif content == "defaults":
        f = rng.integers(-2, 3, (n_in, C), dtype=np.int8)
        w = rng.integers(-2, 3, (K, kv, C), dtype=np.int8)
    else:
        # full-range operands in every other case; the scale spreads the sums over the int8 range and past both ends
        # (the rule of test_gpu_int8._int8_case: rms of a sum of C * kv / 4 products)
        hi = 128 if zlib.crc32(_seed_id(c).encode()) & 1 else 9
        f = rng.integers(1 - hi, hi, (n_in, C), dtype=np.int8)
        w = rng.integers(1 - hi, hi, (K, kv, C), dtype=np.int8)
        mag = (hi * hi / 3.0) * np.sqrt(C * max(1.0, 0.25 * kv))
        scale = (rng.uniform(0.5, 1.5, K) * 60.0 / mag).astype(np.float32)
        bias = rng.uniform(-5, 5, K).astype(np.float32)
    add = None
    if c["add"]:
        add = rng.integers(-128, 128, (n_out, K), dtype=np.int8)
        add[0, 0], add[0, -1] = -128, 127                         # both ends of the residual's range
    return f, w, scale, bias, add


def assert_content(content, acc, v, want_i8):
    """The reference data really holds the edge the case is about.  acc: int32 accumulators, v: fp32 value in front of
    the rounding, want_i8: the expected int8 output."""
    if content == "ties":
        tie = ((v - np.floor(v)) == 0.5) & (np.abs(v) < 127)
        assert (tie & (v > 0)).mean() >= 0.10 and (tie & (v < 0)).mean() >= 0.10, "too few rounding ties"
        below = np.floor(v[tie]).astype(np.int64)
        assert (below % 2 == 0).any() and (below % 2 == 1).any(), "ties next to even and to odd integers"
    elif content == "clip":
        assert (want_i8 == -128).any() and (want_i8 == 127).any()
        assert (v > 128.5).any() and (v < -128.5).any()
        assert (v == 127.5).any() and (v == -128.5).any(), "the exact clip edges are missing"
        tie = ((v - np.floor(v)) == 0.5) & (np.abs(v) < 127)
        assert (tie & (v > 0)).any() and (tie & (v < 0)).any()
    elif content == "bigacc":
        assert np.abs(acc.astype(np.int64)).max() > 2 ** 24
        lost = acc.astype(np.float32).astype(np.float64) != acc.astype(np.float64)
        assert lost.mean() >= 0.10, f"only {lost.mean():.3f} of the accumulators are not representable in fp32"
    elif content == "defaults":
        sat = (want_i8 == 127) | (want_i8 == -128)
        assert sat.mean() < 0.5, "the output saturates"


# ---------------------------------------------------------------- scenes, pairs, rulebooks (shared, never modified)
@functools.lru_cache(maxsize=None)
def ref_pairs(scene, geom):
    idx, shape, bs = scene_indices(scene)
    ks, st, pd, dl, subm = GEOMS[geom]
    return pairs(idx, bs, shape, ks, st, pd, dl, subm)


_RB = {}


def rulebook(scene, geom, table):
    key = (scene, geom, table)
    if key not in _RB:
        from util import gpu_rulebook
        if len(_RB) > 24:
            _RB.clear()
        idx, shape, bs = scene_indices(scene)
        ks, st, pd, dl, subm = GEOMS[geom]
        sort = {"row": False, "sort": True, "layout": "layout"}[table]
        _RB[key] = gpu_rulebook(idx, bs, shape, ks, st, pd, dl, subm, do_sort=sort)[0]
    return _RB[key]


def _wipe(cand, perm, n_out):
    """rows of the launch whose every neighbour goes, and the pair list without them"""
    dead = np.arange(3, n_out, max(7, n_out // 40))
    gone = torch.from_numpy(perm[dead])
    return dead, [(k, i[~torch.isin(o, gone)], o[~torch.isin(o, gone)]) for k, i, o in cand]


def expected(c, acc, scale, bias, add, mutate=None):
    return refint8.epilogue(acc, scale, bias, add, c["add_scale"] if c["add"] else 0.0, c["act"], c["alpha"], c["out"], mutate)


# ---------------------------------------------------------------- running a case
def _run(c, dev):
    from spconv_amd import _lib
    from spconv_amd.pytorch import ops
    L = _lib.load()
    idx, shape, bs = scene_indices(c["scene"])
    ks, st, pd, dl, subm = GEOMS[c["geom"]]
    kv = int(np.prod(ks))
    identity = kv // 2 if subm else -1
    C, K = c["C"], c["K"]
    rb = rulebook(c["scene"], c["geom"], c["table"] if c["table"] in ("sort", "layout") else "row")
    out_idx, cand = ref_pairs(c["scene"], c["geom"])
    n_in, n_out = idx.shape[0], out_idx.shape[0]
    assert rb.n_out == n_out and rb.n_in == n_in
    perm = match_rows(rb.out_indices.cpu().numpy(), out_idx.numpy(), out_spatial_shape(shape, ks, st, pd, dl, subm))
    f, w, scale, bias, add = _operands(c, n_in, n_out, kv, identity)
    # tables
    hint, hint_rows, blob, stale_before = False, 0, None, None
    if c["table"] == "null":
        assert kv == 1
        tabs = (None, None, None, 0)
    elif c["table"] == "row":
        tabs = (rb.pair_fwd, rb.mask_fwd, None, 0)
    elif c["table"] == "argsort":
        tabs = (rb.pair_fwd, rb.mask_fwd, ops.mask_argsort(rb.mask_fwd[:, :1].contiguous()), 0)
    else:
        tabs = ops.tables_of(rb, "fwd", K)
        assert tabs[3] == {"sort": 1, "layout": 2}[c["table"]], "the rulebook does not carry the table form"
    if c["hint"]:
        blob = tabs[2]
        sparse = ops.sparse_neighbourhoods(rb)            # the host reads the class word (and M) of this blob
        if c["hint"] == "stale":
            assert not sparse, "the scene is meant to be of the dense class"
            stale_before = blob._spx_heavy
            blob._spx_heavy = hint_rows = 4096
        else:
            assert sparse and rb.heavy_rows > 0, "the scene is meant to be of the sparse class"
            hint_rows = rb.heavy_rows
        hint = True
    dead = None
    if c["wipe"]:
        assert c["table"] == "row"
        dead, cand = _wipe(cand, perm, n_out)
        pair, mask = rb.pair_fwd.clone(), rb.mask_fwd.clone()
        pair[:, torch.from_numpy(dead).to(dev)] = -1
        mask[torch.from_numpy(dead).to(dev)] = 0
        tabs = (pair, mask, None, 0)
    # reference, in the launch's row order
    acc = refint8.int_acc(out_idx, cand, f, w.reshape(K, *ks, C), dev)[perm]
    v = refint8.pre_activation(acc, scale, bias, add, c["add_scale"] if c["add"] else 0.0)
    assert_content(c["content"], acc, v, refint8.quantise(v))
    if add is not None:
        assert (add == -128).any() and (add == 127).any()
    # the launch
    key = c["key"].encode()
    before, stream_before = L.spx_launch_count(key), L.spx_launch_count(STREAM.encode())
    assert before >= 0, f"unknown instance key {c['key']}"
    t = lambda a: None if a is None else torch.from_numpy(a).to(dev)
    act = {None: ops.Activation.None_, "relu": ops.Activation.ReLU, "leaky": ops.Activation.LeakyReLU,
           "sigmoid": ops.Activation.Sigmoid}[c["act"]]
    try:
        got = ops.igemm_fwd_int8(t(f), t(w.reshape(K, *ks, C)), tabs[0], tabs[1], tabs[2], n_out, identity,
                                 None if scale is None else torch.from_numpy(scale),
                                 None if bias is None else torch.from_numpy(bias), t(add),
                                 c["add_scale"] if c["add"] else 0.0, OUT_DTYPES[c["out"]], act, c["alpha"],
                                 tile_order=tabs[3], sparse_hint=hint, hint_rows=hint_rows)
        torch.cuda.synchronize()
    finally:
        if stale_before is not None:
            blob._spx_heavy = stale_before
    after = L.spx_launch_count(key)
    assert after > before, f"{c['key']} was not launched (counter {before} -> {after})"
    if c["key"] != STREAM:
        assert L.spx_launch_count(STREAM.encode()) == stream_before, "the streaming kernel ran"
    assert tuple(got.shape) == (n_out, K) and got.is_contiguous() and got.dtype == OUT_DTYPES[c["out"]]
    # every element
    if c["act"] == "sigmoid":
        A = np.abs(acc.astype(np.float64)) * np.abs(scale.astype(np.float64)) + np.abs(bias.astype(np.float64))
        if add is not None:
            A = A + np.abs(add.astype(np.float64) * np.float64(np.float32(c["add_scale"])))
        assert_close_abs_sum(got.cpu().numpy(), refint8.sigmoid64(v), A, torch.float32, 1e-5, name="sigmoid")
        return
    want = expected(c, acc, scale, bias, add)
    if c["out"] == "bf16":
        bad = got.cpu() != want
        assert not bool(bad.any()), f"{int(bad.sum())} of {bad.numel()} bf16 elements differ"
    else:
        np.testing.assert_array_equal(got.cpu().numpy(), want)
    if dead is not None:
        # rows without a neighbour: the epilogue of a zero accumulator, the residual and the activation included
        zero = expected(c, np.zeros((dead.size, K), np.int32), scale, bias, None if add is None else add[dead])
        rows = got[torch.from_numpy(dead).to(dev)].cpu()
        assert (acc[dead] == 0).all()
        assert torch.equal(rows, zero if c["out"] == "bf16" else torch.from_numpy(zero)), "rows without neighbours"
        if c["act"] == "leaky":
            assert (bias < 0).any(), "no negative bias to take the slope"


@pytest.mark.gpu
@pytest.mark.parametrize("c", CASES, ids=[_case_id(c) for c in CASES])
def test_int8_instance_bit_exact(cuda, c):
    _run(c, cuda)


@pytest.mark.gpu
@pytest.mark.parametrize("kv", [33, 45])
def test_kernel_volumes_beyond_32_are_refused(cuda, kv):
    """The entry takes kernel volumes up to 32 and says so; nothing is launched (the tables are those of the k45 layer)."""
    from spconv_amd import _lib
    from spconv_amd.pytorch import ops
    L = _lib.load()
    rb = rulebook("mid", "k45", "row")
    assert rb.kv == 45
    f = torch.ones((rb.n_in, 16), dtype=torch.int8, device=cuda)
    w = torch.ones((16, kv, 16), dtype=torch.int8, device=cuda)
    fams = (b"igemm_v4", b"igemm_v4w", STREAM.encode())
    before = [L.spx_launch_count(k) for k in fams]
    with pytest.raises(RuntimeError, match="int8 supports kernel volumes up to 32"):
        ops.igemm_fwd_int8(f, w, rb.pair_fwd, rb.mask_fwd, None, rb.n_out, kv // 2)
    assert [L.spx_launch_count(k) for k in fams] == before


# ---------------------------------------------------------------- CPU: coverage, the key rules and the checker
def _i8_reachable():
    keys = {k for k in reachable() if fnmatch.fnmatchcase(k, "igemm_v4/*/*/i8/*")}
    assert len(keys) == 12
    return keys | {"igemm_v4w/128/i8/fwd/1/1", "igemm_v4w/128/i8/fwd/2/1"}


def test_cases_claim_every_int8_instance():
    from spconv_amd import _lib
    L = _lib.load()
    claimed = {c["key"] for c in CASES}
    missing = _i8_reachable() - claimed
    assert not missing, f"int8 instances without a case: {sorted(missing)}"
    assert claimed <= _i8_reachable() | {STREAM}, sorted(claimed - _i8_reachable())
    for k in sorted(claimed):
        assert L.spx_launch_count(k.encode()) >= 0, k
    # the streaming kernel: both instantiations, each with one and with two reduction pieces; the class-word fallback
    stream = {(round_cout(c["K"]), pad16(c["C"]) > 64) for c in CASES if c["key"] == STREAM and c["hint"] is True}
    assert stream == {(64, False), (64, True), (128, False), (128, True)}, sorted(stream)
    assert any(c["key"] == STREAM and c["hint"] == "stale" for c in CASES)


def test_cases_name_the_key_the_dispatch_rules_give():
    for c in CASES:
        assert expected_key(c) == c["key"], (_case_id(c), expected_key(c))
        assert c["scene"] in SCENES and SCENES[c["scene"]][2] * SCENES[c["scene"]][3] <= 33025, "nothing larger is needed"
    assert len({_case_id(c) for c in CASES}) == len(CASES), "two cases share an id (and a seed)"
    # the entry conditions the issue lists
    by = lambda f: {f(c) for c in CASES}
    assert {"n1", "n63", "n65", "small", "empty1", "mid", "n32769", "n33025"} <= by(lambda c: c["scene"])
    assert {"subm3", "subm3d2", "s2", "k2s2", "line", "k1", "k32"} <= by(lambda c: c["geom"])
    assert {"row", "argsort", "sort", "layout", "null"} <= by(lambda c: c["table"])
    assert {4, 40, 72} <= by(lambda c: c["C"]) and {5, 40, 96, 200, 320} <= by(lambda c: c["K"])
    assert any(c["C"] == 144 and c["K"] == 128 and c["hint"] is True and c["key"] == "igemm_v4/128/1/i8/fwd/2/1" for c in CASES)
    for o in ("f16", "bf16", "f32"):
        keys = {c["key"] for c in CASES if c["out"] == o}
        for part in ("igemm_v4/16/", "igemm_v4/64/", "igemm_v4/128/1/", "igemm_v4/256/", STREAM):
            assert any(k.startswith(part) for k in keys), (o, part)


@functools.lru_cache(maxsize=None)
def _host_data(content):
    """Operands, accumulators and pairs of a content case on the CPU (the `small` scene, SubM 3x3x3)."""
    c = next(c for c in CASES if c["content"] == content and c["scene"] == "small" and c["geom"] == "subm3"
             and c["out"] == "i8")
    idx, _, _ = scene_indices("small")
    out_idx, cand = ref_pairs("small", "subm3")
    n = idx.shape[0]
    f, w, scale, bias, add = _operands(c, n, n, 27, 13)
    acc = refint8.int_acc(out_idx, cand, f, w.reshape(c["K"], 3, 3, 3, c["C"]))
    v = refint8.pre_activation(acc, scale, bias)
    assert_content(content, acc, v, refint8.quantise(v))
    return c, out_idx, cand, f, w, scale, bias, acc


def _differs(a, b):
    return not np.array_equal(a, b)


@pytest.mark.parametrize("content,mutate", [("ties", "half_away"), ("ties", "floor_half"), ("clip", "half_away"),
                                            ("clip", "floor_half"), ("clip", "clip127")])
def test_checker_tells_rounding_and_clamp_mistakes(content, mutate):
    c, _, _, _, _, scale, bias, acc = _host_data(content)
    want = refint8.epilogue(acc, scale, bias)
    bad = refint8.epilogue(acc, scale, bias, mutate=mutate)
    assert _differs(want, bad), f"{mutate} passes on the {content} data"
    if mutate != "clip127":       # ... and by more than a stray element
        assert (want != bad).mean() > 0.001


def test_checker_tells_a_fused_multiply_add_on_big_accumulators():
    c, _, _, _, _, scale, bias, acc = _host_data("bigacc")
    want = refint8.epilogue(acc, scale, bias, out="f32")
    bad = refint8.epilogue(acc, scale, bias, out="f32", mutate="fma64")
    assert (want != bad).mean() > 0.01, "a float64 multiply-add rounded once equals the formula on this data"


@pytest.mark.parametrize("content", ["ties", "clip", "bigacc"])
def test_checker_tells_a_dropped_pair_swapped_channels_and_shifted_vectors(content):
    c, out_idx, cand, f, w, scale, bias, acc = _host_data(content)
    K, C = c["K"], c["C"]
    want = refint8.epilogue(acc, scale, bias)
    w5 = w.reshape(K, 3, 3, 3, C)
    # one pair of a non-centre offset gone
    k = next(t[0] for t in cand if t[0] != 13 and t[1].numel() > 0)
    cut = [(kk, ii[1:], oo[1:]) if kk == k else (kk, ii, oo) for kk, ii, oo in cand]
    assert _differs(want, refint8.epilogue(refint8.int_acc(out_idx, cut, f, w5), scale, bias)), "a dropped pair passes"
    # two input channels of the features swapped (channels 4 and 5: none that the clip data's probe columns read)
    fs = f.copy()
    fs[:, [4, 5]] = f[:, [5, 4]]
    assert _differs(want, refint8.epilogue(refint8.int_acc(out_idx, cand, fs, w5), scale, bias)), "swapped channels pass"
    # scale and bias read one channel off
    assert _differs(want, refint8.epilogue(acc, np.roll(scale, 1), np.roll(bias, 1))), "shifted scale / bias pass"


def test_reference_epilogue_rounds_each_operation_in_float32():
    """the documented order on values where the order and the precision show"""
    acc = np.array([[16777217, -16777219, 3, 5]], np.int32)            # 2^24 + 1 -> 2^24;  -(2^24 + 3) -> -(2^24 + 4)
    one, zero = np.ones(4, np.float32), np.zeros(4, np.float32)
    v = refint8.epilogue(acc, one, zero, out="f32")
    assert v.dtype == np.float32 and v.tolist() == [[16777216.0, -16777220.0, 3.0, 5.0]]
    half = np.full(4, 0.5, np.float32)
    assert refint8.epilogue(acc, half, zero).tolist() == [[127, -128, 2, 2]]       # 1.5 -> 2, 2.5 -> 2
    assert refint8.epilogue(acc, half, zero, mutate="half_away").tolist() == [[127, -128, 2, 3]]
    assert refint8.epilogue(-acc, half, zero, mutate="floor_half").tolist() == [[-128, 127, -1, -2]]
    assert refint8.epilogue(-acc, half, zero).tolist() == [[-128, 127, -2, -2]]
    assert refint8.epilogue(-acc, half, zero, mutate="clip127").tolist() == [[-127, 127, -2, -2]]
    leaky = refint8.epilogue(np.array([[-10, 10]], np.int32), None, None, act="leaky", alpha=0.1, out="f32")
    assert leaky.tolist() == [[float(np.float32(-10) * np.float32(0.1)), 10.0]]
    add = np.array([[-128, 127]], np.int8)
    got = refint8.epilogue(np.zeros((1, 2), np.int32), None, None, add, -0.37, out="f32")
    assert got.tolist() == [[float(np.float32(-128) * np.float32(-0.37)), float(np.float32(127) * np.float32(-0.37))]]
