"""Every code path of the normalisation kernels (csrc/norm.hip), every output element against refnorm.py.

The gather-GEMM kernels have test_gpu_kernel_matrix.py and the int8 ones test_gpu_int8_matrix.py; this is the same
treatment of BatchNorm / SyncBatchNorm through the C ABI: spx_batchnorm_fwd (training and inference), spx_batchnorm_bwd
(batch and running statistics), spx_batchnorm_fwd_stats and spx_batchnorm_local_stats with hand-built records, and the
SyncBatchNorm cut spx_batchnorm_local_stats / spx_batchnorm_bwd_sums / spx_batchnorm_bwd_apply.  Every output buffer
starts as NaN, the running buffers at non-trivial values and num_batches_tracked at 5.  Every element of y, dx, dweight,
dbias, sums, save_mean, save_invstd, the record, running_mean and running_var must satisfy

    |got - ref| <= u |ref| + c A                                   (util.assert_close_abs_sum: no free floor)

with ref the float64 reference of refnorm.py on the inputs as the kernel reads them, u half an ulp of the dtype the tensor
is written in and A the magnitude refnorm.py derives for that output -- for the variance-like outputs the SPREAD, so that
a channel of mean 1e3 and spread 1 is held as tightly as a centred one.  Exact: padding rows of y and dx are bit zero, y
is 0 wherever the reference pre-activation lies below minus its bound, record[0] is the live row count,
num_batches_tracked is 6.  Where the reference pre-activation is within 64 bounds of the ReLU kink the mask is anyone's
choice: dy is zeroed there for the kernel and the reference alike, and a case may lose at most 1 % of its elements so.

The constant c (C_BOUND), per output kind.  util.assert_close_abs_sum derives c = 1e-6 for fp32 accumulation in unknown
order.  Measured on MI355X over this table (the one failing case below left out): the worst excess
(|got - ref| - u |ref|) / A, next to the same figure for a straight fp32 evaluation of the formulas by torch on the host,
and the c in force with its margin over the measured figure:

    kind          kernel     fp32 yardstick   c        margin
    dbias         5.1e-8     4.0e-8           1e-6     20
    save_mean     3.1e-7     1.5e-7           1e-6     3.3
    running_mean  1.5e-7     1.4e-7           1e-6     6.6
    record (M2)   2.8e-6     1.5e-7           1e-5     3.6
    running_var   4.8e-7     5.6e-8           1e-5     21
    save_invstd   1.3e-6     5.4e-8           5e-6     3.8
    y             2.8e-6     (u only)         6e-6     2.1
    dweight       2.1e-7     9.0e-8           6e-6     29
    sums          2.1e-7     9.0e-8           6e-6     28
    dx            5.1e-7     1.7e-7           1.1e-5   22

dbias, save_mean and running_mean sit under 1e-6 / 8 or close to the yardstick and keep c = 1e-6.  The variance-like kinds
need more, and are more than an order of magnitude worse than the yardstick -- a FINDING about bn_partial_kernel, not
about the merge: a block forms M2 = sum d^2 - (sum d)^2 / rows with d = x - x0 around its FIRST ROW x0.  With
z0 = (x0 - mean) / sigma of that block and channel the two terms are (1 + z0^2) M2 and z0^2 M2, so the roundings of their
accumulations (about 4 u each: eight sequential additions per thread, then the DPP / LDS tree) are relative to
(1 + 2 z0^2) M2, not to M2.  Among the ~1e5 block-channels of this table the largest |z0| of Gaussian rows is ~4.3:
38 * 4 u = 9e-6, hence c = 1e-5 for the record and running_var; invstd = (var + eps)^-1/2 takes half of it, c = 5e-6.
What multiplies by invstd inherits that: y = x sc + (b - mean sc) errs by c_invstd |x - mean| |sc| <= c_invstd A_y plus
its own roundings (1e-6): c = 6e-6, likewise dweight and the sums through xhat; dx holds invstd twice (w invstd and xhat):
2 * 5e-6 + 1e-6.  Every c stays within 50 times the measured figure.

WHAT THE TABLE FOUND: case train-1000-16-f32 "cond1e4", the channel of mean -1e4 and spread 0.1.  With block means kept as
plain fp32 numbers in the records of a pass over the rows, the excess over u |ref| as a fraction of the spread was 6.8e-4
for the record's M2, 3.4e-4 for save_invstd and 6.7e-5 for running_var: a mean at -1e4 is good to u |mean| = 5e-4, the
means of two 63-row blocks differ by ~sigma / 8 = 0.012, and Chan's update squares that difference.  norm.hip now keeps
those means relative to row 0 of the matrix wherever a channel sits far from zero (|row 0| more than 16 times what the
first four rows differ by; every other channel keeps plain means and the bits of before) and adds it back once, to the
merged mean; after the change that case measures 7.2e-8 for M2, 2.2e-8 for save_invstd and 1.5e-8 for running_var.  Records that come from outside -- a
convolution's epilogue, another rank -- still hold plain fp32 means: that rounding is the record format's.
"""
import functools
import os
import re
import zlib

import numpy as np
import pytest
import torch

import refnorm
from util import HALF_ULP, assert_close_abs_sum

KINDS = ("y", "dx", "dweight", "dbias", "sums", "save_mean", "save_invstd", "record", "running_mean", "running_var")
C_BOUND = dict(y=6e-6, dx=1.1e-5, dweight=6e-6, dbias=1e-6, sums=6e-6, save_mean=1e-6, save_invstd=5e-6, record=1e-5,
               running_mean=1e-6, running_var=1e-5)
# half the spacing of the subnormals: below the smallest normal number u |ref| is not what a rounding costs (an fp16
# gradient of 1e-5 sits on a grid of 6e-8)
HALF_SUBNORMAL = {"float16": 2.0 ** -25, "bfloat16": 2.0 ** -134, "float32": 2.0 ** -150}
KINK_BOUNDS, KINK_SHARE = 64, 0.01
TORCH = {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32}
DTYPES = tuple(TORCH)
VPL = {"f16": 8, "bf16": 8, "f32": 4}
SHARDS = (0, 1, 333, 666)                      # test_gpu_syncbn_abi.py: an empty rank, a one-row rank, uneven counts
RECORD_ROWS = (0, 1, 2, 0, 3, 1, 2, 3)         # rows of record i % 8 (the last record of G > 1 is empty as well)
WORST, YARD = {}, {}                           # kind -> (excess, case): the kernels / a straight fp32 evaluation
MISSES = []                                    # what the running case has outside its bound (asserted at its end)


# ---------------------------------------------------------------- the case table
def case(entry, n, C, dt, live=None, relu=False, pdt="f32", affine=True, running=True, dparams=True, momentum=0.1,
         eps=1e-5, content="plain", G=0):
    """entry: train = spx_batchnorm_fwd (training) + spx_batchnorm_bwd (batch statistics) + the SyncBatchNorm cut on the
    same matrix (local_stats, bwd_sums, bwd_apply);  eval = spx_batchnorm_fwd (inference) + spx_batchnorm_bwd (running
    statistics);  records = spx_batchnorm_fwd_stats + spx_batchnorm_local_stats over G hand-built records;  sync = the
    SHARDS as ranks.  pdt: dtype of parameters and running buffers ("same" = the matrix's)."""
    c = dict(entry=entry, n=n, C=C, dt=dt, live=live, relu=relu, pdt=dt if pdt == "same" else pdt, affine=affine,
             running=running, dparams=dparams, momentum=momentum, eps=eps, content=content, G=G)
    c["id"] = "-".join(str(v) for v in (entry, n, C, dt, f"live{live}", "relu" if relu else "lin", f"p{c['pdt']}",
                                         "" if affine else "noaffine", "" if running else "norunning",
                                         "" if dparams else "nodparams", f"m{momentum}", f"e{eps}", content,
                                         f"G{G}") if v != "")
    return c


@functools.lru_cache(maxsize=None)
def _cases():
    out = []
    for dt in DTYPES:
        # piece counts: P = 1 ... 8, 16, 25, 32 (f32 also 64); wide: last block P = 1, serial, 8 / 16, three blocks
        widths = [8, 16, 24, 32, 40, 48, 56, 64, 128, 200, 256] + ([4, 12, 20] if dt == "f32" else [])
        for C in widths + [264, 280, 320, 520]:
            out.append(case("train", 300, C, dt, relu=C % 16 == 0))
        # row counts at the block boundaries
        for C in (16, 256):
            for n in (2, 63, 64, 65, 127, 128, 129, 1000):
                out.append(case("train", n, C, dt, relu=n % 2 == 1))
        # static rows in every dtype: a partly filled matrix, both clamps (f16 at C = 16: the n_live block below)
        for C in (64, 264 if dt != "f16" else 280):
            for live in (65, 1500, -3):
                out.append(case("train", 1000, C, dt, live=live, relu=True))
        out.append(case("eval", 300, 64, dt, relu=True))
        out.append(case("eval", 300, 280, dt))
        # records: one, a few, one full merge trip, one more, ~ a 400 k-row convolution's
        for C in (16, 264):
            for G in (1, 7, 2048, 2049, 4500):
                if dt == "f16" or G in (7, 2049):
                    out.append(case("records", 0, C, dt, G=G, relu=G == 7))
        for C in (24, 280):
            out.append(case("sync", sum(SHARDS), C, dt, relu=dt != "f32", eps=1e-3))
    out.append(case("sync", sum(SHARDS), 24, "f16", eps=1e-3))
    # the long cases: second batch trip + reload, the 1024-block cap, the grid-stride loop of the narrow apply kernels
    out.append(case("train", 66_000, 256, "f16", relu=True))
    out.append(case("train", 66_000, 256, "bf16"))
    out.append(case("train", 66_000, 64, "f32", relu=True))
    # the grid cap of the wide apply kernels
    out.append(case("train", 20_000, 520, "f16", relu=True))
    out.append(case("train", 11_000, 520, "bf16"))
    out.append(case("train", 5_500, 520, "f32", relu=True))
    # n_live: the padding holds 1e4
    for live in (1000, 999, 65, 64, 1, 0, 1500, -3):
        for entry in ("train", "eval"):
            for relu in (False, True):
                for C in (16, 264):
                    out.append(case(entry, 1000, C, "f16", live=live, relu=relu))
    # parameters
    for dt in ("f16", "bf16"):
        out.append(case("train", 300, 64, dt, pdt="same"))
        out.append(case("train", 300, 264, dt, pdt="same", relu=True))
        out.append(case("eval", 300, 64, dt, pdt="same", relu=True))
        out.append(case("records", 0, 16, dt, pdt="same", G=7))
        out.append(case("sync", sum(SHARDS), 24, dt, pdt="same", eps=1e-3))
    for dt in DTYPES:
        out.append(case("train", 300, 32, dt, affine=False, relu=True))
        out.append(case("eval", 300, 32, dt, affine=False))
        out.append(case("train", 300, 32, dt, running=False))
        out.append(case("train", 300, 32, dt, dparams=False, relu=True))
        out.append(case("train", 300, 32, dt, momentum=0.01, eps=1e-3))
        out.append(case("train", 300, 32, dt, momentum=1.0))
    # conditioning, by channel (see _inputs)
    out.append(case("train", 1000, 16, "f32", content="cond"))
    out.append(case("train", 1000, 16, "f32", content="cond1e4"))
    out.append(case("eval", 1000, 16, "f32", content="cond1e4"))
    out.append(case("train", 1000, 16, "f16", content="cond16"))
    ids = [c["id"] for c in out]
    assert len(set(ids)) == len(ids), [i for i in ids if ids.count(i) > 1]
    return out


def record_rows(G):
    rows = [RECORD_ROWS[i % 8] for i in range(G)]
    if G == 1:
        rows[0] = 3
    else:
        rows[-1] = 0
    return rows


# ---------------------------------------------------------------- which paths a case takes (csrc/norm.hip restated)
def bn_blocks(n):
    """norm.hip bn_blocks (:712-717)"""
    g = n // 64 + (n % 64 != 0) if n > 0 else 1
    return min(max(g, 1), 1024)


def row_split(rows, G, b):
    """norm.hip row_split (:146-156): the rows [r0, r1) of block b"""
    per = -(-rows // G)
    return min(rows, per * b), min(rows, per * (b + 1))


def stream_grid(pieces):
    """norm.hip stream_grid (:740-743)"""
    return min(max(-(-pieces // 256), 1), 4096)


def wide_stream_grid(n, C, vpl):
    """norm.hip wide_stream_grid (:735-738)"""
    want, cap = -(-n // vpl), 4096 // -(-C // 256)
    return 1 if want < 1 else (max(cap, 1) if want > cap else want)


def reduce_paths(P):
    """norm.hip piece_reduce (:169-215)"""
    if 64 % P:
        return {"reduce_serial"}
    s = {f"reduce_dpp_le{t}" for t in (8, 4, 2, 1) if P <= t}          # :176-179
    s.add("reduce_lds_step%d" % (1 if P <= 16 else P // 16))             # :194
    return s


GLOBAL_PATHS = {"block_cap", "merge_second_trip", "merge_one_trip"}     # host code / kernels without a dtype
ENTRY_PATHS = {"train": ("fwd_train", "bwd_batch", "local_stats", "bwd_sums", "bwd_apply"),
               "eval": ("fwd_eval", "bwd_running"), "records": ("fwd_stats", "local_stats_in"),
               "sync": ("fwd_stats", "local_stats", "bwd_sums", "bwd_apply", "fwd_stats_no_rows")}


def _stream_paths(n, rows, C, dt):
    """one matrix through the statistics / sums kernels (bn_partial_kernel :224-305, bn_bwd_partial_kernel :531-608) and
    the apply kernels (bn_apply_kernel :446-521, bn_bwd_apply_kernel :645-710)"""
    vpl, wide, G = VPL[dt], C > 256, bn_blocks(n)
    s = {"wide" if wide else "narrow"}
    if n // 64 + (n % 64 != 0) > 1024:
        s.add("block_cap")
    spans = [row_split(rows, G, b) for b in range(G)]
    longest = max(r1 - r0 for r0, r1 in spans)
    if any(r1 <= r0 for r0, r1 in spans):
        s |= {"empty_block", "zero_row_record"}                 # (a block without rows leaves a record of zero rows)
    for c0 in range(0, C, 256):                                 # col_block (:124-137)
        P = min(256, C - c0) // vpl
        s |= reduce_paths(P)
        if 256 % P:
            s.add("idle_threads")                               # row_split: lane_row >= rows_per_sweep
        if longest > 8 * (256 // P):
            s |= {"second_batch_trip", "bwd_reload"}            # :242, :574 / :591
    if wide:
        if C % 256:
            s.add("wide_narrow_last_block")
        if wide_stream_grid(n, C, vpl) * vpl < n:
            s.add("wide_apply_multi_sweep")                     # :472, :675
    elif n * (C // vpl) > stream_grid(n * (C // vpl)) * 256:
        s.add("narrow_apply_grid_stride")                       # :505, :694
    return s


def paths(c):
    """the set of (dtype, path) a case claims"""
    n, C, dt = c["n"], c["C"], c["dt"]
    s = set(ENTRY_PATHS[c["entry"]])
    if c["live"] is not None:
        s.add("n_live")
        if c["live"] > n:
            s.add("live_clamp_above")                           # live_rows (:112-116)
        if c["live"] < 0:
            s.add("live_clamp_below")
    if c["entry"] == "records":
        rows = record_rows(c["G"])
        s.add("merge_second_trip" if c["G"] > 256 * 8 else "merge_one_trip")          # :317, :371
        if 0 in rows:
            s.add("zero_row_record")
        if 1 in rows:
            s.add("one_row_record")
        s.add("wide" if C > 256 else "narrow")
    elif c["entry"] == "sync":
        for rows in SHARDS:
            if rows:
                s |= _stream_paths(rows, rows, C, dt)
        s |= {"zero_row_record", "one_row_record", "merge_one_trip"}
    else:
        s |= _stream_paths(n, refnorm.live_rows(c["live"], n), C, dt)
        if refnorm.live_rows(c["live"], n) == 0:
            s.add("no_live_rows")                               # bn_partial_kernel: no origin (:284)
        s.add("merge_one_trip")
    if c["content"] != "plain" and c["entry"] == "train":
        s.add("origin_row0")                                    # a channel far from zero (:281-298); host-checked below
    s.add("param_" + ("f32" if c["pdt"] == "f32" else "16bit"))
    for flag in ("affine", "running", "dparams"):
        if not c[flag]:
            s.add("null_" + flag)
    if c["relu"]:
        s.add("relu")
    return {(None if p in GLOBAL_PATHS else dt, p) for p in s}


def required():
    """every path, for every dtype it exists in"""
    per_dtype = {"narrow", "wide", "empty_block", "zero_row_record", "one_row_record", "idle_threads", "second_batch_trip",
                 "bwd_reload", "wide_narrow_last_block", "wide_apply_multi_sweep", "narrow_apply_grid_stride", "n_live",
                 "live_clamp_above", "live_clamp_below", "no_live_rows", "param_f32", "null_affine", "null_running", "null_dparams",
                 "relu", "reduce_serial", "reduce_dpp_le8", "reduce_dpp_le4", "reduce_dpp_le2", "reduce_dpp_le1",
                 "reduce_lds_step1", "reduce_lds_step2"}
    for v in ENTRY_PATHS.values():
        per_dtype |= set(v)
    need = {(dt, p) for dt in DTYPES for p in per_dtype}
    need |= {("f32", "reduce_lds_step4")}                       # P = 64: four floats per piece only
    need |= {("f16", "param_16bit"), ("bf16", "param_16bit")}
    need |= {("f32", "origin_row0"), ("f16", "origin_row0")}    # (bf16 at 512 has a spacing of 4: no such channel)
    need |= {(None, p) for p in GLOBAL_PATHS}
    return need


def test_cases_claim_every_path():
    claimed = {}
    for c in _cases():
        for p in paths(c):
            claimed.setdefault(p, []).append(c["id"])
    missing = sorted(required() - set(claimed), key=str)
    assert not missing, missing
    unknown = sorted(set(claimed) - required(), key=str)
    assert not unknown, unknown                                 # a path the model knows and required() forgot


def test_a_sole_claimant_cannot_leave():
    """the table holds no slack the model cannot see: without a case that alone claims a path, the claim fails"""
    taken = {c["id"]: paths(c) for c in _cases()}
    claimed = {}
    for i, ps in taken.items():
        for p in ps:
            claimed.setdefault(p, set()).add(i)
    sole = {next(iter(v)) for v in claimed.values() if len(v) == 1}
    assert sole, "no path has a single claimant"
    for gone in sole:
        left = set().union(*(ps for i, ps in taken.items() if i != gone))
        assert required() - left, gone


def test_issue_shapes_reach_what_they_are_for():
    f = lambda *a, **k: {p for _, p in paths(case(*a, **k))}
    long16 = f("train", 66_000, 256, "f16")
    assert {"block_cap", "second_batch_trip", "bwd_reload", "narrow_apply_grid_stride", "reduce_lds_step2"} <= long16
    assert "second_batch_trip" not in f("train", 65_536, 256, "f16")      # 64 rows per block: one trip of 8 * 8 rows
    assert "second_batch_trip" in f("train", 300, 256, "f32")             # 60 rows per block, 8 * 4 per trip
    assert "wide_apply_multi_sweep" in f("train", 20_000, 520, "f16")
    assert "wide_apply_multi_sweep" not in f("train", 10_920, 520, "f16")
    assert {"reduce_serial", "idle_threads"} <= f("train", 300, 200, "f16")                # P = 25
    assert {"reduce_serial", "reduce_lds_step2"} <= f("train", 300, 280, "f16")            # 256 + 24 channels
    assert {"reduce_lds_step4", "reduce_serial"} <= f("train", 300, 280, "f32")            # P = 64 and P = 6
    assert "reduce_dpp_le1" in f("train", 300, 264, "f16") and "reduce_dpp_le1" in f("train", 300, 520, "f16")
    assert "empty_block" in f("train", 1000, 16, "f16", live=65)
    assert "empty_block" not in f("train", 129, 16, "f16")
    assert "merge_second_trip" in f("records", 0, 16, "f16", G=2049)
    assert "merge_second_trip" not in f("records", 0, 16, "f16", G=2048)


def origin_is_row0(col):
    """norm.hip bn_partial_kernel (:281-298): block means are kept relative to row 0 of a channel that sits far from zero"""
    col = np.asarray(col, dtype=np.float64)
    return abs(col[0]) > 16 * np.abs(col[1:4] - col[0]).max(initial=0.0)


def test_conditioning_cases_hold_what_they_claim():
    far = {"cond": (0, 2), "cond1e4": (0, 1, 2), "cond16": (0,)}
    for c in _cases():
        if c["entry"] == "train" and c["content"] != "plain":
            x = _f64(_inputs(c)["x"])
            got = {k for k in range(c["C"]) if origin_is_row0(x[:, k])}
            assert set(far[c["content"]]) <= got, (c["id"], got)
            assert len(got) < c["C"], c["id"]                   # and channels that keep plain means next to them
    plain = _f64(_inputs(case("train", 300, 64, "f32"))["x"])
    assert not any(origin_is_row0(plain[:, k]) for k in range(64))


# the lines the model above restates: a change to one of them, or a new branch in the file, fails here until the model
# and the case table have been read against it again
RESTATED = ("return v < 0 ? 0 : (v < n ? v : n);",
            "const long long per = (static_cast<long long>(n) + nblocks - 1) / nblocks;",
            "s.rows_per_sweep = kT / P;",
            "s.active = s.lane_row < s.rows_per_sweep;",
            "if (64 % P == 0) {",
            "if (P <= 8) {", "if (P <= 4) {", "if (P <= 2) {", "if (P <= 1) {",
            "const int step = P <= 16 ? 1 : P / 16, first = P <= 16 ? 0 : piece / 16, jj = piece % 16;",
            "if (live > 0) {",
            "constexpr int kOriginRows = 4;",
            "if (fabsf(x0) > 16.f * spread) origin = x0;",
            "if (blockIdx.x == 0) partial[3 * static_cast<size_t>(C) * G + c] = origin;",
            "mean = origin ? lm[0] + origin[c] : lm[0];",
            "constexpr int U = 8;",
            "for (int r = s.r0 + s.lane_row; r < s.r1; r += U * s.rows_per_sweep) {",
            "constexpr int kBwdBatch = 8;",
            "r += U * s.rows_per_sweep;\n      if (r < s.r1) {",
            "for (int b0 = threadIdx.x; b0 < G; b0 += kT * U) {",
            "if (nb[u] > 0.f) {",
            "int g = n > 0 ? n / 64 + (n % 64 != 0) : 1;",
            "return g < 1 ? 1 : (g > 1024 ? 1024 : g);",
            "const long long want = div_up(n, vpl), cap = 4096 / div_up(C, kT);",
            "return static_cast<unsigned>(b < 1 ? 1 : (b > 4096 ? 4096 : b));",
            "constexpr int kT = 256;",
            "const bool wide = C > kT;")
BRANCH_WORDS = {"if (": 76, "for (": 38, "while (": 4, "? ": 77}


def test_the_model_restates_the_source():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "spconv_amd", "csrc", "norm.hip")).read()
    for line in RESTATED:
        assert line in src, line
    code = "\n".join(re.sub(r"//.*", "", l) for l in src.splitlines())
    assert {w: code.count(w) for w in BRANCH_WORDS} == BRANCH_WORDS


# ---------------------------------------------------------------- inputs
def _round(t, dt):
    return t.to(TORCH[dt])


def _f64(t):
    return None if t is None else t.double().cpu().numpy()


def _inputs(c):
    """CPU tensors in the dtypes the kernels read: x, dy, w, b, rm, rv (+ live rows L).  Padding rows hold 1e4 / 1."""
    g = torch.Generator().manual_seed(zlib.crc32(c["id"].encode()))
    n, C = c["n"], c["C"]
    if c["entry"] == "records":
        n = sum(record_rows(c["G"]))
    x = torch.randn(n, C, generator=g) * 1.7 + torch.linspace(-3, 3, C)
    dy = torch.randn(n, C, generator=g)
    w, b = torch.rand(C, generator=g) + 0.5, torch.rand(C, generator=g) - 0.5
    rm, rv = torch.randn(C, generator=g) * 0.5, torch.rand(C, generator=g) + 0.5
    if c["content"] in ("cond", "cond1e4"):
        z = torch.randn(n, 6, generator=g, dtype=torch.float64)
        x = x.double()
        x[:, 0] = 1e3 + z[:, 0]                                 # mean 1e3, spread 1
        if c["content"] == "cond1e4":
            x[:, 1] = -1e4 + 0.1 * z[:, 1]                      # mean -1e4, spread 0.1
        x[:, 2] = 7.25                                          # constant: M2 = 0, invstd = 1 / sqrt(eps)
        w[3], w[4] = 0.0, 1e-4                                  # weight 0 and tiny
        x[:, 5] = torch.linspace(-50, 50, n, dtype=torch.float64) + 0.5 * z[:, 5]        # a trend along the rows
        b[6], b[7] = 100.0, -100.0                              # bias far from 0
        x = x.float()
        rm[0], rm[1], rv[1], rv[2] = 1e3, -1e4, 0.01, 0.0       # (evaluation: running statistics of such channels)
    elif c["content"] == "cond16":
        x[:, 0] = 512 + 8 * torch.randn(n, generator=g)         # fp16 spacing at 512 is 0.5: still distinct values
    x, dy = _round(x, c["dt"]), _round(dy, c["dt"])
    L = refnorm.live_rows(c["live"], n)
    x[L:], dy[L:] = 1e4, 1.0
    w, b, rm, rv = (_round(t, c["pdt"]) for t in (w, b, rm, rv))
    if not c["affine"]:
        w = b = None
    return dict(x=x, dy=dy, w=w, b=b, rm=rm, rv=rv, L=L, n=n)


def _ref_kwargs(c, d):
    return dict(weight=_f64(d["w"]), bias=_f64(d["b"]), live=c["live"], relu=c["relu"], momentum=c["momentum"],
                eps=c["eps"], running_mean=_f64(d["rm"]), running_var=_f64(d["rv"]))


def _silence_the_kink(c, d, **kw):
    """dy = 0 where the reference pre-activation is within KINK_BOUNDS bounds of 0; -> share of elements silenced"""
    if not c["relu"]:
        return 0.0
    out, A = refnorm.batchnorm(_f64(d["x"]), None, **kw)
    pre = out["pre"]
    kink = np.abs(pre) <= KINK_BOUNDS * (HALF_ULP[str(TORCH[c["dt"]])[6:]] * np.abs(pre) + C_BOUND["y"] * A["y"])
    kink[d["L"]:] = False
    d["dy"][torch.from_numpy(kink)] = 0
    # share of the live elements; a matrix of one live row (whose claim is the zeros, the record and finite statistics)
    # has C of them and is measured against all its elements instead
    return float(kink.sum()) / max(1, (d["L"] if d["L"] > 1 else d["n"]) * c["C"])


def _record_stats(x64, G):
    """[3][C][G] records of consecutive row blocks of record_rows(G) rows, from float64, as fp32"""
    stats, at = np.zeros((3, x64.shape[1], G)), 0
    for i, rows in enumerate(record_rows(G)):
        if rows:
            stats[:, :, i] = refnorm.record(x64[at:at + rows])[0]
            at += rows
    return stats.astype(np.float32)


def _reference(c, d):
    """-> (out, A, share silenced, stats or None): the float64 reference of a case on its inputs"""
    kw, stats = _ref_kwargs(c, d), None
    kw["training"] = c["entry"] != "eval"
    if c["entry"] == "records":
        stats = _record_stats(_f64(d["x"]), c["G"])
        rows, mean, M2, A_mean = refnorm.merge_records(stats)
        kw["stats"] = (rows[0], mean, M2, A_mean)
    share = _silence_the_kink(c, d, **kw)
    out, A = refnorm.batchnorm(_f64(d["x"]), _f64(d["dy"]), **kw)
    return out, A, share, stats


@pytest.mark.parametrize("c", [c for c in _cases() if c["relu"] and c["n"] * c["C"] <= 300_000], ids=lambda c: c["id"])
def test_relu_cases_keep_their_gradient(c):
    """CPU: the reference alone silences at most 1 % of a ReLU case's elements (random data: ~1e-4)"""
    assert _reference(c, _inputs(c))[2] <= KINK_SHARE


# ---------------------------------------------------------------- the ABI
def _p(t):
    return None if t is None else t.data_ptr()


def _dt(name):
    from spconv_amd import _lib
    return {"f16": _lib.DTYPE_F16, "bf16": _lib.DTYPE_BF16, "f32": _lib.DTYPE_F32}[name]


def _nan(shape, dtype, dev):
    return torch.full(shape, float("nan"), dtype=dtype, device=dev)


class _Abi:
    def __init__(self, c, d, dev):
        from spconv_amd import _lib
        self.lib, self.L, self.c, self.dev = _lib, _lib.load(), c, dev
        self.stream = torch.cuda.current_stream().cuda_stream
        self.dt, self.pdt, self.ptd = _dt(c["dt"]), _dt(c["pdt"]), TORCH[c["pdt"]]
        self.w, self.b = (None if t is None else t.to(dev) for t in (d["w"], d["b"]))
        self.rm0, self.rv0 = d["rm"], d["rv"]

    def ws(self, n):
        return torch.empty((max(self.L.spx_batchnorm_ws_bytes(n, self.c["C"]), 16),), dtype=torch.uint8, device=self.dev)

    def n_live(self):
        live = self.c["live"]
        return None if live is None else torch.tensor([live], dtype=torch.int32, device=self.dev)

    def state(self):
        """NaN statistics, running buffers at their non-trivial start, the step counter at 5"""
        C, c = self.c["C"], self.c
        r = dict(mean=_nan((C,), torch.float32, self.dev), invstd=_nan((C,), torch.float32, self.dev),
                 nbt=torch.full((), 5, dtype=torch.int64, device=self.dev))
        r["rm"] = self.rm0.to(self.dev) if c["running"] else None
        r["rv"] = self.rv0.to(self.dev) if c["running"] else None
        return r

    def fwd(self, x, r, training, nl):
        n, c = x.shape[0], self.c
        r["y"], ws = torch.full_like(x, float("nan")), self.ws(x.shape[0])
        self.lib.check(self.L.spx_batchnorm_fwd(
            x.data_ptr(), r["y"].data_ptr(), n, c["C"], self.dt, _p(self.w), _p(self.b), _p(r["rm"]), _p(r["rv"]),
            _p(r["nbt"]), self.pdt, int(training), c["momentum"], c["eps"], int(c["relu"]), _p(r["mean"]),
            _p(r["invstd"]), ws.data_ptr(), ws.numel(), _p(nl), self.stream))

    def fwd_stats(self, x, r, stats, records, nl):
        n, c = x.shape[0], self.c
        r["y"] = torch.full_like(x, float("nan"))
        self.lib.check(self.L.spx_batchnorm_fwd_stats(
            x.data_ptr(), r["y"].data_ptr(), n, c["C"], self.dt, _p(self.w), _p(self.b), _p(r["rm"]), _p(r["rv"]),
            _p(r["nbt"]), self.pdt, c["momentum"], c["eps"], int(c["relu"]), _p(r["mean"]), _p(r["invstd"]),
            stats.data_ptr(), records, _p(nl), self.stream))

    def params_out(self, r):
        C, want = self.c["C"], self.c["dparams"]
        r["dw"] = _nan((C,), self.ptd, self.dev) if want else None
        r["db"] = _nan((C,), self.ptd, self.dev) if want else None

    def bwd(self, x, dy, r, mean, invstd, batch, nl):
        n, c = x.shape[0], self.c
        r["dx"], ws = torch.full_like(x, float("nan")), self.ws(x.shape[0])
        self.params_out(r)
        self.lib.check(self.L.spx_batchnorm_bwd(
            x.data_ptr(), dy.data_ptr(), r["dx"].data_ptr(), n, c["C"], self.dt, _p(self.w), _p(self.b), self.pdt,
            _p(mean), _p(invstd), int(batch), int(c["relu"]), _p(r["dw"]), _p(r["db"]), ws.data_ptr(), ws.numel(),
            _p(nl), self.stream))

    def local_stats(self, x, nl, stats_in=None, records=0):
        n, C = x.shape[0], self.c["C"]
        rec, ws = _nan((3, C), torch.float32, self.dev), self.ws(x.shape[0])
        self.lib.check(self.L.spx_batchnorm_local_stats(x.data_ptr(), n, C, self.dt, _p(stats_in), records,
                                                        rec.data_ptr(), ws.data_ptr(), ws.numel(), _p(nl), self.stream))
        return rec

    def bwd_sums(self, x, dy, r, mean, invstd, nl):
        n, c = x.shape[0], self.c
        r["sums"], ws = _nan((2, c["C"]), torch.float32, self.dev), self.ws(x.shape[0])
        self.params_out(r)
        self.lib.check(self.L.spx_batchnorm_bwd_sums(
            x.data_ptr(), dy.data_ptr(), n, c["C"], self.dt, _p(self.w), _p(self.b), self.pdt, _p(mean), _p(invstd),
            int(c["relu"]), _p(r["sums"]), _p(r["dw"]), _p(r["db"]), ws.data_ptr(), ws.numel(), _p(nl), self.stream))

    def bwd_apply(self, x, dy, r, mean, invstd, sums, total, nl):
        n, c = x.shape[0], self.c
        r["dx"] = torch.full_like(x, float("nan"))
        self.lib.check(self.L.spx_batchnorm_bwd_apply(
            x.data_ptr(), dy.data_ptr(), r["dx"].data_ptr(), n, c["C"], self.dt, _p(self.w), _p(self.b), self.pdt,
            _p(mean), _p(invstd), int(c["relu"]), sums.data_ptr(), total.data_ptr(), _p(nl), self.stream))


# ---------------------------------------------------------------- judging
def excess(got, ref, A, dtype):
    """the worst (|got - ref| - u |ref|) / A over the elements with A > 0"""
    got, ref, A = (np.asarray(t, dtype=np.float64) for t in (got, ref, A))
    ok = A > 0
    if not ok.any():
        return 0.0
    e = (np.abs(got - ref) - np.maximum(HALF_ULP[dtype] * np.abs(ref), HALF_SUBNORMAL[dtype]))[ok] / A[ok]
    return float(np.nanmax(e)) if np.isfinite(e).any() else float("inf")


def _judge(c, kind, got, ref, A, what=None, book=WORST):
    dtype = str(got.dtype)[6:]
    g = _f64(got)
    e = excess(g, ref, A, dtype)
    if e > book.get(kind, (-1.0, ""))[0]:
        book[kind] = (e, c["id"])
    if book is WORST:
        print(f"excess {kind:13s} {e:10.3e}  {what or ''} {c['id']}")
        assert np.isfinite(g).all(), (c["id"], kind, what, "not every element was written")
        try:          # (the subnormal grid enters as magnitude: c * (A + h / c) = c A + h)
            assert_close_abs_sum(g, ref, np.asarray(A) + HALF_SUBNORMAL[dtype] / C_BOUND[kind], dtype, C_BOUND[kind],
                                 name=f"{c['id']} {kind} {what or ''}")
        except AssertionError as err:
            MISSES.append(str(err))


def _judge_y(c, y, out, A, L, what="y"):
    _judge(c, "y", y, out["y"], A["y"], what)
    assert not y[L:].any(), (c["id"], what, "padding rows of y")
    if c["relu"]:
        u = HALF_ULP[str(y.dtype)[6:]]
        below = out["pre"] < -(u * np.abs(out["pre"]) + C_BOUND["y"] * A["y"])
        assert not y.cpu()[torch.from_numpy(below)].any(), (c["id"], what, "y > 0 below the kink")


def _judge_state(c, r, out, A, what):
    _judge(c, "save_mean", r["mean"], out["mean"], A["mean"], what)
    _judge(c, "save_invstd", r["invstd"], out["invstd"], A["invstd"], what)
    if c["running"]:
        _judge(c, "running_mean", r["rm"], out["running_mean"], A["running_mean"], what)
        _judge(c, "running_var", r["rv"], out["running_var"], A["running_var"], what)
    assert int(r["nbt"]) == 6, (c["id"], what)


def _judge_record(c, rec, out, A, what):
    assert np.array_equal(_f64(rec[0]), out["record"][0]), (c["id"], what, "record[0] is the live row count")
    _judge(c, "record", rec, out["record"], A["record"], what)


def _judge_grads(c, r, out, A, L, what, sums=None, sums_A=None):
    if "dx" in r:
        _judge(c, "dx", r["dx"], out["dx"], A["dx"], what)
        assert not r["dx"][L:].any(), (c["id"], what, "padding rows of dx")
    if c["dparams"]:
        s, sA = (out["sums"], A["sums"]) if sums is None else (sums, sums_A)
        _judge(c, "dbias", r["db"], s[0], sA[0], what)
        _judge(c, "dweight", r["dw"], s[1], sA[1], what)
    if "sums" in r:
        s, sA = (out["sums"], A["sums"]) if sums is None else (sums, sums_A)
        _judge(c, "sums", r["sums"], s, sA, what)


def _yardstick(c, d, out, A):
    """the same formulas evaluated straight in fp32 by torch on the host, judged like the kernels (never asserted)"""
    L, f = d["L"], torch.float32
    if L < 2:
        return
    x, dy = d["x"][:L].to(f), d["dy"][:L].to(f)
    C, tdt, ptd = c["C"], TORCH[c["dt"]], TORCH[c["pdt"]]
    w = torch.ones(C) if d["w"] is None else d["w"].to(f)
    b = torch.zeros(C) if d["b"] is None else d["b"].to(f)
    mean, var = x.mean(0), x.var(0, unbiased=False)
    invstd = torch.rsqrt(var + c["eps"])
    sc = w * invstd
    pre = x * sc + (b - mean * sc)
    y = torch.relu(pre) if c["relu"] else pre
    xhat = x * invstd + (-mean * invstd)
    dyp = dy * (pre > 0) if c["relu"] else dy
    db, dw = dyp.sum(0), (dyp * xhat).sum(0)
    dx = w * invstd * (dyp - db / L - xhat * (dw / L))
    rm = (1 - c["momentum"]) * d["rm"].to(f) + c["momentum"] * mean
    rv = (1 - c["momentum"]) * d["rv"].to(f) + c["momentum"] * x.var(0, unbiased=True)
    j = functools.partial(_judge, c, book=YARD)
    j("y", y.to(tdt), out["y"][:L], A["y"][:L])
    j("dx", dx.to(tdt), out["dx"][:L], A["dx"][:L])
    j("dbias", db.to(ptd), out["dbias"], A["dbias"])
    j("dweight", dw.to(ptd), out["dweight"], A["dweight"])
    j("sums", torch.stack([db, dw]), out["sums"], A["sums"])
    j("save_mean", mean, out["mean"], A["mean"])
    j("save_invstd", invstd, out["invstd"], A["invstd"])
    j("record", torch.stack([torch.full((C,), float(L)), mean, var * L]), out["record"], A["record"])
    j("running_mean", rm.to(ptd), out["running_mean"], A["running_mean"])
    j("running_var", rv.to(ptd), out["running_var"], A["running_var"])


# ---------------------------------------------------------------- the runners
def _run_train(c, d, out, A, dev):
    abi, L = _Abi(c, d, dev), d["L"]
    x, dy, nl = d["x"].to(dev), d["dy"].to(dev), abi.n_live()
    r = abi.state()
    abi.fwd(x, r, True, nl)
    _judge_y(c, r["y"], out, A, L)
    _judge_state(c, r, out, A, "fwd")
    abi.bwd(x, dy, r, r["mean"], r["invstd"], True, nl)
    _judge_grads(c, r, out, A, L, "bwd")
    # the SyncBatchNorm cut on the same matrix, a world of one rank
    rec = abi.local_stats(x, nl)
    _judge_record(c, rec, out, A, "local_stats")
    s = {}
    abi.bwd_sums(x, dy, s, r["mean"], r["invstd"], nl)
    abi.bwd_apply(x, dy, s, r["mean"], r["invstd"], s["sums"], rec[0, :1].contiguous(), nl)
    _judge_grads(c, s, out, A, L, "bwd_sums / bwd_apply")
    _yardstick(c, d, out, A)


def _run_eval(c, d, out, A, dev):
    abi, L = _Abi(c, d, dev), d["L"]
    x, dy, nl = d["x"].to(dev), d["dy"].to(dev), abi.n_live()
    r = abi.state()
    rm0, rv0 = r["rm"].clone(), r["rv"].clone()
    abi.fwd(x, r, False, nl)
    _judge_y(c, r["y"], out, A, L)
    # inference touches no state
    assert torch.equal(r["rm"], rm0) and torch.equal(r["rv"], rv0) and int(r["nbt"]) == 5, c["id"]
    assert torch.isnan(r["mean"]).all() and torch.isnan(r["invstd"]).all(), c["id"]
    # the backward pass takes fp32 mean / invstd: the running statistics as the module hands them over
    mean = torch.from_numpy(out["mean"]).float().to(dev)
    invstd = torch.from_numpy(out["invstd"]).float().to(dev)
    abi.bwd(x, dy, r, mean, invstd, False, nl)
    _judge_grads(c, r, out, A, L, "bwd")


def _run_records(c, d, out, A, dev, stats):
    abi, G = _Abi(c, d, dev), c["G"]
    x, st = d["x"].to(dev), torch.from_numpy(stats).to(dev).contiguous()
    r = abi.state()
    abi.fwd_stats(x, r, st, G, None)
    _judge_y(c, r["y"], out, A, d["L"])
    _judge_state(c, r, out, A, "fwd_stats")
    rec = abi.local_stats(torch.full_like(x, float("nan")), None, st, G)        # (x is not read)
    _judge_record(c, rec, out, A, "local_stats(stats_in)")


def _run_sync(c, d, out, A, dev):
    abi, C = _Abi(c, d, dev), c["C"]
    xs = [t.contiguous().to(dev) for t in torch.split(d["x"], SHARDS)]
    dys = [t.contiguous().to(dev) for t in torch.split(d["dy"], SHARDS)]
    x64 = _f64(d["x"])
    bounds = np.cumsum((0,) + SHARDS)
    recs = [abi.local_stats(x, None) for x in xs]
    for k, rec in enumerate(recs):
        own, own_A = refnorm.record(x64[bounds[k]:bounds[k + 1]])
        _judge(c, "record", rec, own, own_A, f"rank {k}")
        assert np.array_equal(_f64(rec[0]), own[0]), (c["id"], k)
    gathered = torch.stack(recs, 0)                                  # the all-gather: [world, 3, C]
    merged = gathered.permute(1, 2, 0).contiguous()                 # [3][C][world]
    total = gathered[:, 0, 0].sum(0, keepdim=True)
    ranks = []
    for k, x in enumerate(xs):
        r = abi.state()
        abi.fwd_stats(x, r, merged, len(xs), None)
        sl = slice(bounds[k], bounds[k + 1])
        if x.shape[0]:
            _judge_y(c, r["y"], {"y": out["y"][sl], "pre": out["pre"][sl]}, {"y": A["y"][sl]}, x.shape[0], f"y rank {k}")
        _judge_state(c, r, out, A, f"rank {k}")
        ranks.append(r)
    for r in ranks:                                                  # every rank, the empty one too, holds the same bits
        for key in ("mean", "invstd", "rm", "rv"):
            assert torch.equal(r[key], ranks[-1][key]), (c["id"], key)
    for k, (x, dy, r) in enumerate(zip(xs, dys, ranks)):
        abi.bwd_sums(x, dy, r, r["mean"], r["invstd"], None)
        sl = slice(bounds[k], bounds[k + 1])
        dyp, xhat, adyp, A_xhat = out["dyp"][sl], out["xhat"][sl], A["dyp"][sl], A["xhat"][sl]
        own = np.stack([dyp.sum(0), (dyp * xhat).sum(0)])
        own_A = np.stack([adyp.sum(0), (adyp * A_xhat).sum(0)])
        _judge_grads(c, r, out, A, x.shape[0], f"bwd_sums rank {k}", own, own_A)
    sums = torch.stack([r["sums"] for r in ranks]).sum(0)            # the all-reduce
    for k, (x, dy, r) in enumerate(zip(xs, dys, ranks)):
        abi.bwd_apply(x, dy, r, r["mean"], r["invstd"], sums, total, None)
        if x.shape[0]:
            sl = slice(bounds[k], bounds[k + 1])
            _judge(c, "dx", r["dx"], out["dx"][sl], A["dx"][sl], f"dx rank {k}")
    assert not ranks[0]["sums"].any() and not recs[0].any() and not recs[1][2].any(), c["id"]


@pytest.mark.gpu
@pytest.mark.parametrize("c", _cases(), ids=lambda c: c["id"])
def test_norm_matrix(cuda, c):
    d = _inputs(c)
    del MISSES[:]
    out, A, share, stats = _reference(c, d)
    assert share <= KINK_SHARE, (c["id"], share)
    if c["entry"] == "train":
        _run_train(c, d, out, A, cuda)
    elif c["entry"] == "eval":
        _run_eval(c, d, out, A, cuda)
    elif c["entry"] == "records":
        _run_records(c, d, out, A, cuda, stats)
    else:
        _run_sync(c, d, out, A, cuda)
    torch.cuda.synchronize()
    assert not MISSES, "\n".join(MISSES)


@pytest.mark.gpu
def test_report_of_the_worst_excess(cuda):
    """prints, per output kind, the worst excess over u |ref| as a fraction of A that the cases above met (run with -s),
    next to the same figure for a straight fp32 evaluation on the host"""
    for kind in KINDS:
        e, where = WORST.get(kind, (float("nan"), "-"))
        ye, ywhere = YARD.get(kind, (float("nan"), "-"))
        print(f"worst {kind:13s} kernel {e:10.3e} ({where})   fp32 yardstick {ye:10.3e} ({ywhere})   c {C_BOUND[kind]:g}")
