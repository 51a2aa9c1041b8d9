#!/usr/bin/env python
"""Device time of one fused BatchNorm1d + ReLU forward and backward (csrc/norm.hip, through the C ABI on preallocated
buffers, hipGraph replays of 20 calls) at the level shapes of the config-4 backbone, next to the time the
passes' bytes would take at 6 TB/s (tools/experiments/bn_two_launch.patch: the two-launch forms this tool compared).
    python tools/bn_probe.py            -> one JSON line per shape
    python tools/bn_probe.py --wide     -> the wide shapes only (--narrow: the others only)
Each launch alone: csrc/build_bn_probe.sh, then SPX_LIB=.../libspconv_amd_bnprobe.so SPX_BN_PHASES=1|2|4 (statistics pass |
merge | apply).  fwd_from_conv_records_us: merge + apply over the records a convolution's epilogue leaves (one per 128 rows).

Beyond 256 channels (the column-blocked launches; row counts of a backbone's 512-wide levels) each pass is timed next to
two baselines, all variants captured first and then replayed in turn, round after round, in this one process:
  torch      torch's own batch-norm + ReLU kernels on the same tensors (what a layer took before the wide launches)
  per_block  the <= 256-channel kernels, one call per 256-channel column block on contiguous copies (copies not timed)
*_GBps: the bytes of the pass (3 tensor passes forward, 5 backward) over the time."""
import json, os, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from spconv_amd import _lib

dev = torch.device("cuda:0")
L = _lib.load()
SHAPES = [(400_000, 16), (313_000, 32), (140_000, 64), (50_000, 64), (20_000, 128)]
WIDE_SHAPES = [(25_000, 512), (6_000, 512), (25_000, 384), (12_000, 1024)]
F16, F32 = _lib.DTYPE_F16, _lib.DTYPE_F32


def timed(fn, s, reps=20, rounds=5):
    with torch.cuda.stream(s):
        for _ in range(3):
            fn()
    s.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        for _ in range(reps):
            fn()
    best = 1e9
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(s):
            a.record(s); g.replay(); b.record(s)
        s.synchronize()
        best = min(best, a.elapsed_time(b) * 1e3 / reps)
    return best


def timed_in_turn(fns, s, reps=20, rounds=7):
    """{name: best us per call}: every variant captured, then one replay of each per round"""
    graphs = {}
    for name, fn in fns.items():
        with torch.cuda.stream(s):
            for _ in range(3):
                fn()
        s.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            for _ in range(reps):
                fn()
        graphs[name] = g
    best = {name: 1e9 for name in fns}
    for _ in range(rounds):
        for name, g in graphs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(s):
                a.record(s); g.replay(); b.record(s)
            s.synchronize()
            best[name] = min(best[name], a.elapsed_time(b) * 1e3 / reps)
    return best


def wide_shape(n, C, s):
    aten = torch.ops.aten
    raw = s.cuda_stream
    x = torch.randn(n, C, device=dev).half()
    dy = torch.randn(n, C, device=dev).half()
    y, dx = torch.empty_like(x), torch.empty_like(x)
    w, b = torch.rand(C, device=dev) + 0.5, torch.rand(C, device=dev) - 0.5
    rm, rv = torch.zeros(C, device=dev), torch.ones(C, device=dev)
    stats = torch.empty(2, C, device=dev)
    dw, db = torch.empty(C, device=dev), torch.empty(C, device=dev)
    ws = torch.empty(L.spx_batchnorm_ws_bytes(n, C), dtype=torch.uint8, device=dev)

    def call_fwd(x, y, C, w, b, rm, rv, stats, ws):
        _lib.check(L.spx_batchnorm_fwd(x.data_ptr(), y.data_ptr(), n, C, F16, w.data_ptr(), b.data_ptr(), rm.data_ptr(),
                                       rv.data_ptr(), None, F32, 1, 0.01, 1e-3, 1, stats[0].data_ptr(), stats[1].data_ptr(),
                                       ws.data_ptr(), ws.numel(), None, raw))

    def call_bwd(x, dy, dx, C, w, b, stats, dw, db, ws):
        _lib.check(L.spx_batchnorm_bwd(x.data_ptr(), dy.data_ptr(), dx.data_ptr(), n, C, F16, w.data_ptr(), b.data_ptr(), F32,
                                       stats[0].data_ptr(), stats[1].data_ptr(), 1, 1, dw.data_ptr(), db.data_ptr(),
                                       ws.data_ptr(), ws.numel(), None, raw))

    # the column blocks as matrices of their own (contiguous), with everything a call of the <= 256 kernels needs
    blocks = []
    for c0 in range(0, C, 256):
        k = slice(c0, min(c0 + 256, C))
        Cb = k.stop - k.start
        blocks.append(dict(C=Cb, x=x[:, k].contiguous(), dy=dy[:, k].contiguous(), y=torch.empty(n, Cb, device=dev).half(),
                           dx=torch.empty(n, Cb, device=dev).half(), w=w[k].clone(), b=b[k].clone(), rm=rm[k].clone(),
                           rv=rv[k].clone(), stats=torch.empty(2, Cb, device=dev), dw=torch.empty(Cb, device=dev),
                           db=torch.empty(Cb, device=dev),
                           ws=torch.empty(L.spx_batchnorm_ws_bytes(n, Cb), dtype=torch.uint8, device=dev)))
    torch.cuda.synchronize()
    t_saved = {}

    def fwd_torch():
        out, t_saved["mean"], t_saved["invstd"] = aten.native_batch_norm(x, w, b, rm, rv, True, 0.01, 1e-3)
        t_saved["y"] = torch.relu_(out)

    def bwd_torch():
        g = aten.threshold_backward(dy, t_saved["y"], 0)
        aten.native_batch_norm_backward(g, x, w, rm, rv, t_saved["mean"], t_saved["invstd"], True, 1e-3, [True, True, True])

    fwd_fns = {"wide": lambda: call_fwd(x, y, C, w, b, rm, rv, stats, ws),
               "per_block": lambda: [call_fwd(k["x"], k["y"], k["C"], k["w"], k["b"], k["rm"], k["rv"], k["stats"], k["ws"])
                                     for k in blocks],
               "torch": fwd_torch}
    bwd_fns = {"wide": lambda: call_bwd(x, dy, dx, C, w, b, stats, dw, db, ws),
               "per_block": lambda: [call_bwd(k["x"], k["dy"], k["dx"], k["C"], k["w"], k["b"], k["stats"], k["dw"], k["db"],
                                              k["ws"]) for k in blocks],
               "torch": bwd_torch}
    with torch.cuda.stream(s):
        fwd_torch()                                    # (saved statistics and y for the backward variants)
        fwd_fns["per_block"]()
        fwd_fns["wide"]()
    s.synchronize()
    tf, tb = timed_in_turn(fwd_fns, s), timed_in_turn(bwd_fns, s)
    nbytes = n * C * 2
    out = {"n": n, "C": C, "dtype": "f16", "tensor_MB": round(nbytes / 1e6, 1), "column_blocks": len(blocks),
           "fwd_us": {k: round(v, 2) for k, v in tf.items()}, "bwd_us": {k: round(v, 2) for k, v in tb.items()},
           "fwd_GBps": {k: round(3 * nbytes / v / 1e3, 0) for k, v in tf.items()},
           "bwd_GBps": {k: round(5 * nbytes / v / 1e3, 0) for k, v in tb.items()},
           "wide_over_per_block": {"fwd": round(tf["wide"] / tf["per_block"], 3), "bwd": round(tb["wide"] / tb["per_block"], 3)},
           "wide_over_torch": {"fwd": round(tf["wide"] / tf["torch"], 3), "bwd": round(tb["wide"] / tb["torch"], 3)},
           "ideal_us_at_6TBps": {"fwd": round(3 * nbytes / 6e6, 2), "bwd": round(5 * nbytes / 6e6, 2)}}
    print(json.dumps(out), flush=True)


s = torch.cuda.Stream()
for n, C in ([] if "--wide" in sys.argv else SHAPES):
    x = torch.randn(n, C, device=dev).half()
    dy = torch.randn(n, C, device=dev).half()
    y, dx = torch.empty_like(x), torch.empty_like(x)
    w, b = torch.rand(C, device=dev) + 0.5, torch.rand(C, device=dev) - 0.5
    rm, rv = torch.zeros(C, device=dev), torch.ones(C, device=dev)
    stats = torch.empty(2, C, device=dev)
    dw, db = torch.empty(C, device=dev), torch.empty(C, device=dev)
    ws = torch.empty(L.spx_batchnorm_ws_bytes(n, C), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    raw = s.cuda_stream

    def fwd():
        _lib.check(L.spx_batchnorm_fwd(x.data_ptr(), y.data_ptr(), n, C, F16, w.data_ptr(), b.data_ptr(), rm.data_ptr(),
                                       rv.data_ptr(), None, F32, 1, 0.01, 1e-3, 1, stats[0].data_ptr(), stats[1].data_ptr(),
                                       ws.data_ptr(), ws.numel(), None, raw))

    def bwd():
        _lib.check(L.spx_batchnorm_bwd(x.data_ptr(), dy.data_ptr(), dx.data_ptr(), n, C, F16, w.data_ptr(), b.data_ptr(), F32,
                                       stats[0].data_ptr(), stats[1].data_ptr(), 1, 1, dw.data_ptr(), db.data_ptr(),
                                       ws.data_ptr(), ws.numel(), None, raw))

    Gc = (n + 127) // 128                      # records a convolution's epilogue leaves: one per 128-row tile
    recs = torch.zeros(3, C, Gc, device=dev)      # [field][channel][record]
    recs[0] = 128.0
    recs[1] = torch.randn(C, Gc, device=dev) * 0.1
    recs[2] = 128.0 + torch.rand(C, Gc, device=dev)

    def fwd_stats():
        _lib.check(L.spx_batchnorm_fwd_stats(x.data_ptr(), y.data_ptr(), n, C, F16, w.data_ptr(), b.data_ptr(), rm.data_ptr(),
                                             rv.data_ptr(), None, F32, 0.01, 1e-3, 1, stats[0].data_ptr(),
                                             stats[1].data_ptr(), recs.data_ptr(), Gc, None, raw))

    out = {"n": n, "C": C, "tensor_MB": round(n * C * 2 / 1e6, 1), "phases": os.environ.get("SPX_BN_PHASES", "7")}
    out["fwd_from_conv_records_us"] = round(timed(fwd_stats, s), 2)
    res = {}
    out["three_launches"] = {"fwd_us": round(timed(fwd, s), 2), "bwd_us": round(timed(bwd, s), 2)}
    out["ideal_us_at_6TBps"] = {"fwd": round(3 * n * C * 2 / 6e6, 2), "bwd": round(5 * n * C * 2 / 6e6, 2)}
    print(json.dumps(out), flush=True)

for n, C in ([] if "--narrow" in sys.argv else WIDE_SHAPES):
    wide_shape(n, C, s)
