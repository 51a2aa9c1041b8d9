#!/usr/bin/env python
"""Layers wider than 256 channels: the column-blocked launch against what there was before.

SubM 3x3x3 at (C, K) = (512, 512), (256, 512), (512, 256) in f16, forward and backward, and (512, 512) int8 forward, on
a 30 k-voxel uniform scene and on tests/golden/lidar_scene.npz.  Variants, alternated in one process:
  a  the generic kernel (SPX_WIDE = 0: the path of every width beyond 256 before the column-blocked launch; int8: n/a)
  b  by hand: one launch of the 256-wide kernel per 256-column slice of the weights + the concatenation
  c  the single column-blocked launch
Protocol of bench.py config 2: device events around hipGraph replays, a warm-up, and a working set of S feature tensors
rotated through HBM.  Prints one JSON object; every figure is the median of R rounds with the min .. max spread.

    python tools/bench_wide.py [--rounds 7] [--quick]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from spconv_amd import _lib                                   # noqa: E402
from spconv_amd.pytorch import ops                            # noqa: E402
from spconv_amd.utils import synthetic                        # noqa: E402

PEAK_F16_TFLOPS, PEAK_I8_TOPS, HBM_TBPS = 2516.0, 5033.0, 6.3      # dense MFMA spec rates; achievable HBM bandwidth


def algorithmic_bytes(n, C, K, kv, s, out_s=None):
    """bench.py algorithmic_bytes: features / outputs once, the rulebook once, the weights once"""
    out_s = s if out_s is None else out_s
    fwd = s * n * C + out_s * n * K + 4 * kv * n + s * kv * C * K
    dgrad = s * n * K + s * n * C + 4 * kv * n + s * kv * C * K
    wgrad = s * n * C + s * n * K + 4 * kv * n + 4 * kv * C * K
    return {"fwd": fwd, "bwd": dgrad + wgrad}


def graph_ms(fn, span, reps):
    """device time per call of fn(0) .. fn(span - 1) captured into one graph, over `reps` replays"""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for i in range(span):
            fn(i)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for i in range(span):
            fn(i)
    g.replay()
    torch.cuda.synchronize()

    def timed():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            g.replay()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / (reps * span)
    return timed


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--quick", action="store_true", help="the 30 k scene only")
    args = ap.parse_args()
    L = _lib.load()
    dev = torch.device("cuda:0")
    from golden import lidar_scene
    scenes = {"uniform30k": (synthetic.uniform_scene([40, 200, 200], 30_000, 1, 0), [40, 200, 200])}
    if not args.quick:
        scenes["lidar"] = lidar_scene()
    res = {"rounds": args.rounds, "cases": {}}
    for sname, (idx, shape) in scenes.items():
        t = torch.from_numpy(np.ascontiguousarray(idx.astype(np.int32))).to(dev)
        one = [1, 1, 1]
        rb, _ = ops.build_rulebook(t, 1, shape, [3] * 3, one, one, one, [0] * 3, True, False, do_sort="layout")
        n = rb.n_out
        pairs = int((rb.pair_fwd >= 0).sum())
        plan = ops._plan_of(rb)
        S = 12 if n < 50_000 else 4
        for dt, C, K in (("f16", 512, 512), ("f16", 256, 512), ("f16", 512, 256), ("i8", 512, 512)):
            i8 = dt == "i8"
            if i8:
                f = [torch.randint(-127, 128, (n, C), dtype=torch.int8, device=dev) for _ in range(S)]
                w = torch.randint(-127, 128, (K, 3, 3, 3, C), dtype=torch.int8, device=dev)
                scale = torch.full((K,), 1e-3, device=dev)
            else:
                f = [(torch.rand((n, C), device=dev) - 0.5).half() for _ in range(S)]
                d = [((torch.rand((n, K), device=dev) - 0.5) * 0.2).half() for _ in range(S)]
                w = ((torch.rand((K, 3, 3, 3, C), device=dev) - 0.5) * 0.1).half()
            bias8 = torch.zeros((K,), device=dev)
            row = (rb.pair_fwd, rb.mask_fwd, None, 0)
            new = ops.tables_of(rb, "fwd", K)                       # (forward and SubM dgrad read the same tables)
            wk = [w[j:j + 256].contiguous() for j in range(0, K, 256)]
            wc = [w[..., j:j + 256].contiguous() for j in range(0, C, 256)]

            def fwd(i, tabs, ww=None):
                ww = w if ww is None else ww
                if i8:
                    return ops.igemm_fwd_int8(f[i % S], ww, tabs[0], tabs[1], tabs[2], n, 13, scale[:ww.shape[0]], bias8[:ww.shape[0]],
                                              tile_order=tabs[3])
                return ops.igemm_fwd(f[i % S], ww, tabs[0], tabs[1], tabs[2], n, 13, tile_order=tabs[3])

            def bwd(i, tabs):
                return ops.igemm_bwd(f[i % S], d[i % S], w, tabs[0], tabs[1], tabs[2], rb.pair_native, rb.num_per_loc,
                                     True, plan, tile_order=tabs[3])

            def bwd_sliced(i, tabs):
                din = torch.cat([ops.igemm_dgrad(d[i % S], v, tabs[0], tabs[1], tabs[2], n, True, tile_order=tabs[3])
                                 for v in wc], 1)
                return din, ops.igemm_wgrad(f[i % S], d[i % S], w.shape, rb.pair_native, rb.num_per_loc, True, plan)

            variants = {}
            if K > 256:
                variants["fwd"] = {"b": lambda i: torch.cat([fwd(i, new, v) for v in wk], 1), "c": lambda i: fwd(i, new)}
                if not i8:
                    variants["fwd"]["a"] = lambda i: fwd(i, row)
            if C > 256 and not i8:
                variants["bwd"] = {"a": lambda i: bwd(i, row), "b": lambda i: bwd_sliced(i, new), "c": lambda i: bwd(i, new)}
            for direction, vs in variants.items():
                timers = {}
                for v, fn in vs.items():
                    L.spx_set_option(b"SPX_WIDE", 0 if v == "a" else 1)
                    slow = v == "a"
                    timers[v] = graph_ms(fn, 2 if slow else S, 2 if slow else max(3, 240 // S // (4 if n > 50_000 else 1)))
                    L.spx_set_option(b"SPX_WIDE", 1)
                samples = {v: [] for v in timers}
                for _ in range(args.rounds):
                    for v, tm in timers.items():                    # alternating
                        samples[v].append(tm())
                es = 1 if i8 else 2
                ab = algorithmic_bytes(n, C, K, 27, es)[direction]
                flops = 2.0 * pairs * C * K * (1 if direction == "fwd" else 2)
                peak = (PEAK_I8_TOPS if i8 else PEAK_F16_TFLOPS) * 1e12
                out = {v: {"ms": round(statistics.median(x), 4), "min": round(min(x), 4), "max": round(max(x), 4)}
                       for v, x in samples.items()}
                c_ms = out["c"]["ms"]
                out["c"].update({"algorithmic_MB": round(ab / 1e6, 2), "ms_at_hbm_rate": round(ab / (HBM_TBPS * 1e12) * 1e3, 4),
                                 "GFLOP": round(flops / 1e9, 2), "ms_at_mfma_peak": round(flops / peak * 1e3, 4),
                                 "TFLOPS": round(flops / (c_ms * 1e-3) / 1e12, 1),
                                 "GBps_algorithmic": round(ab / (c_ms * 1e-3) / 1e9, 1)})
                res["cases"][f"{sname} {dt} C{C} K{K} {direction}"] = dict(voxels=n, pairs=pairs, scenes_rotated=S, **out)
                print(f"[bench_wide] {sname} {dt} C{C} K{K} {direction}: {out}", file=sys.stderr, flush=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
