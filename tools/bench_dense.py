#!/usr/bin/env python
"""SparseConvTensor.dense() at a backbone-end shape: forward, and forward + backward.

B = 4, spatial [2, 200, 176], C = 128, float16, ~10 % of the cells live, channels first (the [N, C * D, H, W] a BEV head
reads).  Uses the public call only, so the same file times any tree that has the package: `--tree` names the checkout
whose `spconv_amd` is imported (default: the one this file lies in), which is how two commits are compared in one
session on one GPU.

Protocol: every call is timed alone between two device events behind a synchronise; the working set rotates through
`--ring` sets of features / results / gradients (results and gradients are 72 MB each: five of them are past the
256 MiB Infinity Cache, so no call finds its output lines or its gradient cached); warm-up calls first; the figure is
the median of `--rounds` (>= 20) calls with the min .. max spread.  Prints one JSON object, with the bytes each path
has to move computed from the shapes.

    python tools/bench_dense.py [--tree DIR] [--rounds 30] [--label NAME]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np


def moved_bytes(cells, n, C, es, ndim):
    """Bytes each implementation moves (reads + writes), pass by pass, from the shapes."""
    out, rows, idx = cells * C * es, n * C * es, n * (ndim + 1) * 4
    native_fwd = {"map_fill": 4 * cells, "map_build": idx, "scatter": 4 * cells + rows + out}
    # (the gather skips tiles without a live cell: `out` is its upper bound, reached when every 256-cell tile has one)
    native_bwd = {"row_clear": rows, "gather": 4 * cells + out + rows}
    torch_fwd = {"int64_indices": 3 * idx, "zero_fill": out, "index_put": 2 * idx + 2 * rows, "permute_copy": 2 * out}
    torch_bwd = {"permute_copy": 2 * out, "index_gather": 2 * idx + 2 * rows}
    tot = lambda d: dict(d, total=sum(d.values()))
    return {"native_fwd": tot(native_fwd), "native_bwd": tot(native_bwd), "torch_fwd": tot(torch_fwd),
            "torch_bwd": tot(torch_bwd), "result": out, "live_rows": rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--ring", type=int, default=5)
    ap.add_argument("--label", default="")
    args = ap.parse_args()
    assert args.rounds >= 20
    sys.path.insert(0, os.path.abspath(args.tree))
    import torch
    import spconv_amd.pytorch as spconv
    assert os.path.abspath(spconv.__file__).startswith(os.path.abspath(args.tree)), spconv.__file__
    if not torch.cuda.is_available():
        raise SystemExit("bench_dense needs the GPU")
    dev = torch.device("cuda:0")
    B, spatial, C, dtype = 4, [2, 200, 176], 128, torch.float16
    cells = B * int(np.prod(spatial))
    n = cells // 10
    rng = np.random.default_rng(0)
    sets = []
    for r in range(args.ring):
        pick = np.sort(rng.permutation(cells)[:n])                  # key order, as a strided layer leaves its rows
        idx = np.stack(np.unravel_index(pick, [B] + spatial), 1).astype(np.int32)
        f = torch.from_numpy(rng.standard_normal((n, C)).astype(np.float16)).to(dev)
        sets.append((f, torch.from_numpy(idx).to(dev)))
    grads = [torch.randn((B, C, *spatial), device=dev, dtype=dtype) for _ in range(args.ring)]
    ring = [None] * args.ring                                      # results kept alive: the allocator cannot hand back a warm block

    def fwd(i):
        f, idx = sets[i % args.ring]
        with torch.no_grad():
            ring[i % args.ring] = spconv.SparseConvTensor(f, idx, spatial, B).dense()

    def fwd_bwd(i):
        f, idx = sets[i % args.ring]
        f = f.detach().requires_grad_(True)
        out = spconv.SparseConvTensor(f, idx, spatial, B).dense()
        out.backward(grads[i % args.ring])
        ring[i % args.ring] = (out.detach(), f.grad)

    def timed(fn):
        for i in range(args.warmup):
            fn(i)
        samples = []
        for i in range(args.rounds):
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn(args.warmup + i)
            b.record()
            torch.cuda.synchronize()
            samples.append(a.elapsed_time(b))
        return {"ms": round(statistics.median(samples), 4), "min": round(min(samples), 4), "max": round(max(samples), 4)}

    res = {"label": args.label, "device": torch.cuda.get_device_name(0),
           "shape": {"B": B, "spatial": spatial, "C": C, "dtype": "float16", "cells": cells, "live_rows": n,
                     "channels_first": True},
           "rounds": args.rounds, "ring": args.ring, "fwd": timed(fwd), "fwd_bwd": timed(fwd_bwd),
           "bytes": moved_bytes(cells, n, C, 2, len(spatial))}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
