#!/usr/bin/env python
"""What does a misaligned add cost?  Times AddTableMisaligned -- forward, and forward + backward -- on two operands of
100 k voxels with about 50 % overlap on [41, 1600, 1408], batch 1, f16, C = 64: the union kernels (csrc/union.hip) against
the torch composite they replace, alternating in one process, plus every native stage on its own.  HIP events, warm-up,
median of the repeats; the merge kernel's bytes over its time are set against 8 TB/s.

    python tools/union_probe.py [--out profiles/union_probe.json] [--repeats 30]

On a commit without the union kernels the same script times what `AddTableMisaligned` is there (the composite)."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import spconv_amd.pytorch as spconv  # noqa: E402
from spconv_amd import _lib  # noqa: E402
from spconv_amd.pytorch import functional as Fsp  # noqa: E402

SHAPE, BATCH, C, ROWS = [41, 1600, 1408], 1, 64, 100_000
KEYS = ("union/mark", "union/prefix", "union/claim", "union/fill", "union/add_fwd", "union/add_bwd")


def operands(dev):
    rng = np.random.default_rng(0)
    cells = int(np.prod(SHAPE))
    keys = rng.choice(cells, size=ROWS * 3 // 2, replace=False)          # A = first 100 k, B = last 100 k: 50 k shared
    out = []
    for part in (keys[:ROWS], keys[ROWS // 2:]):
        part = rng.permutation(part)
        idx = np.stack([np.zeros_like(part)] + list(np.unravel_index(part, SHAPE)), axis=1).astype(np.int32)
        feat = torch.randn((idx.shape[0], C), device=dev).half()
        out.append((torch.from_numpy(idx).to(dev), feat))
    return out


def timed(fn, repeats, warmup=5):
    """median / min of the event time of one call, in microseconds"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(1e3 * a.elapsed_time(b))
    return {"median_us": round(statistics.median(times), 1), "min_us": round(min(times), 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=30)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("union_probe needs the GPU: nothing is measured without one")
    dev = torch.device("cuda:0")
    ops_ = operands(dev)
    native = hasattr(Fsp, "sparse_add_native")
    res = {"shape": SHAPE, "batch": BATCH, "C": C, "dtype": "f16", "rows": [int(i.shape[0]) for i, _ in ops_],
           "native_path": native, "repeats": args.repeats}

    def tensors(grad):
        return [spconv.SparseConvTensor(f.detach().clone().requires_grad_(grad), i, SHAPE, BATCH) for i, f in ops_]

    def run(fn, grad):
        def call():
            out = fn(tensors(grad))
            if grad:
                out.features.backward(gout[:out.features.shape[0]])
            return out
        return call

    module = spconv.AddTableMisaligned()
    forms = {"module": lambda t: module(t)}
    if native:
        forms["composite"] = lambda t: Fsp._sparse_add_hash_composite(*t)
    gout = torch.randn((2 * ROWS, C), device=dev).half()
    before = _lib.launch_counts(KEYS)
    first = module(tensors(False))
    res["union_rows"] = int(first.features.shape[0])
    res["launches_of_one_forward"] = {k: v - before[k] for k, v in _lib.launch_counts(KEYS).items()} if native else "composite"
    for rnd in range(2):                                                 # alternate the forms: two rounds each
        for name, fn in forms.items():
            res[f"{name}_fwd_round{rnd}"] = timed(run(fn, False), args.repeats)
            res[f"{name}_fwd_bwd_round{rnd}"] = timed(run(fn, True), args.repeats)
    if native:
        from spconv_amd.pytorch import _union
        idxs, feats = [i for i, _ in ops_], [f for _, f in ops_]
        u = _union.sparse_union(idxs, BATCH, SHAPE)
        res["stage_union_count_fill"] = timed(lambda: _union.sparse_union(idxs, BATCH, SHAPE), args.repeats)
        res["stage_add_fwd"] = timed(lambda: _union.add_fwd(feats, u.src, u.n_out), args.repeats)
        res["stage_add_bwd"] = timed(lambda: _union.add_bwd(gout[:u.n_out], u.rows, [True, True]), args.repeats)
        present = int((u.src >= 0).sum().item())
        nbytes = (present + u.n_out) * C * 2 + u.src.numel() * 4          # rows read + rows written + the src tables
        t = res["stage_add_fwd"]["median_us"] * 1e-6
        res["add_fwd_bytes"] = nbytes
        res["add_fwd_TBps"] = round(nbytes / t / 1e12, 3)
        res["add_fwd_share_of_8TBps"] = round(nbytes / t / 8e12, 3)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
