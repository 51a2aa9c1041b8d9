#!/usr/bin/env python
"""What does an axis collapse cost?  Times the height compression (axes = (0,), sum, f16) of two scenes -- 4 x 100 k rows
on [41, 1600, 1408] with C = 16, and 4 x 25 k rows on [5, 200, 176] with C = 128 -- on the collapse kernels
(csrc/collapse.hip) against the torch composite a user would write (unique of the projected keys + index_add_),
alternating in one process: the build, the forward and the backward on their own and together.  HIP events, warm-up,
median of the repeats; the forward kernel's bytes over its time are set against 8 TB/s.

    python tools/collapse_probe.py [--out profiles/collapse_probe.json] [--repeats 30]
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
from spconv_amd import _lib  # noqa: E402
from spconv_amd.pytorch import _collapse  # noqa: E402
from spconv_amd.pytorch import functional as Fsp  # noqa: E402

SHAPES = {
    "lidar_41x1600x1408_C16": dict(shape=[41, 1600, 1408], batch=4, rows=100_000, C=16),
    "late_5x200x176_C128": dict(shape=[5, 200, 176], batch=4, rows=25_000, C=128),
}
AXES = (0,)
KEYS = ("collapse/mark", "collapse/prefix", "collapse/rank", "collapse/list", "collapse/fwd", "collapse/bwd")


def scene(cfg, dev):
    """`rows` distinct voxels per batch element, shuffled"""
    rng = np.random.default_rng(0)
    shape, cells = cfg["shape"], int(np.prod(cfg["shape"]))
    parts = []
    for b in range(cfg["batch"]):
        keys = rng.choice(cells, size=cfg["rows"], replace=False)
        parts.append(np.stack([np.full_like(keys, b)] + list(np.unravel_index(keys, shape)), axis=1))
    idx = rng.permutation(np.concatenate(parts)).astype(np.int32)
    feat = torch.randn((idx.shape[0], cfg["C"]), device=dev).half()
    return torch.from_numpy(idx).to(dev), feat


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


class Composite:
    """unique of the projected keys (the count is read back) + index_add_ (float atomics); backward: a row gather"""

    def __init__(self, cfg):
        self.kept = [s for d, s in enumerate(cfg["shape"]) if d not in AXES]

    def build(self, idx):
        key = idx[:, 0].long()
        for d, s in enumerate(self.kept):
            key = key * s + idx[:, 2 + d].long()                # (axes = (0,): the kept coordinates start at column 2)
        uniq, inverse = torch.unique(key, sorted=True, return_inverse=True)
        cols = []
        rest = uniq
        for s in reversed(self.kept):
            cols.append(rest % s)
            rest = rest // s
        out_idx = torch.stack([rest] + cols[::-1], dim=1).int()
        return out_idx, inverse

    @staticmethod
    def fwd(feat, inverse, n_out):
        return torch.zeros((n_out, feat.shape[1]), dtype=feat.dtype, device=feat.device).index_add_(0, inverse, feat)

    @staticmethod
    def bwd(dout, inverse):
        return dout.index_select(0, inverse)


def probe(name, cfg, dev, repeats):
    idx, feat = scene(cfg, dev)
    shape, B, C = cfg["shape"], cfg["batch"], cfg["C"]
    res = {"shape": shape, "batch": B, "rows": int(idx.shape[0]), "C": C, "dtype": "f16", "axes": list(AXES), "reduce": "sum"}
    comp = Composite(cfg)
    before = _lib.launch_counts(KEYS)
    c = _collapse.sparse_collapse_build(idx, B, shape, AXES)
    res["launches_of_one_build"] = {k: v - before[k] for k, v in _lib.launch_counts(KEYS).items()}
    out_idx, inverse = comp.build(idx)
    assert torch.equal(out_idx, c.out_indices) and torch.equal(inverse.int(), c.rows)
    res["out_rows"] = c.n_out
    dout = torch.randn((c.n_out, C), device=dev).half()

    def native_all():
        b = _collapse.sparse_collapse_build(idx, B, shape, AXES)
        x = feat.detach().requires_grad_(True)
        Fsp.SparseCollapseFunction.apply(x, b, "sum", None).backward(dout)

    def composite_all():
        _, inv = comp.build(idx)
        x = feat.detach().requires_grad_(True)
        comp.fwd(x, inv, c.n_out).backward(dout)

    stages = {
        "native_build": lambda: _collapse.sparse_collapse_build(idx, B, shape, AXES),
        "composite_build": lambda: comp.build(idx),
        "native_fwd": lambda: _collapse.fwd(feat, c, "sum"),
        "composite_fwd": lambda: comp.fwd(feat, inverse, c.n_out),
        "native_bwd": lambda: _collapse.bwd(dout, c, "sum"),
        "composite_bwd": lambda: comp.bwd(dout, inverse),
        "native_build_fwd_bwd": native_all,
        "composite_build_fwd_bwd": composite_all,
    }
    for rnd in range(2):                                        # alternate the forms: two rounds each
        for stage, fn in stages.items():
            res[f"{stage}_round{rnd}"] = timed(fn, repeats)
    kept_rows = int((c.rows >= 0).sum().item())
    nbytes = (kept_rows + c.n_out) * C * 2 + (kept_rows + c.n_out + 1) * 4      # rows read + written, list + offsets
    t = min(res[f"native_fwd_round{r}"]["median_us"] for r in range(2)) * 1e-6
    res["fwd_bytes"] = nbytes
    res["fwd_TBps"] = round(nbytes / t / 1e12, 3)
    res["fwd_share_of_8TBps"] = round(nbytes / t / 8e12, 3)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=30)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("collapse_probe needs the GPU: nothing is measured without one")
    dev = torch.device("cuda:0")
    res = {"repeats": args.repeats}
    for name, cfg in SHAPES.items():
        res[name] = probe(name, cfg, dev, args.repeats)
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
