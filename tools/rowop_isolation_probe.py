#!/usr/bin/env python
"""What does NaN propagation cost in the two kernels that took an extra compare per element?  Times, on the library the
process loaded (SPX_LIB picks another build: run once per build and compare),

    collapse max forward / backward   spx_collapse_fwd / _bwd, SPX_COLLAPSE_MAX   (changed)
    collapse sum forward              the same kernel's other instantiation        (control: unchanged code)
    row score absmax                  spx_row_score, SPX_SCORE_ABSMAX              (changed)
    row score absmean                                                              (control)

over 400 000 f16 rows in 100 000 groups (the point-voxel reduction of tools/pointvoxel_probe.py's size), C = 16 and 64.
HIP events around 20 back-to-back calls, warm-up, median and minimum of the repeats, two alternating rounds.

    python tools/rowop_isolation_probe.py [--out FILE] [--repeats 30]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from spconv_amd import _lib  # noqa: E402
from spconv_amd.pytorch import _collapse, _pointvoxel, _select  # noqa: E402

ROWS, GROUPS = 400_000, 100_000


INNER = 20      # calls between two events: a call is 15 to 40 us, of the order of the event pair's own cost


def timed(fn, repeats, warmup=5):
    """median / min of the event time of INNER back-to-back calls, per call, in microseconds"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(INNER):
            fn()
        b.record()
        b.synchronize()
        times.append(1e3 * a.elapsed_time(b) / INNER)
    return {"median_us": round(statistics.median(times), 1), "min_us": round(min(times), 1)}


def probe(C, dev, repeats):
    g = torch.Generator().manual_seed(C)
    ids = torch.randint(0, GROUPS, (ROWS,), generator=g).to(dev)
    feat = torch.randn((ROWS, C), generator=g).half().to(dev)
    groups = _pointvoxel.point_groups(ids, GROUPS)
    out = _collapse.fwd(feat, groups, "max")
    dout = torch.randn((GROUPS, C), generator=g).half().to(dev)
    stages = {
        "collapse_max_fwd": lambda: _collapse.fwd(feat, groups, "max"),
        "collapse_max_bwd": lambda: _collapse.bwd(dout, groups, "max", feat, out),
        "collapse_sum_fwd": lambda: _collapse.fwd(feat, groups, "sum"),
        "score_absmax": lambda: _select.row_score(feat, "absmax"),
        "score_absmean": lambda: _select.row_score(feat, "absmean"),
    }
    res = {"rows": ROWS, "groups": GROUPS, "C": C, "dtype": "f16"}
    for rnd in range(2):
        for stage, fn in stages.items():
            res[f"{stage}_round{rnd}"] = timed(fn, repeats)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=30)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this probe needs the GPU"
    dev = torch.device("cuda:0")
    res = {"repeats": args.repeats, "calls_per_event_pair": INNER, "library": os.path.relpath(_lib.LIB_PATH, ROOT)}
    for C in (16, 64):
        res[f"C{C}"] = probe(C, dev, args.repeats)
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
