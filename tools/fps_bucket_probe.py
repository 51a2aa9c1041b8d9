#!/usr/bin/env python
"""What does farthest-point sampling with bucket pruning cost (csrc/fps_bucket.hip), against the scan path it must equal?
The two clouds of tools/sample_probe.py: 4 scenes x 16 384 points -> 2048 samples and 4 x 75 000 points -> 4096 samples.
Timed: the build alone (boxes, keys, sort, records), the sampling kernel alone (on a finished build: it starts over
at each call), both together, and method "scan" -- the kernel of spx_fps, unchanged -- alternating in the same process;
HIP events around one call, 5 warm-ups, median and minimum of 30, two interleaved rounds.  Also the share of bucket
table entries written, visits / (steps x buckets) per scene, and whether every slot equals the scan path's.

    python tools/fps_bucket_probe.py [--out profiles/fps_bucket_probe.json] [--repeats 30]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sample_probe import BATCH, FPS_CASES, cloud, timed  # noqa: E402
from spconv_amd import _lib  # noqa: E402
from spconv_amd.pytorch import _sample  # noqa: E402
from spconv_amd.pytorch import functional as Fsp  # noqa: E402

WARMUP = 5


def buckets_of(n):
    size = _sample.bucket_points()
    while -(-n // size) > _sample.bucket_cap():
        size *= 2
    return -(-n // size)


def probe(dev, repeats):
    L = _lib.load()
    res = {"batch": BATCH, "bucket_cap": _sample.bucket_cap(), "bucket_points": _sample.bucket_points(), "warmup": WARMUP}
    stages = {}
    for name, n, K in FPS_CASES:
        pts_h, bid_h = cloud(n, seed=n)
        pts, bid = torch.from_numpy(pts_h).to(dev), torch.from_numpy(bid_h).to(dev)
        N = BATCH * n
        groups = Fsp.scene_groups(bid, N, BATCH)
        scan = Fsp.farthest_point_sample_method(pts, bid, BATCH, K, "scan", groups=groups)
        s, visits = Fsp.farthest_point_sample_method(pts, bid, BATCH, K, "bucket", groups=groups, with_visits=True)
        nb = buckets_of(n)
        res[name] = {"points_per_scene": n, "samples": K, "buckets_per_scene": nb,
                     "slots_equal_to_scan": int((s.idx == scan.idx).sum()), "slots": BATCH * K,
                     "counts_equal_to_scan": bool(torch.equal(s.count, scan.count)),
                     "visits": visits.tolist(),
                     "visited_share": [round(v / (c * nb), 5) for v, c in zip(visits.tolist(), s.count.tolist())]}
        idx = torch.empty((BATCH, K), dtype=torch.int32, device=dev)
        count = torch.empty((BATCH,), dtype=torch.int32, device=dev)
        ws = torch.empty((_sample.fps_bucket_ws_bytes(N, BATCH, 3),), dtype=torch.uint8, device=dev)
        stream = torch.cuda.current_stream().cuda_stream

        def build(p=pts, g=groups, m=N, w=ws):
            _lib.check(L.spx_fps_bucket_build(p.data_ptr(), 4, m, 3, g.offsets.data_ptr(), g.list.data_ptr(), BATCH,
                                              w.data_ptr(), w.numel(), stream))

        def sample(m=N, k=K, i=idx, c=count, w=ws):
            _lib.check(L.spx_fps_bucket(m, 3, BATCH, k, i.data_ptr(), c.data_ptr(), None, w.data_ptr(), w.numel(), stream))
        stages[f"{name}_build"] = build
        stages[f"{name}_sampling"] = sample                          # (behind the build stage: its records are in ws)
        stages[f"{name}_bucket"] = lambda p=pts, g=groups, k=K, i=idx, c=count, w=ws: _sample.fps_bucket_into(p, g, k, 3, i, c, w)
        stages[f"{name}_scan"] = lambda p=pts, b=bid, k=K, g=groups: Fsp.farthest_point_sample(p, b, BATCH, k, groups=g)
    for rnd in range(2):                                             # alternate the forms: two rounds each
        for stage, fn in stages.items():
            res[f"{stage}_round{rnd}"] = timed(fn, repeats, warmup=WARMUP)
    verdict = {}
    for name, n, K in FPS_CASES:
        med = {k: [res[f"{name}_{k}_round{r}"]["median_us"] for r in range(2)] for k in ("build", "sampling", "bucket", "scan")}
        verdict[name] = {**{f"{k}_us": v for k, v in med.items()},
                         "sampling_us_per_step": [round(v / K, 3) for v in med["sampling"]],
                         "scan_us_per_step": [round(v / K, 3) for v in med["scan"]],
                         "scan_over_bucket": [round(a / b, 2) for a, b in zip(med["scan"], med["bucket"])],
                         "bucket_no_slower": max(med["bucket"]) <= min(med["scan"])}
    res["verdict"] = verdict
    res["slower_than_scan"] = sorted(k for k, v in verdict.items() if not v["bucket_no_slower"])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=30)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("fps_bucket_probe needs the GPU: nothing is measured without one")
    res = {"repeats": args.repeats}
    res.update(probe(torch.device("cuda:0"), args.repeats))
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
