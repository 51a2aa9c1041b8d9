#!/usr/bin/env python
"""What do the cell-indexed queries cost (csrc/cellquery.hip: ``F.point_cell_index`` + ``F.ball_query_cells`` /
``F.knn_query_cells``) beside the brute-force forms (``F.ball_query`` / ``F.knn_query``), at the README's shapes?
Synthetic lidar-like clouds (knn_probe's: two thirds near a ground sheet in a 70.4 x 80 x 4 m box): 8192 FPS keypoints
over 4 x 75 000 points with radius 0.8 and nsample 16 / 32, k = 16 within 0.8 for the same clouds, and a k = 16 self-query
of 4 x 16 384 points within 1.6.  Per case, in ONE process and alternating: the index build alone, the query alone, both
together, and the brute-force call, each by HIP events round the calls on one stream; 5 warm-ups, the median of
`--repeats` calls, two rounds.  The spread of a case is the largest difference between the two rounds of any of its
items (identical runs); the cell form is NOT SLOWER when build + query is below the brute-force call plus that spread.
The ball tables must equal the brute-force ones and the k-NN tables their leading entries inside the radius: asserted.

    python tools/cellquery_probe.py [--out profiles/cellquery_probe.json] [--repeats 30]
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
from spconv_amd.pytorch import functional as F  # noqa: E402

BATCH, WARMUP = 4, 5
EXTENT = np.array([70.4, 80.0, 4.0])
RANGE = [0.0, 0.0, -1.0, 70.4, 80.0, 5.0]


def cloud(n, seed, dev):
    rng = np.random.default_rng(seed)
    pts = rng.random((BATCH * n, 4))
    pts[:, :3] *= EXTENT
    ground = rng.random(BATCH * n) < 2.0 / 3.0
    pts[ground, 2] = np.clip(0.3 + 0.1 * rng.standard_normal(int(ground.sum())), -0.9, 4.9)
    bid = np.repeat(np.arange(BATCH, dtype=np.int32), n)
    return torch.from_numpy(pts.astype(np.float32)).to(dev), torch.from_numpy(bid).to(dev)


def timed(fn, repeats):
    for _ in range(WARMUP):
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
    return round(statistics.median(times), 1)


def case(pts, bid, qs, qb, radius, n, knn, dev):
    """the four timed items of one case, the tables checked against the brute-force form first"""
    N, M = int(pts.shape[0]), int(qs.shape[0])
    plan = F.cluster_plan(radius, RANGE, BATCH)
    buf = F.cell_index_buffers(N, plan, dev)
    groups = F.scene_groups(bid, N, BATCH)
    r2 = float(np.float32(radius) ** 2)
    i32 = dict(dtype=torch.int32, device=dev)
    rows, count = torch.empty((M, n), **i32), torch.empty((M,), **i32)
    d2, w = torch.empty((M, n), device=dev), torch.empty((M, n), device=dev)
    build = lambda: F.point_cell_index_into(pts, bid, None, plan, buf)
    index = build()
    if knn:
        query = lambda: F.knn_query_cells_into(qs, qb, None, index, n, r2, 1e-8, False, rows, count, d2, w)
        brute = lambda: F.knn_query_into(qs, qb, None, pts, groups, 3, n, 1e-8, False, rows, count, d2, w)
        got, want = F.knn_query_cells(qs, qb, index, n, radius), F.knn_query(qs, qb, pts, bid, BATCH, n)
        inside = (want.dist2 < r2) & (want.rows >= 0)
        assert torch.equal(torch.where(inside, want.rows, -1), got.rows) and torch.equal(inside.sum(1).int(), got.count)
    else:
        query = lambda: F.ball_query_cells_into(qs, qb, None, index, n, r2, False, rows, count, None)
        brute = lambda: F.ball_query_into(qs, qb, None, pts, groups, 3, n, r2, False, rows, count, None)
        got, want = F.ball_query_cells(qs, qb, index, radius, n), F.ball_query(qs, qb, pts, bid, BATCH, radius, n)
        assert torch.equal(got.rows, want.rows) and torch.equal(got.count, want.count)
    both = lambda: (build(), query())
    info = {"points": N, "queries": M, "radius": radius, "entries": n, "grid_zyx": list(plan.grid_zyx),
            "mean_count": round(float(got.count.float().mean()), 2), "full_share": round(float((got.count == n).float().mean()), 3),
            "equal_to_brute_force": True}
    return info, {"build": build, "query": query, "both": both, "brute": brute}


def probe(dev, repeats):
    pts, bid = cloud(75_000, 75_000, dev)
    keys = F.farthest_point_sample(pts, bid, BATCH, 2048)
    kp = F.gather_samples(pts, keys).contiguous()
    sp, sb = cloud(16_384, 16_384, dev)
    cases = {"ball16_8192_over_4x75k": (pts, bid, kp, keys.batch_ids, 0.8, 16, False),
             "ball32_8192_over_4x75k": (pts, bid, kp, keys.batch_ids, 0.8, 32, False),
             "knn16_8192_over_4x75k": (pts, bid, kp, keys.batch_ids, 0.8, 16, True),
             "knn16_self_4x16k": (sp, sb, sp, sb, 1.6, 16, True)}
    res, fns = {"batch": BATCH, "warmup": WARMUP, "range_xyz": RANGE}, {}
    for name, args in cases.items():
        res[name], fns[name] = case(*args, dev)
    for rnd in range(2):
        for name in cases:                                  # the cell form and the brute-force form alternate
            res[name][f"round{rnd}_us"] = {item: timed(fn, repeats) for item, fn in fns[name].items()}
            print(f"round {rnd} {name}: {res[name][f'round{rnd}_us']}", file=sys.stderr, flush=True)
    for name in cases:
        r0, r1 = res[name]["round0_us"], res[name]["round1_us"]
        spread = max(abs(r0[k] - r1[k]) for k in r0)
        res[name]["spread_us"] = round(spread, 1)
        res[name]["not_slower_with_build"] = max(r0["both"], r1["both"]) <= min(r0["brute"], r1["brute"]) + spread
    res["slower_than_brute_force"] = sorted(k for k in cases if not res[k]["not_slower_with_build"])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=30)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("cellquery_probe needs the GPU: nothing is measured without one")
    res = {"repeats": args.repeats}
    res.update(probe(torch.device("cuda:0"), args.repeats))
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
