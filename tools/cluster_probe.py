#!/usr/bin/env python
"""What does instance clustering cost (csrc/cluster.hip, ``F.cluster_points``), against what its users do today: a GPU
ball query, the table copied to the host, a traversal on the CPU?  Synthetic rooms (no dataset is needed): 4 scenes of
100 000 and of 250 000 points, 60 % on the floor and the walls of an 8 x 8 x 3 m room, 40 % in Gaussian blobs, the radius
chosen per size for a mean degree of 13 to 15 (PointGroup's regime, and no ball beyond the query's 128 slots).  Timed: the items of one call -- index build
(voxeliser + point_groups), records, link, flatten (roots + sizes + numbering) and groups -- by HIP events recorded
between them on the one stream they run on, and the whole call by events around it; the composite -- the project's own
``F.ball_query`` of the cloud against itself with nsample 128 (asserted: no count reaches it), ``.cpu()``, and a numpy
union-find (hook the larger root onto the smaller, jump pointers, repeat) -- by a host clock around work that ends on
the host.  5 warm-ups; median and minimum of `--repeats` calls (the composite: of 3), two interleaved rounds.  The
composite's clusters must equal the native ones: asserted.

    python tools/cluster_probe.py [--out profiles/cluster_probe.json] [--repeats 20]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from spconv_amd.pytorch import functional as F  # noqa: E402

BATCH, WARMUP, NSAMPLE, MIN_POINTS = 4, 5, 128, 50
ROOM = (8.0, 8.0, 3.0)
CASES = (("4x100k", 100_000, 0.09), ("4x250k", 250_000, 0.06))
ITEMS = ("index", "records", "link", "flatten", "groups")


def cloud(n, seed):
    """BATCH scenes of n points, interleaved: planar patches (floor and four walls, 1 cm of noise) and 40 blobs"""
    rng = np.random.default_rng(seed)
    pts = np.empty((BATCH, n, 3), np.float32)
    for b in range(BATCH):
        n_plane = int(0.6 * n)
        p = rng.random((n_plane, 3)) * ROOM
        face = rng.integers(0, 5, n_plane)
        p[face == 0, 2] = 0.0
        for k, (ax, v) in enumerate(((0, 0.0), (0, ROOM[0]), (1, 0.0), (1, ROOM[1])), start=1):
            p[face == k, ax] = v
        p += rng.normal(0, 0.01, p.shape)
        centres = rng.random((40, 3)) * (np.array(ROOM) - 1.0) + 0.5
        q = centres[rng.integers(0, 40, n - n_plane)] + rng.normal(0, 0.15, (n - n_plane, 3))
        pts[b] = np.concatenate([p, q])[rng.permutation(n)]
    order = rng.permutation(BATCH * n)
    bid = np.repeat(np.arange(BATCH, dtype=np.int32), n)[order]
    return np.ascontiguousarray(pts.reshape(-1, 3)[order]), bid


def host_components(rows):
    """rows int32 [N, S] (neighbour indices, -1: none) -> the smallest index of every point's component"""
    N = rows.shape[0]
    u = np.repeat(np.arange(N, dtype=np.int64), rows.shape[1])
    v = rows.reshape(-1).astype(np.int64)
    u, v = u[v >= 0], v[v >= 0]
    parent = np.arange(N, dtype=np.int64)
    while True:
        ru, rv = parent[u], parent[v]
        live = ru != rv
        if not live.any():
            return parent
        u, v, ru, rv = u[live], v[live], ru[live], rv[live]
        np.minimum.at(parent, np.maximum(ru, rv), np.minimum(ru, rv))
        while True:                                                  # pointer jumping down to the roots
            nxt = parent[parent]
            if np.array_equal(nxt, parent):
                break
            parent = nxt


def composite(pts, bid, radius):
    nb = F.ball_query(pts, bid, pts, bid, BATCH, radius, NSAMPLE)
    rows, count = nb.rows.cpu().numpy(), nb.count.cpu().numpy()
    assert int(count.max()) < NSAMPLE, f"a ball holds {int(count.max())} points: the table is truncated"
    return host_components(rows), float(count.mean()) - 1.0


def timed_call(fn, repeats):
    """the whole call by events around it, its items by events between them"""
    marks = []
    stage = lambda name: marks.append(torch.cuda.Event(enable_timing=True)) or marks[-1].record()
    for _ in range(WARMUP):
        fn(None)
    torch.cuda.synchronize()
    whole, items = [], {k: [] for k in ITEMS}
    for _ in range(repeats):
        marks.clear()
        a = torch.cuda.Event(enable_timing=True)
        a.record()
        fn(stage)
        marks[-1].synchronize()
        whole.append(1e3 * a.elapsed_time(marks[-1]))
        for k, (e0, e1) in zip(ITEMS, zip([a] + marks[:-1], marks)):
            items[k].append(1e3 * e0.elapsed_time(e1))
    stat = lambda t: {"median_us": round(statistics.median(t), 1), "min_us": round(min(t), 1)}
    return {"whole": stat(whole), **{k: stat(t) for k, t in items.items()}}


def timed_host(fn, repeats):
    fn()
    times = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        times.append(1e6 * (time.perf_counter() - t0))
    return {"median_us": round(statistics.median(times), 1), "min_us": round(min(times), 1)}


def probe(dev, repeats):
    res = {"batch": BATCH, "warmup": WARMUP, "nsample": NSAMPLE, "min_points": MIN_POINTS}
    native, comp = {}, {}
    for name, n, radius in CASES:
        pts_h, bid_h = cloud(n, seed=n)
        pts, bid = torch.from_numpy(pts_h).to(dev), torch.from_numpy(bid_h).to(dev)
        N = BATCH * n
        rng = [-0.5, -0.5, -0.5, ROOM[0] + 0.5, ROOM[1] + 0.5, ROOM[2] + 0.5]
        plan = F.cluster_plan(radius, rng, BATCH)
        buf = F.cluster_buffers(N, plan, F.cluster_cap(N, MIN_POINTS), dev)
        c = F.cluster_points_into(pts, bid, None, plan, None, None, MIN_POINTS, buf)
        root_ref, degree = composite(pts, bid, radius)
        root = c.root.cpu().numpy()
        inside = root >= 0
        assert int(c.status.item()) == 0
        assert inside.all(), "the range covers the room: every point takes part"
        assert np.array_equal(root, root_ref), "the composite finds other clusters"
        sizes = np.bincount(root[inside], minlength=N)
        kept = np.flatnonzero(sizes >= MIN_POINTS)
        assert int(c.count.item()) == len(kept)
        assert np.array_equal(np.flatnonzero(c.cluster_of_point.cpu().numpy() >= 0), np.flatnonzero(inside & (sizes[root] >= MIN_POINTS)))
        res[name] = {"points": N, "radius": radius, "grid_zyx": list(plan.grid_zyx), "mean_degree": round(degree, 2),
                     "components": int((sizes > 0).sum()), "clusters_kept": len(kept), "largest": int(sizes.max()),
                     "equal_to_composite": True}
        native[name] = lambda stage, a=(pts, bid, None, plan, None, None, MIN_POINTS, buf): F.cluster_points_into(*a, stage=stage)
        comp[name] = lambda p=pts, b=bid, r=radius: composite(p, b, r)
    for rnd in range(2):
        for name, _, _ in CASES:
            res[f"native_{name}_round{rnd}"] = timed_call(native[name], repeats)
            res[f"composite_{name}_round{rnd}"] = timed_host(comp[name], 3)
            print(f"round {rnd} {name}: native {res[f'native_{name}_round{rnd}']['whole']['median_us']} us, composite "
                  f"{res[f'composite_{name}_round{rnd}']['median_us']} us", file=sys.stderr, flush=True)
    verdict = {}
    for name, _, _ in CASES:
        c_us = [res[f"composite_{name}_round{r}"]["median_us"] for r in range(2)]
        n_us = {k: [res[f"native_{name}_round{r}"][k]["median_us"] for r in range(2)] for k in ("whole",) + ITEMS}
        verdict[name] = {"composite_us": c_us, **{f"{k}_us": v for k, v in n_us.items()},
                         "link_share_of_whole": [round(a / b, 3) for a, b in zip(n_us["link"], n_us["whole"])],
                         "native_no_slower": max(n_us["whole"]) <= min(c_us)}
    res["verdict"] = verdict
    res["slower_than_composite"] = sorted(k for k, v in verdict.items() if not v["native_no_slower"])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("cluster_probe needs the GPU: nothing is measured without one")
    res = {"repeats": args.repeats}
    res.update(probe(torch.device("cuda:0"), args.repeats))
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
