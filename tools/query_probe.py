#!/usr/bin/env python
"""What do the voxel query and the neighbour grouping cost?  The shape of Voxel R-CNN's Voxel RoI pooling on a stride-4
level: 4 scenes x 128 RoIs x 6^3 grid points = 110 592 queries over about 4 x 30 000 voxels of a lidar-like scene in an
11 x 400 x 352 grid, query range (4, 4, 4) -- 729 cells --, nsample 16, without a radius and with a radius of four
voxel sizes, C = 64, f16.  Timed on the kernels of csrc/query.hip: the query through the level's rank map and through
the hash table, the build of the transposed list, the grouped gather and its gradient.  Each against the torch
composite a user would otherwise write: spconv.HashTable over the level's keys, one query per window cell, topk over
the hit flags for the first nsample hits in visiting order, index_select for the gather, index_add_ for its gradient.
The two forms alternate in one process; HIP events around one call each, warm-up calls first, median and minimum of
the repeats, two interleaved rounds.

    python tools/query_probe.py [--out profiles/query_probe.json] [--repeats 30] [--composite-repeats 8]
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
import spconv_amd.pytorch as spconv  # noqa: E402
from spconv_amd import _lib  # noqa: E402
from spconv_amd.pytorch import _query, ops  # noqa: E402
from spconv_amd.pytorch import functional as Fsp  # noqa: E402
from spconv_amd.pytorch.hash import HashTable  # noqa: E402
from spconv_amd.utils import synthetic  # noqa: E402

GRID = [11, 400, 352]
VSIZE, RANGE = [0.2, 0.2, 0.4], [0.0, -40.0, -3.0, 70.4, 40.0, 1.4]          # a stride-4 level of a 0.05 x 0.05 x 0.1 grid
BATCH, VOXELS, ROIS, SIDE, C = 4, 30_000, 128, 6, 64
QRANGE, NSAMPLE, RADIUS = (4, 4, 4), 16, 4 * 0.2
KEYS = ("query/ranked", "query/hash", "query/group_fwd", "query/group_bwd", "pointvoxel/groups")


def scene():
    """the level's index rows in key order, and ROIS boxes of 3.9 x 1.6 x 1.56 m around occupied voxels per scene with
    SIDE^3 grid points each -> indices int32 [n, 4], queries fp32 [M, 3], batch ids int32 [M]"""
    rng = np.random.default_rng(0)
    idx = synthetic.lidar_like_scene(GRID, VOXELS, BATCH, seed=0).astype(np.int64)
    key = ((idx[:, 0] * GRID[0] + idx[:, 1]) * GRID[1] + idx[:, 2]) * GRID[2] + idx[:, 3]
    idx = idx[np.argsort(key)]
    steps = (np.arange(SIDE) + 0.5) / SIDE - 0.5
    cube = np.stack(np.meshgrid(steps, steps, steps, indexing="ij"), axis=-1).reshape(-1, 3) * np.array([3.9, 1.6, 1.56])
    pts, bids = [], []
    for b in range(BATCH):
        vox = idx[idx[:, 0] == b][:, 1:]
        centre = (vox[rng.integers(0, vox.shape[0], ROIS)][:, ::-1] + 0.5) * np.asarray(VSIZE) + np.asarray(RANGE[:3])
        pts.append((centre[:, None, :] + cube[None, :, :]).reshape(-1, 3))
        bids.append(np.full((ROIS * SIDE ** 3,), b))
    return idx.astype(np.int32), np.concatenate(pts).astype(np.float32), np.concatenate(bids).astype(np.int32)


def timed(fn, repeats, warmup=3):
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
    """the torch form: a hash table over the level's keys, one query per window cell, topk over the hit flags"""

    def __init__(self, pts, bids, indices):
        self.pts, self.bids = pts, bids.long()
        dev = pts.device
        self.lo, self.vs = torch.tensor(RANGE[:3], device=dev), torch.tensor(VSIZE, device=dev)
        self.ext = torch.tensor(GRID[::-1], device=dev)                          # xyz
        idx, nv = indices.long(), indices.shape[0]
        self.table = HashTable(dev, torch.int32, torch.int32, 2 * nv)
        self.table.insert(self.key(idx[:, 0], idx[:, 1:].flip(1)).int(), torch.arange(nv, dtype=torch.int32, device=dev))
        rz, ry, rx = QRANGE
        self.window = [(oz, oy, ox) for oz in range(-rz, rz + 1) for oy in range(-ry, ry + 1) for ox in range(-rx, rx + 1)]
        self.order = torch.arange(len(self.window), 0, -1, device=dev, dtype=torch.int32)      # earlier cell, larger score

    def key(self, b, xyz):
        return ((b * GRID[0] + xyz[:, 2]) * GRID[1] + xyz[:, 1]) * GRID[2] + xyz[:, 0]

    def query(self, radius):
        cell = torch.floor((self.pts - self.lo) / self.vs).long()
        rows, hit = [], []
        for oz, oy, ox in self.window:
            xyz = cell + torch.tensor([ox, oy, oz], device=cell.device)
            inside = ((xyz >= 0) & (xyz < self.ext)).all(dim=1)
            val, missing = self.table.query(self.key(self.bids, xyz.clamp_min(0).minimum(self.ext - 1)).int())
            ok = inside & ~missing
            if radius is not None:
                d = (xyz.float() + 0.5) * self.vs + self.lo - self.pts
                ok = ok & ((d * d).sum(dim=1) < radius * radius)
            rows.append(val)
            hit.append(ok)
        rows, hit = torch.stack(rows, dim=1), torch.stack(hit, dim=1)
        score, first = torch.topk(hit.int() * self.order, NSAMPLE, dim=1)        # the first hits, in visiting order
        kept = torch.where(score > 0, rows.gather(1, first), -1)
        return kept.int(), (score > 0).sum(dim=1).int()

    @staticmethod
    def group(vfeat, rows):
        out = vfeat.index_select(0, rows.clamp_min(0).reshape(-1).long()).view(rows.shape[0], rows.shape[1], -1)
        return out * (rows >= 0).unsqueeze(2).to(vfeat.dtype)


def grad_of(fwd, x, dout):
    """a callable that runs the backward of fwd(x) alone (the graph is kept)"""
    x = x.detach().requires_grad_(True)
    out = fwd(x)
    return lambda: torch.autograd.grad(out, x, dout, retain_graph=True)


def no_grad(fn):
    def run():
        with torch.no_grad():
            return fn()
    return run


def width_sweep(pts, bids, ranked_idx, plain_idx, repeats):
    """the query alone by forced group width (0: the host's own choice), three windows, both forms, no radius: what the
    host's rule in csrc/query.hip was read from"""
    dev, M, n = pts.device, int(pts.shape[0]), int(ranked_idx.shape[0])
    ndim, vsize, crange = _query._geometry(VSIZE, RANGE)
    out = {}
    for qrange, ns in (((1, 1, 1), 8), ((2, 2, 2), 16), ((4, 4, 4), 16)):
        for form, idx in (("ranked", ranked_idx), ("hash", plain_idx)):
            rankmap = _query.level_rankmap(idx, BATCH, GRID) if form == "ranked" else None
            ws = None if rankmap is not None else _query._ws(_query.query_ws_bytes(M, ns, ndim, n, False), dev)
            rows = torch.empty((M, ns), dtype=torch.int32, device=dev)
            count = torch.empty((M,), dtype=torch.int32, device=dev)
            for width in (0, 4, 8, 16, 32, 64):
                call = lambda: _query.voxel_query_into(pts, bids, None, _query._floats(vsize), _query._floats(crange), idx,
                                                       None, BATCH, GRID, rankmap, qrange, ns, None, False, rows, count,
                                                       None, ws, group_width=width)
                out[f"{form}_range{qrange[0]}_nsample{ns}_width{width}_median_us"] = timed(call, repeats)["median_us"]
    return out


def probe(dev, repeats, composite_repeats):
    idx_h, pts_h, bids_h = scene()
    pts, bids = torch.from_numpy(pts_h).to(dev), torch.from_numpy(bids_h).to(dev)
    ranked_idx, plain_idx = torch.from_numpy(idx_h).to(dev), torch.from_numpy(idx_h).to(dev)
    assert ops.attach_rank_map(ranked_idx, BATCH, GRID), "the level is in key order"
    nv, M = int(idx_h.shape[0]), int(pts_h.shape[0])
    res = {"grid": GRID, "batch": BATCH, "queries": M, "voxels": nv, "C": C, "query_range": list(QRANGE),
           "window_cells": 729, "nsample": NSAMPLE, "radius": RADIUS, "dtype": "f16"}
    comp = Composite(pts, bids, plain_idx)
    dummy = torch.zeros((nv, 1), device=dev)
    x_rank = spconv.SparseConvTensor(dummy, ranked_idx, GRID, BATCH)
    x_hash = spconv.SparseConvTensor(dummy, plain_idx, GRID, BATCH)
    native = lambda x, radius, groups=False: Fsp.voxel_query(pts, bids, x, VSIZE, RANGE, QRANGE, NSAMPLE, radius,
                                                            with_groups=groups)
    before = _lib.launch_counts(KEYS)
    nb = native(x_rank, None, True)
    res["launches_of_query_with_groups"] = {k: v - before[k] for k, v in _lib.launch_counts(KEYS).items()}
    stages = {}
    for name, radius in (("no_radius", None), ("radius", RADIUS)):
        a, b = native(x_rank, radius), native(x_hash, radius)
        assert torch.equal(a.rows, b.rows) and torch.equal(a.count, b.count)
        rows_c, count_c = comp.query(radius)
        same = (rows_c == a.rows).all(dim=1)
        res[f"queries_equal_to_composite_{name}"] = int(same.sum())             # (fp32 distances within an ulp of r2 may differ)
        res[f"mean_count_{name}"] = round(float(a.count.float().mean()), 3)
        res[f"queries_truncated_{name}"] = int((a.count == NSAMPLE).sum())
        stages[f"query_ranked_{name}"] = (no_grad(lambda r=radius: native(x_rank, r)), no_grad(lambda r=radius: comp.query(r)))
        stages[f"query_hash_{name}"] = (no_grad(lambda r=radius: native(x_hash, r)), no_grad(lambda r=radius: comp.query(r)))
    vfeat = torch.randn((nv, C), device=dev).half()
    dout = torch.randn((M, NSAMPLE, C), device=dev).half()
    out = Fsp.group_voxels(vfeat, nb)
    assert torch.equal(out, comp.group(vfeat, nb.rows))
    res["entries"] = int((nb.rows >= 0).sum())
    stages.update({
        "groups_build": (lambda: _query.neighbor_groups(nb.rows, nv), None),     # (the composite's index_add_ needs none)
        "group_forward": (no_grad(lambda: Fsp.group_voxels(vfeat, nb)), no_grad(lambda: comp.group(vfeat, nb.rows))),
        "group_backward": (grad_of(lambda v: Fsp.group_voxels(v, nb), vfeat, dout),
                           grad_of(lambda v: comp.group(v, nb.rows), vfeat, dout)),
    })
    for rnd in range(2):                                        # alternate the forms: two rounds each
        for stage, (nat, composite) in stages.items():
            res[f"native_{stage}_round{rnd}"] = timed(nat, repeats)
            if composite is not None:
                res[f"composite_{stage}_round{rnd}"] = timed(composite, composite_repeats if "query" in stage else repeats,
                                                             warmup=1 if "query" in stage else 3)
    verdict = {}
    for stage, (_, composite) in stages.items():
        nat = [res[f"native_{stage}_round{r}"]["median_us"] for r in range(2)]
        if composite is None:
            verdict[stage] = {"native_us": nat}
            continue
        com = [res[f"composite_{stage}_round{r}"]["median_us"] for r in range(2)]
        verdict[stage] = {"native_us": nat, "composite_us": com, "native_no_slower": max(nat) <= min(com)}
    nat = [verdict["groups_build"]["native_us"][r] + verdict["group_backward"]["native_us"][r] for r in range(2)]
    com = verdict["group_backward"]["composite_us"]             # the native backward WITH the list it needs
    verdict["groups_build_and_group_backward"] = {"native_us": [round(v, 1) for v in nat], "composite_us": com,
                                                  "native_no_slower": max(nat) <= min(com)}
    res["verdict"] = verdict
    res["slower_than_composite"] = sorted(k for k, v in verdict.items() if v.get("native_no_slower") is False)
    for name in ("no_radius", "radius"):
        r, h = min(verdict[f"query_ranked_{name}"]["native_us"]), min(verdict[f"query_hash_{name}"]["native_us"])
        res[f"ranked_faster_than_hash_{name}"] = r < h
    res["width_sweep"] = width_sweep(pts, bids, ranked_idx, plain_idx, repeats)
    eb = 2                                                      # bytes the gather must move at least, over its time
    fwd_us = min(verdict["group_forward"]["native_us"])
    nbytes = M * NSAMPLE * 4 + nv * C * eb + M * NSAMPLE * C * eb
    res["group_forward_bytes"] = nbytes
    res["group_forward_TBps"] = round(nbytes / (fwd_us * 1e-6) / 1e12, 3)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--composite-repeats", type=int, default=8)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("query_probe needs the GPU: nothing is measured without one")
    res = {"repeats": args.repeats, "composite_repeats": args.composite_repeats}
    res.update(probe(torch.device("cuda:0"), args.repeats, args.composite_repeats))
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
