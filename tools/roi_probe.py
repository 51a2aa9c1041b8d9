#!/usr/bin/env python
"""What do the kernels of csrc/roi.hip and the poolings composed around them cost?  The second stage of a two-stage
detector at its own shapes: 4 scenes x 75 000 points, 4 x 128 RoIs and 4 x 40 ground-truth boxes, nsample 512, a 12^3
grid, C = 64 float16 features.  Cases: (a) points_in_boxes over the ground-truth boxes (labels) and (b) over the RoIs;
(c) box_query of the RoIs (nsample 512, pad cycle), the public call and (c') the query launches alone over ready
frames and scene lists; (d) roi_point_pool forward and (d') forward + backward; (e) roi_aware_pool max over 12^3 cells
(2048 points per box) forward and (e') forward + backward.  Beside each: what a user without the extension runs -- a
torch composite per scene: the broadcast [N, M] test in the boxes' frames (the same cosines and sines), `argmax` of the
mask for the lowest box, `topk` of the masked point indices for the first nsample hits in ascending order with the
cyclic pad as a `gather`, `index_select` of the rows, and `scatter_reduce_` (amax) over the global cell ids.  The two
forms alternate in one process; HIP events around one call each, warm-up calls first, median and minimum of the
repeats, two interleaved rounds.

    python tools/roi_probe.py [--out profiles/roi_probe.json] [--repeats 20]
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
from spconv_amd.pytorch import _roi  # noqa: E402
from spconv_amd.pytorch import functional as Fsp  # noqa: E402

BATCH, POINTS, ROIS, GTS, NSAMPLE, GRID, MAX_PTS, C = 4, 75000, 128, 40, 512, 12, 2048, 64


def scene(seed):
    """per scene GTS cars in a 70.4 x 80 m field, ROIS jittered proposals around them, POINTS points of which a fifth
    lie inside the cars -> gt fp32 [B * GTS, 7], rois fp32 [B * ROIS, 7], points fp32 [B * POINTS, 4] and the batch ids"""
    rng = np.random.default_rng(seed)
    gts, rois, pts = [], [], []
    for _ in range(BATCH):
        g = np.zeros((GTS, 7))
        g[:, 0], g[:, 1], g[:, 2] = rng.random(GTS) * 70.4, rng.random(GTS) * 80.0 - 40.0, rng.random(GTS) * 2 - 1
        g[:, 3], g[:, 4], g[:, 5] = 3.5 + rng.random(GTS) * 1.5, 1.5 + rng.random(GTS) * 0.5, 1.4 + rng.random(GTS) * 0.4
        g[:, 6] = rng.random(GTS) * 6.28 - 3.14
        r = g[rng.integers(0, GTS, ROIS)]
        r[:, :2] += (rng.random((ROIS, 2)) - 0.5) * 1.2
        r[:, 3:6] *= 1.0 + (rng.random((ROIS, 3)) - 0.5) * 0.2
        r[:, 6] += (rng.random(ROIS) - 0.5) * 0.3
        p = np.zeros((POINTS, 4))
        p[:, 0], p[:, 1], p[:, 2] = rng.random(POINTS) * 70.4, rng.random(POINTS) * 80.0 - 40.0, rng.random(POINTS) * 4 - 3
        k = rng.integers(0, GTS, POINTS // 5)
        u = (rng.random((POINTS // 5, 3)) - 0.5) * g[k, 3:6]
        c, s = np.cos(g[k, 6]), np.sin(g[k, 6])
        p[:POINTS // 5, 0] = g[k, 0] + u[:, 0] * c - u[:, 1] * s
        p[:POINTS // 5, 1] = g[k, 1] + u[:, 0] * s + u[:, 1] * c
        p[:POINTS // 5, 2] = g[k, 2] + u[:, 2]
        p[:, 3] = rng.random(POINTS)
        rng.shuffle(p)
        gts.append(g), rois.append(r), pts.append(p)
    ids = lambda n: np.repeat(np.arange(BATCH, dtype=np.int32), n)
    f32 = lambda parts: np.concatenate(parts).astype(np.float32)
    return f32(gts), ids(GTS), f32(rois), ids(ROIS), f32(pts), ids(POINTS)


def timed(fn, repeats, warmup=2):
    """median / min of one call in microseconds between HIP events"""
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


# ------------------------------------------------------------------------------------------- the torch composite
def composite_mask(frames, pts):
    """bool [M, N] and (lx, ly, lz) of one scene: the broadcast test, every step a torch operation of its own"""
    sx, sy = pts[None, :, 0] - frames[:, 0:1], pts[None, :, 1] - frames[:, 1:2]
    lz = pts[None, :, 2] - frames[:, 2:3]
    c, s = frames[:, 6:7], frames[:, 7:8]
    lx, ly = sx * c + sy * s, sy * c - sx * s
    hx, hy, hz = frames[:, 3:4], frames[:, 4:5], frames[:, 5:6]
    return (lz.abs() <= hz) & (lx > -hx) & (lx < hx) & (ly > -hy) & (ly < hy), lx, ly, lz


def composite_points_in_boxes(frames, per_scene, pts):
    out = []
    for b in range(BATCH):
        mask, _, _, _ = composite_mask(frames[b * per_scene:(b + 1) * per_scene], pts[b * POINTS:(b + 1) * POINTS])
        first = mask.to(torch.int8).argmax(0) + b * per_scene
        out.append(torch.where(mask.any(0), first, torch.full_like(first, -1)))
    return torch.cat(out).int()


def composite_box_query(frames, per_scene, pts, nsample, cycle, grid=None):
    """rows [M, nsample] (global point index, -1), count [M], cells [M, nsample] or None"""
    rows, counts, cells = [], [], []
    slot = torch.arange(nsample, device=pts.device)[None]
    for b in range(BATCH):
        f = frames[b * per_scene:(b + 1) * per_scene]
        mask, lx, ly, lz = composite_mask(f, pts[b * POINTS:(b + 1) * POINTS])
        idx = torch.arange(POINTS, device=pts.device)[None]
        key = torch.where(mask, POINTS - idx, torch.zeros_like(idx))
        top, at = torch.topk(key, nsample, dim=1)                       # descending key = ascending point index
        cnt = mask.sum(1).clamp(max=nsample)
        if cycle:
            at = torch.gather(at, 1, torch.where(slot < cnt[:, None], slot, slot % cnt.clamp(min=1)[:, None]))
            live = (cnt > 0)[:, None].expand(-1, nsample)
        else:
            live = slot < cnt[:, None]
        rows.append(torch.where(live, at + b * POINTS, torch.full_like(at, -1)))
        counts.append(cnt)
        if grid is not None:
            cell = torch.zeros_like(at)
            for l, h in ((lx, f[:, 3:4]), (ly, f[:, 4:5]), (lz, f[:, 5:6])):
                w = (h + h) / float(grid)
                cell = cell * grid + ((torch.gather(l, 1, at) + h) / w).int().clamp(0, grid - 1)
            base = (torch.arange(per_scene, device=pts.device) + b * per_scene)[:, None] * grid ** 3
            cells.append(torch.where(live, cell + base, torch.full_like(cell, -1)))
    return torch.cat(rows), torch.cat(counts), (torch.cat(cells) if grid is not None else None)


def composite_point_pool(frames, pts, feats):
    rows, cnt, _ = composite_box_query(frames, ROIS, pts, NSAMPLE, True)
    flat = rows.clamp(min=0).reshape(-1)
    pooled = torch.cat([pts[:, :3].index_select(0, flat).to(feats.dtype), feats.index_select(0, flat)], 1)
    pooled = pooled.view(rows.shape[0], NSAMPLE, -1) * (rows >= 0)[:, :, None]
    return pooled, (cnt == 0).int()


def composite_aware_pool(frames, pts, feats):
    rows, _, cells = composite_box_query(frames, ROIS, pts, MAX_PTS, False, GRID)
    live = (cells >= 0).reshape(-1)
    src = feats.index_select(0, rows.reshape(-1)[live])
    out = torch.zeros((rows.shape[0] * GRID ** 3, feats.shape[1]), dtype=feats.dtype, device=feats.device)
    out.scatter_reduce_(0, cells.reshape(-1)[live][:, None].expand(-1, feats.shape[1]).long(), src, "amax",
                        include_self=False)
    return out.view(rows.shape[0], GRID, GRID, GRID, -1)


# ------------------------------------------------------------------------------------------- the cases
def probe(dev, repeats):
    gt_h, gid_h, roi_h, rid_h, pts_h, pid_h = scene(1)
    t = lambda a: torch.from_numpy(a).to(dev)
    gt, gid, roi, rid, pts, pid = t(gt_h), t(gid_h), t(roi_h), t(rid_h), t(pts_h), t(pid_h)
    feats = torch.from_numpy(np.random.default_rng(2).integers(-3, 4, (BATCH * POINTS, C)).astype(np.float32)).to(dev).half()
    res = {"batch": BATCH, "points_per_scene": POINTS, "rois_per_scene": ROIS, "gt_per_scene": GTS, "nsample": NSAMPLE,
           "grid": GRID, "max_pts_per_box": MAX_PTS, "C": C, "dtype": "float16"}
    fgt, froi = Fsp.boxes_to_frames(gt), Fsp.boxes_to_frames(roi)
    groups = Fsp.scene_groups(pid, BATCH * POINTS, BATCH)
    M = BATCH * ROIS
    rows = torch.empty((M, NSAMPLE), dtype=torch.int32, device=dev)
    count, hits = torch.empty((M,), dtype=torch.int32, device=dev), torch.empty((M,), dtype=torch.int32, device=dev)

    # what the two forms compute, compared once
    nat, com = Fsp.points_in_boxes(pts, pid, fgt, gid, BATCH), composite_points_in_boxes(fgt.frames, GTS, pts)
    res["points_in_gt"] = {"points_in_a_box": int((nat >= 0).sum()), "equal_to_composite": bool(torch.equal(nat, com))}
    nat, com = Fsp.points_in_boxes(pts, pid, froi, rid, BATCH), composite_points_in_boxes(froi.frames, ROIS, pts)
    res["points_in_rois"] = {"points_in_a_box": int((nat >= 0).sum()), "equal_to_composite": bool(torch.equal(nat, com))}
    q = Fsp.box_query(froi, rid, pts, pid, BATCH, NSAMPLE, pad="cycle", groups=groups)
    crow, ccnt, _ = composite_box_query(froi.frames, ROIS, pts, NSAMPLE, True)
    h = q.hits.float()
    res["box_query_rois"] = {"hits_min_median_max": [int(h.min()), int(h.median()), int(h.max())],
                             "rows_equal_to_composite": bool(torch.equal(q.rows.long(), crow)),
                             "count_equal_to_composite": bool(torch.equal(q.count.long(), ccnt))}
    pn, _ = Fsp.roi_point_pool(pts, pid, feats, froi, rid, BATCH, NSAMPLE, groups=groups)
    pc, _ = composite_point_pool(froi.frames, pts, feats)
    res["roi_point_pool"] = {"equal_to_composite": bool(torch.equal(pn, pc))}
    an = Fsp.roi_aware_pool(pts, pid, feats, froi, rid, BATCH, GRID, MAX_PTS, groups=groups)
    ac = composite_aware_pool(froi.frames, pts, feats)
    res["roi_aware_pool"] = {"cells_in_use": int((an != 0).any(-1).sum()), "equal_to_composite": bool(torch.equal(an, ac))}

    g_point = torch.ones_like(pn)
    g_aware = torch.ones_like(an)

    def train(fn, g):
        f = feats.detach().requires_grad_(True)
        out = fn(f)
        (out[0] if isinstance(out, tuple) else out).backward(g)

    stages = {
        "points_in_gt": (lambda: Fsp.points_in_boxes(pts, pid, fgt, gid, BATCH),
                         lambda: composite_points_in_boxes(fgt.frames, GTS, pts)),
        "points_in_rois": (lambda: Fsp.points_in_boxes(pts, pid, froi, rid, BATCH),
                           lambda: composite_points_in_boxes(froi.frames, ROIS, pts)),
        "box_query_rois": (lambda: Fsp.box_query(roi, rid, pts, pid, BATCH, NSAMPLE, pad="cycle"),
                           lambda: composite_box_query(froi.frames, ROIS, pts, NSAMPLE, True)),
        "box_query_rois_launches_alone": (lambda: _roi.box_query_into(froi, rid, pts, groups, "cycle", rows, count, hits),
                                          lambda: composite_box_query(froi.frames, ROIS, pts, NSAMPLE, True)),
        "roi_point_pool_fwd": (lambda: Fsp.roi_point_pool(pts, pid, feats, roi, rid, BATCH, NSAMPLE),
                               lambda: composite_point_pool(froi.frames, pts, feats)),
        "roi_point_pool_fwd_bwd": (lambda: train(lambda f: Fsp.roi_point_pool(pts, pid, f, roi, rid, BATCH, NSAMPLE), g_point),
                                   lambda: train(lambda f: composite_point_pool(froi.frames, pts, f), g_point)),
        "roi_aware_pool_fwd": (lambda: Fsp.roi_aware_pool(pts, pid, feats, roi, rid, BATCH, GRID, MAX_PTS),
                               lambda: composite_aware_pool(froi.frames, pts, feats)),
        "roi_aware_pool_fwd_bwd": (lambda: train(lambda f: Fsp.roi_aware_pool(pts, pid, f, roi, rid, BATCH, GRID, MAX_PTS), g_aware),
                                   lambda: train(lambda f: composite_aware_pool(froi.frames, pts, f), g_aware)),
    }
    for rnd in range(2):                                        # alternate the forms: two rounds each
        for stage, (native, composite) in stages.items():
            res[f"native_{stage}_round{rnd}"] = timed(native, repeats)
            res[f"composite_{stage}_round{rnd}"] = timed(composite, max(2, repeats // 2), warmup=1)
    verdict = {}
    for stage in stages:
        nat = [res[f"native_{stage}_round{r}"]["median_us"] for r in range(2)]
        com = [res[f"composite_{stage}_round{r}"]["median_us"] for r in range(2)]
        verdict[stage] = {"native_us": nat, "composite_us": com, "native_no_slower": max(nat) <= min(com)}
    res["verdict"] = verdict
    res["slower_than_composite"] = sorted(k for k, v in verdict.items() if not v["native_no_slower"])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("roi_probe needs the GPU: nothing is measured without one")
    res = {"repeats": args.repeats}
    res.update(probe(torch.device("cuda:0"), args.repeats))
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
