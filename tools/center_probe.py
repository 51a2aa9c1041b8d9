#!/usr/bin/env python
"""What do the centre-head targets cost next to the Python loop they replace?  4 scenes x 128 ground-truth boxes (car,
pedestrian and cyclist sizes) on a 468 x 468 map of 0.32 m cells, 3 classes, max_objs 500 -- Waymo's pillar head -- and
the sparse form over 4 x 30 000 rows of that map.  Timed, each against a torch composite that restates OpenPCDet's
assign_target_of_single_head from the rules of include/spconv_amd.h: the records (the composite computes centres and
radii vectorised, as OpenPCDet does), the dense heatmap (the composite walks the boxes one by one, reads centre and radius
back, slices a window out of the map and torch.max-es a fresh Gaussian into it), the nearest rows and the sparse heat
(the composite computes the distance from every row of the scene to one box per iteration), and both chains as a user
calls them.  One process; HIP events around one call each, warm-up calls first, median and minimum of the repeats, two
interleaved rounds; the composites take hundreds of launches and read-backs per call and get fewer repeats (recorded).
Beside the times, the largest difference between the native and the composite results.

    python tools/center_probe.py [--out profiles/center_probe.json] [--repeats 30] [--composite-repeats 3]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from spconv_amd.pytorch import functional as Fsp  # noqa: E402
from sample_probe import no_grad, timed  # noqa: E402

BATCH, BOXES, CLASSES, MAX_OBJS = 4, 128, 3, 500
GRID, VOXEL, RANGE_MIN, STRIDE = (468, 468), (0.32, 0.32), (-74.88, -74.88), 1
ROWS = 30_000
SIZES = np.array([[4.7, 2.1, 1.7], [0.9, 0.85, 1.75], [1.8, 0.8, 1.7]])      # car, pedestrian, cyclist
PARAMS = dict(grid_size=GRID, voxel_size=VOXEL, range_min=RANGE_MIN, stride=STRIDE, num_classes=CLASSES, max_objs=MAX_OBJS)


def scene(seed):
    """boxes fp32 [BATCH * BOXES, 7], batch ids int32, class ids int64; indices int32 [BATCH * ROWS, 3] = (b, y, x)"""
    rng = np.random.default_rng(seed)
    m = BATCH * BOXES
    cls = rng.integers(0, CLASSES, m)
    extent = np.array(GRID) * np.array(VOXEL)
    boxes = np.concatenate([np.array(RANGE_MIN) + rng.random((m, 2)) * extent, rng.random((m, 1)) * 2.0 - 1.0,
                            SIZES[cls] * (0.8 + 0.4 * rng.random((m, 3))), rng.random((m, 1)) * 2.0 * np.pi - np.pi], axis=1)
    idx = np.concatenate([np.stack([np.full(ROWS, b), *np.unravel_index(
        rng.choice(GRID[0] * GRID[1], ROWS, replace=False), (GRID[1], GRID[0]))], 1) for b in range(BATCH)])
    return (boxes.astype(np.float32), np.repeat(np.arange(BATCH, dtype=np.int32), BOXES), cls.astype(np.int64),
            idx.astype(np.int32))


def gaussian_radius(h, w, ov=0.1):
    b1, c1 = h + w, w * h * (1 - ov) / (1 + ov)
    r1 = (b1 + torch.sqrt(b1 * b1 - 4 * c1)) / 2
    b2, c2 = 2 * (h + w), (1 - ov) * w * h
    r2 = (b2 + torch.sqrt(b2 * b2 - 16 * c2)) / 2
    a3, b3, c3 = 4 * ov, -2 * ov * (h + w), (ov - 1) * w * h
    r3 = (b3 + torch.sqrt(b3 * b3 - 4 * a3 * c3)) / 2
    return torch.min(torch.min(r1, r2), r3)


def composite_records(boxes):
    """centres, cells and radii of all boxes, vectorised (OpenPCDet computes them per scene before its loop)"""
    cx = ((boxes[:, 0] - RANGE_MIN[0]) / VOXEL[0] / STRIDE).clamp(0, GRID[0] - 0.5)
    cy = ((boxes[:, 1] - RANGE_MIN[1]) / VOXEL[1] / STRIDE).clamp(0, GRID[1] - 0.5)
    center = torch.stack([cx, cy], 1)
    radius = gaussian_radius(boxes[:, 4] / VOXEL[1] / STRIDE, boxes[:, 3] / VOXEL[0] / STRIDE).int().clamp(min=2)
    return center, center.int(), radius


def composite_dense(boxes, cls):
    """the loop of assign_target_of_single_head: per scene, per box, two read-backs, a window and a maximum"""
    center, cell, radius = composite_records(boxes)
    heat = boxes.new_zeros((BATCH, CLASSES, GRID[1], GRID[0]))
    for b in range(BATCH):
        for k in range(b * BOXES, (b + 1) * BOXES):
            r = int(radius[k].item())
            x, y = int(cell[k, 0].item()), int(cell[k, 1].item())
            d = torch.arange(-r, r + 1, device=boxes.device, dtype=torch.float32)
            sigma = (2 * r + 1) / 6
            g = torch.exp(-(d[None, :] ** 2 + d[:, None] ** 2) / (2 * sigma * sigma))
            left, right, top, bottom = min(x, r), min(GRID[0] - x, r + 1), min(y, r), min(GRID[1] - y, r + 1)
            win = heat[b, int(cls[k].item()), y - top:y + bottom, x - left:x + right]
            torch.max(win, g[r - top:r + bottom, r - left:r + right], out=win)
    return heat


def composite_sparse(boxes, cls, indices):
    """VoxelNeXt's loop: per scene, per box, the distance from every row of the scene, its argmin, a maximum"""
    center, _, radius = composite_records(boxes)
    heat = boxes.new_zeros((indices.shape[0], CLASSES))
    nearest = torch.full((boxes.shape[0],), -1, dtype=torch.long, device=boxes.device)
    for b in range(BATCH):
        rows = torch.nonzero(indices[:, 0] == b)[:, 0]
        xy = indices[rows][:, [2, 1]].float()
        for k in range(b * BOXES, (b + 1) * BOXES):
            dist = ((xy - center[k]) ** 2).sum(1)
            nearest[k] = rows[dist.argmin()]
            sigma = (2 * int(radius[k].item()) + 1) / 6
            c = int(cls[k].item())
            heat[rows, c] = torch.max(heat[rows, c], torch.exp(-dist / (2 * sigma * sigma)))
    return heat, nearest


def probe(dev, repeats, composite_repeats):
    boxes_h, bid_h, cls_h, idx_h = scene(seed=11)
    boxes, bid, cls, idx = (torch.from_numpy(a).to(dev) for a in (boxes_h, bid_h, cls_h, idx_h))
    res = {"batch": BATCH, "boxes_per_scene": BOXES, "classes": CLASSES, "grid": GRID, "voxel": VOXEL, "max_objs": MAX_OBJS,
           "rows_per_scene": ROWS, "tile": Fsp.center_tile()}
    centers = Fsp.box_centers(boxes, bid, cls, BATCH, **PARAMS)
    dense = Fsp.center_heatmap(centers)
    sparse = Fsp.center_heatmap_sparse(centers, idx)
    c_center, c_cell, c_radius = composite_records(boxes)
    c_dense = composite_dense(boxes, cls)
    c_sparse, c_nearest = composite_sparse(boxes, cls, idx)
    res["radius"] = {"min": int(centers.radius.min()), "max": int(centers.radius.max())}
    res["native_against_composite"] = {
        "cells_equal": int((centers.cell == c_cell).all(1).sum()), "radii_equal": int((centers.radius == c_radius).sum()),
        "boxes": int(boxes.shape[0]), "dense_max_abs_diff": float((dense - c_dense).abs().max()),
        "dense_cells_above_zero": [int((dense > 0).sum()), int((c_dense > 0).sum())],
        "nearest_equal": int((sparse.nearest.long() == c_nearest).sum()),
        "sparse_max_abs_diff": float((sparse.heat - c_sparse).abs().max())}
    heat_buf, sparse_buf = torch.empty_like(dense), torch.empty_like(sparse.heat)
    rows = Fsp.scene_groups(idx[:, 0].contiguous(), int(idx.shape[0]), BATCH)
    nearest, inds, mask = torch.empty_like(sparse.nearest), torch.empty_like(sparse.inds), torch.empty_like(sparse.mask)
    stages = {
        "records": (no_grad(lambda: Fsp.box_centers(boxes, bid, cls, BATCH, **PARAMS)), no_grad(lambda: composite_records(boxes))),
        "dense_heatmap": (lambda: Fsp.center_heatmap_into(centers, heat_buf), no_grad(lambda: composite_dense(boxes, cls))),
        "nearest_rows": (lambda: Fsp.center_nearest_into(centers, idx, rows, None, nearest, inds, mask), None),
        "sparse_heat": (lambda: Fsp.center_heatmap_sparse_into(centers, idx, None, None, "center", "none", sparse_buf), None),
        "sparse_heat_nearest_window": (lambda: Fsp.center_heatmap_sparse_into(centers, idx, None, nearest, "nearest", "window",
                                                                             sparse_buf), None),
        "dense_chain": (no_grad(lambda: Fsp.center_heatmap(Fsp.box_centers(boxes, bid, cls, BATCH, **PARAMS))),
                        no_grad(lambda: composite_dense(boxes, cls))),
        "sparse_chain": (no_grad(lambda: Fsp.center_heatmap_sparse(Fsp.box_centers(boxes, bid, cls, BATCH, **PARAMS), idx)),
                         no_grad(lambda: composite_sparse(boxes, cls, idx))),
    }
    for rnd in range(2):                                        # alternate the forms: two rounds each
        for stage, (nat, composite) in stages.items():
            res[f"native_{stage}_round{rnd}"] = timed(nat, repeats)
            if composite is not None:
                res[f"composite_{stage}_round{rnd}"] = timed(composite, composite_repeats, warmup=1)
    verdict = {}
    for stage, (_, composite) in stages.items():
        nat = [res[f"native_{stage}_round{r}"]["median_us"] for r in range(2)]
        verdict[stage] = {"native_us": nat}
        if composite is not None:
            com = [res[f"composite_{stage}_round{r}"]["median_us"] for r in range(2)]
            verdict[stage].update({"composite_us": com, "composite_over_native": round(min(com) / max(nat), 1),
                                   "native_no_slower": max(nat) <= min(com)})
    res["verdict"] = verdict
    res["slower_than_composite"] = sorted(k for k, v in verdict.items() if v.get("native_no_slower") is False)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--composite-repeats", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("center_probe needs the GPU: nothing is measured without one")
    res = {"repeats": args.repeats, "composite_repeats": args.composite_repeats}
    res.update(probe(torch.device("cuda:0"), args.repeats, args.composite_repeats))
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
