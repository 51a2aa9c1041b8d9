#!/usr/bin/env python
"""What does sectorised keypoint sampling cost, and what does it buy?  The clouds of tools/sample_probe.py (4 scenes x
16 384 points -> 2048 samples, 4 x 75 000 points -> 4096 samples), cut into S = 6 azimuth sectors about the centre of the
cloud, with and without 4 x 128 RoIs at radius 1.6.  Timed: sector_ids, the groups of the segment ids, the quota launch,
the segmented sampling, and the whole sector_fps -- against whole-scene farthest_point_sample on the same cloud and K
(spx_fps, the kernel this form exists to beat) and against a torch composite of OpenPCDet's
sectorized_proposal_centric_sampling: its per-sector Python loop (a count read back per sector) around the batched-loop
FPS of sample_probe.py.  One process; HIP events around one call each, warm-up calls first, median and minimum of the
repeats, two interleaved rounds; the composite takes thousands of launches per call and gets fewer repeats (recorded).
Beside the times one coverage figure: the largest distance from a point to its nearest keypoint, per method, on the
75 000-point cloud -- sector sampling is a different sample set from global FPS.

    python tools/sector_probe.py [--out profiles/sector_probe.json] [--repeats 30] [--composite-repeats 2]
"""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from spconv_amd import _lib  # noqa: E402
from spconv_amd.pytorch import _pointvoxel, _sample  # noqa: E402
from spconv_amd.pytorch import functional as Fsp  # noqa: E402
from sample_probe import BATCH, EXTENT, FPS_CASES, cloud, composite_fps, no_grad, timed  # noqa: E402

SECTORS, ROIS, ROI_RADIUS = 6, 128, 1.6
CENTER = (float(EXTENT[0]) / 2.0, float(EXTENT[1]) / 2.0)
KEYS = ("sample/fps", "pointvoxel/groups")              # (the sector launches themselves are uncounted)


def rois(seed):
    """BATCH x ROIS car-sized boxes over the cloud -> fp32 [BATCH * ROIS, 7], int32 [BATCH * ROIS]"""
    rng = np.random.default_rng(seed)
    m = BATCH * ROIS
    boxes = np.concatenate([rng.random((m, 3)) * EXTENT * np.array([1.0, 1.0, 0.25]),
                            np.array([3.9, 1.6, 1.56]) * (0.8 + 0.4 * rng.random((m, 3))),
                            rng.random((m, 1)) * 2.0 * np.pi - np.pi], axis=1)
    return boxes.astype(np.float32), np.repeat(np.arange(BATCH, dtype=np.int32), ROIS)


def composite_sector_fps(pts, n, K, boxes):
    """OpenPCDet's loop over scenes and sectors in torch: the filter by the nearest RoI centre, atan2 sectors, a count
    read back per sector, ceil(n_k / n * K) in Python floats, the batched-loop FPS per sector.  -> per scene the chosen
    point indices (in the whole cloud), sector by sector"""
    out = []
    for b in range(BATCH):
        xyz = pts[b * n:(b + 1) * n, :3]
        index = torch.arange(b * n, (b + 1) * n, device=pts.device)
        if boxes is not None:
            bx = boxes[b * ROIS:(b + 1) * ROIS]
            d = torch.cdist(xyz, bx[:, :3])
            dmin, near = d.min(dim=1)
            keep = dmin < (bx[near, 3:6] / 2).norm(dim=1) + ROI_RADIUS
            xyz, index = xyz[keep], index[keep]
        angle = torch.atan2(xyz[:, 1] - CENTER[1], xyz[:, 0] - CENTER[0]) + math.pi
        sector = torch.floor(angle / (2 * math.pi / SECTORS)).clamp(0, SECTORS - 1)
        total, chosen = xyz.shape[0], []
        for k in range(SECTORS):
            mask = sector == k
            nk = int(mask.sum().item())                                 # (the read-back of the loop)
            if nk == 0:
                continue
            quota = min(nk, math.ceil(nk / total * K))
            chosen.append(index[mask][composite_fps(xyz[mask].unsqueeze(0), quota)[0]])
        out.append(torch.cat(chosen) if chosen else index[:0])
    return out


def coverage(pts, n, picks):
    """per scene the largest distance from a point to its nearest keypoint (picks: per scene the chosen point indices)"""
    worst = []
    for b in range(BATCH):
        xyz, keys = pts[b * n:(b + 1) * n, :3], pts[picks[b].long(), :3]
        far = 0.0
        for c0 in range(0, n, 8192):
            far = max(far, float(torch.cdist(xyz[c0:c0 + 8192], keys).min(dim=1).values.max()))
        worst.append(round(far, 3))
    return worst


def probe(dev, repeats, composite_repeats):
    R = _sample.resident_points()
    res = {"batch": BATCH, "sectors": SECTORS, "center": CENTER, "rois_per_scene": ROIS, "roi_radius": ROI_RADIUS,
           "resident_points": R}
    stages = {}
    boxes_h, box_ids_h = rois(seed=5)
    boxes, box_ids = torch.from_numpy(boxes_h).to(dev), torch.from_numpy(box_ids_h).to(dev)
    for name, n, K in FPS_CASES:
        pts_h, bid_h = cloud(n, seed=n)
        pts, bid = torch.from_numpy(pts_h).to(dev), torch.from_numpy(bid_h).to(dev)
        N = BATCH * n
        scene = Fsp.scene_groups(bid, N, BATCH)
        whole = Fsp.farthest_point_sample(pts, bid, BATCH, K, groups=scene)
        stages[f"whole_scene_fps_{name}"] = (
            no_grad(lambda p=pts, b=bid, k=K, g=scene: Fsp.farthest_point_sample(p, b, BATCH, k, groups=g)), None)
        for tag, kw, bx in (("plain", {}, None),
                            ("rois", dict(rois=boxes, roi_batch_ids=box_ids, roi_radius=ROI_RADIUS), boxes)):
            case = f"{name}_{tag}"
            before = _lib.launch_counts(KEYS)
            s, seg, quota = Fsp.sector_fps(pts, bid, BATCH, K, SECTORS, center=CENTER, return_sectors=True, **kw)
            launched = {k: v - before[k] for k, v in _lib.launch_counts(KEYS).items()}
            sizes = torch.bincount(seg[seg >= 0].long(), minlength=BATCH * SECTORS)
            comp = composite_sector_fps(pts, n, K, bx)
            same = sum(int((c == s.idx[b, :len(c)].long()).sum()) if len(c) == int(s.count[b]) else 0
                       for b, c in enumerate(comp))
            res[f"sector_fps_{case}"] = {
                "points_per_scene": n, "samples": K, "launches": launched, "kept_points": int(sizes.sum()),
                "segment_sizes": sizes.tolist(), "largest_segment": int(sizes.max()),
                "largest_segment_tier": "register" if int(sizes.max()) <= R else "streamed",
                "count": s.count.tolist(), "largest_quota": int(quota.max()),
                "composite_counts": [len(c) for c in comp], "slots_equal_to_composite": same, "slots": int(s.count.sum())}
            if name == "streamed_tier" and tag == "plain":
                res["coverage_largest_point_to_keypoint_distance_m"] = {
                    "whole_scene_fps": coverage(pts, n, [whole.idx[b] for b in range(BATCH)]),
                    "sector_fps": coverage(pts, n, [s.idx[b, :int(s.count[b])] for b in range(BATCH)]),
                    "sector_fps_composite": coverage(pts, n, comp)}
            buf = _sample.sector_buffers(N, BATCH, K, SECTORS, 3, dev)
            rg = None if bx is None else Fsp.scene_groups(box_ids, len(boxes), BATCH)
            groups = Fsp.PointGroups(buf.rows, buf.offsets, buf.list, BATCH * SECTORS)
            _sample.sector_fps_into(pts, bid, None, BATCH, K, SECTORS, CENTER, bx, rg, ROI_RADIUS if bx is not None else None,
                                    3, buf)
            assert torch.equal(buf.idx, s.idx)
            stages[f"sector_ids_{case}"] = (lambda p=pts, b=bid, x=bx, g=rg, f=buf: _sample.sector_ids_into(
                p, b, None, 3, BATCH, SECTORS, CENTER, x, g, ROI_RADIUS if x is not None else None, f.seg), None)
            stages[f"segment_groups_{case}"] = (lambda f=buf: _pointvoxel.point_groups_into(
                f.seg, BATCH * SECTORS, None, f.rows, f.offsets, f.list, f.groups_ws), None)
            stages[f"fps_quota_{case}"] = (lambda f=buf, g=groups, k=K: _sample.fps_quota_into(
                g, BATCH, SECTORS, k, f.quota, f.slot, f.count), None)
            stages[f"fps_segments_{case}"] = (lambda p=pts, f=buf, g=groups, k=K: _sample.fps_segments_into(
                p, g, f.quota, f.slot, SECTORS, k + SECTORS - 1, k, 3, f.idx, f.seg_count, f.ws), None)
            stages[f"sector_fps_{case}"] = (
                no_grad(lambda p=pts, b=bid, k=K, w=kw: Fsp.sector_fps(p, b, BATCH, k, SECTORS, center=CENTER, **w)),
                no_grad(lambda p=pts, m=n, k=K, x=bx: composite_sector_fps(p, m, k, x)))
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
    for name, _, _ in FPS_CASES:
        whole = verdict[f"whole_scene_fps_{name}"]["native_us"]
        for tag in ("plain", "rois"):
            v = verdict[f"sector_fps_{name}_{tag}"]
            v["whole_scene_fps_over_sector_fps"] = round(min(whole) / max(v["native_us"]), 1)
            v["no_slower_than_whole_scene_fps"] = max(v["native_us"]) <= min(whole)
            steps = res[f"sector_fps_{name}_{tag}"]["largest_quota"]
            v["fps_segments_us_per_step_of_the_largest_quota"] = [
                round(t / max(steps, 1), 3) for t in verdict[f"fps_segments_{name}_{tag}"]["native_us"]]
    res["verdict"] = verdict
    res["slower_than_composite"] = sorted(k for k, v in verdict.items() if v.get("native_no_slower") is False)
    res["slower_than_whole_scene_fps"] = sorted(k for k, v in verdict.items()
                                                if v.get("no_slower_than_whole_scene_fps") is False)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--composite-repeats", type=int, default=2)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sector_probe needs the GPU: nothing is measured without one")
    res = {"repeats": args.repeats, "composite_repeats": args.composite_repeats}
    res.update(probe(torch.device("cuda:0"), args.repeats, args.composite_repeats))
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
