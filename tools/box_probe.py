#!/usr/bin/env python
"""What do the rotated-box kernels of csrc/box.hip cost?  Five cases of a detector's post-processing and target
assignment: (a) the corners of 16 384 boxes; (b) boxes_iou3d of 512 x 128 (targets of one scene) and (c) of 4096 x 4096;
(d) NMS of 4 scenes x 4096 candidates to 512 at 0.7, split into its key, sort, mask and reduce launches (the prefixes
of the pipeline timed through the SPX_TEST_NMS_STAGES switch and differenced); (e) NMS of 4 x 1024 to 100.  Beside each:
what a user without the extension runs -- a torch composite with the Sutherland-Hodgman clip vectorised over pairs
(fixed eight slots, masks and scatters, in chunks of rows), and for NMS the IoU matrix of each scene's sorted
candidates thresholded on the device, the mask copied to the host and the greedy loop there.  The two forms alternate
in one process; HIP events around one call each (wall clock for the composite NMS, which synchronises), warm-up calls
first, median and minimum of the repeats, two interleaved rounds.

    python tools/box_probe.py [--out profiles/box_probe.json] [--repeats 20]
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
from spconv_amd import _lib  # noqa: E402
from spconv_amd.pytorch import functional as Fsp  # noqa: E402

BATCH, THRESH = 4, 0.7
KEYS = ("box/corners", "box/pairs", "box/aligned", "box/key", "box/mask", "box/reduce", "serialize/sort")


def head_output(n, seed, objects=None):
    """n boxes as a head emits them: `objects` cars in a 70.4 x 80 m field, n / objects jittered proposals around each
    -> boxes fp32 [n, 7], scores fp32 [n]"""
    rng = np.random.default_rng(seed)
    objects = objects or max(1, n // 20)
    c = np.zeros((objects, 7))
    c[:, 0], c[:, 1], c[:, 2] = rng.random(objects) * 70.4, rng.random(objects) * 80.0 - 40.0, rng.random(objects) * 2 - 1
    c[:, 3], c[:, 4], c[:, 5] = 3.5 + rng.random(objects) * 1.5, 1.5 + rng.random(objects) * 0.5, 1.4 + rng.random(objects) * 0.4
    c[:, 6] = rng.random(objects) * 6.28 - 3.14
    b = c[rng.integers(0, objects, n)]
    b[:, :2] += (rng.random((n, 2)) - 0.5) * 1.2
    b[:, 3:6] *= 1.0 + (rng.random((n, 3)) - 0.5) * 0.2
    b[:, 6] += (rng.random(n) - 0.5) * 0.3
    return b.astype(np.float32), rng.random(n).astype(np.float32)


def timed(fn, repeats, warmup=2, wall=False):
    """median / min of one call in microseconds: HIP events, or the wall clock for a call that synchronises"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        if wall:
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times.append(1e6 * (time.perf_counter() - t0))
        else:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            times.append(1e3 * a.elapsed_time(b))
    return {"median_us": round(statistics.median(times), 1), "min_us": round(min(times), 1)}


# ------------------------------------------------------------------------------------------- the torch composite
def composite_corners(boxes):
    c, s = torch.cos(boxes[:, 6:7]), torch.sin(boxes[:, 6:7])
    sx = torch.tensor([1.0, -1.0, -1.0, 1.0], device=boxes.device)
    sy = torch.tensor([1.0, 1.0, -1.0, -1.0], device=boxes.device)
    lx, ly = sx * boxes[:, 3:4] * 0.5, sy * boxes[:, 4:5] * 0.5
    bev = torch.stack([boxes[:, 0:1] + (lx * c - ly * s), boxes[:, 1:2] + (lx * s + ly * c)], dim=2)
    return bev, torch.stack([boxes[:, 2] - boxes[:, 5] * 0.5, boxes[:, 2] + boxes[:, 5] * 0.5], dim=1)


def _shoelace(poly, cnt):
    idx = torch.arange(poly.shape[1], device=poly.device)
    nxt = torch.where(idx[None] + 1 < cnt[:, None], idx[None] + 1, torch.zeros_like(idx)[None])
    q = torch.gather(poly, 1, nxt[:, :, None].expand(-1, -1, 2))
    cross = poly[:, :, 0] * q[:, :, 1] - q[:, :, 0] * poly[:, :, 1]
    return (cross * (idx[None] < cnt[:, None])).sum(1).abs() * 0.5


def composite_overlap(A, B):
    """A, B [P, 4, 2] (counter-clockwise) -> the area each pair shares [P]: Sutherland-Hodgman over all pairs at once"""
    P, dev = A.shape[0], A.device
    poly = torch.zeros((P, 8, 2), device=dev)
    poly[:, :4] = A
    cnt = torch.full((P,), 4, device=dev, dtype=torch.long)
    idx = torch.arange(8, device=dev)[None]
    for e in range(4):
        a, b = B[:, e], B[:, (e + 1) % 4]
        ex, ey = (b[:, 0] - a[:, 0])[:, None], (b[:, 1] - a[:, 1])[:, None]
        d = ex * (poly[:, :, 1] - a[:, 1:2]) - ey * (poly[:, :, 0] - a[:, 0:1])
        nxt = torch.where(idx + 1 < cnt[:, None], idx + 1, torch.zeros_like(idx))
        q, dq = torch.gather(poly, 1, nxt[:, :, None].expand(-1, -1, 2)), torch.gather(d, 1, nxt)
        live = idx < cnt[:, None]
        inside = (d >= 0) & live
        crossing = ((d >= 0) != (dq >= 0)) & live
        t = (d / (d - dq))[:, :, None]
        cut = poly + t * (q - poly)
        emitted = inside.long() + crossing.long()
        start = torch.cumsum(emitted, 1) - emitted
        new = torch.zeros((P, 17, 2), device=dev)                          # slot 16: what is not emitted
        at = torch.where(inside, start, torch.full_like(start, 16))
        new.scatter_(1, at[:, :, None].expand(-1, -1, 2), poly)
        at = torch.where(crossing, start + inside.long(), torch.full_like(start, 16))
        new.scatter_(1, at[:, :, None].expand(-1, -1, 2), cut)
        poly, cnt = new[:, :8], emitted.sum(1).clamp(max=8)
    return torch.where(cnt >= 3, _shoelace(poly, cnt), torch.zeros((), device=dev))


def composite_iou(bev_a, z_a, bev_b, z_b, space, chunk=256):
    """[M, N] IoU in the plane or in space, `chunk` rows of pairs at a time"""
    area_a, area_b = _shoelace(bev_a, torch.full((bev_a.shape[0],), 4, device=bev_a.device)), \
        _shoelace(bev_b, torch.full((bev_b.shape[0],), 4, device=bev_b.device))
    N, out = bev_b.shape[0], []
    for r0 in range(0, bev_a.shape[0], chunk):
        a = bev_a[r0:r0 + chunk]
        m = a.shape[0]
        inter = composite_overlap(a[:, None].expand(-1, N, -1, -1).reshape(-1, 4, 2),
                                  bev_b[None].expand(m, -1, -1, -1).reshape(-1, 4, 2)).view(m, N)
        aa, ab = area_a[r0:r0 + chunk, None], area_b[None]
        if space:
            za = z_a[r0:r0 + chunk]
            h = (torch.minimum(za[:, None, 1], z_b[None, :, 1]) - torch.maximum(za[:, None, 0], z_b[None, :, 0])).clamp(min=0)
            inter = inter * h
            aa, ab = aa * (za[:, 1] - za[:, 0])[:, None], ab * (z_b[:, 1] - z_b[:, 0])[None]
        out.append(inter / (aa + ab - inter).clamp(min=1e-8))
    return torch.cat(out)


def composite_nms(boxes, scores, bid, pre_max, post_max):
    """per scene: sort, the IoU matrix of the first pre_max, its threshold mask to the host, the greedy loop there"""
    keep = []
    for b in range(BATCH):
        sel = torch.nonzero(bid == b)[:, 0]
        order = sel[torch.argsort(scores[sel], descending=True, stable=True)][:pre_max]
        bev, _ = composite_corners(boxes[order])
        mask = (composite_iou(bev, None, bev, None, False) > THRESH).cpu().numpy()
        gone = np.zeros(len(order), bool)
        kept = []
        for i in range(len(order)):
            if not gone[i]:
                kept.append(i)
                if len(kept) == post_max:
                    break
                gone[i + 1:] |= mask[i, i + 1:]
        keep.append(order[torch.as_tensor(kept, device=order.device, dtype=torch.long)])
    return keep


# ------------------------------------------------------------------------------------------- the cases
def nms_case(dev, per_scene, post_max, repeats, res, name):
    L = _lib.load()
    n = BATCH * per_scene
    boxes_h, score_h = head_output(n, seed=per_scene)
    boxes, scores = torch.from_numpy(boxes_h).to(dev), torch.from_numpy(score_h).to(dev)
    bid = torch.arange(BATCH, dtype=torch.int32, device=dev).repeat_interleave(per_scene)
    corners = Fsp.boxes_to_corners(boxes)
    keep = torch.empty((BATCH, post_max), dtype=torch.int32, device=dev)
    count = torch.empty((BATCH,), dtype=torch.int32, device=dev)
    ws = torch.empty((Fsp.nms_ws_bytes(n, BATCH, per_scene),), dtype=torch.uint8, device=dev)

    def native():
        Fsp.nms_rotated_into(corners, scores, THRESH, keep, count, ws, batch_ids=bid, batch_size=BATCH, pre_max=per_scene)
    before = _lib.launch_counts(KEYS)
    native()
    res[f"launches_of_{name}"] = {k: v - before[k] for k, v in _lib.launch_counts(KEYS).items()}
    torch.cuda.synchronize()
    ref = composite_nms(boxes, scores, bid, per_scene, post_max)
    same = sum(int(count[b]) == len(ref[b]) and torch.equal(keep[b, :len(ref[b])].long(), ref[b]) for b in range(BATCH))
    res[name] = {"candidates_per_scene": per_scene, "post_max": post_max, "kept": count.cpu().tolist(),
                 "scenes_equal_to_composite": same}
    prefix = {}
    for rnd in range(2):
        for stages in (1, 2, 3, 4):
            L.spx_set_option(b"SPX_TEST_NMS_STAGES", stages)
            prefix[(stages, rnd)] = timed(native, repeats)
        L.spx_set_option(b"SPX_TEST_NMS_STAGES", 4)
        res[f"native_{name}_round{rnd}"] = prefix[(4, rnd)]
        res[f"composite_{name}_round{rnd}"] = timed(lambda: composite_nms(boxes, scores, bid, per_scene, post_max),
                                                    max(2, repeats // 10), warmup=1, wall=True)
    split = {}
    for k, stage in enumerate(("key", "sort", "mask", "reduce"), start=1):
        split[stage + "_us"] = [round(prefix[(k, r)]["median_us"] - (prefix[(k - 1, r)]["median_us"] if k > 1 else 0.0), 1)
                                for r in range(2)]
    res[name]["split_of_prefix_medians"] = split
    return name


def probe(dev, repeats):
    res = {"batch": BATCH, "thresh": THRESH, "max_pre": _lib.load().spx_nms_max_pre()}
    stages = {}
    boxes_h, _ = head_output(16384, seed=1)
    boxes = torch.from_numpy(boxes_h).to(dev)
    stages["corners_16384"] = (lambda: Fsp.boxes_to_corners(boxes), lambda: composite_corners(boxes), 1)
    ca, cb = Fsp.boxes_to_corners(boxes[:512]), Fsp.boxes_to_corners(boxes[512:640])
    big = Fsp.boxes_to_corners(boxes[:4096])
    nat, com = Fsp.boxes_iou3d(ca, cb), composite_iou(ca.bev, ca.zrange, cb.bev, cb.zrange, True)
    res["iou3d_512x128"] = {"overlapping_pairs": int((nat > 0).sum()),
                            "max_abs_difference_to_composite": float((nat - com).abs().max())}
    stages["iou3d_512x128"] = (lambda: Fsp.boxes_iou3d(ca, cb),
                               lambda: composite_iou(ca.bev, ca.zrange, cb.bev, cb.zrange, True), 1)
    res["iou3d_4096x4096"] = {"overlapping_pairs": int((Fsp.boxes_iou3d(big, big) > 0).sum())}
    stages["iou3d_4096x4096"] = (lambda: Fsp.boxes_iou3d(big, big),
                                 lambda: composite_iou(big.bev, big.zrange, big.bev, big.zrange, True), 10)
    with torch.no_grad():
        for rnd in range(2):                                    # alternate the forms: two rounds each
            for stage, (native, composite, thin) in stages.items():
                res[f"native_{stage}_round{rnd}"] = timed(native, repeats)
                res[f"composite_{stage}_round{rnd}"] = timed(composite, max(2, repeats // thin), warmup=1)
        names = list(stages) + [nms_case(dev, 4096, 512, repeats, res, "nms_4x4096_to_512"),
                                nms_case(dev, 1024, 100, repeats, res, "nms_4x1024_to_100")]
    verdict = {}
    for stage in names:
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
        raise SystemExit("box_probe needs the GPU: nothing is measured without one")
    res = {"repeats": args.repeats}
    res.update(probe(torch.device("cuda:0"), args.repeats))
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
