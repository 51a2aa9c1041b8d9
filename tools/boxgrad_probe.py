#!/usr/bin/env python
"""What does the differentiable rotated IoU of csrc/boxgrad.hip cost?  The regression loss of a detector head over
4 096 and 65 536 aligned (prediction, target) pairs: the forward (two corners launches and the pair launch), the
backward (the pair launch with its gradient tables and two corners-backward launches) and both together, for the IoU
in space and for its DIoU form.  Beside each: what a user without the extension runs -- the torch composite of
tools/box_probe.py (the Sutherland-Hodgman clip vectorised over pairs: fixed eight slots, masks, gathers and scatters,
all differentiable) with autograd's backward.  The two forms alternate in one process; HIP events around one call each,
warm-up calls first, median and minimum of the repeats, two interleaved rounds.

    python tools/boxgrad_probe.py [--out profiles/boxgrad_probe.json] [--repeats 20]
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
from box_probe import _shoelace, composite_corners, head_output, timed  # noqa: E402
from spconv_amd.pytorch import functional as Fsp  # noqa: E402

SIZES = (4096, 65536)


def pairs(n, seed):
    """targets as a head's ground truth, predictions jittered in all seven numbers, every fourth moved 8 m away (the
    pairs only the penalty moves) -> fp32 [n, 7] each"""
    target, _ = head_output(n, seed)
    rng = np.random.default_rng(seed + 1)
    pred = target.astype(np.float64)
    pred[:, 0:2] += rng.random((n, 2)) * 2.0 - 1.0
    pred[:, 2] += rng.random(n) * 0.8 - 0.4
    pred[:, 3:6] *= 0.7 + rng.random((n, 3)) * 0.6
    pred[:, 6] += rng.random(n) * 0.8 - 0.4
    pred[2::4, 0] += 8.0
    return pred.astype(np.float32), target


def composite_overlap(A, B):
    """box_probe's vectorised clip with every step differentiable: the cut parameter of a slot that is no crossing
    divides by 1 (0 / 0 in a masked-out slot would put NaN into the backward pass of the whole pair).  A, B [P, 4, 2]
    counter-clockwise -> the shared area [P]"""
    P, dev = A.shape[0], A.device
    poly = torch.cat([A, torch.zeros((P, 4, 2), device=dev)], dim=1)
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
        t = (torch.where(crossing, d, torch.zeros_like(d)) / torch.where(crossing, d - dq, torch.ones_like(d)))[:, :, None]
        cut = poly + t * (q - poly)
        emitted = inside.long() + crossing.long()
        start = torch.cumsum(emitted, 1) - emitted
        new = torch.zeros((P, 17, 2), device=dev)                          # slot 16: what is not emitted
        at = torch.where(inside, start, torch.full_like(start, 16))
        new = new.scatter(1, at[:, :, None].expand(-1, -1, 2), poly)
        at = torch.where(crossing, start + inside.long(), torch.full_like(start, 16))
        new = new.scatter(1, at[:, :, None].expand(-1, -1, 2), cut)
        poly, cnt = new[:, :8], emitted.sum(1).clamp(max=8)
    return torch.where(cnt >= 3, _shoelace(poly, cnt), torch.zeros((), device=dev))


def composite_value(pred, target, diou):
    """the IoU in space of aligned pairs (and its DIoU form) from boxes, in differentiable torch ops -> [n]"""
    bev_a, z_a = composite_corners(pred)
    bev_b, z_b = composite_corners(target)
    four = torch.full((pred.shape[0],), 4, device=pred.device)
    inter = composite_overlap(bev_a, bev_b)
    h = (torch.minimum(z_a[:, 1], z_b[:, 1]) - torch.maximum(z_a[:, 0], z_b[:, 0])).clamp(min=0)
    inter3 = inter * h
    va, vb = _shoelace(bev_a, four) * (z_a[:, 1] - z_a[:, 0]), _shoelace(bev_b, four) * (z_b[:, 1] - z_b[:, 0])
    value = inter3 / (va + vb - inter3).clamp(min=1e-6)
    if diou:
        both = torch.cat([bev_a, bev_b], dim=1)
        w = both[:, :, 0].amax(1) - both[:, :, 0].amin(1)
        v = both[:, :, 1].amax(1) - both[:, :, 1].amin(1)
        d = torch.maximum(z_a[:, 1], z_b[:, 1]) - torch.minimum(z_a[:, 0], z_b[:, 0])
        rho2 = ((pred[:, :3] - target[:, :3]) ** 2).sum(1)
        value = value - rho2 / (w * w + v * v + d * d).clamp(min=1e-12)
    return value


def timed_backward(forward, g, repeats, warmup=2):
    """median / min of one backward in microseconds; its forward runs outside the events"""
    times = []
    for k in range(warmup + repeats):
        value = forward()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        value.backward(g)
        b.record()
        b.synchronize()
        if k >= warmup:
            times.append(1e3 * a.elapsed_time(b))
    return {"median_us": round(statistics.median(times), 1), "min_us": round(min(times), 1)}


def probe(dev, repeats):
    res, items = {}, {}
    for n in SIZES:
        pred_h, target_h = pairs(n, seed=n)
        g = torch.from_numpy(np.random.default_rng(n).random(n).astype(np.float32)).to(dev)
        for name, penalty in (("iou3d", "none"), ("diou3d", "diou")):
            def leaves():
                return (torch.from_numpy(pred_h).to(dev).requires_grad_(), torch.from_numpy(target_h).to(dev).requires_grad_())

            def native(p, t, penalty=penalty):
                return Fsp.boxes_iou3d_diff(p, t, penalty=penalty)

            def composite(p, t, diou=penalty == "diou"):
                return composite_value(p, t, diou)
            # the two forms agree before they are timed
            (p1, t1), (p2, t2) = leaves(), leaves()
            v1, v2 = native(p1, t1), composite(p2, t2)
            v1.backward(g), v2.backward(g)
            res[f"{name}_{n}"] = {
                "pairs": n, "overlapping_pairs": int((Fsp.boxes_iou3d_aligned(p1.detach(), t1.detach()) > 0).sum()),
                "max_abs_value_difference_to_composite": float((v1 - v2).abs().max()),
                "max_abs_gradient_difference_to_composite": float(max((p1.grad - p2.grad).abs().max(),
                                                                      (t1.grad - t2.grad).abs().max())),
                "largest_gradient_component": float(max(p1.grad.abs().max(), t1.grad.abs().max()))}
            for form, fn in (("native", native), ("composite", composite)):
                p, t = leaves()

                def fwd(fn=fn, p=p, t=t):
                    return fn(p, t)

                def both(fn=fn, p=p, t=t, g=g):
                    p.grad = t.grad = None
                    fn(p, t).backward(g)
                items[(form, f"forward_{name}_{n}")] = ("call", fwd)
                items[(form, f"backward_{name}_{n}")] = ("backward", fwd)
                items[(form, f"forward_backward_{name}_{n}")] = ("call", both)
    stages = sorted({stage for _, stage in items}, key=lambda s: (int(s.rsplit("_", 1)[1]), s))
    for rnd in range(2):                                        # alternate the forms: two rounds each
        for stage in stages:
            for form in ("native", "composite"):
                kind, fn = items[(form, stage)]
                n = int(stage.rsplit("_", 1)[1])
                g = torch.from_numpy(np.random.default_rng(n).random(n).astype(np.float32)).to(dev)
                reps = repeats if form == "native" else max(4, repeats // 2)
                res[f"{form}_{stage}_round{rnd}"] = timed(fn, reps) if kind == "call" else timed_backward(fn, g, reps)
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
        raise SystemExit("boxgrad_probe needs the GPU: nothing is measured without one")
    res = {"repeats": args.repeats}
    res.update(probe(torch.device("cuda:0"), args.repeats))
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
