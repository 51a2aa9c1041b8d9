#!/usr/bin/env python
"""What do farthest-point sampling and the ball query over raw points cost?  The keypoint stage of a PV-RCNN-style head:
4 scenes x 16 384 points -> 2048 samples (the register tier of spx_fps), 4 x 75 000 points -> 4096 samples (the streamed
tier), and the ball query of 4 x 2048 keypoints over the 4 x 75 000 points at radius 0.8, nsample 16 and 32, with the
gather of C = 64 f16 point features behind it.  Timed on the kernels of csrc/sample.hip, each against the torch composite
a user would otherwise write: FPS as the batched loop of K steps (subtract, square-sum, minimum, argmax, gather), the
ball query as a chunked distance matrix per scene, a mask scored by point index, topk and index_select.  The two forms
alternate in one process; HIP events around one call each, warm-up calls first, median and minimum of the repeats, two
interleaved rounds.  The composite's FPS takes thousands of launches per call and gets fewer repeats (--fps-composite-
repeats, recorded in the output).

    python tools/sample_probe.py [--out profiles/sample_probe.json] [--repeats 30] [--fps-composite-repeats 3]
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
from spconv_amd import _lib  # noqa: E402
from spconv_amd.pytorch import _sample  # noqa: E402
from spconv_amd.pytorch import functional as Fsp  # noqa: E402

BATCH, C, RADIUS = 4, 64, 0.8
FPS_CASES = (("register_tier", 16_384, 2048), ("streamed_tier", 75_000, 4096))
KEYPOINTS, NSAMPLES = 2048, (16, 32)
EXTENT = np.array([70.4, 80.0, 4.0])
KEYS = ("sample/fps", "sample/ball_query", "query/group_fwd", "pointvoxel/groups")


def cloud(n, seed):
    """BATCH scenes x n points, scene-contiguous: a lidar-like mix -- two thirds near a ground sheet, the rest uniform --
    in a 70.4 x 80 x 4 m box -> fp32 [BATCH * n, 4], int32 [BATCH * n]"""
    rng = np.random.default_rng(seed)
    pts = rng.random((BATCH * n, 4))
    pts[:, :3] *= EXTENT
    ground = rng.random(BATCH * n) < 2.0 / 3.0
    pts[ground, 2] = 0.3 + 0.1 * rng.standard_normal(int(ground.sum()))
    return pts.astype(np.float32), np.repeat(np.arange(BATCH, dtype=np.int32), n)


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


def composite_fps(xyz, K):
    """xyz [B, n, 3] -> idx int64 [B, K] (positions inside the scene): the batched loop"""
    Bn, n, _ = xyz.shape
    t = torch.full((Bn, n), float("inf"), device=xyz.device)
    idx = torch.zeros((Bn, K), dtype=torch.long, device=xyz.device)
    last = torch.zeros((Bn,), dtype=torch.long, device=xyz.device)
    rows = torch.arange(Bn, device=xyz.device)
    for s in range(1, K):
        d = xyz - xyz[rows, last].unsqueeze(1)
        t = torch.minimum(t, (d * d).sum(dim=2))
        last = t.argmax(dim=1)
        idx[:, s] = last
    return idx


def composite_ball(q, p, nsample, chunk=256):
    """q [B, m, 3], p [B, n, 3] -> rows int32 [B * m, nsample] (point index in the whole cloud, -1: none), count: a
    distance matrix per chunk of queries, a mask scored by point index, topk"""
    Bn, n, _ = p.shape
    score_of = torch.arange(n, 0, -1, device=p.device, dtype=torch.int32)              # lower index, larger score
    rows, count = [], []
    for b in range(Bn):
        for c0 in range(0, q.shape[1], chunk):
            d = p[b].unsqueeze(0) - q[b, c0:c0 + chunk].unsqueeze(1)
            hit = (d * d).sum(dim=2) < RADIUS * RADIUS
            score, first = torch.topk(hit.int() * score_of, nsample, dim=1)
            rows.append(torch.where(score > 0, first + b * n, -1).int())
            count.append((score > 0).sum(dim=1).int())
    return torch.cat(rows), torch.cat(count)


def composite_group(feat, rows):
    out = feat.index_select(0, rows.clamp_min(0).reshape(-1).long()).view(rows.shape[0], rows.shape[1], -1)
    return out * (rows >= 0).unsqueeze(2).to(feat.dtype)


def no_grad(fn):
    def run():
        with torch.no_grad():
            return fn()
    return run


def probe(dev, repeats, fps_composite_repeats):
    res = {"batch": BATCH, "C": C, "radius": RADIUS, "dtype": "f16", "resident_points": _sample.resident_points()}
    stages, fps_k = {}, {}
    clouds = {}
    for name, n, K in FPS_CASES:
        pts_h, bid_h = cloud(n, seed=n)
        pts, bid = torch.from_numpy(pts_h).to(dev), torch.from_numpy(bid_h).to(dev)
        clouds[name] = (pts, bid, n)
        groups = Fsp.scene_groups(bid, BATCH * n, BATCH)
        xyz = pts[:, :3].reshape(BATCH, n, 3).contiguous()
        before = _lib.launch_counts(KEYS)
        s = Fsp.farthest_point_sample(pts, bid, BATCH, K, groups=groups)
        res[f"launches_of_fps_{name}"] = {k: v - before[k] for k, v in _lib.launch_counts(KEYS).items()}
        comp = composite_fps(xyz, K) + torch.arange(BATCH, device=dev).unsqueeze(1) * n
        assert bool((s.count == K).all())
        res[f"fps_{name}"] = {"points_per_scene": n, "samples": K,
                              "slots_equal_to_composite": int((comp == s.idx.long()).sum()), "slots": BATCH * K}
        fps_k[name] = K
        stages[f"fps_{name}"] = (no_grad(lambda p=pts, b=bid, k=K, g=groups: Fsp.farthest_point_sample(p, b, BATCH, k, groups=g)),
                                 no_grad(lambda x=xyz, k=K: composite_fps(x, k)))
        stages[f"scene_groups_{name}"] = (lambda b=bid, m=BATCH * n: Fsp.scene_groups(b, m, BATCH), None)
    pts, bid, n = clouds["streamed_tier"]
    groups = Fsp.scene_groups(bid, BATCH * n, BATCH)
    keys = Fsp.farthest_point_sample(pts, bid, BATCH, KEYPOINTS, groups=groups)
    q = Fsp.gather_samples(pts, keys)
    feat = torch.randn((BATCH * n, C), device=dev).half()
    p3, q3 = pts[:, :3].reshape(BATCH, n, 3).contiguous(), q[:, :3].reshape(BATCH, KEYPOINTS, 3).contiguous()
    for ns in NSAMPLES:
        before = _lib.launch_counts(KEYS)
        nb = Fsp.ball_query(q, keys.batch_ids, pts, bid, BATCH, RADIUS, ns, groups=groups)
        res[f"launches_of_ball_query_nsample{ns}"] = {k: v - before[k] for k, v in _lib.launch_counts(KEYS).items()}
        rows_c, count_c = composite_ball(q3, p3, ns)
        res[f"ball_query_nsample{ns}"] = {
            "queries": BATCH * KEYPOINTS, "points_per_scene": n, "mean_count": round(float(nb.count.float().mean()), 3),
            "queries_truncated": int((nb.count == ns).sum()),
            "queries_equal_to_composite": int((rows_c == nb.rows).all(dim=1).sum())}   # (d2 within an ulp of r2 may differ)
        assert torch.equal(Fsp.group_voxels(feat, nb), composite_group(feat, nb.rows))
        stages[f"ball_query_nsample{ns}"] = (
            no_grad(lambda k=ns: Fsp.ball_query(q, keys.batch_ids, pts, bid, BATCH, RADIUS, k, groups=groups)),
            no_grad(lambda k=ns: composite_ball(q3, p3, k)))
        stages[f"group_forward_nsample{ns}"] = (no_grad(lambda t=nb: Fsp.group_voxels(feat, t)),
                                                no_grad(lambda t=nb: composite_group(feat, t.rows)))
    for rnd in range(2):                                        # alternate the forms: two rounds each
        for stage, (nat, composite) in stages.items():
            res[f"native_{stage}_round{rnd}"] = timed(nat, repeats)
            if composite is not None:
                slow = stage.startswith("fps_")
                res[f"composite_{stage}_round{rnd}"] = timed(composite, fps_composite_repeats if slow else repeats,
                                                             warmup=1 if slow else 3)
    verdict = {}
    for stage, (_, composite) in stages.items():
        nat = [res[f"native_{stage}_round{r}"]["median_us"] for r in range(2)]
        if composite is None:
            verdict[stage] = {"native_us": nat}
            continue
        com = [res[f"composite_{stage}_round{r}"]["median_us"] for r in range(2)]
        verdict[stage] = {"native_us": nat, "composite_us": com, "native_no_slower": max(nat) <= min(com)}
    for name, K in fps_k.items():                               # what replaces the estimates: the time of one step
        verdict[f"fps_{name}"]["native_us_per_step"] = [round(v / K, 3) for v in verdict[f"fps_{name}"]["native_us"]]
    res["verdict"] = verdict
    res["slower_than_composite"] = sorted(k for k, v in verdict.items() if v.get("native_no_slower") is False)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--fps-composite-repeats", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sample_probe needs the GPU: nothing is measured without one")
    res = {"repeats": args.repeats, "fps_composite_repeats": args.fps_composite_repeats}
    res.update(probe(torch.device("cuda:0"), args.repeats, args.fps_composite_repeats))
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
