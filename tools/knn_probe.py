#!/usr/bin/env python
"""What do the k-nearest-neighbour query and the inverse-distance interpolation over raw points cost?  Three cases of the
code bases that call three_nn / three_interpolate / knn_query: (a) the feature propagation of a PV-RCNN-style point head,
three-NN interpolation of 4 x 75 000 unknown points from 4 x 2048 keypoints, C = 64 f16, forward and backward with its
groups; (b) k = 16 grouping of 4 x 2048 queries over 4 x 75 000 points; (c) the k = 16 self-query of 4 x 16 384 points.
Timed on the kernel of csrc/knn.hip (and the blend of csrc/interp.hip) against the torch composite a user would
otherwise write, per scene: a chunked distance matrix + topk(largest=False), then index_select / mul / sum and autograd's
backward (index_add_ with atomics).  The two forms alternate in one process; HIP events around one call each, warm-up
calls first, median and minimum of the repeats, two interleaved rounds.  The composite leaves ties open: the number of
queries it answers with other rows is recorded.

    python tools/knn_probe.py [--out profiles/knn_probe.json] [--repeats 20]
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
from spconv_amd.pytorch import functional as Fsp  # noqa: E402

BATCH, C, EPS = 4, 64, 1e-8
N_CLOUD, N_SELF, KEYPOINTS, K_GROUP = 75_000, 16_384, 2048, 16
EXTENT = np.array([70.4, 80.0, 4.0])
KEYS = ("sample/knn_query", "interp/fwd", "interp/bwd", "pointvoxel/groups")


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


def composite_knn(q, p, k, chunk):
    """q [B, m, 3], p [B, n, 3] -> rows int64 [B * m, k] (point index in the whole cloud), d2 [B * m, k]: a distance
    matrix per chunk of queries and topk of the smallest (ties: whatever topk does)"""
    Bn, n, _ = p.shape
    rows, dist = [], []
    for b in range(Bn):
        for c0 in range(0, q.shape[1], chunk):
            d = p[b].unsqueeze(0) - q[b, c0:c0 + chunk].unsqueeze(1)
            d2, idx = torch.topk((d * d).sum(dim=2), k, dim=1, largest=False)
            rows.append(idx + b * n)
            dist.append(d2)
    return torch.cat(rows), torch.cat(dist)


def composite_weights(d2):
    r = 1.0 / (d2.sqrt() + EPS)
    return r / r.sum(dim=1, keepdim=True)


def composite_blend(feat, rows, w):
    out = feat.index_select(0, rows.reshape(-1)).view(rows.shape[0], rows.shape[1], -1)
    return (out * w.unsqueeze(2).to(feat.dtype)).sum(dim=1)


def no_grad(fn):
    def run():
        with torch.no_grad():
            return fn()
    return run


def agreement(knn, rows_c, k):
    """queries the composite answers with other rows than the kernel (ties, and distances an ulp apart in its own sum)"""
    same = (rows_c.int() == knn.rows[:, :k]).all(dim=1)
    return {"queries": int(rows_c.shape[0]), "queries_equal_to_composite": int(same.sum()),
            "queries_with_other_rows": int((~same).sum())}


def probe(dev, repeats):
    res = {"batch": BATCH, "C": C, "dtype": "f16", "eps": EPS, "max_k": _lib.load().spx_knn_max_k()}
    stages = {}
    pts_h, bid_h = cloud(N_CLOUD, seed=N_CLOUD)
    pts, bid = torch.from_numpy(pts_h).to(dev), torch.from_numpy(bid_h).to(dev)
    groups = Fsp.scene_groups(bid, BATCH * N_CLOUD, BATCH)
    keys = Fsp.farthest_point_sample(pts, bid, BATCH, KEYPOINTS, groups=groups)
    kp = Fsp.gather_samples(pts, keys).contiguous()
    kp_groups = Fsp.scene_groups(keys.batch_ids, BATCH * KEYPOINTS, BATCH)
    p3 = pts[:, :3].reshape(BATCH, N_CLOUD, 3).contiguous()
    k3 = kp[:, :3].reshape(BATCH, KEYPOINTS, 3).contiguous()

    # (a) three-NN interpolation: unknown = the cloud, known = the keypoints
    feat = torch.randn((BATCH * KEYPOINTS, C), device=dev).half()
    dout = torch.randn((BATCH * N_CLOUD, C), device=dev).half()
    before = _lib.launch_counts(KEYS)
    knn = Fsp.three_nn(pts, bid, kp, keys.batch_ids, BATCH, groups=kp_groups, with_groups=True)
    res["launches_of_three_nn_with_groups"] = {k: v - before[k] for k, v in _lib.launch_counts(KEYS).items()}
    rows_c, d2_c = composite_knn(p3, k3, 3, 8192)
    w_c = composite_weights(d2_c)
    res["three_nn"] = dict(agreement(knn, rows_c, 3), known_per_scene=KEYPOINTS, unknown_per_scene=N_CLOUD,
                           max_abs_weight_difference=float((w_c - knn.weights[:, :3]).abs().max()))
    out_n = Fsp.knn_interpolate(feat, knn)
    out_c = composite_blend(feat, rows_c, w_c)
    res["three_nn"]["max_abs_output_difference"] = float((out_n.float() - out_c.float()).abs().max())
    feat_g = feat.clone().requires_grad_(True)
    stages["three_nn_query"] = (
        no_grad(lambda: Fsp.three_nn(pts, bid, kp, keys.batch_ids, BATCH, groups=kp_groups)),
        no_grad(lambda: composite_weights(composite_knn(p3, k3, 3, 8192)[1])))
    stages["three_nn_groups"] = (lambda: Fsp.three_nn(pts, bid, kp, keys.batch_ids, BATCH, groups=kp_groups,
                                                       with_groups=True), None)
    stages["interpolate_forward"] = (no_grad(lambda: Fsp.knn_interpolate(feat, knn)),
                                     no_grad(lambda: composite_blend(feat, rows_c, w_c)))
    stages["interpolate_forward_backward"] = (
        lambda: torch.autograd.grad(Fsp.knn_interpolate(feat_g, knn), feat_g, dout),
        lambda: torch.autograd.grad(composite_blend(feat_g, rows_c, w_c), feat_g, dout))

    # (b) k = 16 grouping of the keypoints over the cloud
    before = _lib.launch_counts(KEYS)
    nb = Fsp.knn_query(kp, keys.batch_ids, pts, bid, BATCH, K_GROUP, groups=groups)
    res["launches_of_knn_query_k16"] = {k: v - before[k] for k, v in _lib.launch_counts(KEYS).items()}
    res["knn_k16_keypoints_over_cloud"] = dict(agreement(nb, composite_knn(k3, p3, K_GROUP, 256)[0], K_GROUP),
                                               points_per_scene=N_CLOUD)
    stages["knn_k16_keypoints_over_cloud"] = (
        no_grad(lambda: Fsp.knn_query(kp, keys.batch_ids, pts, bid, BATCH, K_GROUP, groups=groups)),
        no_grad(lambda: composite_knn(k3, p3, K_GROUP, 256)))

    # (c) k = 16 self-query
    self_h, sbid_h = cloud(N_SELF, seed=N_SELF)
    sp, sbid = torch.from_numpy(self_h).to(dev), torch.from_numpy(sbid_h).to(dev)
    s_groups = Fsp.scene_groups(sbid, BATCH * N_SELF, BATCH)
    s3 = sp[:, :3].reshape(BATCH, N_SELF, 3).contiguous()
    own = Fsp.knn_query(sp, sbid, sp, sbid, BATCH, K_GROUP, groups=s_groups)
    itself = int((own.rows[:, 0] == torch.arange(BATCH * N_SELF, device=dev)).sum())           # (d2 = 0, the lowest index)
    res["knn_k16_self_query"] = dict(agreement(own, composite_knn(s3, s3, K_GROUP, 1024)[0], K_GROUP),
                                     points_per_scene=N_SELF, queries_that_find_themselves_first=itself)
    stages["knn_k16_self_query"] = (
        no_grad(lambda: Fsp.knn_query(sp, sbid, sp, sbid, BATCH, K_GROUP, groups=s_groups)),
        no_grad(lambda: composite_knn(s3, s3, K_GROUP, 1024)))

    for rnd in range(2):                                        # alternate the forms: two rounds each
        for stage, (nat, composite) in stages.items():
            res[f"native_{stage}_round{rnd}"] = timed(nat, repeats)
            if composite is not None:
                res[f"composite_{stage}_round{rnd}"] = timed(composite, repeats)
    verdict = {}
    for stage, (_, composite) in stages.items():
        nat = [res[f"native_{stage}_round{r}"]["median_us"] for r in range(2)]
        if composite is None:
            verdict[stage] = {"native_us": nat}
            continue
        com = [res[f"composite_{stage}_round{r}"]["median_us"] for r in range(2)]
        verdict[stage] = {"native_us": nat, "composite_us": com, "native_no_slower": max(nat) <= min(com)}
    res["verdict"] = verdict
    res["slower_than_composite"] = sorted(k for k, v in verdict.items() if v.get("native_no_slower") is False)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("knn_probe needs the GPU: nothing is measured without one")
    res = {"repeats": args.repeats}
    res.update(probe(torch.device("cuda:0"), args.repeats))
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
