#!/usr/bin/env python
"""What does a fused set abstraction cost?  `functional.group_linear_max` (csrc/groupmax.hip) against the composite a
user writes without it -- `group_voxels`, the position term in float32, add, ReLU, cast, `matmul`, masked `amax` --
forward and forward + backward (gradients in feats, weight, pos_weight and in_bias), alternating in one process.  HIP
events, 5 warm-up calls, median of the repeats, two rounds.  f16, three tables:

  (a) roi_grid   110 592 RoI grid queries over 120 000 voxels, `voxel_query` at nsample 16, C = 64 -> 64 and 32 -> 32
  (b) ball_cells 8192 keypoints over 4 x 75 000 points, `ball_query_cells` at nsample 32, C = 64 -> 128
  (c) knn_self   4 x 16 384 points, `knn_query` k = 16 self-query, C = 128 -> 128 and 256 -> 256

The backward's three parts (query side, `spx_group_bwd`, weight side) are timed on their own through
`group_linear_max_bwd_into`, and the forward is set against the HBM roofline: the bytes it has to move (M * S valid rows
of Cin elements, out, the table and its offsets, the weight once) over the measured time, as a share of the peak
bandwidth given by --hbm-gbs.  `weight_stream`: the forward with a table whose every slot names row 0 (the gather comes
from cache), as a share of the forward: what is left when the rows cost nothing.

    python tools/groupmax_probe.py [--out profiles/groupmax_probe.json] [--repeats 20]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import query_probe as qp  # noqa: E402
import spconv_amd.pytorch as spconv  # noqa: E402
from serialize_probe import timed  # noqa: E402
from spconv_amd.pytorch import functional as Fsp  # noqa: E402
from spconv_amd.pytorch import ops  # noqa: E402
from spconv_amd.pytorch._query import group_bwd  # noqa: E402

EXTENT = [70.4, 80.0, 4.0]


def composite(feats, weight, pw, bias, nb):
    valid = nb.rows >= 0
    x = Fsp.group_voxels(feats, nb).float() + nb.offsets @ pw + bias
    y = torch.matmul(x.clamp_min(0).to(feats.dtype), weight)
    return y.masked_fill(~valid[:, :, None], float("-inf")).amax(1).masked_fill(~valid.any(1)[:, None], 0)


def tables(dev):
    idx_h, pts_h, bids_h = qp.scene()
    idx = torch.from_numpy(idx_h).to(dev)
    assert ops.attach_rank_map(idx, qp.BATCH, qp.GRID), "the level is in key order"
    x = spconv.SparseConvTensor(torch.zeros((idx.shape[0], 1), device=dev), idx, qp.GRID, qp.BATCH)
    roi = Fsp.voxel_query(torch.from_numpy(pts_h).to(dev), torch.from_numpy(bids_h).to(dev), x, qp.VSIZE, qp.RANGE,
                          qp.QRANGE, 16, with_offsets=True, with_groups=True)
    rng = np.random.default_rng(1)
    cloud = torch.from_numpy((rng.random((4 * 75000, 3)) * EXTENT).astype(np.float32)).to(dev)
    bid = (torch.arange(4 * 75000, device=dev) // 75000).to(torch.int32)
    keys = torch.arange(8192, device=dev) * (4 * 75000 // 8192)
    index = Fsp.point_cell_index(cloud, bid, 4, 1.0, [0, 0, 0] + EXTENT)
    ball = Fsp.ball_query_cells(cloud[keys].contiguous(), bid[keys].contiguous(), index, 1.0, 32, with_offsets=True,
                                with_groups=True)
    small = torch.from_numpy((rng.random((4 * 16384, 3)) * EXTENT).astype(np.float32)).to(dev)
    sbid = (torch.arange(4 * 16384, device=dev) // 16384).to(torch.int32)
    knn = Fsp.knn_query(small, sbid, small, sbid, 4, 16, with_offsets=True, with_groups=True).neighbors()
    return [("roi_grid", roi, (64, 64)), ("roi_grid", roi, (32, 32)), ("ball_cells", ball, (64, 128)),
            ("knn_self", knn, (128, 128)), ("knn_self", knn, (256, 256))]


def probe(dev, repeats, hbm_gbs):
    res, stages = {"dtype": "f16", "hbm_gbs": hbm_gbs}, {}
    for tag, nb, (Cin, Cout) in tables(dev):
        M, S = (int(s) for s in nb.rows.shape)
        key = f"{tag}_c{Cin}x{Cout}"
        torch.manual_seed(Cin + Cout)
        feats = torch.randn((nb.num_voxels, Cin), device=dev).half().requires_grad_(True)
        weight = (torch.randn((Cin, Cout), device=dev) * Cin ** -0.5).half().requires_grad_(True)
        pw, bias = torch.randn((3, Cin), device=dev).requires_grad_(True), torch.randn((Cin,), device=dev).requires_grad_(True)
        g = torch.randn((M, Cout), device=dev).half()
        valid = int((nb.rows >= 0).sum())
        res[key] = {"queries": M, "rows": nb.num_voxels, "nsample": S, "valid_slots": valid,
                    "forward_bytes": 2 * valid * Cin + 2 * M * Cout + 16 * M * S + 2 * Cin * Cout}
        with torch.no_grad():
            diff = Fsp.group_linear_max(feats, nb, weight, pw, bias).float() - composite(feats, weight, pw, bias, nb).float()
            res[key]["max_abs_diff_to_composite"] = float(diff.abs().max())
        forms = {"native": lambda f, w, p, b, nb=nb: Fsp.group_linear_max(f, nb, w, p, b),
                 "composite": lambda f, w, p, b, nb=nb: composite(f, w, p, b, nb)}
        for name, fn in forms.items():
            def fwd(fn=fn, a=(feats, weight, pw, bias)):
                with torch.no_grad():
                    fn(*a)

            def both(fn=fn, a=(feats, weight, pw, bias), g=g):
                for t in a:
                    t.grad = None
                fn(*a).backward(g)

            stages[f"{key}_{name}_fwd"] = fwd
            stages[f"{key}_{name}_fwd_bwd"] = both
        # the forward over cached rows, and the backward's parts, on buffers of their own
        f, w, p, b = (t.detach() for t in (feats, weight, pw, bias))
        out, arg = torch.empty((M, Cout), device=dev).half(), torch.empty((M, Cout), dtype=torch.uint8, device=dev)
        dg, dfe, dwe, dpe, dbe = torch.empty((M, S, Cin), device=dev).half(), torch.empty_like(f), torch.empty_like(w), \
            torch.empty_like(p), torch.empty_like(b)
        ws = torch.empty((Fsp.group_linear_max_ws_bytes(M, S, Cin, Cout),), dtype=torch.uint8, device=dev)
        bws = torch.empty((Fsp.group_linear_max_ws_bytes(M, S, Cin, Cout, True),), dtype=torch.uint8, device=dev)
        Fsp.group_linear_max_into(f, nb, w, p, b, True, out, arg, ws)
        bare = nb._replace(groups=None)
        cached = bare._replace(rows=torch.where(nb.rows >= 0, torch.zeros_like(nb.rows), nb.rows))
        stages[f"{key}_fwd_cached_rows"] = lambda a=(f, cached, w, p, b, True, torch.empty_like(out), None, ws): \
            Fsp.group_linear_max_into(*a)
        stages[f"{key}_bwd_query_and_group"] = lambda a=(f, nb, w, p, b, True, arg, g, dg, dfe, None, dpe, dbe, bws): \
            Fsp.group_linear_max_bwd_into(*a)
        stages[f"{key}_bwd_group"] = lambda dg=dg, nb=nb: group_bwd(dg, nb)
        stages[f"{key}_bwd_weight"] = lambda a=(f, bare, w, p, b, True, arg, g, None, None, dwe, None, None, bws): \
            Fsp.group_linear_max_bwd_into(*a)
    for rnd in range(2):                                        # alternate the forms: two rounds each
        for stage, fn in stages.items():
            res[f"{stage}_round{rnd}"] = timed(fn, repeats)
    for key in [k for k in res if isinstance(res[k], dict) and "forward_bytes" in res[k]]:
        us = min(res[f"{key}_native_fwd_round{r}"]["median_us"] for r in range(2))
        hot = min(res[f"{key}_fwd_cached_rows_round{r}"]["median_us"] for r in range(2))
        res[key]["forward_share_of_hbm_roofline"] = round(res[key]["forward_bytes"] / (us * 1e-6) / (hbm_gbs * 1e9), 3)
        res[key]["cached_rows_share_of_forward"] = round(hot / us, 3)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "groupmax_probe.json"))
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--hbm-gbs", type=float, default=8000.0, help="peak HBM bandwidth the roofline share is taken of")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("groupmax_probe needs the GPU: nothing is measured without one")
    res = {"repeats": args.repeats, "probe": probe(torch.device("cuda:0"), args.repeats, args.hbm_gbs)}
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
