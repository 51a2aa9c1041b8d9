#!/usr/bin/env python
"""What does a kernel point convolution cost?  `functional.kpconv` (csrc/kpconv.hip) against the composite a user
writes without it -- `group_voxels`, the influence in float32 cast to the rows' dtype, two einsums -- forward and
forward + backward (gradients in feats and weight), alternating in one process.  HIP events, 5 warm-up calls, median of
the repeats, two rounds.  f16, K = 15, Cin = Cout in {64, 128}, two tables:

  (a) knn_self   4 x 16 384 points, `knn_query` k = 16 self-query
  (b) ball_cells 4 x 75 000 points, `ball_query_cells` at nsample 32

The backward's three parts (query side, `spx_group_bwd`, weight side) are timed on their own through `kpconv_bwd_into`,
and the forward's gather is set against the HBM roofline: the bytes a forward has to move (M * S valid rows of Cin
elements, out, the table and its offsets) over the measured time, as a share of the peak bandwidth given by --hbm-gbs.

    python tools/kpconv_probe.py [--out profiles/kpconv_probe.json] [--repeats 20]
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
from serialize_probe import timed  # noqa: E402
from spconv_amd.pytorch import functional as Fsp  # noqa: E402
from spconv_amd.pytorch._kpconv import default_kernel_points  # noqa: E402
from spconv_amd.pytorch._query import group_bwd  # noqa: E402

K, SIGMA, EXTENT = 15, 0.6, [70.4, 80.0, 4.0]


def composite(feats, weight, nb, kp, normalize=False):
    valid = nb.rows >= 0
    d = (nb.offsets[:, :, None, :] - kp[None, None]).square().sum(3).sqrt()
    h = (1 - d / SIGMA).clamp_min(0).masked_fill(~valid[:, :, None], 0).to(feats.dtype)
    out = torch.einsum("mkc,kcd->md", torch.einsum("msk,msc->mkc", h, Fsp.group_voxels(feats, nb)), weight)
    return out / valid.sum(1).clamp_min(1)[:, None].to(feats.dtype) if normalize else out


def tables(dev):
    rng = np.random.default_rng(1)
    out = {}
    for tag, per in (("knn_self", 16384), ("ball_cells", 75000)):
        cloud = torch.from_numpy((rng.random((4 * per, 3)) * EXTENT).astype(np.float32)).to(dev)
        bid = (torch.arange(4 * per, device=dev) // per).to(torch.int32)
        if tag == "knn_self":
            out[tag] = Fsp.knn_query(cloud, bid, cloud, bid, 4, 16, with_offsets=True, with_groups=True).neighbors()
        else:
            index = Fsp.point_cell_index(cloud, bid, 4, 1.0, [0, 0, 0] + EXTENT)
            out[tag] = Fsp.ball_query_cells(cloud, bid, index, 1.0, 32, with_offsets=True, with_groups=True)
    return out


def probe(dev, repeats, hbm_gbs):
    res, stages = {"K": K, "dtype": "f16", "sigma": SIGMA, "hbm_gbs": hbm_gbs}, {}
    kp = (default_kernel_points(1.0) * 0.8).to(dev)
    for tag, nb in tables(dev).items():
        M, S = (int(s) for s in nb.rows.shape)
        for C in (64, 128):
            key = f"{tag}_c{C}"
            torch.manual_seed(C)
            feats = torch.randn((nb.num_voxels, C), device=dev).half().requires_grad_(True)
            weight = (torch.randn((K, C, C), device=dev) * (K * C) ** -0.5).half().requires_grad_(True)
            g = torch.randn((M, C), device=dev).half()
            valid = int((nb.rows >= 0).sum())
            res[key] = {"queries": M, "rows": nb.num_voxels, "nsample": S, "valid_slots": valid,
                        "forward_bytes": 2 * valid * C + 2 * M * C + 16 * M * S + 2 * K * C * C}
            with torch.no_grad():
                diff = Fsp.kpconv(feats, nb, kp, weight, SIGMA).float() - composite(feats, weight, nb, kp).float()
                res[key]["max_abs_diff_to_composite"] = float(diff.abs().max())
            forms = {"native": lambda f, w, nb=nb: Fsp.kpconv(f, nb, kp, w, SIGMA),
                     "composite": lambda f, w, nb=nb: composite(f, w, nb, kp)}
            for name, fn in forms.items():
                def fwd(fn=fn, f=feats, w=weight):
                    with torch.no_grad():
                        fn(f, w)

                def both(fn=fn, f=feats, w=weight, g=g):
                    f.grad = w.grad = None
                    fn(f, w).backward(g)

                stages[f"{key}_{name}_fwd"] = fwd
                stages[f"{key}_{name}_fwd_bwd"] = both
            # the backward's parts, on buffers of their own
            f, w = feats.detach(), weight.detach()
            wf, dg = torch.empty((M, K, C), device=dev).half(), torch.empty((M, S, C), device=dev).half()
            dfe, dwe = torch.empty_like(f), torch.empty_like(w)
            ws = torch.empty((Fsp.kpconv_ws_bytes(M, K, C, C),), dtype=torch.uint8, device=dev)
            bws = torch.empty((Fsp.kpconv_ws_bytes(M, K, C, C, True),), dtype=torch.uint8, device=dev)
            Fsp.kpconv_into(f, nb, kp, w, SIGMA, False, torch.empty((M, C), device=dev).half(), wf, ws)
            bare = nb._replace(groups=None)
            stages[f"{key}_bwd_query_and_group"] = lambda a=(wf, nb, kp, w, SIGMA, False, g, dg, dfe, None, None): \
                Fsp.kpconv_bwd_into(*a)
            stages[f"{key}_bwd_group"] = lambda dg=dg, nb=nb: group_bwd(dg, nb)
            stages[f"{key}_bwd_weight"] = lambda a=(wf, bare, kp, w, SIGMA, False, g, None, None, dwe, bws): \
                Fsp.kpconv_bwd_into(*a)
    for rnd in range(2):                                        # alternate the forms: two rounds each
        for stage, fn in stages.items():
            res[f"{stage}_round{rnd}"] = timed(fn, repeats)
    for key in [k for k in res if isinstance(res[k], dict) and "forward_bytes" in res[k]]:
        us = min(res[f"{key}_native_fwd_round{r}"]["median_us"] for r in range(2))
        res[key]["forward_share_of_hbm_roofline"] = round(res[key]["forward_bytes"] / (us * 1e-6) / (hbm_gbs * 1e9), 3)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kpconv_probe.json"))
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--hbm-gbs", type=float, default=8000.0, help="peak HBM bandwidth the roofline share is taken of")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("kpconv_probe needs the GPU: nothing is measured without one")
    res = {"repeats": args.repeats, "probe": probe(torch.device("cuda:0"), args.repeats, args.hbm_gbs)}
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
