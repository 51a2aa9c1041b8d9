#!/usr/bin/env python
"""What does neighbour attention cost?  `functional.neighbor_attention` / `neighbor_aggregate` (csrc/nattn.hip) against
the two composites a user writes today -- `group_voxels` twice + einsum / masked softmax / einsum, and the same with
torch's own index gather in place of `group_voxels` -- forward and forward + backward (gradients in q, k and v),
alternating in one process.  HIP events, 5 warm-up calls, median of the repeats, two rounds.  Three sizes, f16, C = 64,
H = 4:

  (a) roi_grid   the Voxel R-CNN size of tools/query_probe.py: 110 592 RoI grid points over 120 000 voxels,
                 `voxel_query` range (4, 4, 4), S = 16
  (b) voxel_self the 120 000 voxels of that level over their own `voxel_query` window, range (2, 2, 2), S = 32
  (c) knn_self   4 x 16 384 points, `knn_query` k = 16 self-query, with `neighbor_aggregate` at G = 8 beside the attention

    python tools/nattn_probe.py [--out profiles/nattn_probe.json] [--repeats 30]
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

C, H, G = 64, 4, 8


def gather_native(t, nb):
    return Fsp.group_voxels(t, nb)


def gather_torch(t, nb):
    return t[nb.rows.clamp(min=0).long()]


def attention_composite(gather, q, k, v, nb):
    M, S = nb.rows.shape
    key = nb.rows >= 0
    kg, vg = gather(k, nb).view(M, S, H, -1), gather(v, nb).view(M, S, H, -1)
    x = torch.einsum("mhd,mshd->msh", q.view(M, H, -1), kg).float() * (C // H) ** -0.5
    x = x.masked_fill(~key[:, :, None], -torch.inf).masked_fill(~key.any(1)[:, None, None], 0)
    P = torch.softmax(x, dim=1).masked_fill(~key[:, :, None], 0).to(q.dtype)
    return torch.einsum("msh,mshd->mhd", P, vg).reshape(M, C)


def aggregate_composite(gather, w, v, nb):
    M, S = nb.rows.shape
    vg = gather(v, nb).view(M, S, G, -1)
    return torch.einsum("msg,msgd->mgd", w.masked_fill(~(nb.rows >= 0)[:, :, None], 0), vg).reshape(M, C)


def tables(dev):
    idx_h, pts_h, bids_h = qp.scene()
    idx = torch.from_numpy(idx_h).to(dev)
    assert ops.attach_rank_map(idx, qp.BATCH, qp.GRID), "the level is in key order"
    x = spconv.SparseConvTensor(torch.zeros((idx.shape[0], 1), device=dev), idx, qp.GRID, qp.BATCH)
    roi = Fsp.voxel_query(torch.from_numpy(pts_h).to(dev), torch.from_numpy(bids_h).to(dev), x, qp.VSIZE, qp.RANGE,
                          qp.QRANGE, 16, with_groups=True)
    centres = ((idx[:, 1:].flip(1).float() + 0.5) * torch.tensor(qp.VSIZE, device=dev)
               + torch.tensor(qp.RANGE[:3], device=dev)).contiguous()
    own = Fsp.voxel_query(centres, idx[:, 0].contiguous(), x, qp.VSIZE, qp.RANGE, (2, 2, 2), 32, with_groups=True)
    rng = np.random.default_rng(1)
    cloud = torch.from_numpy((rng.random((4 * 16384, 3)) * [70.4, 80.0, 4.0]).astype(np.float32)).to(dev)
    cbid = (torch.arange(4 * 16384, device=dev) // 16384).to(torch.int32)
    knn = Fsp.knn_query(cloud, cbid, cloud, cbid, 4, 16, with_groups=True).neighbors()
    return {"roi_grid": roi, "voxel_self": own, "knn_self": knn}


def probe(dev, repeats):
    res, stages = {"C": C, "H": H, "G": G, "dtype": "f16"}, {}
    for tag, nb in tables(dev).items():
        M, S = (int(s) for s in nb.rows.shape)
        torch.manual_seed(S)
        q = torch.randn((M, C), device=dev).half().requires_grad_(True)
        k, v = (torch.randn((nb.num_voxels, C), device=dev).half().requires_grad_(True) for _ in range(2))
        w = torch.softmax(torch.randn((M, S, G), device=dev), dim=1).half().requires_grad_(True)
        g = torch.randn((M, C), device=dev).half()
        res[tag] = {"queries": M, "rows": nb.num_voxels, "nsample": S, "mean_keys": round(float(nb.count.float().mean()), 2)}
        forms = {"attention_native": (lambda q, k, v, nb=nb: Fsp.neighbor_attention(q, k, v, nb, H), (q, k, v)),
                 "attention_group_voxels": (lambda q, k, v, nb=nb: attention_composite(gather_native, q, k, v, nb), (q, k, v)),
                 "attention_index_select": (lambda q, k, v, nb=nb: attention_composite(gather_torch, q, k, v, nb), (q, k, v))}
        if tag == "knn_self":
            forms.update({
                "aggregate_native": (lambda w, v, nb=nb: Fsp.neighbor_aggregate(w, v, nb), (w, v)),
                "aggregate_group_voxels": (lambda w, v, nb=nb: aggregate_composite(gather_native, w, v, nb), (w, v)),
                "aggregate_index_select": (lambda w, v, nb=nb: aggregate_composite(gather_torch, w, v, nb), (w, v))})
        with torch.no_grad():
            diff = forms["attention_native"][0](q, k, v).float() - forms["attention_index_select"][0](q, k, v).float()
            res[tag]["max_abs_diff_to_composite"] = float(diff.abs().max())
        for name, (fn, leaves) in forms.items():
            def fwd(fn=fn, leaves=leaves):
                with torch.no_grad():
                    fn(*leaves)

            def both(fn=fn, leaves=leaves, g=g):
                for t in leaves:
                    t.grad = None
                fn(*leaves).backward(g)

            stages[f"{tag}_{name}_fwd"] = fwd
            stages[f"{tag}_{name}_fwd_bwd"] = both
    for rnd in range(2):                                        # alternate the forms: two rounds each
        for stage, fn in stages.items():
            res[f"{stage}_round{rnd}"] = timed(fn, repeats)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nattn_probe.json"))
    ap.add_argument("--repeats", type=int, default=30)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("nattn_probe needs the GPU: nothing is measured without one")
    res = {"repeats": args.repeats, "probe": probe(torch.device("cuda:0"), args.repeats)}
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
