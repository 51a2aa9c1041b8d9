#!/usr/bin/env python
"""What does serialised patch attention cost?  4 x 100 k voxels on [41, 1600, 1408], f16, at C = 64 / H = 4 / D = 16 and
C = 256 / H = 4 / D = 64, patches of 128 and 1024 slots: `functional.patch_attention` (csrc/attn.hip) against the two
torch composites a user writes between `rows_to_patches` and `patches_to_rows` -- the 16-bit padded bmm / masked softmax
/ bmm, and `scaled_dot_product_attention` with the same boolean mask -- forward and forward + backward, alternating in one
process.  HIP events, 5 warm-up calls, median of the repeats, two rounds.

    python tools/attn_probe.py [--out profiles/attn_probe.json] [--repeats 30]

--bias measures the same four cases with Point Transformer V3's relative position bias (default pos_bnd, a random fp32
table): the native biased call against the native unbiased call on the same inputs and against
`scaled_dot_product_attention` given the bias as a materialised additive fp32 mask [P_cap, H, K, K]; building that mask
from the table is timed on its own and is in no other item.

    python tools/attn_probe.py --bias [--out profiles/attn_bias_probe.json]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from serialize_probe import BATCH, SHAPE, scene, timed  # noqa: E402
from spconv_amd.pytorch import functional as Fsp  # noqa: E402

CASES = [(4, 16), (4, 64)]
PATCHES = [128, 1024]


def heads(x, plan, H, D):
    """[n, 3 * H * D] rows -> q, k, v [P_cap, H, K, D] in patch order"""
    P_cap, K = plan.patch_rows.shape
    return Fsp.rows_to_patches(x, plan).reshape(P_cap, K, 3, H, D).permute(2, 0, 3, 1, 4).unbind(0)


def bmm_composite(x, plan, H, D):
    q, k, v = heads(x, plan, H, D)
    s = torch.matmul(q, k.transpose(2, 3)) * D ** -0.5
    s = s.masked_fill((plan.patch_rows < 0)[:, None, None, :], torch.finfo(s.dtype).min)
    o = torch.matmul(torch.softmax(s, dim=-1), v)
    return Fsp.patches_to_rows(o.transpose(1, 2).reshape(o.shape[0], o.shape[2], H * D), plan)


def sdpa_composite(x, plan, H, D):
    q, k, v = heads(x, plan, H, D)
    keep = (plan.patch_rows >= 0) | ~(plan.patch_rows >= 0).any(dim=1, keepdim=True)      # (an empty patch keeps all)
    o = torch.nn.functional.scaled_dot_product_attention(q, k, v, attn_mask=keep[:, None, None, :])
    return Fsp.patches_to_rows(o.transpose(1, 2).reshape(o.shape[0], o.shape[2], H * D), plan)


def bias_mask(table, coords, plan, pos_bnd):
    """the additive fp32 mask [P_cap, H, K, K] of the SDPA composite: the bias of every pair, -inf on invalid keys"""
    c = coords.long()[plan.patch_rows.long().clamp(min=0)]                                    # [P, K, 3]
    R = 2 * pos_bnd + 1
    bias = None
    for a in range(3):
        d = (c[:, :, None, a] - c[:, None, :, a]).clamp(-pos_bnd, pos_bnd) + pos_bnd + a * R
        bias = table[d] if bias is None else bias + table[d]                                 # [P, K, K, H]
    keep = (plan.patch_rows >= 0) | ~(plan.patch_rows >= 0).any(dim=1, keepdim=True)
    return bias.permute(0, 3, 1, 2).masked_fill(~keep[:, None, None, :], float("-inf")).contiguous()


def sdpa_bias_composite(x, plan, H, D, mask):
    q, k, v = heads(x, plan, H, D)
    o = torch.nn.functional.scaled_dot_product_attention(q, k, v, attn_mask=mask)
    return Fsp.patches_to_rows(o.transpose(1, 2).reshape(o.shape[0], o.shape[2], H * D), plan)


def probe_bias(dev, repeats):
    from spconv_amd.pytorch import _attn
    idx = scene(dev)
    n, coords = int(idx.shape[0]), idx[:, 1:].contiguous()
    ser = Fsp.serialize(idx, SHAPE, BATCH, orders=("hilbert",))
    res = {"shape": SHAPE, "batch": BATCH, "rows": n, "dtype": "f16"}
    stages = {}
    for H, D in CASES:
        torch.manual_seed(D)
        qkv = torch.randn((n, 3 * H * D), device=dev).half().requires_grad_(True)
        g = torch.randn((n, H * D), device=dev).half()
        for K in PATCHES:
            plan, pb = Fsp.patch_plan(ser, K, pad="borrow"), _attn.default_pos_bnd(K)
            table = (torch.randn((3 * (2 * pb + 1), H), device=dev) * 0.5).requires_grad_(True)
            tag = f"C{H * D}_K{K}"
            res[f"{tag}_pos_bnd"] = pb
            with torch.no_grad():
                res[f"{tag}_mask_build"] = timed(lambda: bias_mask(table, coords, plan, pb), 3, warmup=1)
                mask = bias_mask(table, coords, plan, pb)
                res[f"{tag}_mask_bytes"] = mask.numel() * 4
                got = Fsp.patch_attention(qkv, plan, H, rel_bias=table, coords=coords)
                res[f"{tag}_max_abs_diff_to_composite_sdpa"] = float((got.float() - sdpa_bias_composite(qkv, plan, H, D, mask).float()).abs().max())
            forms = {"native": lambda x, p=plan, H=H: Fsp.patch_attention(x, p, H),
                     "native_bias": lambda x, p=plan, H=H, t=table: Fsp.patch_attention(x, p, H, rel_bias=t, coords=coords),
                     "composite_sdpa_bias": lambda x, p=plan, H=H, D=D, m=mask: sdpa_bias_composite(x, p, H, D, m)}
            for name, fn in forms.items():
                def fwd(fn=fn, x=qkv.detach()):
                    with torch.no_grad():
                        fn(x)

                def both(fn=fn, x=qkv, g=g, t=table):
                    x.grad = t.grad = None
                    fn(x).backward(g)

                stages[f"{tag}_{name}_fwd"] = fwd
                stages[f"{tag}_{name}_fwd_bwd"] = both
    for rnd in range(2):
        for stage, fn in stages.items():
            res[f"{stage}_round{rnd}"] = timed(fn, repeats)
    return res


def probe(dev, repeats):
    idx = scene(dev)
    n = int(idx.shape[0])
    ser = Fsp.serialize(idx, SHAPE, BATCH, orders=("hilbert",))
    res = {"shape": SHAPE, "batch": BATCH, "rows": n, "dtype": "f16"}
    stages = {}
    for H, D in CASES:
        torch.manual_seed(D)
        qkv = torch.randn((n, 3 * H * D), device=dev).half().requires_grad_(True)
        g = torch.randn((n, H * D), device=dev).half()
        for K in PATCHES:
            plan = Fsp.patch_plan(ser, K, pad="borrow")
            forms = {"native": lambda x, p=plan, H=H: Fsp.patch_attention(x, p, H),
                     "composite_bmm": lambda x, p=plan, H=H, D=D: bmm_composite(x, p, H, D),
                     "composite_sdpa": lambda x, p=plan, H=H, D=D: sdpa_composite(x, p, H, D)}
            with torch.no_grad():
                want = forms["composite_bmm"](qkv).float()
                res[f"C{H * D}_K{K}_max_abs_diff_to_composite_bmm"] = float((forms["native"](qkv).float() - want).abs().max())
            for name, fn in forms.items():
                def fwd(fn=fn, x=qkv.detach()):
                    with torch.no_grad():
                        fn(x)

                def both(fn=fn, x=qkv, g=g):
                    x.grad = None
                    fn(x).backward(g)

                stages[f"C{H * D}_K{K}_{name}_fwd"] = fwd
                stages[f"C{H * D}_K{K}_{name}_fwd_bwd"] = both
    for rnd in range(2):                                        # alternate the forms: two rounds each
        for stage, fn in stages.items():
            res[f"{stage}_round{rnd}"] = timed(fn, repeats)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bias", action="store_true", help="the biased cases (profiles/attn_bias_probe.json)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=30)
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "attn_bias_probe.json" if args.bias else "attn_probe.json")
    if not torch.cuda.is_available():
        raise SystemExit("attn_probe needs the GPU: nothing is measured without one")
    res = {"repeats": args.repeats,
           "lidar_41x1600x1408": (probe_bias if args.bias else probe)(torch.device("cuda:0"), args.repeats)}
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
