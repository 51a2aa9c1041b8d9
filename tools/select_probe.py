#!/usr/bin/env python
"""What does a voxel pruning step cost?  Times `sparse_prune(ratio = 0.5)` of 4 x 100 k rows on [41, 1600, 1408], f16,
C = 16 and C = 64, on the kernels of csrc/select.hip against the torch composite a user would write (abs().mean(1),
topk, boolean indexing of features and indices), alternating in one process: the score, the flags, the build (with and
without the rank map), the forward gather and the backward on their own, and the whole prune.  Then the build of one
SubMConv3d(64, 64, 3) rulebook behind each of the two results: from the rank map the native result carries, and through
the hash table the composite's untagged rows need.  HIP events, warm-up, median of the repeats.

    python tools/select_probe.py [--out profiles/select_probe.json] [--repeats 30]
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
import spconv_amd.pytorch as spconv  # noqa: E402
from spconv_amd.pytorch import _select, ops  # noqa: E402
from spconv_amd.pytorch import functional as Fsp  # noqa: E402

SHAPE, BATCH, ROWS, RATIO = [41, 1600, 1408], 4, 100_000, 0.5
SCENES = {"lidar_41x1600x1408_C16": 16, "lidar_41x1600x1408_C64": 64}
KEYS = ("select/score", "select/hist", "select/pick", "select/ties", "select/flags", "select/count", "select/scan",
        "select/scatter", "select/map")


def scene(C, dev):
    """ROWS distinct voxels per batch element in ascending key order, the level's rank map attached"""
    rng = np.random.default_rng(0)
    cells = int(np.prod(SHAPE))
    parts = []
    for b in range(BATCH):
        keys = np.sort(rng.choice(cells, size=ROWS, replace=False))
        parts.append(np.stack([np.full_like(keys, b)] + list(np.unravel_index(keys, SHAPE)), axis=1))
    idx = torch.from_numpy(np.concatenate(parts).astype(np.int32)).to(dev)
    feat = torch.randn((idx.shape[0], C), device=dev).half()
    return idx, feat


def timed(fn, repeats, warmup=5):
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


def probe(C, dev, repeats):
    idx, feat = scene(C, dev)
    n = int(idx.shape[0])
    k = int(RATIO * n)
    res = {"shape": SHAPE, "batch": BATCH, "rows": n, "C": C, "dtype": "f16", "ratio": RATIO}
    tagged = idx.clone()
    assert ops.attach_rank_map(tagged, BATCH, SHAPE)
    x = spconv.SparseConvTensor(feat, tagged, SHAPE, BATCH)
    plain = spconv.SparseConvTensor(feat, idx, SHAPE, BATCH)

    before = _lib.launch_counts(KEYS)
    kept = Fsp.sparse_prune(x, ratio=RATIO)
    res["launches_of_one_prune"] = {key: v - before[key] for key, v in _lib.launch_counts(KEYS).items()}
    score = _select.row_score(feat)
    keep, sel = _select.topk_flags(score, None, RATIO)
    res["sel"] = sel.cpu().tolist()
    build = _select.select_build(idx, BATCH, SHAPE, keep)
    n_out = build.n_out
    dout = torch.randn((n_out, C), device=dev).half()
    # the composite: the same rows when no score ties at the threshold (fp16 mean in torch's own order)
    c_score = feat.abs().mean(1)
    c_mask = torch.zeros((n,), dtype=torch.bool, device=dev)
    c_mask[torch.topk(c_score, k).indices] = True
    res["rows_kept"] = n_out
    res["composite_picks_other_rows"] = int((c_mask != keep.bool()).sum().item())

    def composite_flags():
        m = torch.zeros((n,), dtype=torch.bool, device=dev)
        m[torch.topk(c_score, k).indices] = True
        return m

    def native_all():
        f = feat.detach().requires_grad_(True)
        out = Fsp.sparse_prune(spconv.SparseConvTensor(f, tagged, SHAPE, BATCH), ratio=RATIO)
        out.features.backward(dout)

    def composite_all():
        f = feat.detach().requires_grad_(True)
        m = torch.zeros((n,), dtype=torch.bool, device=dev)
        m[torch.topk(f.detach().abs().mean(1), k).indices] = True
        out = spconv.SparseConvTensor(f[m], idx[m], SHAPE, BATCH)
        out.features.backward(dout)

    stages = {
        "native_score": lambda: _select.row_score(feat),
        "composite_score": lambda: feat.abs().mean(1),
        "native_flags": lambda: _select.topk_flags(score, None, RATIO),
        "composite_flags": composite_flags,
        "native_build": lambda: _select.select_build(idx, BATCH, SHAPE, keep),
        "native_build_with_rank_map": lambda: _select.select_build(idx, BATCH, SHAPE, keep, rank_map=True),
        "composite_build": lambda: idx[c_mask],
        "native_fwd": lambda: _select.fwd(feat, build),
        "composite_fwd": lambda: feat[c_mask],
        "native_bwd": lambda: _select.bwd(dout, build),
        "composite_bwd": lambda: torch.zeros_like(feat).index_put_((c_mask,), dout),
        "native_prune_fwd_bwd": native_all,
        "composite_prune_fwd_bwd": composite_all,
    }
    # one SubMConv3d(64, 64, 3) rulebook behind each result: from the rank map / through the hash table
    ranked_idx = kept.indices
    hashed_idx = idx[c_mask].contiguous()
    assert ops._rankmap_of(ranked_idx, BATCH, SHAPE, n_out, 27) is not None
    assert ops._rankmap_of(hashed_idx, BATCH, SHAPE, hashed_idx.shape[0], 27) is None

    def rulebook(indices):
        return lambda: ops.build_rulebook(indices, BATCH, SHAPE, [3] * 3, [1] * 3, [1] * 3, [1] * 3, [0] * 3, subm=True,
                                          need_native=False)

    stages["subm_k3_rulebook_behind_native_ranked"] = rulebook(ranked_idx)
    stages["subm_k3_rulebook_behind_composite_hashed"] = rulebook(hashed_idx)
    for rnd in range(2):                                        # alternate the forms: two rounds each
        for stage, fn in stages.items():
            res[f"{stage}_round{rnd}"] = timed(fn, repeats)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "select_probe.json"))
    ap.add_argument("--repeats", type=int, default=30)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("select_probe needs the GPU: nothing is measured without one")
    dev = torch.device("cuda:0")
    res = {"repeats": args.repeats}
    for name, C in SCENES.items():
        res[name] = probe(C, dev, args.repeats)
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
