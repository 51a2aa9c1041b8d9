#!/usr/bin/env python
"""What does voxel serialisation cost?  4 x 100 k voxels on [41, 1600, 1408] (depth 11: keys of 36 bits) on the kernels
of csrc/serialize.hip against the torch composite a user of a serialised transformer writes, alternating in one
process: the keys of four orders (a bit-loop Hilbert / Z encoder), one sort and four sorts (`torch.argsort` on int64, a
scatter for the inverse, `bincount` + `cumsum`), the patch plan (padding arithmetic with read-backs), and both row
moves forward and backward at C = 64 f16 (`index_select` / `index_add_`).  HIP events, warm-up, median of the repeats.

    python tools/serialize_probe.py [--out profiles/serialize_probe.json] [--repeats 30]
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
from spconv_amd.pytorch import _serialize  # noqa: E402
from spconv_amd.pytorch import functional as Fsp  # noqa: E402

SHAPE, BATCH, ROWS, C, PATCH = [41, 1600, 1408], 4, 100_000, 64, 1024
ORDERS = ("z", "z-trans", "hilbert", "hilbert-trans")
KEYS = ("serialize/keys", "serialize/sort", "serialize/offsets", "serialize/plan", "serialize/bwd")


def scene(dev):
    """ROWS distinct voxels per batch element, rows shuffled"""
    rng = np.random.default_rng(0)
    cells = int(np.prod(SHAPE))
    parts = []
    for b in range(BATCH):
        keys = rng.choice(cells, size=ROWS, replace=False)
        parts.append(np.stack([np.full_like(keys, b)] + list(np.unravel_index(keys, SHAPE)), axis=1))
    idx = np.concatenate(parts).astype(np.int32)
    return torch.from_numpy(idx[rng.permutation(idx.shape[0])]).to(dev)


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


# ---- the composite: what the open-source serialised transformers do in torch ----------------------------------------

def z_torch(X, depth):
    code = torch.zeros_like(X[0])
    nd = len(X)
    for b in range(depth):
        for j in range(nd):
            code |= ((X[j] >> b) & 1) << (b * nd + (nd - 1 - j))
    return code


def hilbert_torch(X, depth):
    """Skilling's AxesToTranspose over int64 tensors: a loop over bits and axes, some hundreds of elementwise launches"""
    X = [x.clone() for x in X]
    nd = len(X)
    Q = 1 << (depth - 1)
    while Q > 1:
        P = Q - 1
        for i in range(nd):
            hit = (X[i] & Q) != 0
            t = (X[0] ^ X[i]) & P
            X[0] = torch.where(hit, X[0] ^ P, X[0] ^ t)
            if i > 0:
                X[i] = torch.where(hit, X[i], X[i] ^ t)
        Q >>= 1
    for i in range(1, nd):
        X[i] = X[i] ^ X[i - 1]
    t = torch.zeros_like(X[0])
    Q = 1 << (depth - 1)
    while Q > 1:
        t = torch.where((X[nd - 1] & Q) != 0, t ^ (Q - 1), t)
        Q >>= 1
    return z_torch([x ^ t for x in X], depth)


def keys_torch(idx, depth, orders):
    cols = [idx[:, c].long() for c in range(idx.shape[1])]
    out = []
    for o in orders:
        X = cols[:0:-1]
        if o.endswith("-trans"):
            X = [X[1], X[0]] + X[2:]
        code = hilbert_torch(X, depth) if o.startswith("hilbert") else z_torch(X, depth)
        out.append((cols[0] << (depth * len(X))) | code)
    return torch.stack(out)


def sort_torch(code, batch, shift=33):
    order = torch.argsort(code, dim=1)
    inverse = torch.zeros_like(order).scatter_(1, order, torch.arange(code.shape[1], device=code.device).repeat(code.shape[0], 1))
    offsets = torch.nn.functional.pad(torch.cumsum(torch.bincount(code[0] >> shift, minlength=batch), 0), (1, 0))
    return order, inverse, offsets


def plan_torch(offsets, K):
    """The padding of Point Transformer V3's patch attention, as its users write it: per-scene slices of two aranges,
    the scene boundaries read back to the host."""
    count = offsets[1:] - offsets[:-1]
    padded = torch.where(count > K, (count + K - 1) // K * K, count)
    off = offsets.tolist()
    off_pad = torch.nn.functional.pad(torch.cumsum(padded, 0), (1, 0)).tolist()
    pad = torch.arange(off_pad[-1], device=offsets.device)
    unpad = torch.arange(off[-1], device=offsets.device)
    for i in range(len(off) - 1):
        unpad[off[i]:off[i + 1]] += off_pad[i] - off[i]
        c = off[i + 1] - off[i]
        if c != off_pad[i + 1] - off_pad[i]:
            pad[off_pad[i + 1] - K + c % K:off_pad[i + 1]] = pad[off_pad[i + 1] - 2 * K + c % K:off_pad[i + 1] - K]
        pad[off_pad[i]:off_pad[i + 1]] -= off_pad[i] - off[i]
    return pad, unpad


def probe(dev, repeats):
    L = _lib.load()
    idx = scene(dev)
    n, ndim = int(idx.shape[0]), 3
    depth = _serialize.default_depth(SHAPE)
    bits = _serialize.key_bits(ndim, depth, BATCH)
    res = {"shape": SHAPE, "batch": BATCH, "rows": n, "depth": depth, "key_bits": bits, "C": C, "dtype": "f16",
           "patch_size": PATCH}
    before = _lib.launch_counts(KEYS)
    ser = Fsp.serialize(idx, SHAPE, BATCH)
    plan = Fsp.patch_plan(ser, PATCH)
    res["launches_of_serialize_and_plan"] = {k: v - before[k] for k, v in _lib.launch_counts(KEYS).items()}
    want = keys_torch(idx, depth, ORDERS)
    res["codes_equal_the_composite"] = bool(torch.equal(ser.code, want))
    c_order, c_inverse, c_offsets = sort_torch(want, BATCH)
    res["orders_equal_the_composite"] = bool(torch.equal(ser.order.long(), c_order) and torch.equal(ser.inverse.long(), c_inverse)
                                             and torch.equal(ser.offsets.long(), c_offsets))
    c_pad, c_unpad = plan_torch(c_offsets, PATCH)
    gather = c_order[0][c_pad]
    res["patches_in_use"] = int(plan.n_patches_dev.item())

    stream = torch.cuda.current_stream().cuda_stream
    code = torch.empty((4, n), dtype=torch.int64, device=dev)
    order = torch.empty((4, n), dtype=torch.int32, device=dev)
    inverse = torch.empty((4, n), dtype=torch.int32, device=dev)
    offsets = torch.empty((BATCH + 1,), dtype=torch.int32, device=dev)
    ws = torch.empty((_serialize.serialize_ws_bytes(n, 4, bits),), dtype=torch.uint8, device=dev)
    codes, axes = _lib.ints([_serialize.ORDERS[o] for o in ORDERS]), _lib.ints([2, 1, 0])

    def native_keys():
        _lib.check(L.spx_curve_keys(idx.data_ptr(), n, None, ndim, BATCH, depth, 4, codes, axes, code.data_ptr(), stream))

    def native_sort(K):
        return lambda: _lib.check(L.spx_serialize(ser.code.data_ptr(), n, K, bits, BATCH, ndim * depth, order.data_ptr(),
                                                  inverse.data_ptr(), offsets.data_ptr(), ws.data_ptr(), ws.numel(), stream))

    feat = torch.randn((n, C), device=dev).half()
    P_cap = int(plan.patch_rows.shape[0])
    g_patches = torch.randn((P_cap, PATCH, C), device=dev).half()
    g_flat = torch.randn((int(gather.shape[0]), C), device=dev).half()
    patches = Fsp.rows_to_patches(feat, plan)
    c_patches = feat[gather]
    g_rows = torch.randn((n, C), device=dev).half()
    back = c_inverse[0]

    stages = {
        "native_keys_4_orders": native_keys,
        "composite_keys_4_orders": lambda: keys_torch(idx, depth, ORDERS),
        "native_sort_1_order": native_sort(1),
        "composite_sort_1_order": lambda: sort_torch(want[:1], BATCH),
        "native_sort_4_orders": native_sort(4),
        "composite_sort_4_orders": lambda: sort_torch(want, BATCH),
        "native_serialize_4_orders": lambda: Fsp.serialize(idx, SHAPE, BATCH),
        "native_plan": lambda: Fsp.patch_plan(ser, PATCH),
        "composite_plan": lambda: plan_torch(c_offsets, PATCH),
        "native_rows_to_patches_fwd": lambda: _serialize.rows_fwd(feat, plan),
        "composite_rows_to_patches_fwd": lambda: feat.index_select(0, gather),
        "native_rows_to_patches_bwd": lambda: _serialize.rows_bwd(g_patches, plan),
        "composite_rows_to_patches_bwd": lambda: torch.zeros_like(feat).index_add_(0, gather, g_flat),
        "native_patches_to_rows_fwd": lambda: _serialize.patches_fwd(patches, plan),
        "composite_patches_to_rows_fwd": lambda: c_patches.index_select(0, c_unpad).index_select(0, back),
        "native_patches_to_rows_bwd": lambda: _serialize.patches_bwd(g_rows, plan),
        "composite_patches_to_rows_bwd": lambda: torch.zeros_like(c_patches).index_add_(
            0, c_unpad, g_rows.index_select(0, c_order[0])),
    }
    for rnd in range(2):                                        # alternate the forms: two rounds each
        for stage, fn in stages.items():
            res[f"{stage}_round{rnd}"] = timed(fn, repeats)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "serialize_probe.json"))
    ap.add_argument("--repeats", type=int, default=30)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("serialize_probe needs the GPU: nothing is measured without one")
    res = {"repeats": args.repeats, "lidar_41x1600x1408": probe(torch.device("cuda:0"), args.repeats)}
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
