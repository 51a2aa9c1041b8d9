"""float64 vs float32 forward + backward of the BASELINE layer (one 3x3x3 SubMConv3d, C = K = 64, 100 k uniform voxels
in the KITTI-shaped grid of bench.py), timed with device events; prints one JSON line.

The f64 step's share of its byte roofline: the compulsory bytes of a forward + backward (features and outputs touched
once, the pair table read once, weights once: the rule of bench.algorithmic_bytes with 8-byte elements, i.e. twice the
f32 bytes of the features, outputs and weights) over the measured HBM copy rate of MI355X_MICROARCH.md (6.29 TB/s).

    python tools/fp64_bench.py [--voxels 100000] [--iters 50] [--warmup 10]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPE = [40, 1280, 1600]
HBM_BYTES_PER_S = 6.29e12


def compulsory_bytes(n, C, K, kv, s):
    fwd = s * n * C + s * n * K + 4 * kv * n + s * kv * C * K
    dgrad = s * n * K + s * n * C + 4 * kv * n + s * kv * C * K
    wgrad = s * n * C + s * n * K + 4 * kv * n + s * kv * C * K
    return fwd + dgrad + wgrad


def time_step(dtype, idx, n, C, K, iters, warmup, dev):
    import spconv_amd.pytorch as spconv
    torch.manual_seed(0)
    net = spconv.SubMConv3d(C, K, 3, bias=False, indice_key="b").to(dev, dtype)
    rng = np.random.default_rng(0)
    feats = torch.from_numpy(rng.uniform(-1, 1, (n, C))).to(dev, dtype).requires_grad_(True)
    gout = torch.from_numpy(rng.uniform(-0.2, 0.2, (n, K))).to(dev, dtype)
    x = spconv.SparseConvTensor(feats, idx, SHAPE, 1)
    # the rulebook is built once, as in a network whose layers share an indice key; the step times the convolution
    y = net(x)
    x = x.replace_feature(feats)
    x.indice_dict = dict(y.indice_dict)

    def step():
        feats.grad, net.weight.grad = None, None
        net(x).features.backward(gout)

    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        step()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times)), float(np.min(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--voxels", type=int, default=100000)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("fp64_bench needs an MI355X (no CPU timing is meaningful)")
    from spconv_amd.utils import synthetic
    dev = torch.device("cuda:0")
    idx_np = synthetic.uniform_scene(SHAPE, args.voxels, 1, 0)
    idx = torch.from_numpy(idx_np).to(dev)
    n, C, K, kv = idx_np.shape[0], 64, 64, 27
    res = {}
    for name, dt in (("f32", torch.float32), ("f64", torch.float64), ("f32_again", torch.float32)):
        med, best = time_step(dt, idx, n, C, K, args.iters, args.warmup, dev)
        res[name] = {"median_ms": round(med, 4), "min_ms": round(best, 4)}
    f64_bytes = compulsory_bytes(n, C, K, kv, 8)
    floor_ms = f64_bytes / HBM_BYTES_PER_S * 1e3
    out = {"layer": "SubMConv3d 3x3x3 C=K=64 fwd+bwd", "voxels": n, **res,
           "f64_over_f32": round(res["f64"]["median_ms"] / res["f32"]["median_ms"], 3),
           "f64_compulsory_bytes": f64_bytes, "f64_byte_floor_ms": round(floor_ms, 4),
           "f64_roofline_fraction": round(floor_ms / res["f64"]["median_ms"], 4)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
