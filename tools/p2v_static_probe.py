#!/usr/bin/env python
"""Points -> backbone output on BASELINE config 4's network (4 scenes of ~100 k voxels each, batch of 4 clouds), two ways:

  parent   PointToVoxel(key_order=True) per cloud (one synchronisation each, torch.argsort + gathers), batch column and
           concatenation, the torch mean `voxels.sum(1) / num`, then a StaticInference replay with its entry sort --
           what a caller had before StaticPointToVoxel; none of that code is changed by it
  static   StaticInference(net, voxelizer=StaticPointToVoxel(...)).run_points(pc, batch_ids): one copy, one replay

and the voxelisers alone.  Host clock around work that ends in a device synchronise (the parent path synchronises
inside); the two paths alternate inside every repeat, the scenes rotate, nothing else may run on the card.
    python tools/p2v_static_probe.py [voxels per cloud] [output json]"""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
import spconv_amd.pytorch as spconv  # noqa: E402
from spconv_amd.pytorch.static import StaticInference, strided_layers  # noqa: E402
from spconv_amd.pytorch.utils import PointToVoxel, StaticPointToVoxel  # noqa: E402
from spconv_amd.utils import nets  # noqa: E402

VSIZE = [0.05, 0.05, 0.1]
RANGE = [0.0, -40.0, -3.0, 70.4, 40.0, 1.1]          # -> the 41 x 1600 x 1408 grid of nets.SECOND_SHAPE
BS, SCENES, MAX_POINTS = 4, 4, 5


def cloud_of(idx, seed):
    """1-3 points inside every voxel of a scene, shuffled: (points [N, 4] fp32, batch ids [N] int32)."""
    rng = np.random.default_rng(seed)
    rep = rng.integers(1, 4, idx.shape[0])
    rows = np.repeat(np.arange(idx.shape[0]), rep)
    rows = rows[rng.permutation(rows.shape[0])]
    zyx = idx[rows, 1:].astype(np.float32) + rng.uniform(0.2, 0.8, (rows.shape[0], 3)).astype(np.float32)
    lo = np.asarray(RANGE[:3], np.float32)
    xyz = zyx[:, ::-1] * np.asarray(VSIZE, np.float32) + lo
    pts = np.concatenate([xyz, rng.uniform(0, 1, (rows.shape[0], 1)).astype(np.float32)], axis=1)
    return pts.astype(np.float32), idx[rows, 0].astype(np.int32)


def timed(fn, repeats, iters):
    """Median and range over `repeats` windows of `iters` calls each, in us per call."""
    out = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(iters):
            fn(i)
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) / iters * 1e6)
    return out


def main():
    voxels = int(sys.argv[1]) if len(sys.argv) > 1 else 100_000
    out_path = sys.argv[2] if len(sys.argv) > 2 else None
    dev = torch.device("cuda:0")
    shape = nets.SECOND_SHAPE
    torch.manual_seed(0)
    net = nets.second_backbone(4).to(dev).half().eval()
    clouds = []
    for si in range(SCENES):
        idx, _ = bench.make_scene("lidar", voxels, seed=si, batch=BS, shape=shape)
        pts, ids = cloud_of(idx, si)
        clouds.append((torch.from_numpy(pts).to(dev), torch.from_numpy(ids).to(dev), idx.shape[0]))
    n_vox = max(c[2] for c in clouds)
    n_pts = max(c[0].shape[0] for c in clouds)
    max_voxels = int(n_vox * 1.05) + 1

    eager_gen = PointToVoxel(VSIZE, RANGE, 4, max_voxels, MAX_POINTS, device=dev, key_order=True)
    assert eager_gen.grid_size == shape, eager_gen.grid_size

    def parent_voxels(pc, ids):
        feats, inds = [], []
        for b in range(BS):
            v, c, n, _ = eager_gen.generate_voxel_with_id(pc[ids == b])
            feats.append((v.sum(1) / n.unsqueeze(1).float()).half())
            inds.append(torch.cat([torch.full_like(c[:, :1], b), c], dim=1))
        return torch.cat(feats), torch.cat(inds).contiguous()

    # bounds of the strided layers: the largest count over the scenes + 10 %
    seen = {}
    hooks = [m.register_forward_hook(lambda mod, a, o, k=k: seen.__setitem__(k, max(seen.get(k, 0), o.features.shape[0])))
             for k, m in strided_layers(net).items()]
    want = []
    with torch.no_grad():
        for pc, ids, _ in clouds:
            f, ind = parent_voxels(pc, ids)
            y = net(spconv.SparseConvTensor(f, ind, shape, BS))
            want.append((y.indices.clone(), y.features.clone()))
    for h in hooks:
        h.remove()
    bounds = {k: int(v * 1.1) + 1 for k, v in seen.items()}

    parent = StaticInference(net, max_voxels, 4, shape, BS, torch.float16, bounds=bounds)
    gen = StaticPointToVoxel(VSIZE, RANGE, 4, max_voxels, MAX_POINTS, int(n_pts * 1.05) + 1, batch_size=BS,
                             key_order=True, mean_dtype=torch.float16, keep_voxels=False, device=dev)
    static = StaticInference(net, max_voxels, 4, shape, BS, torch.float16, bounds=bounds, voxelizer=gen)
    alone = StaticPointToVoxel(VSIZE, RANGE, 4, max_voxels, MAX_POINTS, int(n_pts * 1.05) + 1, batch_size=BS,
                               key_order=True, mean_dtype=torch.float16, keep_voxels=True, device=dev)

    def parent_step(i):
        pc, ids, _ = clouds[i % SCENES]
        return parent(*parent_voxels(pc, ids))

    def static_step(i):
        pc, ids, _ = clouds[i % SCENES]
        return static.run_points(pc, ids)

    # the parent path against the eager pass bit for bit; the static path's coordinates too, its features within fp16
    # noise (its mean adds a voxel's points in point order in fp32, torch's reduction picks its own order; the bit-exact
    # check against a sequential reference is tests/test_gpu_point2voxel_static.py)
    identical, worst = True, 0.0
    for i, (wi, wf) in enumerate(want):
        n = wi.shape[0]
        got = parent_step(i)
        identical &= bool(torch.equal(got.indices[:n], wi) and torch.equal(got.features[:n], wf))
        got = static_step(i)
        identical &= bool(torch.equal(got.indices[:n], wi) and bool((got.indices[n:, 0] < 0).all()))
        worst = max(worst, float((got.features[:n].float() - wf.float()).abs().max() / wf.float().abs().max()))
    identical &= parent.overflowed() == {} and static.overflowed() == {} and worst < 2e-2

    steps = {"parent_points_to_output": parent_step, "static_points_to_output": static_step,
             "parent_voxeliser_and_mean": lambda i: parent_voxels(*clouds[i % SCENES][:2]),
             "static_voxeliser_with_voxels": lambda i: alone(*clouds[i % SCENES][:2]),
             "static_voxeliser_mean_only": lambda i: gen(*clouds[i % SCENES][:2]),
             "replay_with_entry_sort_only": lambda i: parent.graph.replay()}
    for fn in steps.values():
        for i in range(8):
            fn(i)
    repeats, iters = 7, 20
    samples = {k: [] for k in steps}
    for _ in range(repeats):                           # the paths alternate inside every repeat
        for k, fn in steps.items():
            samples[k] += timed(fn, 1, iters)
    result = {"scenes": SCENES, "clouds_per_scene": BS, "voxels_per_scene": [c[2] for c in clouds],
              "points_per_scene": [int(c[0].shape[0]) for c in clouds], "max_voxels": max_voxels,
              "rows_identical_to_the_eager_pass": identical, "static_features_max_rel_diff": worst, "repeats": repeats, "iters_per_repeat": iters,
              "unit": "us per scene, host clock to device synchronise",
              "paths": {k: {"median": round(statistics.median(v), 1), "min": round(min(v), 1), "max": round(max(v), 1)}
                        for k, v in samples.items()}}
    p, s = result["paths"]["parent_points_to_output"], result["paths"]["static_points_to_output"]
    result["static_not_slower_than_parent_within_spread"] = bool(s["median"] <= p["median"] + (p["max"] - p["min"]))
    print(json.dumps(result))
    if out_path:
        with open(out_path, "w") as fh:
            json.dump(result, fh, indent=1)
            fh.write("\n")
    assert identical, "the two paths do not give the eager pass's rows"


if __name__ == "__main__":
    main()
