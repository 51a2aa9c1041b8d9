#!/usr/bin/env python
"""What do the point <-> voxel operations cost?  4 scenes x 75 000 synthetic points (points jittered inside the voxels of
utils/synthetic.lidar_like_scene) in a 41 x 1600 x 1408 grid, C = 64, f16: the groups build, the reductions and their
backwards, the gather and its backward, the decoration and a whole DynamicVFE eval pass on the kernels of
csrc/pointvoxel.hip / csrc/collapse.hip, each against the torch composite a user would otherwise write, alternating in
one process.  HIP events, warm-up, median and minimum of the repeats, two interleaved rounds; the three new kernels'
bytes over their time are set against 8 TB/s.

    python tools/pointvoxel_probe.py [--out profiles/pointvoxel_probe.json] [--repeats 30]
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
from spconv_amd.pytorch import _collapse  # noqa: E402
from spconv_amd.pytorch import functional as Fsp  # noqa: E402
from spconv_amd.pytorch.utils import StaticPointToVoxel  # noqa: E402
from spconv_amd.pytorch.vfe import DynamicVFE  # noqa: E402
from spconv_amd.utils import synthetic  # noqa: E402

GRID = [41, 1600, 1408]
VSIZE, RANGE = [0.05, 0.05, 0.1], [0.0, -40.0, -3.0, 70.4, 40.0, 1.1]
BATCH, POINTS, VOXELS, C = 4, 75_000, 30_000, 64
KEYS = ("pointvoxel/groups", "pointvoxel/gather", "pointvoxel/decorate", "collapse/fwd", "collapse/bwd")


def scene():
    """POINTS points per scene, uniformly jittered inside VOXELS occupied voxels of a lidar-like scene (every point inside
    the range).  -> points fp32 [N, 4] (x, y, z, intensity), batch ids int32 [N]"""
    rng = np.random.default_rng(0)
    idx = synthetic.lidar_like_scene(GRID, VOXELS, BATCH, seed=0)
    pts, bids = [], []
    for b in range(BATCH):
        vox = idx[idx[:, 0] == b][:, 1:]
        pick = vox[rng.integers(0, vox.shape[0], POINTS)]
        frac = rng.uniform(0.05, 0.95, (POINTS, 3))
        xyz = (pick[:, ::-1] + frac) * np.asarray(VSIZE) + np.asarray(RANGE[:3])
        pts.append(np.concatenate([xyz, rng.uniform(0, 1, (POINTS, 1))], axis=1))
        bids.append(np.full((POINTS,), b))
    return np.concatenate(pts).astype(np.float32), np.concatenate(bids).astype(np.int32)


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


class Composite:
    """the torch forms: ids int64 [N] (every point has a voxel), nv voxels"""

    def __init__(self, ids, nv, indices):
        self.ids, self.nv, self.indices = ids, nv, indices
        self.counts = torch.bincount(ids, minlength=nv)

    def groups(self):
        order = torch.argsort(self.ids, stable=True)
        counts = torch.bincount(self.ids, minlength=self.nv)
        return order, torch.cumsum(counts, 0)

    def amax(self, feat):
        out = torch.zeros((self.nv, feat.shape[1]), dtype=feat.dtype, device=feat.device)
        return out.scatter_reduce_(0, self.ids[:, None].expand(-1, feat.shape[1]), feat, "amax", include_self=False)

    def mean(self, feat):
        out = torch.zeros((self.nv, feat.shape[1]), dtype=feat.dtype, device=feat.device).index_add_(0, self.ids, feat)
        return out / self.counts[:, None].to(feat.dtype)

    def gather(self, vfeat, invalid_value=0):
        """utils.gather_features_by_pc_voxel_id as it was: four launches, three [N, C] temporaries"""
        inside = self.ids >= 0
        rows = vfeat.index_select(0, self.ids.clamp_min(0))
        return torch.where(inside.view(-1, 1), rows, torch.full_like(rows, invalid_value))

    def decorate(self, pts, dtype):
        mean = self.mean(pts)
        lo = torch.tensor(RANGE[:3], device=pts.device)
        vs = torch.tensor(VSIZE, device=pts.device)
        cell = self.indices.index_select(0, self.ids)[:, 1:].flip(1).float()
        centre = (cell + 0.5) * vs + lo
        return torch.cat([pts, pts[:, :3] - mean.index_select(0, self.ids)[:, :3], pts[:, :3] - centre], dim=1).to(dtype)

    def vfe(self, mod, pts):
        x = self.decorate(pts, mod.linears[0].weight.dtype)
        voxels = None
        for i, (lin, bn) in enumerate(zip(mod.linears, mod.norms)):
            y = torch.relu(bn(lin(x)))
            voxels = self.amax(y)
            if i + 1 < len(mod.linears):
                x = torch.cat([y, self.gather(voxels)], dim=1)
        return voxels


def grad_of(fwd, x, dout):
    """a callable that runs the backward of fwd(x) alone (the graph is kept)"""
    x = x.detach().requires_grad_(True)
    out = fwd(x)
    return lambda: torch.autograd.grad(out, x, dout, retain_graph=True)


def probe(dev, repeats):
    pts_h, bids_h = scene()
    N = pts_h.shape[0]
    gen = StaticPointToVoxel(VSIZE, RANGE, 4, 160_000, 5, N, batch_size=BATCH, key_order=True, keep_voxels=False, device=dev)
    assert gen.grid_size == GRID, gen.grid_size
    gen(torch.from_numpy(pts_h).to(dev), torch.from_numpy(bids_h).to(dev))
    nv, found = gen.n_voxels.tolist()
    assert nv == found, "the probe's scene must fit the voxeliser"
    ids = gen.pc_voxel_id[:N].clone()
    assert int(ids.min()) >= 0, "every point of the probe's scene lies inside the range"
    pts, indices = gen.points[:N].clone(), gen.indices[:nv].clone()
    res = {"grid": GRID, "batch": BATCH, "points": N, "voxels": nv, "C": C, "dtype": "f16"}
    comp = Composite(ids, nv, indices)

    before = _lib.launch_counts(KEYS)
    g = Fsp.point_groups(ids, nv)
    res["launches_of_one_groups_build"] = {k: v - before[k] for k, v in _lib.launch_counts(KEYS).items()}
    order, ends = comp.groups()
    assert torch.equal(order.int(), g.list) and torch.equal(ends.int(), g.offsets[1:])

    feat = torch.randn((N, C), device=dev).half()
    vfeat = torch.randn((nv, C), device=dev).half()
    dvox = torch.randn((nv, C), device=dev).half()
    dpts = torch.randn((N, C), device=dev).half()
    assert torch.equal(Fsp.points_to_voxels(feat, g, "max"), comp.amax(feat))
    assert torch.equal(Fsp.voxels_to_points(vfeat, g), comp.gather(vfeat))
    torch.manual_seed(0)
    vfe = DynamicVFE(4, (64, 64)).to(dev).half().eval()
    before = _lib.launch_counts(KEYS)
    with torch.no_grad():
        ref = vfe(pts, g, indices, VSIZE, RANGE)
    res["launches_of_one_vfe_pass"] = {k: v - before[k] for k, v in _lib.launch_counts(KEYS).items()}
    with torch.no_grad():
        alt = comp.vfe(vfe, pts)
    res["vfe_max_abs_difference_from_composite"] = float((ref.float() - alt.float()).abs().max())

    def no_grad(fn):
        def run():
            with torch.no_grad():
                return fn()
        return run

    stages = {
        "groups": (lambda: Fsp.point_groups(ids, nv), comp.groups),
        "max_fwd": (no_grad(lambda: Fsp.points_to_voxels(feat, g, "max")), no_grad(lambda: comp.amax(feat))),
        "mean_fwd": (no_grad(lambda: Fsp.points_to_voxels(feat, g, "mean")), no_grad(lambda: comp.mean(feat))),
        "max_bwd": (grad_of(lambda x: Fsp.points_to_voxels(x, g, "max"), feat, dvox), grad_of(comp.amax, feat, dvox)),
        "mean_bwd": (grad_of(lambda x: Fsp.points_to_voxels(x, g, "mean"), feat, dvox), grad_of(comp.mean, feat, dvox)),
        "gather_fwd": (no_grad(lambda: Fsp.voxels_to_points(vfeat, g)), no_grad(lambda: comp.gather(vfeat))),
        "gather_bwd": (grad_of(lambda v: Fsp.voxels_to_points(v, g), vfeat, dpts), grad_of(comp.gather, vfeat, dpts)),
        "decorate": (no_grad(lambda: Fsp.decorate_points(pts, g, indices, VSIZE, RANGE, dtype=torch.float16)),
                     no_grad(lambda: comp.decorate(pts, torch.float16))),
        "vfe_eval": (no_grad(lambda: vfe(pts, g, indices, VSIZE, RANGE)), no_grad(lambda: comp.vfe(vfe, pts))),
    }
    for rnd in range(2):                                        # alternate the forms: two rounds each
        for stage, (native, composite) in stages.items():
            res[f"native_{stage}_round{rnd}"] = timed(native, repeats)
            res[f"composite_{stage}_round{rnd}"] = timed(composite, repeats)
    verdict = {}
    for stage in stages:
        nat = [res[f"native_{stage}_round{r}"]["median_us"] for r in range(2)]
        com = [res[f"composite_{stage}_round{r}"]["median_us"] for r in range(2)]
        verdict[stage] = {"native_us": nat, "composite_us": com, "native_no_slower": max(nat) <= min(com)}
    res["verdict"] = verdict

    # bytes the three new kernels must move, over the better median, as a share of 8 TB/s
    cluster = _collapse.fwd(pts, g, "mean")
    mean_only = timed(lambda: _collapse.fwd(pts, g, "mean"), repeats)["median_us"]
    raw = lambda: _lib.check(_lib.load().spx_point_decorate(
        pts.data_ptr(), 4, N, g.rows.data_ptr(), indices.data_ptr(), 3, *gen._host[:2], cluster.data_ptr(), 3,
        deco_out.data_ptr(), _lib.DTYPE_F16, 10, torch.cuda.current_stream().cuda_stream))
    deco_out = torch.empty((N, 10), dtype=torch.float16, device=dev)
    deco_kernel = timed(raw, repeats)["median_us"]
    res["decorate_kernel_alone_us"], res["cluster_mean_alone_us"] = deco_kernel, mean_only
    traffic = {
        "groups": (N * 8 + N * 4 * 2 + (nv + 1) * 4, min(verdict["groups"]["native_us"])),      # ids in; rows, list, offsets out
        "gather": (N * 4 + 2 * N * C * 2, min(verdict["gather_fwd"]["native_us"])),              # rows; voxel rows in, point rows out
        "decorate": (N * (16 + 4 + 12 + 12 + 20), deco_kernel),      # point, row, mean xyz, index row, the f16 row out
    }
    for name, (nbytes, us) in traffic.items():
        res[f"{name}_bytes"] = nbytes
        res[f"{name}_TBps"] = round(nbytes / (us * 1e-6) / 1e12, 3)
        res[f"{name}_share_of_8TBps"] = round(nbytes / (us * 1e-6) / 8e12, 4)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=30)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pointvoxel_probe needs the GPU: nothing is measured without one")
    res = {"repeats": args.repeats}
    res.update(probe(torch.device("cuda:0"), args.repeats))
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
