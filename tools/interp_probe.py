#!/usr/bin/env python
"""What does trilinear devoxelisation cost?  4 scenes x 75 000 synthetic points (points jittered inside the voxels of
utils/synthetic.lidar_like_scene) in a 41 x 1600 x 1408 grid, C = 64, f16 and f32: the corner table through the level's
rank map and through the hash table, the forward, the build of the transposed corner list, the backward and the whole
forward + backward on the kernels of csrc/interp.hip, each against the torch composite a user would otherwise write
(spconv.HashTable insert + 8 queries, the weight arithmetic in torch, then the PRESENT corners compacted once and
index_select / mul / index_add_ over them, autograd's index_add_ backward over the same entries), alternating in one
process; the naive dense form ([N, 8, C] index_select / mul / sum with absent corners clamped to row 0) is timed beside it
for the record.  HIP events, 5 warm-up calls, median and minimum of the repeats, two
interleaved rounds; the forward's and the backward's bytes over their time are set against 8 TB/s.

    python tools/interp_probe.py [--out profiles/interp_probe.json] [--repeats 30]
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
import spconv_amd.pytorch as spconv  # noqa: E402
from spconv_amd import _lib  # noqa: E402
from spconv_amd.pytorch import _interp, ops  # noqa: E402
from spconv_amd.pytorch import functional as Fsp  # noqa: E402
from spconv_amd.pytorch.hash import HashTable  # noqa: E402
from spconv_amd.pytorch.utils import StaticPointToVoxel  # noqa: E402
from spconv_amd.utils import synthetic  # noqa: E402

GRID = [41, 1600, 1408]
VSIZE, RANGE = [0.05, 0.05, 0.1], [0.0, -40.0, -3.0, 70.4, 40.0, 1.1]
BATCH, POINTS, VOXELS, C, K = 4, 75_000, 30_000, 64, 8
KEYS = ("interp/corners_ranked", "interp/corners_hash", "interp/fwd", "interp/bwd", "pointvoxel/groups")


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
    """the torch form: a hash table over the level's keys, 8 queries, the weights in torch, index_select / mul / sum"""

    def __init__(self, pts, bids, indices):
        self.pts, self.bids, self.indices = pts, bids.long(), indices
        self.lo = torch.tensor(RANGE[:3], device=pts.device)
        self.vs = torch.tensor(VSIZE, device=pts.device)
        self.ext = torch.tensor(GRID[::-1], device=pts.device)               # xyz

    def key(self, b, xyz):
        return ((b * GRID[0] + xyz[:, 2]) * GRID[1] + xyz[:, 1]) * GRID[2] + xyz[:, 0]

    def corners(self):
        idx, nv = self.indices.long(), self.indices.shape[0]
        table = HashTable(self.pts.device, torch.int32, torch.int32, 2 * nv)
        table.insert(self.key(idx[:, 0], idx[:, 1:].flip(1)).int(), torch.arange(nv, dtype=torch.int32, device=idx.device))
        g = (self.pts[:, :3] - self.lo) / self.vs - 0.5
        base = torch.floor(g)
        f = g - base
        base = base.long()
        rows, weights = [], []
        for c in range(K):
            bit = torch.tensor([(c >> j) & 1 for j in range(3)], device=g.device)
            xyz = base + bit
            inside = ((xyz >= 0) & (xyz < self.ext)).all(dim=1)
            val, missing = table.query(self.key(self.bids, xyz.clamp_min(0).minimum(self.ext - 1)).int())
            ok = inside & ~missing
            w = torch.where(bit.bool(), f, 1.0 - f)
            rows.append(torch.where(ok, val, -1))
            weights.append(torch.where(ok, (w[:, 0] * w[:, 1]) * w[:, 2], 0.0))
        rows, weights = torch.stack(rows, dim=1), torch.stack(weights, dim=1)
        s = weights.sum(dim=1, keepdim=True)
        return rows, torch.where(s > 0, weights / s, 0.0)

    @staticmethod
    def compact(rows, weights):
        """the present corners as flat lists: (point, voxel row, weight) -- part of the composite's corner step"""
        point, corner = torch.nonzero(rows >= 0, as_tuple=True)
        return point, rows[point, corner].long(), weights[point, corner]

    @staticmethod
    def forward_compact(vfeat, entries, n):
        point, row, w = entries
        x = vfeat.index_select(0, row) * w.unsqueeze(1).to(vfeat.dtype)
        return torch.zeros((n, vfeat.shape[1]), dtype=vfeat.dtype, device=vfeat.device).index_add_(0, point, x)

    @staticmethod
    def forward(vfeat, rows, weights):
        """the naive dense form"""
        n, k = rows.shape
        x = vfeat.index_select(0, rows.clamp_min(0).reshape(-1).long()).view(n, k, -1)
        return (x * weights.unsqueeze(2).to(vfeat.dtype)).sum(dim=1)         # (an absent corner carries weight 0)


def grad_of(fwd, x, dout):
    """a callable that runs the backward of fwd(x) alone (the graph is kept)"""
    x = x.detach().requires_grad_(True)
    out = fwd(x)
    return lambda: torch.autograd.grad(out, x, dout, retain_graph=True)


def no_grad(fn):
    def run():
        with torch.no_grad():
            return fn()
    return run


def probe(dev, repeats):
    pts_h, bids_h = scene()
    N = pts_h.shape[0]
    gen = StaticPointToVoxel(VSIZE, RANGE, 4, 160_000, 5, N, batch_size=BATCH, key_order=True, keep_voxels=False, device=dev)
    assert gen.grid_size == GRID, gen.grid_size
    gen(torch.from_numpy(pts_h).to(dev), torch.from_numpy(bids_h).to(dev))
    nv, found = gen.n_voxels.tolist()
    assert nv == found, "the probe's scene must fit the voxeliser"
    pts, bids = gen.points[:N].clone(), gen.batch_ids[:N].clone()
    ranked_idx, plain_idx = gen.indices[:nv].clone(), gen.indices[:nv].clone()
    assert ops.attach_rank_map(ranked_idx, BATCH, GRID), "the voxeliser's level is in key order"
    res = {"grid": GRID, "batch": BATCH, "points": N, "voxels": nv, "C": C, "K": K}
    comp = Composite(pts, bids, plain_idx)
    level = lambda idx, feat: spconv.SparseConvTensor(feat, idx, GRID, BATCH)
    dummy = torch.zeros((nv, 1), device=dev)
    x_rank, x_hash = level(ranked_idx, dummy), level(plain_idx, dummy)
    native_corners = lambda x, groups=False: Fsp.point_corners(pts, bids, x, VSIZE, RANGE, with_groups=groups)

    before = _lib.launch_counts(KEYS)
    c = native_corners(x_rank, True)
    res["launches_of_corners_with_groups"] = {k: v - before[k] for k, v in _lib.launch_counts(KEYS).items()}
    c_hash = native_corners(x_hash)
    assert torch.equal(c.rows, c_hash.rows) and torch.equal(c.weights, c_hash.weights)
    rows_c, w_c = comp.corners()
    assert torch.equal(rows_c, c.rows), "the composite finds other rows"
    entries_c = comp.compact(rows_c, w_c)
    comp_corners = lambda: comp.compact(*comp.corners())
    res["corners_present_per_point"] = round(float((c.rows >= 0).sum()) / N, 3)
    res["weights_max_abs_difference_from_composite"] = float((w_c - c.weights).abs().max())
    entries = int((c.rows >= 0).sum())

    stages = {
        "corners_rank": (no_grad(lambda: native_corners(x_rank)), no_grad(comp_corners)),
        "corners_hash": (no_grad(lambda: native_corners(x_hash)), no_grad(comp_corners)),
        "groups": (lambda: _interp.corner_groups(c.rows, nv), None),           # (the composite's index_add_ needs none)
    }
    naive = {}
    for name, dtype in (("f16", torch.float16), ("f32", torch.float32)):
        vfeat = torch.randn((nv, C), device=dev).to(dtype)
        dout = torch.randn((N, C), device=dev).to(dtype)
        out = Fsp.voxels_to_points_trilinear(vfeat, c)
        alt = comp.forward_compact(vfeat, entries_c, N)
        res[f"forward_max_abs_difference_from_composite_{name}"] = float((out.float() - alt.float()).abs().max())

        def whole_native(vfeat=vfeat, dout=dout):
            v = vfeat.detach().requires_grad_(True)
            cc = native_corners(level(ranked_idx, v), True)
            return torch.autograd.grad(Fsp.voxels_to_points_trilinear(v, cc), v, dout)

        def whole_composite(vfeat=vfeat, dout=dout):
            v = vfeat.detach().requires_grad_(True)
            with torch.no_grad():
                entries = comp_corners()
            return torch.autograd.grad(comp.forward_compact(v, entries, N), v, dout)
        stages.update({
            f"forward_{name}": (no_grad(lambda vfeat=vfeat: Fsp.voxels_to_points_trilinear(vfeat, c)),
                                no_grad(lambda vfeat=vfeat: comp.forward_compact(vfeat, entries_c, N))),
            f"backward_{name}": (grad_of(lambda v: Fsp.voxels_to_points_trilinear(v, c), vfeat, dout),
                                 grad_of(lambda v: comp.forward_compact(v, entries_c, N), vfeat, dout)),
            f"forward_backward_{name}": (whole_native, whole_composite),
        })
        naive[f"forward_{name}"] = no_grad(lambda vfeat=vfeat: comp.forward(vfeat, rows_c, w_c))
        naive[f"backward_{name}"] = grad_of(lambda v: comp.forward(v, rows_c, w_c), vfeat, dout)
    for rnd in range(2):                                        # alternate the forms: two rounds each
        for stage, (native, composite) in stages.items():
            res[f"native_{stage}_round{rnd}"] = timed(native, repeats)
            if composite is not None:
                res[f"composite_{stage}_round{rnd}"] = timed(composite, repeats)
    res["naive_dense_composite_us"] = {k: timed(fn, repeats)["median_us"] for k, fn in naive.items()}
    verdict = {}
    for stage, (_, composite) in stages.items():
        nat = [res[f"native_{stage}_round{r}"]["median_us"] for r in range(2)]
        if composite is None:
            verdict[stage] = {"native_us": nat}
            continue
        com = [res[f"composite_{stage}_round{r}"]["median_us"] for r in range(2)]
        verdict[stage] = {"native_us": nat, "composite_us": com, "native_no_slower": max(nat) <= min(com)}
    for name in ("f16", "f32"):                                 # the native backward WITH the list it needs, against index_add_
        nat = [verdict["groups"]["native_us"][r] + verdict[f"backward_{name}"]["native_us"][r] for r in range(2)]
        com = verdict[f"backward_{name}"]["composite_us"]
        verdict[f"groups_and_backward_{name}"] = {"native_us": [round(v, 1) for v in nat], "composite_us": com,
                                                  "native_no_slower": max(nat) <= min(com)}
    res["verdict"] = verdict
    res["slower_than_composite"] = sorted(k for k, v in verdict.items() if v.get("native_no_slower") is False)

    # bytes over the better median, as a share of 8 TB/s: `unique` counts every row once (what must cross the memory
    # interface at least), `gathered` counts a voxel / point row once per corner that reads it (what the lanes request)
    table = N * K * 8                                           # corner rows + weights
    for name, eb in (("f16", 2), ("f32", 4)):
        fwd_us, bwd_us = min(verdict[f"forward_{name}"]["native_us"]), min(verdict[f"backward_{name}"]["native_us"])
        traffic = {
            f"forward_{name}_unique": (table + nv * C * eb + N * C * eb, fwd_us),
            f"forward_{name}_gathered": (table + entries * C * eb + N * C * eb, fwd_us),
            f"backward_{name}_unique": (entries * 8 + (nv + 1) * 4 + N * C * eb + nv * C * eb, bwd_us),
            f"backward_{name}_gathered": (entries * 8 + (nv + 1) * 4 + entries * C * eb + nv * C * eb, bwd_us),
        }
        for key, (nbytes, us) in traffic.items():
            res[f"{key}_bytes"] = nbytes
            res[f"{key}_TBps"] = round(nbytes / (us * 1e-6) / 1e12, 3)
            res[f"{key}_share_of_8TBps"] = round(nbytes / (us * 1e-6) / 8e12, 4)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=30)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("interp_probe needs the GPU: nothing is measured without one")
    res = {"repeats": args.repeats}
    res.update(probe(torch.device("cuda:0"), args.repeats))
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
