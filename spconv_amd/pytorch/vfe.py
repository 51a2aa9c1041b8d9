"""Learned voxel feature encoders over the point <-> voxel kernels (csrc/pointvoxel.hip, csrc/collapse.hip).

Not part of the reference: spconv stops at the voxeliser, and the detection code bases that use it (OpenPCDet,
mmdet3d) write this step with ``torch_scatter``."""
from __future__ import annotations

from typing import Sequence

import torch
from torch import nn

from spconv_amd.pytorch import _pointvoxel


class DynamicVFE(nn.Module):
    """Dynamic voxel feature encoder (the DynamicVFE / DynamicPillarVFE of OpenPCDet and mmdet3d; NOT part of the
    reference): every point of a voxel takes part, not the first few.

        gen = StaticPointToVoxel(...) or PointToVoxel(...)
        groups = gen.point_groups()  /  F.point_groups(pc_voxel_id, num_voxels)
        vfe = DynamicVFE(4, channels=(32, 64))
        feats = vfe(points, groups, indices, vsize_xyz, coors_range_xyz)        # [num_voxels, 64]

    The points are decorated (``decorate_points``: the point, its offset from the voxel's cluster mean with
    `with_cluster`, from the voxel centre with `with_center`); every layer is ``Linear(bias = not norm)`` ->
    ``BatchNorm1d`` (with `norm`) -> ``ReLU`` on the point rows, then ``points_to_voxels(reduce)``; between layers the
    reduced rows go back to their points (``voxels_to_points``) and are concatenated onto the point rows.  The linear
    layers and norms are torch's; the reductions, the gather and their gradients are the library's kernels: no atomics,
    ascending point index, identical run to run.  In training, BatchNorm statistics see the points that have a voxel
    only (a data-dependent selection: eager).  In eval mode nothing is read back, so the pass can be captured
    (``StaticInference(net, ..., voxelizer=gen, point_encoder=vfe)``); a point without a voxel then rides along and
    reaches no voxel.  `indices` holds the batch index, then zyx: a voxeliser whose index rows are zyx only
    (``PointToVoxel``) needs the batch column in front."""

    def __init__(self, num_point_features: int, channels: Sequence[int] = (64,), ndim: int = 3, reduce: str = "max",
                 with_cluster: bool = True, with_center: bool = True, norm: bool = True):
        super().__init__()
        from spconv_amd.pytorch import _collapse
        if reduce not in _collapse.OPS:
            raise ValueError(f"DynamicVFE: reduce must be 'sum', 'mean' or 'max', got {reduce!r}")
        channels = [int(c) for c in channels]
        if not channels or min(channels) < 1:
            raise ValueError(f"DynamicVFE: channels must name at least one positive width, got {channels}")
        if int(num_point_features) < int(ndim) or not 1 <= int(ndim) <= 4:
            raise ValueError(f"DynamicVFE: points carry at least ndim = {ndim} columns (ndim in [1, 4])")
        self.num_point_features, self.ndim, self.reduce = int(num_point_features), int(ndim), reduce
        self.with_cluster, self.with_center, self.norm = bool(with_cluster), bool(with_center), bool(norm)
        self.in_channels = self.num_point_features + self.ndim * (int(self.with_cluster) + int(self.with_center))
        self.out_channels = channels[-1]
        self.linears, self.norms = nn.ModuleList(), nn.ModuleList()
        width = self.in_channels
        for c in channels:
            self.linears.append(nn.Linear(width, c, bias=not self.norm))
            self.norms.append(nn.BatchNorm1d(c, eps=1e-3, momentum=0.01) if self.norm else nn.Identity())
            width = 2 * c

    def forward(self, points: torch.Tensor, groups: _pointvoxel.PointGroups, indices: torch.Tensor,
                vsize_xyz: Sequence[float], coors_range_xyz: Sequence[float]) -> torch.Tensor:
        dtype = self.linears[0].weight.dtype        # (float64 weights: the decoration is fp32 arithmetic, widened)
        x = _pointvoxel.decorate_points(points, groups, indices, vsize_xyz, coors_range_xyz, cluster=self.with_cluster,
                                        center=self.with_center,
                                        dtype=dtype if dtype in _pointvoxel._OUT_DTYPES else torch.float32).to(dtype)
        real = None
        if self.training and self.norm:
            real = (groups.rows >= 0).nonzero().squeeze(1)
        voxels = None
        for i, (lin, bn) in enumerate(zip(self.linears, self.norms)):
            y = lin(x)
            if real is not None:        # statistics over the real points; the others stay zero and reach no voxel
                y = torch.zeros_like(y).index_copy(0, real, torch.relu(bn(y.index_select(0, real))))
            else:
                y = torch.relu(bn(y))
            voxels = _pointvoxel.points_to_voxels(y, groups, self.reduce)
            if i + 1 < len(self.linears):
                x = torch.cat([y, _pointvoxel.voxels_to_points(voxels, groups)], dim=1)
        return voxels
