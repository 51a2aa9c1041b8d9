"""Point cloud -> voxel conversion (reference: ``spconv/pytorch/utils.py:23-200``).

``PointToVoxel`` keeps the reference's constructor and call signatures and its conventions:
parameters are given in XYZ order, the returned ``indices`` are ZYX (``docs/USAGE.md:222``),
voxels are numbered in first-seen point order and keep their first
``max_num_points_per_voxel`` points -- exactly what the reference's CPU generator produces
(``csrc/sparse/pointops.py``), here computed on the GPU by ``spx_point2voxel``."""
from __future__ import annotations

import ctypes
from typing import List, Optional, Union

import numpy as np
import torch

from spconv_amd import _lib, constants


def calc_point2voxel_meta_data(vsize_xyz: List[float], coors_range_xyz: List[float]):
    """(vsize, grid_size, grid_stride, coors_range) in ZYX order -- Point2VoxelCommon::calc_meta_data
    (csrc/sparse/pointops.py, all.py:1349-1386): float32 arithmetic, std::round."""
    ndim = len(vsize_xyz)
    assert len(coors_range_xyz) == 2 * ndim, "your params size not equal to ndim"
    vs = np.asarray(vsize_xyz, dtype=np.float32)[::-1].copy()
    lo = np.asarray(coors_range_xyz[:ndim], dtype=np.float32)[::-1].copy()
    hi = np.asarray(coors_range_xyz[ndim:], dtype=np.float32)[::-1].copy()
    q = (hi - lo) / vs                                   # float32 division, like the C++
    grid = np.where(q >= 0, np.floor(q + np.float32(0.5)), np.ceil(q - np.float32(0.5))).astype(np.int64)
    stride, prod = [0] * ndim, 1
    for i in range(ndim - 1, -1, -1):
        stride[i] = prod
        prod *= int(grid[i])
    return ([float(v) for v in vs], [int(v) for v in grid], stride,
            [float(v) for v in lo] + [float(v) for v in hi])


class PointToVoxel(object):
    """WARNING: you MUST construct PointToVoxel AFTER set device.

    A point with a non-finite coordinate (NaN, +inf, -inf) is outside the range: it makes no voxel and its
    ``pc_voxel_id`` is -1; non-finite values in the feature columns behind the coordinates are stored as they are."""

    def __init__(self, vsize_xyz: List[float], coors_range_xyz: List[float], num_point_features: int,
                 max_num_voxels: int, max_num_points_per_voxel: int,
                 device: torch.device = torch.device("cuda:0"), key_order: bool = False):
        # key_order (not in the reference, pytorch/utils.py:23-160, whose voxels come out in point / hash-slot order):
        # voxels numbered by ascending (z, y, x) key instead of by their first point -- the order the first level of a
        # backbone wants (sort_voxels_by_coordinate below; DESIGN.md sections 3.15 / 3.17).  Scenes concatenated in
        # batch order stay in key order; pc_voxel_id follows the renumbering.
        self.key_order = bool(key_order)
        self.ndim = len(vsize_xyz)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise NotImplementedError("spconv_amd runs on MI355X only: construct PointToVoxel with a "
                                      "cuda device (there is no CPU path)")
        vsize, grid_size, grid_stride, coors_range = calc_point2voxel_meta_data(vsize_xyz, coors_range_xyz)
        self.num_point_features = num_point_features
        self.max_num_voxels = max_num_voxels
        self.max_num_points_per_voxel = max_num_points_per_voxel
        self.vsize = vsize
        self.grid_size = grid_size
        self.grid_stride = grid_stride
        self.coors_range = coors_range
        self.voxels = torch.zeros([max_num_voxels, max_num_points_per_voxel, num_point_features],
                                  dtype=torch.float32, device=self.device)
        self.indices = torch.zeros([max_num_voxels, self.ndim], dtype=torch.int32, device=self.device)
        self.num_per_voxel = torch.zeros([max_num_voxels], dtype=torch.int32, device=self.device)

    def __call__(self, pc: torch.Tensor, clear_voxels: bool = True, empty_mean: bool = False):
        """pc [N, 3+] -> (voxels, indices (zyx), num_per_voxel)."""
        res = self.generate_voxel_with_id(pc, clear_voxels, empty_mean)
        return res[0], res[1], res[2]

    def generate_voxel_with_id(self, pc: torch.Tensor, clear_voxels: bool = True,
                               empty_mean: bool = False):
        """-> (voxels, indices, num_per_voxel, pc_voxel_id [N] int64, -1 for dropped points)."""
        assert pc.device.type == self.device.type, "your pc device is wrong"
        assert pc.ndim == 2 and pc.shape[1] == self.num_point_features, \
            "your points num features doesn't equal to voxel."
        if pc.is_cuda and pc.device.index != torch.cuda.current_device():
            with torch.cuda.device(pc.device):         # DeviceGuard convention (ops._on_device)
                return self.generate_voxel_with_id(pc, clear_voxels, empty_mean)
        L = _lib.load()
        with torch.no_grad():
            pc = pc.contiguous().float()
            n = pc.shape[0]
            pc_voxel_id = torch.empty([n], dtype=torch.int64, device=pc.device)
            ws = torch.empty((max(int(L.spx_point2voxel_ws_bytes(n, self.max_num_voxels)), 16),),
                             dtype=torch.uint8, device=pc.device)
            nv = ctypes.c_int(0)
            f = lambda v: (ctypes.c_float * len(v))(*v)
            _lib.check(L.spx_point2voxel(
                pc.data_ptr(), n, self.num_point_features, self.ndim, f(self.vsize), f(self.coors_range),
                _lib.ints(self.grid_size), self.max_num_voxels, self.max_num_points_per_voxel,
                (2 if constants.REFERENCE_QUIRKS else 1) if empty_mean else 0, int(clear_voxels),
                self.voxels.data_ptr(), self.indices.data_ptr(),
                self.num_per_voxel.data_ptr(), pc_voxel_id.data_ptr(), ctypes.byref(nv), ws.data_ptr(),
                ws.numel(), torch.cuda.current_stream(pc.device).cuda_stream))
            num_voxels = int(nv.value)
            if self.key_order and num_voxels > 1:
                idx = self.indices[:num_voxels]
                key = idx[:, 0].to(torch.int64)
                for d in range(1, self.ndim):          # (indices and grid_size are both in zyx order)
                    key = key * int(self.grid_size[d]) + idx[:, d].to(torch.int64)
                order = torch.argsort(key)
                rank = torch.empty_like(order)
                rank[order] = torch.arange(num_voxels, device=order.device)
                pc_voxel_id = torch.where(pc_voxel_id >= 0, rank[pc_voxel_id.clamp_min(0)], pc_voxel_id)
                return (self.voxels[:num_voxels][order].contiguous(), idx[order].contiguous(),
                        self.num_per_voxel[:num_voxels][order].contiguous(), pc_voxel_id)
            return (self.voxels[:num_voxels].clone(), self.indices[:num_voxels].clone(),
                    self.num_per_voxel[:num_voxels].clone(), pc_voxel_id)


class StaticPointToVoxel(object):
    """The voxeliser with static shapes (``spx_point2voxel_static``; not in the reference): points in, key-ordered
    voxels and their mean feature rows out, nothing read back -- so it can be recorded in a stream capture, in front of a
    captured backbone pass (``StaticInference(net, ..., voxelizer=...)``).

        gen = StaticPointToVoxel([0.1, 0.1, 0.2], [0, -40, -3, 70.4, 40, 1], 4, max_num_voxels=120_000,
                                 max_num_points_per_voxel=5, max_num_points=300_000, mean_dtype=torch.float16)
        voxels, indices, num_per_voxel, pc_voxel_id = gen(pc)      # the static buffers, full length
        gen.mean, gen.n_voxels                                      # [max_num_voxels, F]; device {kept, found}

    The object owns every buffer -- points, batch ids, the point count, all outputs, the scratch -- and allocates nothing
    per call.  ``load(pc, batch_ids=None)`` copies one batch of points in (stream-ordered; more than ``max_num_points``
    raises ValueError), ``run(empty_mean=False)`` is the one C call, ``__call__`` does both.  Rows behind the voxels
    kept come out DEAD on every call: -1 in every column of ``indices`` ([max_num_voxels, ndim + 1]: batch index, then
    zyx -- what a SparseConvTensor takes), count 0, zeros in ``voxels`` and ``mean``: the padding contract of
    ``spconv_amd.pytorch.static``.  ``n_voxels`` stays on the device; ``overflowed()`` reads it (one synchronisation).

    ``key_order=True`` (default): voxels numbered by ascending coordinate key (batch-major, last axis fastest) -- the set
    kept at the cap is still the first ``max_num_voxels`` in first-seen order -- and ``indices`` carries the level's rank
    map as its tag, the way ``ops.key_argsort(..., rank_map=True)`` attaches it: the SubM layers of the first level build
    their rulebooks without a hash table.  A grid whose key space has no rank map (``batch_size`` x grid beyond 0xffe00000
    cells, or beyond the size gates of ``ops.attach_rank_map``) raises ValueError: construct with ``key_order=False``
    (first-seen numbering, as ``PointToVoxel``) and let the runner sort.
    ``mean_dtype`` (float32 / float16 / bfloat16, None = no mean): ``mean[v]`` = the stored points of voxel v added in
    point order in fp32, divided by their number in fp32, rounded to nearest-even.  ``keep_voxels=False`` drops the
    ``[max_num_voxels, max_num_points_per_voxel, F]`` tensor (``voxels`` is None) when only the mean is wanted."""

    def __init__(self, vsize_xyz: List[float], coors_range_xyz: List[float], num_point_features: int,
                 max_num_voxels: int, max_num_points_per_voxel: int, max_num_points: int, batch_size: int = 1,
                 key_order: bool = True, mean_dtype: Optional[torch.dtype] = None, keep_voxels: bool = True,
                 device: torch.device = torch.device("cuda:0")):
        from spconv_amd.pytorch import _rulebook
        self.ndim = len(vsize_xyz)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise NotImplementedError("spconv_amd runs on MI355X only: construct StaticPointToVoxel with a "
                                      "cuda device (there is no CPU path)")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        if min(int(max_num_voxels), int(max_num_points_per_voxel), int(max_num_points), int(batch_size)) < 1:
            raise ValueError("max_num_voxels, max_num_points_per_voxel, max_num_points and batch_size must be positive")
        if mean_dtype is not None and mean_dtype not in (torch.float32, torch.float16, torch.bfloat16):
            raise ValueError(f"mean_dtype must be float32, float16 or bfloat16, got {mean_dtype}")
        vsize, grid_size, grid_stride, coors_range = calc_point2voxel_meta_data(vsize_xyz, coors_range_xyz)
        self.num_point_features = int(num_point_features)
        self.max_num_voxels = int(max_num_voxels)
        self.max_num_points_per_voxel = int(max_num_points_per_voxel)
        self.max_num_points = int(max_num_points)
        self.batch_size = int(batch_size)
        self.key_order = bool(key_order)
        self.mean_dtype = mean_dtype
        self.vsize, self.grid_size, self.grid_stride, self.coors_range = vsize, grid_size, grid_stride, coors_range
        self.vsize_xyz, self.coors_range_xyz = [float(v) for v in vsize_xyz], [float(v) for v in coors_range_xyz]
        self._groups = None
        self._corners = {}          # point_corners(): outputs and scratch by (level, options)
        L = _lib.load()
        grid_c = _lib.ints(grid_size)
        rank_bytes = 0
        if self.key_order:
            cells = _rulebook._cells(self.batch_size, grid_size)
            rank_bytes = int(L.spx_rankmap_bytes(self.ndim, self.batch_size, grid_c)) if cells <= 0xffe00000 else 0
            if not _rulebook._rankmap_fits(rank_bytes, cells, self.max_num_voxels):
                raise ValueError(f"key_order=True numbers voxels through the level's rank map, and {self.batch_size} x "
                                 f"{grid_size} ({cells} cells for {self.max_num_voxels} voxels) has none: construct "
                                 f"with key_order=False")
        ws_bytes = int(L.spx_point2voxel_static_ws_bytes(self.max_num_points, self.max_num_voxels, self.ndim,
                                                         self.batch_size, grid_c, int(self.key_order)))
        if ws_bytes == 0:
            raise ValueError(f"no static voxeliser for {self.batch_size} x {grid_size} with key_order={self.key_order}")
        with torch.cuda.device(self.device):
            new = dict(device=self.device)
            self.points = torch.zeros([self.max_num_points, self.num_point_features], dtype=torch.float32, **new)
            self.batch_ids = torch.zeros([self.max_num_points], dtype=torch.int32, **new)
            self.n_points = torch.zeros([1], dtype=torch.int32, **new)
            self.voxels = (torch.zeros([self.max_num_voxels, self.max_num_points_per_voxel, self.num_point_features],
                                       dtype=torch.float32, **new) if keep_voxels else None)
            self.indices = torch.full([self.max_num_voxels, self.ndim + 1], -1, dtype=torch.int32, **new)
            self.num_per_voxel = torch.zeros([self.max_num_voxels], dtype=torch.int32, **new)
            self.pc_voxel_id = torch.full([self.max_num_points], -1, dtype=torch.int64, **new)
            self.n_voxels = torch.zeros([2], dtype=torch.int32, **new)          # {kept, found}
            self.mean = (None if mean_dtype is None else
                         torch.zeros([self.max_num_voxels, self.num_point_features], dtype=mean_dtype, **new))
            self._ws = torch.empty([ws_bytes], dtype=torch.uint8, **new)
            self._rankmap = torch.zeros([rank_bytes // 4], dtype=torch.int32, **new) if self.key_order else None
        if self._rankmap is not None:       # (behind the last in-place write of `indices`: the tag records its version)
            _rulebook._tag_rank_map(self.indices, self._rankmap, self.batch_size, grid_size, self.max_num_voxels)
        self._ids_loaded = False
        f = lambda v: (ctypes.c_float * len(v))(*v)
        self._host = (f(vsize), f(coors_range), grid_c)        # host arrays of the call, made once
        self._L = L

    def load(self, pc: torch.Tensor, batch_ids: Optional[torch.Tensor] = None) -> None:
        """Copies one batch of points (and the scene index of each, default scene 0) into the static buffers:
        stream-ordered, no synchronisation."""
        assert pc.ndim == 2 and pc.shape[1] == self.num_point_features, \
            "your points num features doesn't equal to voxel."
        n = pc.shape[0]
        if n > self.max_num_points:
            raise ValueError(f"{n} points, the buffers were sized for at most {self.max_num_points}")
        with torch.cuda.device(self.device), torch.no_grad():
            self.points[:n].copy_(pc, non_blocking=True)
            if batch_ids is not None:
                assert batch_ids.shape == (n,), "one batch index per point"
                self.batch_ids[:n].copy_(batch_ids, non_blocking=True)
                self._ids_loaded = True
            elif self._ids_loaded:
                self.batch_ids.zero_()
                self._ids_loaded = False
            self.n_points.fill_(n)

    def run(self, empty_mean: bool = False) -> None:
        """The one C call over whatever `load` left in the buffers: no allocation, nothing read back."""
        if empty_mean and self.voxels is None:
            raise ValueError("empty_mean fills the unused slots of `voxels`: construct with keep_voxels=True")
        p = lambda t: None if t is None else t.data_ptr()
        vsize, coors_range, grid = self._host
        _lib.check(self._L.spx_point2voxel_static(
            self.points.data_ptr(), self.batch_ids.data_ptr(), self.max_num_points, self.n_points.data_ptr(),
            self.num_point_features, self.ndim, vsize, coors_range, grid, self.batch_size, self.max_num_voxels,
            self.max_num_points_per_voxel, int(bool(empty_mean)), int(self.key_order), p(self.voxels),
            self.indices.data_ptr(), self.num_per_voxel.data_ptr(), self.pc_voxel_id.data_ptr(),
            self.n_voxels.data_ptr(), p(self.mean),
            0 if self.mean is None else {torch.float32: _lib.DTYPE_F32, torch.float16: _lib.DTYPE_F16,
                                         torch.bfloat16: _lib.DTYPE_BF16}[self.mean.dtype],
            p(self._rankmap), 0 if self._rankmap is None else self._rankmap.numel() * 4,
            self._ws.data_ptr(), self._ws.numel(), torch._C._cuda_getCurrentRawStream(self.device.index)))

    def __call__(self, pc: torch.Tensor, batch_ids: Optional[torch.Tensor] = None, empty_mean: bool = False):
        """pc [N, F] -> (voxels, indices, num_per_voxel, pc_voxel_id): the static buffers, full length (rows behind
        ``n_voxels[0]`` dead, ``pc_voxel_id`` -1 behind the N points)."""
        self.load(pc, batch_ids)
        with torch.cuda.device(self.device):
            self.run(empty_mean)
        return self.voxels, self.indices, self.num_per_voxel, self.pc_voxel_id

    def point_groups(self):
        """The points of every voxel of the last ``run()`` as ``functional.PointGroups`` (``spx_point_groups`` over the
        object's own ``pc_voxel_id``, ``n_points`` and ``n_voxels[0:1]``): what ``points_to_voxels``, ``voxels_to_points``
        and ``vfe.DynamicVFE`` take.  Its outputs and scratch are allocated once, at first use, so the call can be
        recorded in a stream capture behind ``run()``.  (The points are sorted a second time: the voxeliser's own
        sorted list stays private in its scratch.)"""
        from spconv_amd.pytorch import _pointvoxel
        with torch.cuda.device(self.device):
            if self._groups is None:
                i32 = dict(dtype=torch.int32, device=self.device)
                ws = torch.empty([max(int(self._L.spx_point_groups_ws_bytes(self.max_num_points, self.max_num_voxels)), 16)],
                                 dtype=torch.uint8, device=self.device)
                self._groups = (_pointvoxel.PointGroups(
                    torch.full([self.max_num_points], -1, **i32), torch.zeros([self.max_num_voxels + 1], **i32),
                    torch.zeros([self.max_num_points], **i32), self.max_num_voxels, self.n_points, self.n_voxels[0:1]), ws)
            g, ws = self._groups
            _pointvoxel.point_groups_into(self.pc_voxel_id, self.max_num_voxels, self.n_points, g.rows, g.offsets, g.list, ws)
        return g

    def point_corners(self, x=None, vsize_xyz=None, normalize: bool = True, with_groups: bool = False):
        """The trilinear corner table of the last ``run()``'s points as ``functional.PointCorners``
        (``spx_point_corners`` over the object's own ``points``, ``batch_ids`` and ``n_points``): what
        ``functional.voxels_to_points_trilinear`` takes.  By default the corners are taken against the voxeliser's own
        level, through the rank map it leaves behind (``key_order=True``) or a hash table built from ``indices``; `x` (a
        SparseConvTensor over the same range, e.g. a strided level) with `vsize_xyz` = that level's voxel size reads
        another one.  ``with_groups=True`` adds the transposed list a gradient in the voxel rows walks.  Outputs and
        scratch are allocated once per (index tensor, level shape, normalize, with_groups), at first use -- a second call
        with the same four overwrites the first one's result -- so the call can be recorded in a stream
        capture behind ``run()``.  No gradient with respect to the points."""
        from spconv_amd.pytorch import _interp, _level, _pointvoxel
        if x is None:
            indices, shape, B, n_live = self.indices, list(self.grid_size), self.batch_size, self.n_voxels[0:1]
            vsize_xyz = self.vsize_xyz if vsize_xyz is None else vsize_xyz
        else:
            if vsize_xyz is None:
                raise ValueError("point_corners: a level other than the voxeliser's own needs its voxel size (vsize_xyz)")
            indices, shape, B = x.indices, [int(v) for v in x.spatial_shape], int(x.batch_size)
            n_live = getattr(x, "n_live_dev", None)
        ndim, vsize, coors_range = _level._geometry(vsize_xyz, self.coors_range_xyz)
        if ndim != self.ndim or len(shape) != ndim or B != self.batch_size:
            raise ValueError("point_corners: the level does not match the voxeliser's dimensions or batch size")
        n, K, N = int(indices.shape[0]), 1 << ndim, self.max_num_points
        with torch.cuda.device(self.device):
            rankmap = _level.level_rankmap(indices, B, shape)
            key = (indices.data_ptr(), tuple(shape), n, rankmap is None, bool(normalize), bool(with_groups))
            cache = self._corners
            if key not in cache:
                i32 = dict(dtype=torch.int32, device=self.device)
                u8 = lambda nbytes: torch.empty([max(int(nbytes), 16)], dtype=torch.uint8, device=self.device)
                rows = torch.full([N, K], -1, **i32)
                weights = torch.zeros([N, K], dtype=torch.float32, device=self.device)
                ws = u8(_interp.corners_ws_bytes(N, ndim, n)) if rankmap is None else None
                groups = None
                if with_groups and n > 0:
                    groups = (_pointvoxel.PointGroups(torch.full([N * K], -1, **i32), torch.zeros([n + 1], **i32),
                                                      torch.zeros([N * K], **i32), n, None, n_live),
                              u8(self._L.spx_point_groups_ws_bytes(N * K, n)))
                cache[key] = (rows, weights, ws, groups)
            rows, weights, ws, groups = cache[key]
            _interp.point_corners_into(self.points, self.batch_ids, self.n_points, _level._floats(vsize),
                                       _level._floats(coors_range), indices, n_live, B, shape, rankmap, normalize, rows,
                                       weights, ws)
            g = None
            if groups is not None:
                g, gws = groups
                g = g._replace(n_live=n_live)
                _pointvoxel.point_groups_into(rows.view(-1), n, None, g.rows, g.offsets, g.list, gws)
        return _interp.PointCorners(rows, weights, g, n, self.n_points, n_live)

    def overflowed(self) -> bool:
        """True when the last run found more voxels than ``max_num_voxels`` (one synchronisation)."""
        kept, found = self.n_voxels.tolist()
        return found > kept


def gather_features_by_pc_voxel_id(seg_res_features: torch.Tensor, pc_voxel_id: torch.Tensor,
                                   invalid_value: Union[int, float] = 0):
    """Per-voxel results back to the points: row i of the result is the row of point i's voxel,
    `invalid_value` for points that fell outside the grid (pc_voxel_id == -1).  Same contract as
    the reference helper (spconv/pytorch/utils.py:163-176).

    CUDA rows [num_voxels, C] of 1, 2, 4 or 8 bytes per element go through ``functional.voxels_to_points``: one launch
    (spx_voxel_to_point) instead of four and three [N, C] temporaries, and a gradient that is a segment sum in ascending
    point index instead of ``index_add_``'s float atomics.  Other inputs take the composite below."""
    ids = pc_voxel_id.to(seg_res_features.device)
    if (seg_res_features.is_cuda and seg_res_features.ndim == 2 and ids.ndim == 1
            and ids.dtype in (torch.int64, torch.int32) and not seg_res_features.is_quantized
            and not seg_res_features.is_complex() and seg_res_features.element_size() in (1, 2, 4, 8)
            and seg_res_features.shape[0] > 0 and seg_res_features.shape[1] > 0):
        from spconv_amd.pytorch import _pointvoxel
        num_voxels = int(seg_res_features.shape[0])
        if seg_res_features.requires_grad and torch.is_grad_enabled() and seg_res_features.is_floating_point():
            groups = _pointvoxel.point_groups(ids, num_voxels)      # (the gradient walks the groups)
        else:
            groups = _pointvoxel.PointGroups(ids.to(torch.int32), None, None, num_voxels)
        return _pointvoxel.voxels_to_points(seg_res_features, groups, invalid_value)
    inside = ids >= 0
    rows = seg_res_features.index_select(0, ids.clamp_min(0))
    shape = [-1] + [1] * (seg_res_features.ndim - 1)
    fill = torch.full_like(rows, invalid_value)
    return torch.where(inside.view(shape), rows, fill)


def _row_keys(indices: torch.Tensor, spatial_shape) -> torch.Tensor:
    key = indices[:, 0].to(torch.int64)
    for d, s in enumerate(spatial_shape):
        key = key * int(s) + indices[:, 1 + d].to(torch.int64)
    return key


def sort_voxels_by_coordinate(indices: torch.Tensor, spatial_shape: List[int], *row_tensors: torch.Tensor,
                              batch_size: int = 0, rank_map: bool = True):
    """Rows in ascending coordinate-key order (batch-major, last axis fastest): ``(indices, *row_tensors, order)``.

    Not part of the reference's API.  The FIRST level of a backbone runs in the order the caller hands over; a
    voxeliser returns voxels in point or hash-slot order, i.e. shuffled in space.  Every gather of a level is cheaper when
    x-neighbours sit in adjacent rows (on the 4 x 100 k voxel level of BASELINE config 4 a SubM
    forward takes 40 instead of 49 us, its backward 84 instead of 96): a data loader that sorts once gives the first level
    what the layer modules give every level behind a strided layer.  ``order`` maps sorted rows to input rows
    (``x_sorted = x[order]``) for carrying labels along.

    ``rank_map=True`` with ``batch_size`` given (CUDA tensors): the sorted index tensor additionally carries the level's
    rank map (``ops.attach_rank_map``: row = rank, built by one pass over the rows), so the SubM layers of the first
    level build their rulebook without a hash table, like the levels behind a strided layer do.  Coordinates that occur
    twice are detected on the device (one synchronisation, here in the data loader) and leave the tensor untagged."""
    assert indices.dim() == 2 and indices.shape[1] == len(spatial_shape) + 1
    if (batch_size > 0 and indices.is_cuda and indices.dtype == torch.int32 and indices.is_contiguous()
            and indices.shape[0] > 0):
        # the library's own sort (spx_key_argsort: four launches, the rank map written by the same pass -- ~60 us for
        # 420 k rows where torch.argsort of the keys takes 160); a coordinate that occurs twice (one read of the
        # device-side verdict, here in the data loader) takes the general path below
        from spconv_amd.pytorch import ops
        flag = torch.zeros((1,), dtype=torch.int32, device=indices.device)
        res = ops.key_argsort(indices, int(batch_size), [int(v) for v in spatial_shape], rank_map=rank_map, violation=flag)
        if res is not None:
            order32, out = res
            tagged = getattr(out, "_spx_rankmap", None) is not None
            unique = bool(int(flag.item()) == 0) if tagged else bool((_row_keys(out, spatial_shape).diff() > 0).all())
            if unique:
                order = order32.long()
                return (out, *[t.index_select(0, order) for t in row_tensors], order)
    key = indices[:, 0].to(torch.int64)
    for d, s in enumerate(spatial_shape):
        key = key * int(s) + indices[:, 1 + d].to(torch.int64)
    order = torch.argsort(key)
    out = indices[order].contiguous()
    if rank_map and batch_size > 0 and out.is_cuda and out.dtype == torch.int32:
        from spconv_amd.pytorch import ops
        ops.attach_rank_map(out, int(batch_size), [int(v) for v in spatial_shape], check=True)
    return (out, *[t[order].contiguous() for t in row_tensors], order)
