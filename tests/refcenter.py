"""The centre-head targets of csrc/center.hip restated twice.

``records`` / ``dense_args`` / ``nearest_rows`` / ``sparse_args`` are the numpy FLOAT32 loop of the rules in
include/spconv_amd.h: every operation rounded on its own, in the header's order; the device must reproduce every table
bit for bit.  The heat tables hold the float32 ARGUMENT of the winning box per element (NaN: no box reaches; the
maximum of exp is the exp of the maximum), ``to_heat`` / ``heat_of`` turn it into float32(exp(float64(arg))), which the
GPU test holds ``expf`` to within 3 ulp.

``records64`` / ``dense_heat64`` / ``nearest_rows64`` / ``sparse_heat64`` are an independent FLOAT64 formulation written
the way OpenPCDet's Python loop is: ``gaussian_radius`` with Python floats, ``gaussian2D`` arrays sliced into the map box
by box (``draw_gaussian_to_heatmap``), a distance vector per box over the rows of the scene
(``draw_gaussian_to_heatmap_voxels``)."""
import numpy as np


def _f(v):
    return np.float32(v)


def live_boxes(M, n_boxes):
    return M if n_boxes is None else max(min(int(n_boxes), M), 0)


def slots(bids, B, live, max_objs):
    """slot of every box (-1: none), and the boxes of every scene in ascending index"""
    M = len(bids)
    slot = np.full(M, -1, np.int32)
    scenes = [[] for _ in range(B)]
    for i in range(live):
        b = int(bids[i])
        if 0 <= b < B:
            if len(scenes[b]) < max_objs:
                slot[i] = len(scenes[b])
            scenes[b].append(i)
    return slot, scenes


def radius32(h, w, ov):
    """CornerNet's gaussian_radius in float32, the header's order; NaN when a root is"""
    one, two, four = _f(1), _f(2), _f(4)
    with np.errstate(all="ignore"):
        b1 = h + w
        c1 = ((w * h) * (one - ov)) / (one + ov)
        r1 = (b1 + np.sqrt(b1 * b1 - four * c1)) / two
        b2 = two * (h + w)
        c2 = ((one - ov) * w) * h
        r2 = (b2 + np.sqrt(b2 * b2 - _f(16) * c2)) / two
        a3 = four * ov
        b3 = (_f(-2) * ov) * (h + w)
        c3 = ((ov - one) * w) * h
        r3 = (b3 + np.sqrt(b3 * b3 - (four * a3) * c3)) / two
    return np.minimum(np.minimum(r1, r2), r3)            # (np.minimum propagates NaN)


def records(boxes, bids, cls_ids, B, n_boxes=None, *, grid_size, voxel_size, range_min, stride, num_classes,
            max_objs=500, min_overlap=0.1, min_radius=2):
    """every table of spx_box_centers as a dict of numpy arrays"""
    boxes = np.asarray(boxes, np.float32)
    M = boxes.shape[0]
    W, H = grid_size
    vx, vy, x0, y0, s, ov = _f(voxel_size[0]), _f(voxel_size[1]), _f(range_min[0]), _f(range_min[1]), _f(stride), \
        _f(min_overlap)
    bids = np.zeros(M, np.int32) if bids is None else np.asarray(bids)
    cls_ids = np.zeros(M, np.int64) if cls_ids is None else np.asarray(cls_ids)
    live = live_boxes(M, n_boxes)
    slot, scenes = slots(bids, B, live, max_objs)
    center, cell = np.zeros((M, 2), np.float32), np.zeros((M, 2), np.int32)
    radius, cls = np.zeros(M, np.int32), np.full(M, -1, np.int32)
    for i in range(live):
        v = boxes[i, :7]
        if not (np.all(np.isfinite(v)) and v[3] > 0 and v[4] > 0 and v[5] > 0):
            continue
        with np.errstate(all="ignore"):
            cx = ((v[0] - x0) / vx) / s
            cy = ((v[1] - y0) / vy) / s
            cx = min(max(cx, _f(0)), _f(W) - _f(0.5))
            cy = min(max(cy, _f(0)), _f(H) - _f(0.5))
            w, h = (v[3] / vx) / s, (v[4] / vy) / s
            ret = radius32(h, w, ov)
        if not (np.isfinite(ret) and abs(ret) < 2 ** 20):
            continue
        center[i] = (cx, cy)
        cell[i] = (int(cx), int(cy))
        radius[i] = max(int(ret), min_radius)
        if slot[i] >= 0 and 0 <= int(cls_ids[i]) < num_classes:
            cls[i] = int(cls_ids[i])
    box_index = np.full((B, max_objs), -1, np.int32)
    mask, inds = np.zeros((B, max_objs), np.int32), np.zeros((B, max_objs), np.int32)
    for b in range(B):
        for k, i in enumerate(scenes[b][:max_objs]):
            box_index[b, k] = i
            if cls[i] >= 0:
                mask[b, k] = 1
                inds[b, k] = cell[i, 1] * W + cell[i, 0]
    return dict(center=center, cell=cell, radius=radius, cls=cls, slot=slot, box_index=box_index, mask=mask, inds=inds,
                scenes=scenes, bids=bids, B=B, W=W, H=H, C=num_classes, max_objs=max_objs)


def gauss_arg(d2, r):
    """the float32 argument of expf for a float32 d2 (array) and a radius"""
    sigma = _f(2 * r + 1) / _f(6)
    with np.errstate(all="ignore"):
        return -np.asarray(d2, np.float32) / ((_f(2) * sigma) * sigma)


def heat_of(arg):
    """float32(exp(float64(arg))): what expf is compared with"""
    with np.errstate(all="ignore"):
        return np.exp(np.asarray(arg, np.float64)).astype(np.float32)


def dense_args(rec):
    """float32 [B, C, H, W]: the largest argument any box brings to a cell, NaN where no box reaches"""
    B, C, H, W = rec["B"], rec["C"], rec["H"], rec["W"]
    arg = np.full((B, C, H, W), np.nan, np.float32)
    for b in range(B):
        for i in rec["scenes"][b]:
            c = rec["cls"][i]
            if c < 0:
                continue
            ix, iy, r = int(rec["cell"][i, 0]), int(rec["cell"][i, 1]), int(rec["radius"][i])
            xs, ys = np.arange(max(ix - r, 0), min(ix + r, W - 1) + 1), np.arange(max(iy - r, 0), min(iy + r, H - 1) + 1)
            d2 = ((xs[None, :] - ix) ** 2 + (ys[:, None] - iy) ** 2).astype(np.float32)
            a = gauss_arg(d2, r)
            win = arg[b, c, ys[0]:ys[-1] + 1, xs[0]:xs[-1] + 1]
            win[...] = np.where(np.isnan(win) | (a > win), a, win)
    return arg


def to_heat(arg):
    """the heat of an argument table: 0 where no box reaches"""
    return np.where(np.isnan(arg), _f(0), heat_of(np.nan_to_num(arg, nan=0.0))).astype(np.float32)


def live_rows(indices, B, W, H, n_live=None):
    indices = np.asarray(indices)
    N = indices.shape[0]
    live = N if n_live is None else max(min(int(n_live), N), 0)
    ok = np.arange(N) < live
    return ok & (indices[:, 0] >= 0) & (indices[:, 0] < B) & (indices[:, 1] >= 0) & (indices[:, 1] < H) & \
        (indices[:, 2] >= 0) & (indices[:, 2] < W)


def _d2_center(indices, rows, cx, cy):
    dx = indices[rows, 2].astype(np.float32) - _f(cx)
    dy = indices[rows, 1].astype(np.float32) - _f(cy)
    return dx * dx + dy * dy


def nearest_rows(rec, indices, n_live=None):
    """nearest int32 [M], sparse inds and mask [B, max_objs]"""
    indices = np.asarray(indices)
    ok = live_rows(indices, rec["B"], rec["W"], rec["H"], n_live)
    M = len(rec["cls"])
    nearest = np.full(M, -1, np.int32)
    for i in range(M):
        if rec["cls"][i] < 0:
            continue
        rows = np.nonzero(ok & (indices[:, 0] == rec["bids"][i]))[0]
        if len(rows):
            d2 = _d2_center(indices, rows, rec["center"][i, 0], rec["center"][i, 1])
            keys = (d2.view(np.uint32).astype(np.uint64) << np.uint64(32)) | rows.astype(np.uint64)
            nearest[i] = rows[np.argmin(keys)]
    inds, mask = np.zeros_like(rec["inds"]), np.zeros_like(rec["mask"])
    for b in range(rec["B"]):
        for k in range(rec["max_objs"]):
            i = rec["box_index"][b, k]
            if i >= 0 and rec["mask"][b, k] and nearest[i] >= 0:
                mask[b, k], inds[b, k] = 1, nearest[i]
    return nearest, inds, mask


def sparse_args(rec, indices, nearest, anchor="center", cutoff="none", n_live=None):
    """float32 [N, C]: the largest argument any box brings to a row, NaN where none does"""
    indices = np.asarray(indices)
    ok = live_rows(indices, rec["B"], rec["W"], rec["H"], n_live)
    arg = np.full((indices.shape[0], rec["C"]), np.nan, np.float32)
    for b in range(rec["B"]):
        rows = np.nonzero(ok & (indices[:, 0] == b))[0]
        if not len(rows):
            continue
        for i in rec["scenes"][b]:
            c = rec["cls"][i]
            if c < 0:
                continue
            r = int(rec["radius"][i])
            if anchor == "nearest":
                if nearest[i] < 0:
                    continue
                wx, wy = int(indices[nearest[i], 2]), int(indices[nearest[i], 1])
                ddx, ddy = indices[rows, 2].astype(np.int64) - wx, indices[rows, 1].astype(np.int64) - wy
                d2 = (ddx * ddx + ddy * ddy).astype(np.float32)
            else:
                wx, wy = int(rec["cell"][i, 0]), int(rec["cell"][i, 1])
                d2 = _d2_center(indices, rows, rec["center"][i, 0], rec["center"][i, 1])
            sel = rows
            if cutoff == "window":
                keep = (np.abs(indices[rows, 2] - wx) <= r) & (np.abs(indices[rows, 1] - wy) <= r)
                sel, d2 = rows[keep], d2[keep]
            a = gauss_arg(d2, r)
            cur = arg[sel, c]
            arg[sel, c] = np.where(np.isnan(cur) | (a > cur), a, cur)
    return arg


# ------------------------------------------------------------------------------------------------ float64, loop style

def gaussian_radius64(height, width, min_overlap=0.5):
    a1 = 1
    b1 = (height + width)
    c1 = width * height * (1 - min_overlap) / (1 + min_overlap)
    sq1 = (b1 ** 2 - 4 * a1 * c1) ** 0.5
    r1 = (b1 + sq1) / 2
    a2 = 4
    b2 = 2 * (height + width)
    c2 = (1 - min_overlap) * width * height
    sq2 = (b2 ** 2 - 4 * a2 * c2) ** 0.5
    r2 = (b2 + sq2) / 2
    a3 = 4 * min_overlap
    b3 = -2 * min_overlap * (height + width)
    c3 = (min_overlap - 1) * width * height
    sq3 = (b3 ** 2 - 4 * a3 * c3) ** 0.5
    r3 = (b3 + sq3) / 2
    return min(r1, r2, r3)


def gaussian2D(shape, sigma=1.0):
    m, n = [(ss - 1.) / 2. for ss in shape]
    y, x = np.ogrid[-m:m + 1, -n:n + 1]
    h = np.exp(-(x * x + y * y) / (2 * sigma * sigma))
    h[h < np.finfo(h.dtype).eps * h.max()] = 0
    return h


def draw_gaussian(heatmap, center, radius):
    diameter = 2 * radius + 1
    gaussian = gaussian2D((diameter, diameter), sigma=diameter / 6)
    x, y = int(center[0]), int(center[1])
    height, width = heatmap.shape[0:2]
    left, right = min(x, radius), min(width - x, radius + 1)
    top, bottom = min(y, radius), min(height - y, radius + 1)
    masked_heatmap = heatmap[y - top:y + bottom, x - left:x + right]
    masked_gaussian = gaussian[radius - top:radius + bottom, radius - left:radius + right]
    if min(masked_gaussian.shape) > 0 and min(masked_heatmap.shape) > 0:
        np.maximum(masked_heatmap, masked_gaussian, out=masked_heatmap)
    return heatmap


def records64(boxes, bids, cls_ids, B, n_boxes=None, *, grid_size, voxel_size, range_min, stride, num_classes,
              max_objs=500, min_overlap=0.1, min_radius=2):
    """the loop of assign_target_of_single_head over a scene's boxes in float64 (Python floats for the parameters)"""
    boxes = np.asarray(boxes, np.float32).astype(np.float64)
    M = boxes.shape[0]
    W, H = grid_size
    bids = np.zeros(M, np.int64) if bids is None else np.asarray(bids)
    cls_ids = np.zeros(M, np.int64) if cls_ids is None else np.asarray(cls_ids)
    live = live_boxes(M, n_boxes)
    out = dict(center=np.zeros((M, 2)), cell=np.zeros((M, 2), np.int64), radius=np.zeros(M, np.int64),
               cls=np.full(M, -1, np.int64), slot=np.full(M, -1, np.int64), box_index=np.full((B, max_objs), -1, np.int64),
               mask=np.zeros((B, max_objs), np.int64), inds=np.zeros((B, max_objs), np.int64), bids=bids, B=B, W=W, H=H,
               C=num_classes, max_objs=max_objs)
    for i in range(live):                                 # the geometry of every box, also of one without a slot
        x, y, z, dx, dy, dz, _ = boxes[i, :7]
        if not np.all(np.isfinite(boxes[i, :7])) or dx <= 0 or dy <= 0 or dz <= 0:
            continue
        coord_x = min(max((x - range_min[0]) / voxel_size[0] / stride, 0.0), W - 0.5)
        coord_y = min(max((y - range_min[1]) / voxel_size[1] / stride, 0.0), H - 0.5)
        ret = gaussian_radius64(dy / voxel_size[1] / stride, dx / voxel_size[0] / stride, min_overlap)
        if not (np.isfinite(ret) and abs(ret) < 2 ** 20):
            continue
        out["center"][i] = (coord_x, coord_y)
        out["cell"][i] = (int(coord_x), int(coord_y))
        out["radius"][i] = max(int(ret), min_radius)
        out["cls"][i] = -2                                # (a geometry; the class follows with the slot)
    for b in range(B):
        mine = [i for i in range(live) if bids[i] == b]
        for k, i in enumerate(mine[:max_objs]):
            out["slot"][i] = k
            out["box_index"][b, k] = i
            if out["cls"][i] == -2 and 0 <= cls_ids[i] < num_classes:
                out["cls"][i] = cls_ids[i]
                out["mask"][b, k] = 1
                out["inds"][b, k] = out["cell"][i, 1] * W + out["cell"][i, 0]
    out["cls"][out["cls"] == -2] = -1
    return out


def dense_heat64(rec):
    heat = np.zeros((rec["B"], rec["C"], rec["H"], rec["W"]))
    for b in range(rec["B"]):
        for i in rec["box_index"][b]:
            if i >= 0 and rec["cls"][i] >= 0:
                draw_gaussian(heat[b, rec["cls"][i]], rec["cell"][i], int(rec["radius"][i]))
    return heat


def nearest_rows64(rec, indices, n_live=None):
    indices = np.asarray(indices)
    ok = live_rows(indices, rec["B"], rec["W"], rec["H"], n_live)
    nearest = np.full(len(rec["cls"]), -1, np.int64)
    for i in range(len(rec["cls"])):
        rows = np.nonzero(ok & (indices[:, 0] == rec["bids"][i]))[0]
        if rec["cls"][i] >= 0 and len(rows):
            dist = (indices[rows, 2] - rec["center"][i, 0]) ** 2 + (indices[rows, 1] - rec["center"][i, 1]) ** 2
            nearest[i] = rows[np.argmin(dist)]               # (the first minimum: the lowest row)
    inds, mask = np.zeros_like(rec["inds"]), np.zeros_like(rec["mask"])
    for b in range(rec["B"]):
        for k, i in enumerate(rec["box_index"][b]):
            if i >= 0 and rec["mask"][b, k] and nearest[i] >= 0:
                mask[b, k], inds[b, k] = 1, nearest[i]
    return nearest, inds, mask


def sparse_heat64(rec, indices, nearest, anchor="center", cutoff="none", n_live=None):
    indices = np.asarray(indices)
    ok = live_rows(indices, rec["B"], rec["W"], rec["H"], n_live)
    heat = np.zeros((indices.shape[0], rec["C"]))
    for b in range(rec["B"]):
        rows = np.nonzero(ok & (indices[:, 0] == b))[0]
        for i in rec["box_index"][b]:
            if i < 0 or rec["cls"][i] < 0 or not len(rows) or (anchor == "nearest" and nearest[i] < 0):
                continue
            radius = int(rec["radius"][i])
            if anchor == "nearest":
                anchor_xy = indices[nearest[i], [2, 1]].astype(np.float64)
                window = anchor_xy
            else:
                anchor_xy, window = rec["center"][i], rec["cell"][i]
            distances = (indices[rows, 2] - anchor_xy[0]) ** 2 + (indices[rows, 1] - anchor_xy[1]) ** 2
            sigma = (2 * radius + 1) / 6
            gaussian = np.exp(-distances / (2 * sigma * sigma))
            if cutoff == "window":
                inside = (np.abs(indices[rows, 2] - window[0]) <= radius) & (np.abs(indices[rows, 1] - window[1]) <= radius)
                gaussian = np.where(inside, gaussian, 0.0)
            heat[rows, rec["cls"][i]] = np.maximum(heat[rows, rec["cls"][i]], gaussian)
    return heat
