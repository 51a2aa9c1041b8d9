"""Plain numpy float32 restatement of csrc/roi.hip (include/spconv_amd.h, "points in rotated boxes"): the frames of
boxes GIVEN the cosine and sine of their headings, the containment test, the point-major table, the box-major tables
(rows / count / hits / local / cells) with the three pads, and seeded scenes.  Every float32 operation is one numpy
float32 operation: rounded on its own, in the order the header writes.  tests/test_refroi.py holds this file to an
independent float64 formulation on the CPU; tests/test_gpu_roi.py compares the kernels with it bit for bit from the
frames the device wrote."""
import numpy as np

F32 = np.float32
PAD_NONE, PAD_FIRST, PAD_CYCLE = 0, 2, 4


def valid_boxes(boxes, n_boxes=None):
    """the rule of spx_boxes_to_corners: below n_boxes, seven finite numbers, dx, dy, dz > 0"""
    b = np.asarray(boxes, F32)
    ok = np.isfinite(b[:, :7]).all(1) & (b[:, 3] > 0) & (b[:, 4] > 0) & (b[:, 5] > 0)
    if n_boxes is not None:
        ok &= np.arange(len(b)) < n_boxes
    return ok


def frames_given_trig(boxes, c, s, extra=(0.0, 0.0, 0.0), n_boxes=None):
    """fp32 [M, 8] = (x, y, z, dx * 0.5f + ex, dy * 0.5f + ey, dz * 0.5f + ez, c, s); eight NaNs for an invalid box"""
    b = np.asarray(boxes, F32)
    out = np.full((len(b), 8), np.nan, F32)
    ok = valid_boxes(b, n_boxes)
    out[ok, 0:3] = b[ok, 0:3]
    for j in range(3):
        out[ok, 3 + j] = b[ok, 3 + j] * F32(0.5) + F32(extra[j])
    out[ok, 6] = np.asarray(c, F32)[ok]
    out[ok, 7] = np.asarray(s, F32)[ok]
    return out


def local(frames, points):
    """(lx, ly, lz) fp32 [M, N]: every point in every frame"""
    f, p = np.asarray(frames, F32), np.asarray(points, F32)
    with np.errstate(invalid="ignore", over="ignore"):
        sx = p[None, :, 0] - f[:, None, 0]
        sy = p[None, :, 1] - f[:, None, 1]
        lz = p[None, :, 2] - f[:, None, 2]
        lx = sx * f[:, None, 6] + sy * f[:, None, 7]
        ly = sy * f[:, None, 6] - sx * f[:, None, 7]
    return lx, ly, lz


def inside(frames, points):
    """bool [M, N] with (lx, ly, lz): inclusive in z, strict in the plane; a point with a coordinate that is not
    finite is in no box, a frame with a NaN contains nothing"""
    f, p = np.asarray(frames, F32), np.asarray(points, F32)
    lx, ly, lz = local(f, p)
    hx, hy, hz = f[:, None, 3], f[:, None, 4], f[:, None, 5]
    with np.errstate(invalid="ignore"):
        hit = (np.abs(lz) <= hz) & (lx > -hx) & (lx < hx) & (ly > -hy) & (ly < hy)
    hit &= np.isfinite(p[:, :3]).all(1)[None, :]
    return hit, lx, ly, lz


def _ids(ids, n):
    return np.zeros(n, np.int64) if ids is None else np.asarray(ids).astype(np.int64)


def incidence(frames, b_ids, points, p_ids, batch, n_boxes=None, n_points=None):
    """bool [M, N]: box m contains point i, both exist and they share a scene in [0, batch)"""
    M, N = len(frames), len(points)
    hit, lx, ly, lz = inside(frames, points)
    bi, pi = _ids(b_ids, M), _ids(p_ids, N)
    box_ok = (bi >= 0) & (bi < batch) & (np.arange(M) < (M if n_boxes is None else n_boxes))
    pt_ok = (pi >= 0) & (pi < batch) & (np.arange(N) < (N if n_points is None else n_points))
    hit &= box_ok[:, None] & pt_ok[None, :] & (bi[:, None] == pi[None, :])
    return hit, lx, ly, lz


def points_in_boxes(frames, b_ids, points, p_ids, batch, n_boxes=None, n_points=None):
    """int32 [N]: the lowest box index of the point's scene that contains it, -1 for none"""
    hit, _, _, _ = incidence(frames, b_ids, points, p_ids, batch, n_boxes, n_points)
    out = np.full(len(points), -1, np.int32)
    if hit.shape[0]:
        any_ = hit.any(0)
        out[any_] = hit.argmax(0)[any_]
    return out


def cell_index(l, h, o):
    """min(max(int((l + h) / w), 0), o - 1) with w = (h + h) / float(o)"""
    w = (h + h) / F32(o)
    return np.clip(((l + h) / w).astype(np.int32), 0, o - 1)


def box_query(frames, b_ids, points, p_ids, batch, nsample, pad=PAD_NONE, grid=None, n_boxes=None, n_points=None):
    """dict(rows int32 [M, nsample], count, hits int32 [M], local fp32 [M, nsample, 3], cells int32 [M, nsample] or
    None): the first nsample points inside each box in ascending point index, then the pad"""
    f = np.asarray(frames, F32)
    M = len(f)
    hit, lx, ly, lz = incidence(f, b_ids, points, p_ids, batch, n_boxes, n_points)
    rows = np.full((M, nsample), -1, np.int32)
    loc = np.zeros((M, nsample, 3), F32)
    cells = None if grid is None else np.full((M, nsample), -1, np.int32)
    count, hits = np.zeros(M, np.int32), np.zeros(M, np.int32)
    for m in range(M):
        idx = np.flatnonzero(hit[m])
        hits[m] = len(idx)
        idx = idx[:nsample]
        c = count[m] = len(idx)
        rows[m, :c] = idx
        loc[m, :c] = np.stack([lx[m, idx], ly[m, idx], lz[m, idx]], -1)
        if grid is not None and c:
            ox, oy, oz = grid
            ix = cell_index(lx[m, idx], f[m, 3], ox)
            iy = cell_index(ly[m, idx], f[m, 4], oy)
            iz = cell_index(lz[m, idx], f[m, 5], oz)
            cells[m, :c] = m * (ox * oy * oz) + (ix * oy + iy) * oz + iz
        if pad != PAD_NONE and 0 < c < nsample:
            src = np.arange(c, nsample) % c if pad == PAD_CYCLE else np.zeros(nsample - c, np.int64)
            rows[m, c:] = rows[m, src]
            loc[m, c:] = loc[m, src]
            if cells is not None:
                cells[m, c:] = cells[m, src]
    return dict(rows=rows, count=count, hits=hits, local=loc, cells=cells)


def scene(seed, n_points, n_boxes, batch=1, field=40.0, wild=8):
    """(boxes fp32 [M, 7], b_ids int32 [M], points fp32 [N, 3], p_ids int32 [N]): boxes in +-field metres with car-like
    sizes x U(0.5, 4), headings in +-pi but `wild` of them in +-100 rad; half of the points uniform over the field, half
    drawn inside a box (up to its faces) with that box's scene"""
    rng = np.random.default_rng(seed)
    M, N = n_boxes, n_points
    boxes = np.zeros((M, 7))
    boxes[:, 0:2] = rng.uniform(-field, field, (M, 2))
    boxes[:, 2] = rng.uniform(-2.0, 2.0, M)
    boxes[:, 3:6] = np.array([3.9, 1.6, 1.56]) * rng.uniform(0.5, 4.0, (M, 3))
    boxes[:, 6] = rng.uniform(-np.pi, np.pi, M)
    w = min(wild, M)
    boxes[:w, 6] = rng.uniform(-100.0, 100.0, w)
    b_ids = rng.integers(0, batch, M).astype(np.int32)
    points = np.zeros((N, 3))
    points[:, 0:2] = rng.uniform(-field - 5.0, field + 5.0, (N, 2))
    points[:, 2] = rng.uniform(-5.0, 5.0, N)
    p_ids = rng.integers(0, batch, N).astype(np.int32)
    if M:
        own = rng.random(N) < 0.5
        k = rng.integers(0, M, N)
        u = rng.uniform(-1.0, 1.0, (N, 3)) * boxes[k, 3:6] * 0.5
        c, s = np.cos(boxes[k, 6]), np.sin(boxes[k, 6])
        inbox = np.stack([boxes[k, 0] + u[:, 0] * c - u[:, 1] * s, boxes[k, 1] + u[:, 0] * s + u[:, 1] * c,
                          boxes[k, 2] + u[:, 2]], -1)
        points[own] = inbox[own]
        p_ids[own] = b_ids[k[own]]
    return boxes.astype(F32), b_ids, points.astype(F32), p_ids


def faces():
    """(box fp32 [1, 7], points fp32 [15, 3], inside [15]): an axis-aligned box at the origin (c = 1, s = 0 exactly, so
    lx = px and ly = py to the bit) with points exactly on its faces and one float32 step either side: strict in the
    plane, inclusive in z"""
    up = lambda v: np.nextafter(F32(v), F32(np.inf))
    down = lambda v: np.nextafter(F32(v), F32(-np.inf))
    box = np.array([[0.0, 0.0, 0.0, 4.0, 2.0, 1.0, 0.0]], F32)
    cases = [((2.0, 0.0, 0.0), False), ((-2.0, 0.0, 0.0), False), ((down(2.0), 0.0, 0.0), True),
             ((up(-2.0), 0.0, 0.0), True), ((up(2.0), 0.0, 0.0), False), ((down(-2.0), 0.0, 0.0), False),
             ((0.0, 1.0, 0.0), False), ((0.0, down(1.0), 0.0), True), ((0.0, -1.0, 0.0), False),
             ((0.0, up(-1.0), 0.0), True), ((0.0, 0.0, 0.5), True), ((0.0, 0.0, -0.5), True),
             ((0.0, 0.0, up(0.5)), False), ((0.0, 0.0, down(-0.5)), False), ((0.0, 0.0, down(0.5)), True)]
    return box, np.array([c[0] for c in cases], F32), np.array([c[1] for c in cases])


def trig32(boxes):
    """float32(cos), float32(sin) of the float32 headings, through float64 (the host's stand-in for cosf / sinf)"""
    h = np.asarray(boxes, F32)[:, 6].astype(np.float64)
    with np.errstate(invalid="ignore"):
        return np.cos(h).astype(F32), np.sin(h).astype(F32)
