"""The rotated-box entry points of csrc/box.hip restated in numpy float32, every operation rounded on its own (numpy
float32 scalars: one IEEE operation per Python operator): the contract the kernels are held to bit for bit.  Corners
come from the caller (the device's own in the GPU tests, ``boxscenes.corners64`` on the CPU): the sine and cosine are
the one step a host does not reproduce.

  area      a = a + (x_i * y_{i+1} - x_{i+1} * y_i) from a = 0 in vertex order, area = |a| * 0.5; a quad with a < 0 is
            walked in reverse (3, 2, 1, 0) and its area is that of the reversed walk: clockwise corners give the bits
            of counter-clockwise ones
  reject    bounding rectangles on exact comparisons
  clip      Sutherland-Hodgman of the subject A against the edges of B in order; a ninth vertex of a pass is dropped
  inter     min(area(clipped), min(area(A), area(B)))
"""
import numpy as np

F = np.float32
F0, HALF = F(0.0), F(0.5)
OVERLAP_BEV, IOU_BEV, IOU_3D = 0, 1, 2


def _signed(q):
    a = F0
    for i in range(4):
        j = (i + 1) & 3
        a = a + (q[i][0] * q[j][1] - q[j][0] * q[i][1])
    return a


class Table:
    """A corner table prepared once: per box the counter-clockwise corners as float32 scalars, the area, the bounding
    rectangle (arrays) and validity."""

    def __init__(self, bev, zrange=None, n_boxes=None):
        bev = np.ascontiguousarray(bev, dtype=np.float32).reshape(-1, 4, 2)
        n = bev.shape[0]
        self.n = n
        live = n if n_boxes is None else max(0, min(int(n_boxes), n))
        self.valid = np.isfinite(bev).all(axis=(1, 2)) & (np.arange(n) < live)
        self.z = None
        if zrange is not None:
            self.z = np.ascontiguousarray(zrange, dtype=np.float32).reshape(-1, 2)
            self.valid3 = self.valid & np.isfinite(self.z).all(axis=1)
        self.quad = [None] * n
        self.area = np.zeros(n, np.float32)
        safe = np.where(self.valid[:, None, None], bev, 0).astype(np.float32)
        self.minx, self.maxx = safe[:, :, 0].min(1), safe[:, :, 0].max(1)
        self.miny, self.maxy = safe[:, :, 1].min(1), safe[:, :, 1].max(1)
        with np.errstate(all="ignore"):
            for i in np.nonzero(self.valid)[0]:
                q = [(F(bev[i, k, 0]), F(bev[i, k, 1])) for k in range(4)]
                a = _signed(q)
                if a < 0:
                    q = q[::-1]
                    a = _signed(q)
                self.quad[i] = q
                self.area[i] = abs(a) * HALF


def clip_area(A, B):
    """Area of the quad A clipped against the four edges of the quad B (both counter-clockwise)."""
    poly = list(A)
    for e in range(4):
        ax, ay = B[e]
        bx, by = B[(e + 1) & 3]
        ex, ey = bx - ax, by - ay
        d = [ex * (p[1] - ay) - ey * (p[0] - ax) for p in poly]
        n = len(poly)
        out = []
        for i in range(n):
            j = i + 1 if i + 1 < n else 0
            p, q = poly[i], poly[j]
            ip, iq = d[i] >= 0, d[j] >= 0
            if ip:
                out.append(p)
            if ip != iq:
                t = d[i] / (d[i] - d[j])
                out.append((p[0] + t * (q[0] - p[0]), p[1] + t * (q[1] - p[1])))
        poly = out[:8]
        if len(poly) < 3:
            return F0
    a = F0
    n = len(poly)
    for i in range(n):
        j = i + 1 if i + 1 < n else 0
        a = a + (poly[i][0] * poly[j][1] - poly[j][0] * poly[i][1])
    return abs(a) * HALF


def rect_pass(ta, i, tb, js):
    """Of the boxes js of tb (an index array), those whose bounding rectangle is not apart from that of box i of ta."""
    apart = ((ta.maxx[i] < tb.minx[js]) | (tb.maxx[js] < ta.minx[i]) | (ta.maxy[i] < tb.miny[js]) |
             (tb.maxy[js] < ta.miny[i]))
    return ~apart


def value(ta, i, tb, j, mode):
    """The value of the pair (subject box i of ta, box j of tb); both valid and past the rectangle test."""
    with np.errstate(all="ignore"):
        aa, ab = F(ta.area[i]), F(tb.area[j])
        inter = min(clip_area(ta.quad[i], tb.quad[j]), min(aa, ab))
        if mode == OVERLAP_BEV:
            return inter
        if mode == IOU_BEV:
            return inter / max((aa + ab) - inter, F(1e-8))
        za, zb = ta.z[i], tb.z[j]
        h = max(min(F(za[1]), F(zb[1])) - max(F(za[0]), F(zb[0])), F0)
        inter3 = inter * h
        va, vb = aa * (F(za[1]) - F(za[0])), ab * (F(zb[1]) - F(zb[0]))
        return inter3 / max((va + vb) - inter3, F(1e-6))


def pairs(ta, tb, mode):
    """fp32 [M, N]: spx_boxes_overlap over two Tables."""
    out = np.zeros((ta.n, tb.n), np.float32)
    va = ta.valid3 if mode == IOU_3D else ta.valid
    vb = tb.valid3 if mode == IOU_3D else tb.valid
    js = np.nonzero(vb)[0]
    for i in np.nonzero(va)[0]:
        for j in js[rect_pass(ta, i, tb, js)]:
            out[i, j] = value(ta, i, tb, j, mode)
    return out


def aligned(ta, tb, mode):
    """fp32 [N]: spx_boxes_overlap_aligned."""
    out = np.zeros(ta.n, np.float32)
    va = ta.valid3 if mode == IOU_3D else ta.valid
    vb = tb.valid3 if mode == IOU_3D else tb.valid
    for i in np.nonzero(va & vb)[0]:
        if rect_pass(ta, i, tb, np.array([i]))[0]:
            out[i] = value(ta, i, tb, i, mode)
    return out


def rank_keys(scores):
    """uint32 per score, ascending = score descending under the total order on the bits (-0.0 below +0.0)."""
    bits = np.ascontiguousarray(scores, dtype=np.float32).view(np.uint32)
    orderable = bits ^ np.where(bits >> 31 != 0, np.uint32(0xffffffff), np.uint32(0x80000000))
    return ~orderable


def nms(t, scores, thresh, batch_ids=None, batch_size=1, class_ids=None, pre_max=4096, post_max=512, score_thresh=None,
        cache=None):
    """spx_nms_rotated over a Table (its n_boxes folded into validity): (keep int32 [batch_size, post_max], count int32
    [batch_size]).  cache: a dict of IoUs by (subject, other) shared by calls over the same table."""
    n = t.n
    scores = np.ascontiguousarray(scores, dtype=np.float32)
    thresh = F(thresh)
    bid = np.zeros(n, np.int64) if batch_ids is None else np.asarray(batch_ids).astype(np.int64)
    cand = t.valid & (bid >= 0) & (bid < batch_size) & ~np.isnan(scores)
    if score_thresh is not None:
        with np.errstate(invalid="ignore"):
            cand &= scores > F(score_thresh)
    keys = rank_keys(scores)
    keep = np.full((batch_size, post_max), -1, np.int32)
    count = np.zeros(batch_size, np.int32)
    cache = {} if cache is None else cache
    for b in range(batch_size):
        idx = np.nonzero(cand & (bid == b))[0]
        idx = idx[np.argsort(keys[idx], kind="stable")][:pre_max]
        kept = []
        for i in idx:
            if len(kept) == post_max:
                break
            ks = np.asarray(kept, dtype=np.int64)
            if class_ids is not None and len(ks):
                ks = ks[np.asarray(class_ids)[ks] == class_ids[i]]
            if len(ks):
                ks = ks[rect_pass(t, i, t, ks)]          # (the rectangle test is symmetric)
            gone = False
            for k in ks:
                v = cache.get((int(k), int(i)))
                if v is None:
                    v = cache[(int(k), int(i))] = value(t, k, t, i, IOU_BEV)
                if v > thresh:
                    gone = True
                    break
            if not gone:
                kept.append(int(i))
        keep[b, :len(kept)] = kept
        count[b] = len(kept)
    return keep, count
