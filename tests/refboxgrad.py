"""The gradient entry points of csrc/boxgrad.hip restated in numpy scalars, one IEEE operation per Python operator, in the
operation order the header gives: the contract ``spx_boxes_iou_aligned_grad`` is held to bit for bit.  Corners come from
the caller, as in refbox.py.  Every rule is written once over a scalar type ``T``: ``T = numpy.float32`` is the
restatement of the kernel, ``T = numpy.float64`` the same rules in double precision (what the central differences of an
independent value are compared with).  ``chain64`` is the backward of the corners launch in float64
(``spx_boxes_to_corners_bwd`` is held to it within a derived bound).

  record      the corners walked counter-clockwise (a quad of negative signed area reversed), the area, the bounding
              rectangle: refbox.Table's arithmetic
  inter       min(clip, min(area_a, area_b)); its gradient is the shoelace gradient of the smaller area when the clamp
              binds (clip > min), else the edge integral: each of the eight edges clipped to [t0, t1] by the other
              quad's four half-planes, n * w0 to its first corner and n * w1 to its second
  value       the forward's IoU; with the DIoU penalty minus rho2 / max(c2, 1e-12)
"""
import numpy as np

import refbox

IOU_BEV, IOU_3D = refbox.IOU_BEV, refbox.IOU_3D
NONE, DIOU = 0, 1


class Rec:
    """One box as the kernels hold it: x[4], y[4] counter-clockwise, area, bounding rectangle, z range, `rev` (the
    caller's corners were clockwise: record corner k is the caller's 3 - k)."""

    def __init__(self, quad, z, T):
        q = [(T(quad[k][0]), T(quad[k][1])) for k in range(4)]
        a = self._signed(q, T)
        self.rev = bool(a < 0)
        if self.rev:
            q = q[::-1]
            a = self._signed(q, T)
        self.x, self.y = [p[0] for p in q], [p[1] for p in q]
        self.q = q
        self.area = abs(a) * T(0.5)
        self.minx, self.maxx, self.miny, self.maxy = min(self.x), max(self.x), min(self.y), max(self.y)
        self.zmin, self.zmax = (T(0), T(0)) if z is None else (T(z[0]), T(z[1]))

    @staticmethod
    def _signed(q, T):
        a = T(0)
        for i in range(4):
            j = (i + 1) & 3
            a = a + (q[i][0] * q[j][1] - q[j][0] * q[i][1])
        return a


def area_grad(R, T):
    """([gx_k], [gy_k]): the shoelace gradient of the area of a counter-clockwise quad."""
    h = T(0.5)
    return ([(R.y[(k + 1) & 3] - R.y[(k + 3) & 3]) * h for k in range(4)],
            [(R.x[(k + 3) & 3] - R.x[(k + 1) & 3]) * h for k in range(4)])


def edge_integral(P, Q, gx, gy, T):
    """Adds to gx / gy (lists of 4) the gradient of the shared area with respect to the corners of P from the parts of
    P's edges inside Q."""
    zero, one, half = T(0), T(1), T(0.5)
    for k in range(4):
        j = (k + 1) & 3
        px, py, qx, qy = P.x[k], P.y[k], P.x[j], P.y[j]
        t0, t1, dead = zero, one, False
        for e in range(4):
            ax, ay = Q.x[e], Q.y[e]
            ex, ey = Q.x[(e + 1) & 3] - ax, Q.y[(e + 1) & 3] - ay
            dp = ex * (py - ay) - ey * (px - ax)
            dq = ex * (qy - ay) - ey * (qx - ax)
            ip, iq = dp >= 0, dq >= 0
            if not ip and not iq:
                dead = True
            elif ip != iq:
                t = dp / (dp - dq)
                if not ip:
                    t0 = max(t0, t)
                else:
                    t1 = min(t1, t)
        if dead or not t0 < t1:
            continue
        nx, ny = qy - py, px - qx
        w1 = (t1 * t1 - t0 * t0) * half
        w0 = (t1 - t0) - w1
        gx[k] = gx[k] + nx * w0
        gy[k] = gy[k] + ny * w0
        gx[j] = gx[j] + nx * w1
        gy[j] = gy[j] + ny * w1


def pair_grad(qa, za, qb, zb, mode, penalty=NONE, go=1.0, T=np.float32, info=None):
    """(value, gbev_a [4][2], gz_a [2], gbev_b [4][2], gz_b [2]) of one pair of VALID boxes, gradients at the caller's
    corner indices, everything in T.  za / zb may be None in the plane.  info: a dict that receives clip, the smaller
    area and h (the kink tests of the CPU comparison)."""
    zero, one = T(0), T(1)
    space = mode == IOU_3D
    go = T(go)
    with np.errstate(all="ignore"):
        A, B = Rec(qa, za if space else None, T), Rec(qb, zb if space else None, T)
        aa, ab = A.area, B.area
        gix_a, giy_a, gix_b, giy_b = [zero] * 4, [zero] * 4, [zero] * 4, [zero] * 4
        gax_a, gay_a = area_grad(A, T)
        gax_b, gay_b = area_grad(B, T)
        small = min(aa, ab)
        clip = zero
        if A.maxx < B.minx or B.maxx < A.minx or A.maxy < B.miny or B.maxy < A.miny:
            inter = zero
        else:
            clip = T(refbox.clip_area(A.q, B.q))
            inter = min(clip, small)
            if clip > small:
                if aa <= ab:
                    gix_a, giy_a = list(gax_a), list(gay_a)
                else:
                    gix_b, giy_b = list(gax_b), list(gay_b)
            else:
                edge_integral(A, B, gix_a, giy_a, T)
                edge_integral(B, A, gix_b, giy_b, T)
        # the value and the coefficients of d inter, d area, d h, d height
        if space:
            top, bot = min(A.zmax, B.zmax), max(A.zmin, B.zmin)
            hraw = top - bot
            h = max(hraw, zero)
            ha, hb = A.zmax - A.zmin, B.zmax - B.zmin
            i3 = inter * h
            sa, sb = aa * ha, ab * hb
            floor = T(np.float32(1e-6))
        else:
            hraw = h = one
            i3, sa, sb = inter, aa, ab
            floor = T(np.float32(1e-8))
        s = sa + sb
        uraw = s - i3
        u = max(uraw, floor)
        value = i3 / u
        if uraw > floor:
            u2 = u * u
            ci, cs = s / u2, i3 / u2
        else:
            ci, cs = one / u, zero
        ki, ks = go * ci, go * cs
        if space:
            kin, kh = ki * h, ki * inter
            kaa, kab = ks * ha, ks * hb
            kha, khb = ks * aa, ks * ab
        else:
            kin, kaa, kab = ki, ks, ks
        gxa = [kin * gix_a[k] - kaa * gax_a[k] for k in range(4)]
        gya = [kin * giy_a[k] - kaa * gay_a[k] for k in range(4)]
        gxb = [kin * gix_b[k] - kab * gax_b[k] for k in range(4)]
        gyb = [kin * giy_b[k] - kab * gay_b[k] for k in range(4)]
        gza, gzb = [zero, zero], [zero, zero]
        if space:
            th = kh if hraw > 0 else zero
            top_a, bot_a = A.zmax <= B.zmax, A.zmin >= B.zmin
            gza = [kha - (th if bot_a else zero), (th if top_a else zero) - kha]
            gzb = [khb - (zero if bot_a else th), (zero if top_a else th) - khb]
        if penalty == DIOU:
            half = T(0.5)
            dx = (A.x[0] + A.x[2]) * half - (B.x[0] + B.x[2]) * half
            dy = (A.y[0] + A.y[2]) * half - (B.y[0] + B.y[2]) * half
            rho2 = dx * dx + dy * dy
            x0, x1 = min(A.minx, B.minx), max(A.maxx, B.maxx)
            y0, y1 = min(A.miny, B.miny), max(A.maxy, B.maxy)
            w, v = x1 - x0, y1 - y0
            c2 = w * w + v * v
            if space:
                dz = (A.zmin + A.zmax) * half - (B.zmin + B.zmax) * half
                rho2 = rho2 + dz * dz
                z0, z1 = min(A.zmin, B.zmin), max(A.zmax, B.zmax)
                d = z1 - z0
                c2 = c2 + d * d
            tiny = T(np.float32(1e-12))
            c = max(c2, tiny)
            value = value - rho2 / c
            kr = go / c
            kc = go * (rho2 / (c * c)) if c2 > tiny else zero
            px, py = kr * dx, kr * dy                    # d rho2 / d centre = 2 * (the difference); a corner has half
            for k in (0, 2):
                gxa[k], gya[k] = gxa[k] - px, gya[k] - py
                gxb[k], gyb[k] = gxb[k] + px, gyb[k] + py
            qx, qy = kc * (w + w), kc * (v + v)
            for g, lo, hi, q, ca, cb in ((0, x0, x1, qx, A.x, B.x), (1, y0, y1, qy, A.y, B.y)):
                ga, gb = (gxa, gxb) if g == 0 else (gya, gyb)
                found_hi = found_lo = False
                for tab, src in ((ga, ca), (gb, cb)):
                    for k in range(4):
                        if not found_hi and src[k] == hi:
                            tab[k] = tab[k] + q
                            found_hi = True
                        if not found_lo and src[k] == lo:
                            tab[k] = tab[k] - q
                            found_lo = True
            if space:
                pz = kr * dz
                gza = [gza[0] - pz, gza[1] - pz]
                gzb = [gzb[0] + pz, gzb[1] + pz]
                qz = kc * (d + d)
                if A.zmax >= B.zmax:
                    gza[1] = gza[1] + qz
                else:
                    gzb[1] = gzb[1] + qz
                if A.zmin <= B.zmin:
                    gza[0] = gza[0] - qz
                else:
                    gzb[0] = gzb[0] - qz
    if info is not None:
        info.update(clip=clip, small=small, h=hraw, aa=aa, ab=ab, A=A, B=B)
    ra = [3 - k if A.rev else k for k in range(4)]
    rb = [3 - k if B.rev else k for k in range(4)]
    return (value, [(gxa[ra[k]], gya[ra[k]]) for k in range(4)], gza, [(gxb[rb[k]], gyb[rb[k]]) for k in range(4)], gzb)


def aligned_grad(bev_a, z_a, bev_b, z_b, mode, penalty=NONE, grad_out=None, n_a=None, n_b=None, T=np.float32):
    """spx_boxes_iou_aligned_grad over two corner tables: (value [n], gbev_a [n, 4, 2], gz_a [n, 2], gbev_b, gz_b) as
    arrays of T.  An invalid pair -- the forward's rule, the counts included -- is all zeros."""
    bev_a = np.asarray(bev_a).reshape(-1, 4, 2)
    bev_b = np.asarray(bev_b).reshape(-1, 4, 2)
    n = bev_a.shape[0]
    space = mode == IOU_3D
    ta = refbox.Table(bev_a, z_a if space else None, n_a)
    tb = refbox.Table(bev_b, z_b if space else None, n_b)
    ok = (ta.valid3 & tb.valid3) if space else (ta.valid & tb.valid)
    value = np.zeros(n, T)
    ga, gb = np.zeros((n, 4, 2), T), np.zeros((n, 4, 2), T)
    gza, gzb = np.zeros((n, 2), T), np.zeros((n, 2), T)
    for i in np.nonzero(ok)[0]:
        go = 1.0 if grad_out is None else grad_out[i]
        v, a, za, b, zb = pair_grad(bev_a[i], z_a[i] if space else None, bev_b[i], z_b[i] if space else None, mode,
                                    penalty, go, T)
        value[i], ga[i], gb[i] = v, a, b
        if space:
            gza[i], gzb[i] = za, zb
    return value, ga, gza, gb, gzb


SX, SY = np.array([1.0, -1.0, -1.0, 1.0]), np.array([1.0, 1.0, -1.0, -1.0])


def corners_f64(boxes):
    """The corners of spx_boxes_to_corners in float64, unrounded: (bev [n, 4, 2], zrange [n, 2])."""
    b = np.asarray(boxes, np.float64)
    c, s = np.cos(b[:, 6:7]), np.sin(b[:, 6:7])
    lx, ly = SX[None] * b[:, 3:4] * 0.5, SY[None] * b[:, 4:5] * 0.5
    bev = np.stack([b[:, 0:1] + (lx * c - ly * s), b[:, 1:2] + (lx * s + ly * c)], -1)
    return bev, np.stack([b[:, 2] - b[:, 5] * 0.5, b[:, 2] + b[:, 5] * 0.5], -1)


def chain_terms(boxes, gbev, gz=None):
    """The backward of the corners launch as its TERMS in float64: [n, 7, 16], the gradient of box number c is
    terms[:, c].sum(-1) (``chain64``) and the sum of their absolute values is what a float32 evaluation's error is
    measured against.  Products are expanded fully: a term is one corner gradient times its factor."""
    b = np.asarray(boxes, np.float64)[:, :7]
    g = np.asarray(gbev, np.float64).reshape(-1, 4, 2)
    n = b.shape[0]
    gz = np.zeros((n, 2)) if gz is None else np.asarray(gz, np.float64).reshape(-1, 2)
    c, s = np.cos(b[:, 6:7]), np.sin(b[:, 6:7])
    lx, ly = SX[None] * b[:, 3:4] * 0.5, SY[None] * b[:, 4:5] * 0.5
    gx, gy = g[:, :, 0], g[:, :, 1]
    t = np.zeros((n, 7, 16))
    t[:, 0, :4], t[:, 1, :4] = gx, gy
    t[:, 2, :2] = gz
    t[:, 3, :4], t[:, 3, 4:8] = 0.5 * SX * gx * c, 0.5 * SX * gy * s
    t[:, 4, :4], t[:, 4, 4:8] = -0.5 * SY * gx * s, 0.5 * SY * gy * c
    t[:, 5, 0], t[:, 5, 1] = -0.5 * gz[:, 0], 0.5 * gz[:, 1]
    t[:, 6, :4], t[:, 6, 4:8] = -gx * lx * s, -gx * ly * c
    t[:, 6, 8:12], t[:, 6, 12:16] = gy * lx * c, -gy * ly * s
    return t


def chain64(boxes, gbev, gz=None):
    """gboxes float64 [n, 7]: the gradient with respect to (x, y, z, dx, dy, dz, heading)."""
    return chain_terms(boxes, gbev, gz).sum(-1)
