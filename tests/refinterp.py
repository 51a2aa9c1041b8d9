"""Numpy restatement of trilinear devoxelisation as include/spconv_amd.h specifies it (spx_point_corners,
spx_interp_fwd, spx_interp_bwd): numpy float32 arithmetic rounds every multiply, add, subtract and divide on its own,
which is the contract; the sums are sequential, in the orders the header fixes (ascending corner index per point,
ascending entry e = i * K + c per voxel)."""
import numpy as np


def level_table(indices, n_live, batch, shape_zyx):
    """coordinate -> lowest live row (a duplicate coordinate goes to the lowest row)"""
    table = {}
    indices = np.asarray(indices)
    live = indices.shape[0] if n_live is None else min(int(n_live), indices.shape[0])
    for r in range(live):
        row = indices[r]
        if not 0 <= row[0] < batch:
            continue
        if any(not 0 <= row[1 + d] < shape_zyx[d] for d in range(len(shape_zyx))):
            continue
        table.setdefault(tuple(int(v) for v in row), r)
    return table


def corners(points, batch_ids, n_points, vsize_xyz, lo_xyz, indices, n_live, batch, shape_zyx, normalize=True,
            ftype=np.float32):
    """rows int32 [N, K], weights ftype [N, K].  `ftype` = float32 is the contract; float64 serves the reference's own
    checks."""
    ndim = len(shape_zyx)
    K = 1 << ndim
    points = np.asarray(points)
    N = points.shape[0]
    table = level_table(indices, n_live, batch, shape_zyx)
    vs, lo = np.asarray(vsize_xyz, dtype=ftype), np.asarray(lo_xyz, dtype=ftype)
    half, one = ftype(0.5), ftype(1.0)
    extent_xyz = np.asarray(shape_zyx[::-1])
    b = np.zeros(N, dtype=np.int64) if batch_ids is None else np.asarray(batch_ids).astype(np.int64)
    rows = np.full((N, K), -1, dtype=np.int32)
    weights = np.zeros((N, K), dtype=ftype)
    if N == 0:
        return rows, weights
    with np.errstate(invalid="ignore", over="ignore"):
        p = points[:, :ndim].astype(ftype)
        t = (p - lo) / vs
        cell = np.floor(t)
        valid = (np.arange(N) < (N if n_points is None else int(n_points))) & (b >= 0) & (b < batch)
        valid &= ((cell >= 0) & (cell < extent_xyz)).all(axis=1)            # (false for NaN)
        g = t - half
        base = np.floor(g)
        f = g - base
    for i in np.nonzero(valid)[0]:
        bi = [int(v) for v in base[i]]
        present = []
        for c in range(K):
            w = None
            coord = [0] * ndim
            inside = True
            for j in range(ndim):
                bit = (c >> j) & 1
                wj = f[i, j] if bit else one - f[i, j]
                w = wj if w is None else w * wj                             # ((wx * wy) * wz)
                v = bi[j] + bit
                inside = inside and 0 <= v < shape_zyx[ndim - 1 - j]
                coord[ndim - 1 - j] = v
            r = table.get((int(b[i]), *coord), -1) if inside else -1
            if r >= 0:
                rows[i, c] = r
                weights[i, c] = w
                present.append(c)
        if normalize:
            s = ftype(0.0)
            for c in present:
                s = s + weights[i, c]
            if s == 0:
                rows[i, :] = -1
                weights[i, :] = 0
            else:
                for c in present:
                    weights[i, c] = weights[i, c] / s
    return rows, weights


def forward(vfeat, rows, weights, acc=np.float32):
    """out[i] = sum over ascending c of weights[i, c] * vfeat[rows[i, c]] in `acc` arithmetic (vfeat already raised to
    it, exactly), acc = acc + (w * x) from zero; corners with a row outside [0, n) are skipped.  Not yet rounded into
    the feature type."""
    vfeat = np.asarray(vfeat, dtype=acc)
    n = vfeat.shape[0]
    N, K = rows.shape
    out = np.zeros((N, vfeat.shape[1]), dtype=acc)
    for c in range(K):
        r = rows[:, c]
        m = (r >= 0) & (r < n)
        out[m] = out[m] + (weights[m, c].astype(acc)[:, None] * vfeat[r[m]])
    return out


def transposed(rows, n):
    """offsets [n + 1], list: the entries e = i * K + c of every voxel in ascending e (what spx_point_groups returns
    over the flattened corner table)"""
    flat = rows.reshape(-1).astype(np.int64)
    ok = (flat >= 0) & (flat < n)
    key = np.where(ok, flat, n)
    order = np.argsort(key, kind="stable")
    offsets = np.searchsorted(key[order], np.arange(n + 1), side="left")
    return offsets, order[:offsets[-1]]


def backward(dout, rows, weights, n, n_live=None, acc=np.float32):
    """dvfeat[v] = sum over the entries of voxel v's group, in list order, of weights_flat[e] * dout[e // K]; zeros for
    an empty group and for rows at or beyond n_live.  A sequential loop, entry by entry."""
    dout = np.asarray(dout, dtype=acc)
    K = rows.shape[1]
    wflat = weights.reshape(-1).astype(acc)
    offsets, lst = transposed(rows, n)
    live = n if n_live is None else min(int(n_live), n)
    dv = np.zeros((n, dout.shape[1]), dtype=acc)
    for v in range(live):
        a = np.zeros((dout.shape[1],), dtype=acc)
        for e in lst[offsets[v]:offsets[v + 1]]:
            a = a + (wflat[e] * dout[e // K])
        dv[v] = a
    return dv
