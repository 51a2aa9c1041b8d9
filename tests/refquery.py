"""A plain numpy restatement of the voxel query and the neighbour grouping (csrc/query.hip), for the tests: loops over
queries and window cells, numpy float32 SCALARS (every multiply, add, subtract and divide is rounded on its own, which
is the contract), the gather, and the gradient as a sequential sum over the entries.  Nothing here is fast."""
import numpy as np

f32 = np.float32


def keys_of(idx, shape):
    key = idx[:, 0].astype(np.int64)
    for d, s in enumerate(shape):
        key = key * int(s) + idx[:, 1 + d]
    return key


def live_table(indices, n_live, batch, shape):
    """key -> row of the live rows (below n_live, batch index and coordinates in range); a key held twice goes to the
    LOWEST row"""
    n = len(indices)
    live = n if n_live is None else min(int(n_live), n)
    idx = np.asarray(indices[:live]).astype(np.int64)
    ok = (idx[:, 0] >= 0) & (idx[:, 0] < batch)
    for d, s in enumerate(shape):
        ok &= (idx[:, 1 + d] >= 0) & (idx[:, 1 + d] < s)
    table = {}
    keys = keys_of(idx, shape)
    for r in np.nonzero(ok)[0][::-1]:
        table[int(keys[r])] = int(r)
    return table


def query_cell(q, b, vsize_xyz, lo_xyz, batch, shape):
    """the query's own cell by grid axis (zyx), or None for an invalid query"""
    ndim = len(shape)
    if not 0 <= int(b) < batch:
        return None
    cell = [0] * ndim
    for j in range(ndim):
        t = (f32(q[j]) - f32(lo_xyz[j])) / f32(vsize_xyz[j])
        c = np.floor(t)
        if not (c >= f32(0) and c < f32(shape[ndim - 1 - j])):       # (false for NaN)
            return None
        cell[ndim - 1 - j] = int(c)
    return cell


def query(queries, batch_ids, n_queries, vsize_xyz, lo_xyz, indices, n_live, batch, shape, query_range, nsample,
          radius=None, pad="none"):
    """rows int32 [M, nsample], count int32 [M], offsets float32 [M, nsample, ndim], and two diagnostics the kernel does
    not return: hits [M] (the hits of the whole window, before the cut at nsample) and rejected [M] (occupied window
    cells that the radius turned down)"""
    ndim, M = len(shape), len(queries)
    table = live_table(indices, n_live, batch, shape)
    with np.errstate(all="ignore"):
        r2 = None if radius is None else f32(radius) * f32(radius)
        vs, lo = [f32(v) for v in vsize_xyz], [f32(v) for v in lo_xyz]
        rows = np.full((M, nsample), -1, dtype=np.int32)
        count = np.zeros(M, dtype=np.int32)
        offsets = np.zeros((M, nsample, ndim), dtype=f32)
        hits, rejected = np.zeros(M, dtype=np.int64), np.zeros(M, dtype=np.int64)
        nq = M if n_queries is None else min(int(n_queries), M)
        for m in range(nq):
            b = 0 if batch_ids is None else int(batch_ids[m])
            cell = query_cell(queries[m], b, vsize_xyz, lo_xyz, batch, shape)
            if cell is None:
                continue
            q = [f32(queries[m][j]) for j in range(ndim)]
            spans = [range(max(cell[d] - query_range[d], 0), min(cell[d] + query_range[d], shape[d] - 1) + 1)
                     for d in range(ndim)]
            outer = [(v0,) for v0 in spans[0]] if ndim == 2 else [(v0, v1) for v0 in spans[0] for v1 in spans[1]]
            k = 0
            for lead in outer:                                      # ascending linear key: the last axis innermost
                base = b
                for d, v in enumerate(lead):
                    base = base * shape[d] + v
                base *= shape[ndim - 1]
                for vx in spans[ndim - 1]:
                    r = table.get(base + vx)
                    if r is None:
                        continue
                    v = list(lead) + [vx]
                    d_ = [((f32(v[ndim - 1 - j]) + f32(0.5)) * vs[j] + lo[j]) - q[j] for j in range(ndim)]
                    if r2 is not None:
                        d2 = d_[0] * d_[0] + d_[1] * d_[1]
                        if ndim == 3:
                            d2 = d2 + d_[2] * d_[2]
                        if not d2 < r2:
                            rejected[m] += 1
                            continue
                    if k < nsample:
                        rows[m, k] = r
                        offsets[m, k] = d_
                        k += 1
                    hits[m] += 1
            count[m] = k
    if pad == "first":
        rows, offsets = pad_first(rows, count, offsets)
    return rows, count, offsets, hits, rejected


def pad_first(rows, count, offsets):
    """the slots at or beyond count repeat slot 0 where count > 0 (copies; the inputs stay as they are)"""
    rows, offsets = rows.copy(), offsets.copy()
    for m in np.nonzero(count > 0)[0]:
        rows[m, count[m]:] = rows[m, 0]
        offsets[m, count[m]:] = offsets[m, 0]
    return rows, offsets


def group(vfeat, rows):
    """out[m, s] = vfeat[rows[m, s]], zeros for -1: works on any array whose rows are to be moved (bit patterns too)"""
    out = np.zeros(rows.shape + vfeat.shape[1:], dtype=vfeat.dtype)
    ok = rows >= 0
    out[ok] = vfeat[rows[ok]]
    return out


def transposed(rows, n):
    """offsets [n + 1] and list: the entries e of the flattened rows by voxel, ascending e inside a voxel"""
    flat = rows.reshape(-1)
    e = np.nonzero((flat >= 0) & (flat < n))[0]
    order = np.argsort(flat[e], kind="stable")
    offsets = np.zeros(n + 1, dtype=np.int64)
    np.add.at(offsets, flat[e] + 1, 1)
    return np.cumsum(offsets).astype(np.int32), e[order].astype(np.int32)


def group_backward(dout, rows, n, n_live=None, acc=np.float32):
    """dvfeat[v] = the sum of dout[e] over the entries e of voxel v, one addition after the other in ascending e in the
    accumulator type; zeros for rows at or beyond n_live.  dout [M * nsample, C] in the accumulator type."""
    flat = rows.reshape(-1)
    dout = dout.reshape(len(flat), -1)
    live = n if n_live is None else min(int(n_live), n)
    out = np.zeros((n, dout.shape[1]), dtype=acc)
    for e in range(len(flat)):
        r = flat[e]
        if 0 <= r < live:
            out[r] = out[r] + dout[e].astype(acc)
    return out
