"""Reference of the rulebook builders that derives every artefact from the coordinates alone.

Plain numpy and Python: a dict from coordinate to row, one loop per kernel offset.  Nothing of this project's is used
(not the C++ oracle, not the library), so a rulebook that equals this one is right for a reason that does not depend on
either.  Slow by design: meant for scenes of a few thousand voxels.

The pairs, as the reference's ConvAlgo.Native CPU loops define them (offsets k over ksize, last spatial axis fastest):
  rows       a row whose batch index lies outside [0, batch_size) is dead: it is never found and reaches nothing.  Of
             several rows with one coordinate only the FIRST is ever found.
  SubM       padding is (ksize // 2) * dilation.  For k below the centre kv // 2, in ascending row order: row i looks
             for the row j at x_i + (ksize // 2 - r_k) * dilation; a hit is the entry (in i, out j) of list k and the
             entry (in j, out i) of list kv - 1 - k.  The centre list is the identity over ALL rows.  Counts exist for
             k < kv // 2 only, the rest of num_per_loc is 0.
  regular    offset-major, then row-major: input x reaches y with y * s = x + p - r_k * d (y inside the output grid).
  transposed y = x * s - p + r_k * d.
             Outputs are numbered in the order in which that loop first sees them.
From the lists: pair [2, kv, n_in] (-1 behind a list's end), the dense tables fwd[k, out] = in and bwd[k, in] = out (-1
where no pair; where two pairs compete -- duplicate rows -- the earlier list entry stays) and the mask words (bit k % 32
of word k // 32: the table entry exists)."""
import itertools

import numpy as np


def out_spatial_shape(spatial_shape, ksize, stride, padding, dilation, subm, transpose=False, out_padding=None):
    if subm:
        return [int(v) for v in spatial_shape]
    out = []
    for a, n in enumerate(spatial_shape):
        if transpose:
            out.append((n - 1) * stride[a] - 2 * padding[a] + ksize[a] + (out_padding[a] if out_padding else 0))
        else:
            out.append((n + 2 * padding[a] - dilation[a] * (ksize[a] - 1) - 1) // stride[a] + 1)
    return out


def _subm_lists(rows, bs, dims, ksize, dilation):
    nd, n = len(dims), len(rows)
    offsets = list(itertools.product(*[range(k) for k in ksize]))
    kv = len(offsets)
    first = {}
    for i, row in enumerate(rows):
        if 0 <= row[0] < bs:
            first.setdefault(tuple(row), i)
    lists = [[] for _ in range(kv)]
    for k in range(kv // 2):
        step = [(ksize[a] // 2 - offsets[k][a]) * dilation[a] for a in range(nd)]
        direct, mirror = lists[k], lists[kv - 1 - k]
        for i, row in enumerate(rows):
            if not 0 <= row[0] < bs:
                continue
            q = [row[1 + a] + step[a] for a in range(nd)]
            if any(v < 0 or v >= dims[a] for a, v in enumerate(q)):
                continue
            j = first.get((row[0], *q))
            if j is not None:
                direct.append((i, j))
                mirror.append((j, i))
    lists[kv // 2] = [(i, i) for i in range(n)]
    counted = [len(lists[k]) if k < kv // 2 else 0 for k in range(kv)]
    return lists, counted


def _conv_lists(rows, bs, out_dims, ksize, stride, padding, dilation, transpose):
    nd = len(out_dims)
    offsets = list(itertools.product(*[range(k) for k in ksize]))
    outputs = {}                                   # coordinate -> output row, in first-seen order (dicts keep it)
    lists = []
    for r in offsets:
        entries = []
        for i, row in enumerate(rows):
            if not 0 <= row[0] < bs:
                continue
            q = []
            for a in range(nd):
                if transpose:
                    y = row[1 + a] * stride[a] - padding[a] + r[a] * dilation[a]
                else:
                    h = row[1 + a] + padding[a] - r[a] * dilation[a]
                    if h % stride[a]:
                        break
                    y = h // stride[a]
                if y < 0 or y >= out_dims[a]:
                    break
                q.append(y)
            else:
                entries.append((i, outputs.setdefault((row[0], *q), len(outputs))))
        lists.append(entries)
    return lists, [len(e) for e in lists], list(outputs)


def _artefacts(lists, n_in, n_out):
    kv = len(lists)
    words = (kv + 31) // 32
    pair = np.full((2, kv, n_in), -1, np.int32)
    fwd = np.full((kv, n_out), -1, np.int32)
    bwd = np.full((kv, n_in), -1, np.int32)
    mfwd = np.zeros((n_out, words), np.uint32)
    mbwd = np.zeros((n_in, words), np.uint32)
    for k, entries in enumerate(lists):
        bit = np.uint32(1 << (k % 32))
        for pos, (i, o) in enumerate(entries):
            pair[0, k, pos], pair[1, k, pos] = i, o
            if fwd[k, o] < 0:
                fwd[k, o] = i
            if bwd[k, i] < 0:
                bwd[k, i] = o
            mfwd[o, k // 32] |= bit
            mbwd[i, k // 32] |= bit
    return pair, fwd, bwd, mfwd, mbwd


def rulebook(idx, bs, shape, ksize, stride, padding, dilation, subm, transpose=False, out_padding=None):
    """The dict util.oracle_rulebook returns: out_inds, pair, num, out_shape, fwd, bwd, mfwd, mbwd, n_in, n_out."""
    idx = np.asarray(idx)
    nd = len(shape)
    assert idx.ndim == 2 and idx.shape[1] == nd + 1 and len(ksize) == nd
    rows = idx.tolist()
    n_in = len(rows)
    out_shape = out_spatial_shape(shape, ksize, stride, padding, dilation, subm, transpose, out_padding)
    if subm:
        assert all(k % 2 == 1 for k in ksize)
        lists, counted = _subm_lists(rows, bs, out_shape, ksize, dilation)
        out_inds = idx.astype(np.int32)
    else:
        lists, counted, outs = _conv_lists(rows, bs, out_shape, ksize, stride, padding, dilation, transpose)
        out_inds = np.asarray(outs, np.int32).reshape(len(outs), nd + 1)
    n_out = out_inds.shape[0]
    pair, fwd, bwd, mfwd, mbwd = _artefacts(lists, n_in, n_out)
    return dict(out_inds=out_inds, pair=pair, num=np.asarray(counted, np.int32), out_shape=out_shape, fwd=fwd, bwd=bwd,
                mfwd=mfwd, mbwd=mbwd, n_in=n_in, n_out=n_out)
