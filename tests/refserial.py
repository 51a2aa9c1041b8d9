"""A plain-Python restatement of voxel serialisation (csrc/serialize.hip): curve codes, keys, orders, offsets and the
patch plan, written as loops over rows, bits and axes on Python integers -- nothing here is shaped like the kernels.
tests/test_refserial.py holds it to properties of the curves; tests/test_gpu_serialize.py holds the kernels to it.

Coordinates handed to a curve are in the curve's own axis order: X[0] is the most significant axis.
"""
import numpy as np

ORDERS = ("z", "z-trans", "hilbert", "hilbert-trans")
DEAD_KEY = (1 << 64) - 1


def interleave(X, depth):
    """Bit b of X[j] lands at bit b * ndim + (ndim - 1 - j): MSB first, X[0] ahead."""
    ndim = len(X)
    code = 0
    for b in range(depth):
        for j in range(ndim):
            code |= ((X[j] >> b) & 1) << (b * ndim + (ndim - 1 - j))
    return code


def z_code(coords, depth):
    return interleave([int(c) for c in coords], depth)


def hilbert_code(coords, depth):
    """Skilling's AxesToTranspose (AIP Conf. Proc. 707, 2004), then the transposed bits interleaved."""
    X = [int(c) for c in coords]
    n = len(X)
    M = 1 << (depth - 1)
    Q = M
    while Q > 1:                     # inverse undo
        P = Q - 1
        for i in range(n):
            if X[i] & Q:
                X[0] ^= P
            else:
                t = (X[0] ^ X[i]) & P
                X[0] ^= t
                X[i] ^= t
        Q >>= 1
    for i in range(1, n):            # Gray encode
        X[i] ^= X[i - 1]
    t = 0
    Q = M
    while Q > 1:
        if X[n - 1] & Q:
            t ^= Q - 1
        Q >>= 1
    for i in range(n):
        X[i] ^= t
    return interleave(X, depth)


def curve_axes(ndim, order, axes=None):
    """Spatial axes (0 = the first spatial index column) in the order the curve takes them."""
    ax = list(range(ndim - 1, -1, -1)) if axes is None else [int(a) for a in axes]
    if order.endswith("-trans") and ndim >= 2:
        ax[0], ax[1] = ax[1], ax[0]
    return ax


def default_depth(spatial_shape):
    return max(1, (max(int(v) for v in spatial_shape) - 1).bit_length())


def key_bits(ndim, depth, batch_size):
    return ndim * depth + int(batch_size).bit_length()


def codes(indices, batch_size, depth, orders=ORDERS, axes=None, n_live=None):
    """code [K][n] as Python integers: (batch << (ndim * depth)) | curve code, -1 for a dead row."""
    indices = np.asarray(indices)
    n, ndim = indices.shape[0], indices.shape[1] - 1
    live = n if n_live is None else min(int(n_live), n)
    rows = indices.tolist()
    out = []
    for order in orders:
        ax = curve_axes(ndim, order, axes)
        fn = hilbert_code if order.startswith("hilbert") else z_code
        line = []
        for i in range(n):
            row = rows[i]
            b = row[0]
            dead = i >= live or b < 0 or b >= batch_size
            for c in row[1:]:
                if c < 0 or c >= (1 << depth):
                    dead = True
            if dead:
                line.append(-1)
            else:
                line.append((b << (ndim * depth)) | fn([row[1 + a] for a in ax], depth))
        out.append(line)
    return out


def serialize(indices, batch_size, depth, orders=ORDERS, axes=None, n_live=None):
    """(code int64 [K, n], order int32 [K, n], inverse int32 [K, n], offsets int32 [batch_size + 1])."""
    code = codes(indices, batch_size, depth, orders, axes, n_live)
    n = len(code[0]) if code else 0
    order, inverse = [], []
    for line in code:
        key = [DEAD_KEY if c < 0 else c for c in line]
        o = sorted(range(n), key=lambda i: key[i])          # (stable: equal keys stay in ascending row)
        inv = [0] * n
        for t in range(n):
            inv[o[t]] = t
        order.append(o)
        inverse.append(inv)
    count = [0] * batch_size
    shift = (np.asarray(indices).shape[1] - 1) * depth
    for c in (code[0] if code else []):
        if c >= 0:
            count[c >> shift] += 1
    offsets = [0] * (batch_size + 1)
    for b in range(batch_size):
        offsets[b + 1] = offsets[b] + count[b]
    K = len(code)
    return (np.array(code, dtype=np.int64).reshape(K, n), np.array(order, dtype=np.int32).reshape(K, n),
            np.array(inverse, dtype=np.int32).reshape(K, n), np.array(offsets, dtype=np.int32))


def patch_plan(order, offsets, patch_size, pad="borrow"):
    """The fixed-shape patch layout over one order row: dict of patch_rows / patch_rows_canon [P_cap, K], row_slot /
    row_slot2 [n], patch_scene [P_cap], n_patches."""
    order = [int(v) for v in order]
    offsets = [int(v) for v in offsets]
    n, B, K = len(order), len(offsets) - 1, int(patch_size)
    P_cap = n // K + B
    rows = [[-1] * K for _ in range(P_cap)]
    canon = [[-1] * K for _ in range(P_cap)]
    slot, slot2, scene = [-1] * n, [-1] * n, [-1] * P_cap
    p0 = 0
    for b in range(B):
        beg, c = offsets[b], offsets[b + 1] - offsets[b]
        np_b = (c + K - 1) // K
        for p in range(np_b):
            scene[p0 + p] = b
            for j in range(K):
                q = p * K + j
                s = (p0 + p) * K + j
                if q < c:
                    r = order[beg + q]
                    rows[p0 + p][j] = canon[p0 + p][j] = r
                    slot[r] = s
                elif pad == "borrow" and c >= K:
                    r = order[beg + q - K]
                    rows[p0 + p][j] = r
                    slot2[r] = s
        p0 += np_b
    i32 = lambda v, shape: np.array(v, dtype=np.int32).reshape(shape)
    return dict(patch_rows=i32(rows, (P_cap, K)), patch_rows_canon=i32(canon, (P_cap, K)), row_slot=i32(slot, (n,)),
                row_slot2=i32(slot2, (n,)), patch_scene=i32(scene, (P_cap,)), n_patches=p0)
