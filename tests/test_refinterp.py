"""CPU: the numpy restatement of trilinear devoxelisation (tests/refinterp.py) checked on its own, before the kernels
are held to it: partition of unity, a point at a voxel centre, the point's own voxel among its corners, and exactness
on linear functions."""
import itertools

import numpy as np
import pytest

import refinterp as ri

ULP = float(np.spacing(np.float32(1.0)))        # 2^-23


def full_level(batch, shape):
    """every cell of the grid as a row, in key order"""
    idx = np.array([(b, *c) for b in range(batch) for c in itertools.product(*[range(s) for s in shape])], dtype=np.int32)
    return idx


def interior_points(rng, n, shape_zyx, vs, lo):
    """points whose 2^ndim corners all lie inside the grid: t in [0.5, extent - 0.5)"""
    ndim = len(shape_zyx)
    ext = np.asarray(shape_zyx[::-1], dtype=np.float64)
    t = 0.5 + rng.random((n, ndim)) * (ext - 1.0) * 0.999
    return (t * np.asarray(vs, dtype=np.float64) + np.asarray(lo, dtype=np.float64)).astype(np.float32)


@pytest.mark.parametrize("ndim", [2, 3])
@pytest.mark.parametrize("normalize", [False, True])
def test_weights_of_a_full_corner_set_sum_to_one(ndim, normalize):
    rng = np.random.default_rng(ndim)
    shape = [5, 7, 6][:ndim]
    vs, lo = [0.3, 0.25, 0.7][:ndim], [-1.7, 2.3, 0.4][:ndim]
    idx = full_level(1, shape)
    pts = interior_points(rng, 400, shape, vs, lo)
    rows, w = ri.corners(pts, None, None, vs, lo, idx, None, 1, shape, normalize)
    full = (rows >= 0).all(axis=1)
    assert full.sum() > 300
    K = 1 << ndim
    total = w[full].astype(np.float64).sum(axis=1)
    assert np.abs(total - 1.0).max() <= (2 if normalize else K) * ULP


@pytest.mark.parametrize("ndim", [2, 3])
def test_a_point_at_a_voxel_centre_reads_its_own_voxel(ndim):
    shape = [4, 5, 6][:ndim]
    vs, lo = [0.5, 0.25, 2.0][:ndim], [-1.0, 3.0, 0.5][:ndim]       # binary fractions: the centres are exact in fp32
    idx = full_level(2, shape)
    cells = idx[:, 1:][:, ::-1].astype(np.float64)                  # xyz
    pts = ((cells + 0.5) * np.asarray(vs) + np.asarray(lo)).astype(np.float32)
    b = idx[:, 0].astype(np.int32)
    for normalize in (False, True):
        rows, w = ri.corners(pts, b, None, vs, lo, idx, None, 2, shape, normalize)
        np.testing.assert_array_equal(rows[:, 0], np.arange(len(idx)))
        assert (w[:, 0] == np.float32(1.0)).all() and (w[:, 1:] == 0).all()


@pytest.mark.parametrize("ndim", [2, 3])
def test_the_points_own_voxel_is_among_its_corners(ndim):
    rng = np.random.default_rng(7 + ndim)
    shape = [8, 20, 24][:ndim]
    vs, lo = [0.3] * ndim, [-1.7, 2.3, 0.4][:ndim]
    idx = full_level(1, shape)
    ext = np.asarray(shape[::-1], dtype=np.float64)
    pts = ((rng.random((2000, ndim)) * 1.2 - 0.1) * ext * 0.3 + np.asarray(lo)).astype(np.float32)
    pts[:50] = (np.floor(rng.random((50, ndim)) * ext) * np.float32(0.3) + np.asarray(lo, dtype=np.float32))   # on cell faces
    rows, _ = ri.corners(pts, None, None, vs, lo, idx, None, 1, shape, False)
    t = (pts.astype(np.float32) - np.asarray(lo, dtype=np.float32)) / np.asarray(vs, dtype=np.float32)
    cell = np.floor(t).astype(np.int64)                             # xyz
    inside = ((cell >= 0) & (cell < ext)).all(axis=1)
    assert 1000 < inside.sum() < 2000
    own = np.zeros(len(pts), dtype=np.int64)
    for d in range(ndim):                                           # key of the own voxel = its row on the full level
        own = own * shape[d] + cell[:, ndim - 1 - d]
    assert (rows[inside] == own[inside, None]).any(axis=1).all()
    assert (rows[~inside] == -1).all()


@pytest.mark.parametrize("ndim", [2, 3])
def test_linear_functions_are_reproduced_in_float64(ndim):
    rng = np.random.default_rng(11 + ndim)
    shape = [5, 6, 7][:ndim]
    vs, lo = [0.3, 0.45, 0.2][:ndim], [-1.7, 2.3, 0.4][:ndim]
    idx = full_level(1, shape)
    centres = (idx[:, 1:][:, ::-1].astype(np.float64) + 0.5) * np.asarray(vs) + np.asarray(lo)     # xyz
    coef = rng.standard_normal((ndim, 3))
    linear = lambda xyz: xyz @ coef + np.array([0.5, -2.0, 1.25])
    pts = interior_points(rng, 300, shape, vs, lo).astype(np.float64)
    for normalize in (False, True):
        rows, w = ri.corners(pts, None, None, vs, lo, idx, None, 1, shape, normalize, ftype=np.float64)
        assert (rows >= 0).all()
        out = ri.forward(linear(centres), rows, w, acc=np.float64)
        assert np.abs(out - linear(pts)).max() <= 1e-12


def test_transposed_list_and_sequential_sums_agree_with_a_dense_product():
    rng = np.random.default_rng(3)
    n, N, K, C = 9, 40, 8, 3
    rows = rng.integers(-1, n, (N, K)).astype(np.int32)
    w = np.where(rows >= 0, rng.random((N, K)), 0).astype(np.float32)
    offsets, lst = ri.transposed(rows, n)
    flat = rows.reshape(-1)
    for v in range(n):
        np.testing.assert_array_equal(lst[offsets[v]:offsets[v + 1]], np.nonzero(flat == v)[0])
    dense = np.zeros((N, n))
    for i in range(N):
        for c in range(K):
            if rows[i, c] >= 0:
                dense[i, rows[i, c]] += w[i, c]
    vfeat, dout = rng.standard_normal((n, C)), rng.standard_normal((N, C))
    np.testing.assert_allclose(ri.forward(vfeat, rows, w, acc=np.float64), dense @ vfeat, atol=1e-12)
    np.testing.assert_allclose(ri.backward(dout, rows, w, n, acc=np.float64), dense.T @ dout, atol=1e-12)
    assert (ri.backward(dout, rows, w, n, n_live=4, acc=np.float64)[4:] == 0).all()
