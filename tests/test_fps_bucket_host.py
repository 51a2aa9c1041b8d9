"""CPU: the argument checks of the bucket path of farthest-point sampling (csrc/fps_bucket.hip) come before any pointer
is looked at (no kernel is launched in this file); the Python layer has the new names and refuses bad arguments."""
import pytest

from capi import fails as _fails
from spconv_amd import _lib


def test_constants_and_ws_bytes():
    L = _lib.load()
    cap, size = L.spx_fps_bucket_cap(), L.spx_fps_bucket_points()
    assert cap > 1024 and size == 64                                 # (a lane may own two buckets; a bucket is whole waves)
    ws, limit = L.spx_fps_bucket_ws_bytes, cap * (size << 8)
    ns = (0, 1, 63, 64, 65, cap * size, cap * size + 1, 300_000, limit)
    for ndim in (2, 3):
        for batch in (1, 4, 64):
            sizes = [ws(n, batch, ndim) for n in ns]
            assert sizes == sorted(sizes) and sizes[0] > 0, sizes
            assert all(s >= 36 * n for s, n in zip(sizes, ns))      # record, point index, key, order, inverse per point
    assert ws(10, 4, 1) == 0 and ws(10, 4, 4) == 0 and ws(-1, 4, 3) == 0 and ws(10, 0, 3) == 0 and ws(limit + 1, 4, 3) == 0


def test_argument_checks_need_no_pointer():
    L = _lib.load()
    limit = L.spx_fps_bucket_cap() * (L.spx_fps_bucket_points() << 8)

    def build(nfeat=4, n_cap=100, ndim=3, batch=2):
        return L.spx_fps_bucket_build(None, nfeat, n_cap, ndim, None, None, batch, None, 0, None)

    def sample(n_cap=100, ndim=3, batch=2, K=16):
        return L.spx_fps_bucket(n_cap, ndim, batch, K, None, None, None, None, 0, None)
    for call in (build, sample):
        _fails(call(ndim=1), "ndim")
        _fails(call(ndim=4), "ndim")
        _fails(call(n_cap=-1), "counts")
        _fails(call(batch=0), "batch")
        _fails(call(n_cap=limit + 1), "buckets")
        _fails(call(), "NULL")                                       # data is required, the pointers are null: no launch
        _fails(call(n_cap=0), "NULL")
    _fails(build(nfeat=2), "columns")
    _fails(sample(K=0), "num_samples")
    _fails(sample(K=65_537), "num_samples")
    _fails(sample(batch=1 << 15, K=65_536), "2^31")


def test_python_names_and_refusals():
    import torch
    import spconv_amd
    import spconv_amd.pytorch as sp
    from spconv_amd.pytorch import functional as F
    p, bid = torch.zeros((20, 4)), torch.zeros((20,), dtype=torch.int32)
    for method in ("nonsense", None, "Bucket"):
        with pytest.raises(ValueError, match="method"):
            F.farthest_point_sample_method(p, bid, 2, 4, method)
        with pytest.raises(ValueError, match="method"):
            sp.FarthestPointSample(16, method=method)
    with pytest.raises(ValueError, match="with_visits"):
        F.farthest_point_sample_method(p, bid, 2, 4, "scan", with_visits=True)
    with pytest.raises(ValueError, match="num_samples"):
        F.farthest_point_sample_method(p, bid, 2, 0, "bucket")
    for method in ("scan", "bucket"):
        with pytest.raises(NotImplementedError, match="MI355X"):     # every check passed: there is no CPU path
            F.farthest_point_sample_method(p, bid, 2, 4, method)
    assert sp.FarthestPointSample(16).method == "scan" and "method=bucket" in repr(sp.FarthestPointSample(16, method="bucket"))
    assert callable(F.fps_bucket_into)
    spconv_amd.install_as_spconv()
    import spconv.pytorch as spconv
    assert spconv.farthest_point_sample_method is F.farthest_point_sample_method
    assert spconv.functional.fps_bucket_into is F.fps_bucket_into
