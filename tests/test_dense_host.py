"""CPU: the dense-conversion entry points exist on every layer (header, binding, library), their host-side answers
are right, and CPU tensors keep torch's code in dense() / from_dense (no kernel is launched in this file)."""
import os
import re

import pytest
import torch

from spconv_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["spx_dense_ws_bytes", "spx_dense_map", "spx_to_dense", "spx_dense_gather", "spx_from_dense_ws_bytes",
           "spx_from_dense_count", "spx_from_dense_fill"]


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


def test_entries_are_declared_bound_and_built(lib):
    header = open(os.path.join(ROOT, "include", "spconv_amd.h")).read()
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert getattr(lib, name) is not None
    units = {os.path.splitext(os.path.basename(o))[0] for o in _lib.linked_objects()}
    assert "dense" in units


def test_map_workspace_size(lib):
    I = _lib.ints
    al = lambda b: (b + 255) // 256 * 256
    assert lib.spx_dense_ws_bytes(3, 1, I([41, 1600, 1408])) == al(4 * 41 * 1600 * 1408)     # one int32 per cell
    assert lib.spx_dense_ws_bytes(3, 2, I([3, 5, 7])) == al(4 * 210)
    assert lib.spx_dense_ws_bytes(1, 1, I([1])) == 256
    assert lib.spx_dense_ws_bytes(3, 2, I([8, 0, 8])) == 0 and lib.spx_dense_ws_bytes(2, 0, I([8, 8])) == 0
    assert lib.spx_dense_ws_bytes(3, 64, I([41, 1600, 1408])) == 0        # more than 2^31 - 1 cells: no map
    assert lib.spx_dense_ws_bytes(5, 1, I([2] * 5)) == 0                  # ndim outside 1..4
    # compaction scratch: a flag per cell and two counters per 256 cells
    assert 4 * 210 < lib.spx_from_dense_ws_bytes(3, 2, I([3, 5, 7])) <= al(4 * 210) + 3 * 256
    assert lib.spx_from_dense_ws_bytes(3, 2, I([8, 0, 8])) <= 3 * 256


def test_bad_arguments_are_errors_not_launches(lib):
    I = _lib.ints
    before = lib.spx_launch_count(b"dense/map")
    assert lib.spx_dense_map(None, 0, None, 7, 1, I([2] * 3), None, None) != 0 and b"ndim" in lib.spx_last_error()
    assert lib.spx_dense_map(None, 0, None, 3, 64, I([41, 1600, 1408]), None, None) != 0
    assert b"2^31" in lib.spx_last_error()
    assert lib.spx_to_dense(None, 0, 4, None, None, 4, 3, 1, 0, 3, 1, I([2] * 3), None) != 0          # 3-byte elements
    assert b"element size" in lib.spx_last_error()
    assert lib.spx_dense_gather(None, None, None, 0, 4, 16, 1, 3, 1, I([2] * 3), None) != 0
    # empty problems return at once
    assert lib.spx_dense_map(None, 0, None, 3, 1, I([4, 0, 4]), None, None) == 0
    assert lib.spx_to_dense(None, 0, 4, None, None, 4, 2, 1, 0, 3, 1, I([4, 0, 4]), None) == 0
    assert lib.spx_dense_gather(None, None, None, 0, 4, 2, 1, 3, 1, I([4, 4, 4]), None) == 0
    assert lib.spx_launch_count(b"dense/map") == before


def test_launch_counter_keys(lib):
    for k in ("dense/map", "dense/scatter_cl", "dense/scatter_cf", "dense/gather_cl", "dense/gather_cf", "dense/compact"):
        assert lib.spx_launch_count(k.encode()) >= 0, k
    for bad in ("dense", "dense/", "dense/scatter", "dense/map/1"):
        assert lib.spx_launch_count(bad.encode()) == -1, bad


def test_cpu_tensors_keep_torch_indexing():
    import spconv_amd.pytorch as spconv
    from spconv_amd.pytorch import _dense
    g = torch.Generator().manual_seed(0)
    B, spatial, C, n = 2, [3, 5, 7], 4, 50
    pick = torch.randperm(B * 105, generator=g)[:n]
    idx = torch.stack([pick // 105, pick % 105 // 35, pick % 35 // 7, pick % 7], 1).int()
    f = torch.randn((n, C), generator=g) + 3.0
    assert not _dense.supported(f)
    want = torch.zeros([B] + spatial + [C])
    want[tuple(idx[:, i].long() for i in range(4))] = f
    x = spconv.SparseConvTensor(f, idx, spatial, B)
    assert torch.equal(x.dense(channels_first=False), want)
    assert torch.equal(x.dense(), want.permute(0, 4, 1, 2, 3).contiguous())
    assert torch.equal(spconv.ToDense()(x), x.dense())
    y = spconv.SparseConvTensor.from_dense(want)
    sp = want.to_sparse(4)
    assert torch.equal(y.indices, sp.indices().T.int()) and torch.equal(y.features, sp.values())
    assert y.batch_size == B and list(y.spatial_shape) == spatial
    assert torch.equal(y.dense(channels_first=False), want)
    with pytest.raises(NotImplementedError):
        _dense.to_dense(f, idx, B, spatial)
