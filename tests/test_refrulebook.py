"""The rulebook reference (refrulebook.py: pairs from the coordinates, plain Python) against the CPU oracle (oracle.cpp:
the reference's CPU loops restated), on the CPU.  The two share no code; tests/test_gpu_rulebook_matrix.py compares the
HIP builders with the first at small sizes and with the second where the first is too slow, which this file licenses."""
import numpy as np
import pytest

import refrulebook
from test_gpu_rulebook import CONV_CASES, SUBM_CASES, _far_corner_scene
from util import dense_scene, oracle_rulebook, scene

KEYS = ("out_inds", "pair", "num", "fwd", "bwd", "mfwd", "mbwd")


def same(ref, orc):
    assert (ref["n_in"], ref["n_out"]) == (orc["n_in"], orc["n_out"])
    assert list(ref["out_shape"]) == list(orc["out_shape"])
    for key in KEYS:
        assert ref[key].dtype == orc[key].dtype and ref[key].shape == orc[key].shape, key
        np.testing.assert_array_equal(ref[key], orc[key], err_msg=key)


def both(idx, bs, shape, ksize, stride, pad, dil, subm, transpose=False, out_padding=None):
    args = (idx, bs, shape, ksize, stride, pad, dil, subm, transpose, out_padding)
    ref, orc = refrulebook.rulebook(*args), oracle_rulebook(*args)
    same(ref, orc)
    return ref


def holes(idx, bs):
    """The scene with duplicate rows behind it, one deleted row and one row of a batch item that does not exist."""
    idx = np.concatenate([idx, idx[:50], idx[10:30]], axis=0)
    idx[5, 0] = -1
    idx[77, 0] = bs + 2
    return np.ascontiguousarray(idx)


@pytest.mark.parametrize("shape,n,bs,ksize,dil", SUBM_CASES)
def test_subm_cases(shape, n, bs, ksize, dil):
    nd = len(shape)
    pad = [(k // 2) * d for k, d in zip(ksize, dil)]
    ref = both(scene(shape, min(n, 300), bs, seed=3), bs, shape, ksize, [1] * nd, pad, dil, True)
    assert ref["num"][len(ref["num"]) // 2:].sum() == 0


@pytest.mark.parametrize("ksize", [[3, 3, 3], [1, 1, 1], [5, 5, 5], [5, 5, 7], [5, 3, 3], [3, 1, 3]])
def test_subm_dense_scenes(ksize):
    shape = [24, 24, 24]
    idx = dense_scene(shape, 250, 2, seed=5)
    ref = both(idx, 2, shape, ksize, [1] * 3, [k // 2 for k in ksize], [1] * 3, True)
    kv = int(np.prod(ksize))
    assert ref["pair"].shape[1] == kv
    if kv > 1:
        assert ref["num"].sum() > idx.shape[0]
    np.testing.assert_array_equal(ref["fwd"][kv // 2], np.arange(idx.shape[0]))


def test_subm_duplicates_and_dead_rows():
    shape = [36, 36, 36]
    idx = holes(dense_scene(shape, 400, 1, seed=9), 1)
    assert idx.shape[0] == 470
    ref = both(idx, 1, shape, [3] * 3, [1] * 3, [1] * 3, [1] * 3, True)
    assert (np.delete(ref["fwd"][:, [5, 77]], 13, 0) == -1).all()              # a dead row keeps its centre pair only
    # a later row of a coordinate is never FOUND (the out side of the lists below the centre) -- but row 405, the copy
    # of the deleted row 5, is the first live row of its coordinate
    found = ref["pair"][1, :13]
    assert set(found[found >= 400].tolist()) <= {405}


def test_subm_far_corner():
    shape = [3000, 2500, 2000]
    idx = _far_corner_scene(shape, 300, 2, seed=2)
    ref = both(idx, 2, shape, [3] * 3, [1] * 3, [1] * 3, [1] * 3, True)
    assert ref["num"].sum() > idx.shape[0]


@pytest.mark.parametrize("shape,n,bs,ksize,stride,pad,dil,transposed", CONV_CASES)
def test_conv_cases(shape, n, bs, ksize, stride, pad, dil, transposed):
    both(scene(shape, min(n, 300), bs, seed=11), bs, shape, ksize, stride, pad, dil, False, transposed)


CONV_MORE = [
    # shape, n, bs, ksize, stride, padding, dilation, transposed, out_padding
    ([301], 120, 2, [3], [2], [1], [1], False, None),                                   # 1-d: two candidates
    ([9, 8, 7, 6], 300, 1, [3] * 4, [2] * 4, [1] * 4, [1] * 4, False, None),            # 4-d: sixteen candidates
    ([10, 9, 9], 300, 2, [3] * 3, [2] * 3, [1] * 3, [1] * 3, True, [1, 1, 1]),          # transposed, out_padding
    ([10, 9, 9], 300, 1, [3] * 3, [2] * 3, [0] * 3, [1] * 3, True, [1, 0, 1]),
    ([31, 30, 29], 300, 1, [3] * 3, [2] * 3, [2] * 3, [2] * 3, False, None),            # 27 candidates
    ([19, 18, 17], 300, 1, [6] * 3, [2] * 3, [2] * 3, [1] * 3, False, None),            # kv = 216
    ([19, 18, 17], 300, 1, [5, 5, 5], [2] * 3, [2] * 3, [1] * 3, False, None),          # kv = 125
]


@pytest.mark.parametrize("shape,n,bs,ksize,stride,pad,dil,transposed,outpad", CONV_MORE)
def test_conv_more(shape, n, bs, ksize, stride, pad, dil, transposed, outpad):
    ref = both(scene(shape, n, bs, seed=7), bs, shape, ksize, stride, pad, dil, False, transposed, outpad)
    assert ref["n_out"] > 0


@pytest.mark.parametrize("transposed", [False, True])
def test_conv_duplicates_and_dead_rows(transposed):
    shape = [36, 36, 36]
    idx = holes(dense_scene(shape, 400, 1, seed=9), 1)
    ref = both(idx, 1, shape, [3] * 3, [2] * 3, [1] * 3, [1] * 3, False, transposed)
    assert (ref["bwd"][:, [5, 77]] == -1).all()


def test_conv_far_corner():
    shape = [4000, 4000, 4000]
    idx = _far_corner_scene(shape, 300, 1, seed=4)
    ref = both(idx, 1, shape, [3] * 3, [2] * 3, [1] * 3, [1] * 3, False)
    assert ref["out_shape"] == [2000] * 3
