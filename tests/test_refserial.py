"""CPU: tests/refserial.py (the restatement the serialisation kernels are compared with) against properties of the
curves themselves -- anchors computed by hand-checked runs of Skilling's algorithm, bijection, unit steps, the nesting
of levels."""
import itertools

import pytest

import refserial as R

ANCHORS = [
    (2, (0, 0, 0), "hilbert", 0),
    (2, (0, 1, 0), "hilbert", 1),
    (2, (1, 1, 0), "hilbert", 2),
    (2, (0, 1, 1), "hilbert", 6),
    (2, (0, 0, 1), "hilbert", 7),
    (2, (3, 3, 3), "hilbert", 45),
    (2, (3, 0, 0), "hilbert", 63),
    (3, (3, 5), "hilbert", 28),
    (11, (5, 9, 1000), "hilbert", 1073733990),
    (11, (1407, 1599, 40), "hilbert", 4718963346),
    (16, (65535, 0, 12345), "hilbert", 279423209514058),
    (11, (5, 9, 1000), "z", 153388806),
]

GRIDS = [(ndim, depth) for ndim in range(1, 5) for depth in range(1, 5) if ndim * depth <= 14]


def _cells(ndim, depth):
    return itertools.product(range(1 << depth), repeat=ndim)


@pytest.mark.parametrize("depth,coords,order,code", ANCHORS)
def test_anchors(depth, coords, order, code):
    fn = R.hilbert_code if order == "hilbert" else R.z_code
    assert fn(coords, depth) == code


def test_first_cells_of_the_3d_curve():
    want = [(0, 0, 0), (0, 1, 0), (1, 1, 0), (1, 0, 0), (1, 0, 1), (1, 1, 1), (0, 1, 1), (0, 0, 1), (0, 0, 2)]
    by_code = {R.hilbert_code(c, 2): c for c in _cells(3, 2)}
    assert [by_code[t] for t in range(9)] == want


@pytest.mark.parametrize("ndim,depth", GRIDS)
def test_hilbert_is_a_bijection_of_unit_steps(ndim, depth):
    by_code = {}
    for c in _cells(ndim, depth):
        by_code[R.hilbert_code(c, depth)] = c
    total = 1 << (ndim * depth)
    assert sorted(by_code) == list(range(total))
    assert by_code[0] == (0,) * ndim
    for t in range(1, total):
        assert sum(abs(a - b) for a, b in zip(by_code[t], by_code[t - 1])) == 1, t


@pytest.mark.parametrize("ndim,depth", [(nd, d) for nd in (2, 3) for d in (2, 3, 4)])
def test_hilbert_levels_nest(ndim, depth):
    """A pooled level can shift its parent's codes: the parent cell's code is the child's without its last ndim bits."""
    for c in _cells(ndim, depth):
        assert R.hilbert_code([v >> 1 for v in c], depth - 1) == R.hilbert_code(c, depth) >> ndim


@pytest.mark.parametrize("ndim,depth", GRIDS)
def test_z_is_a_bijection(ndim, depth):
    seen = sorted(R.z_code(c, depth) for c in _cells(ndim, depth))
    assert seen == list(range(1 << (ndim * depth)))


def test_axes_and_trans():
    assert R.curve_axes(3, "z") == [2, 1, 0] and R.curve_axes(3, "hilbert-trans") == [1, 2, 0]
    assert R.curve_axes(1, "z-trans") == [0]
    assert R.curve_axes(3, "z-trans", (0, 1, 2)) == [1, 0, 2]
    assert R.default_depth([41, 1600, 1408]) == 11 and R.default_depth([1, 1]) == 1
    assert R.key_bits(3, 11, 4) == 36 and R.key_bits(3, 16, 32767) == 63


def test_serialize_and_plan_on_a_small_case():
    idx = [[0, 0, 0, 1], [1, 0, 0, 0], [0, 0, 0, 0], [-1, 0, 0, 0], [0, 0, 4, 0], [1, 0, 0, 0]]
    code, order, inverse, offsets = R.serialize(idx, 3, 2, orders=("z",))
    assert code[0].tolist() == [4, 64, 0, -1, -1, 64]           # x is the most significant axis
    assert order[0].tolist() == [2, 0, 1, 5, 3, 4] and offsets.tolist() == [0, 2, 4, 4]
    assert [int(inverse[0][order[0][t]]) for t in range(6)] == list(range(6))
    plan = R.patch_plan(order[0], offsets, 2)
    assert plan["n_patches"] == 2 and plan["patch_rows"].shape == (6, 2)
    assert plan["patch_rows"][:2].tolist() == [[2, 0], [1, 5]] and plan["patch_scene"].tolist() == [0, 1, -1, -1, -1, -1]
    plan = R.patch_plan([0, 1, 2], [0, 3], 2, "borrow")
    assert plan["patch_rows"].tolist() == [[0, 1], [2, 1]]
    assert plan["patch_rows_canon"].tolist() == [[0, 1], [2, -1]]
    assert plan["row_slot"].tolist() == [0, 1, 2] and plan["row_slot2"].tolist() == [-1, 3, -1]
    assert R.patch_plan([0, 1, 2], [0, 3], 2, "mask")["patch_rows"].tolist() == [[0, 1], [2, -1]]
