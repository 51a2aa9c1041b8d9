"""Misaligned add (csrc/union.hip): what can be checked without a GPU -- the unit is linked, the size query, the
launch-count keys, and the argument checks that come before anything touches the device."""
import ctypes
import os

import pytest

from spconv_amd import _lib


def test_union_unit_is_linked():
    units = {os.path.splitext(os.path.basename(o))[0] for o in _lib.linked_objects()}
    assert "union" in units


@pytest.mark.parametrize("batch,shape,fits", [
    (2, [3, 160, 160], True), (1, [7], True), (1, [41, 1600, 1408], True),
    (1, [0, 4, 4], False), (2, [4, 0], False),                       # an empty grid
    (1, [2048, 1024, 1024], False), (2, [1024, 1024, 1024], False),  # batch x grid >= 2^31 cells
    (4096, [1024, 512], False),
])
def test_ws_bytes(batch, shape, fits):
    L = _lib.load()
    got = L.spx_union_ws_bytes(len(shape), batch, _lib.ints(shape), 2, 1000)
    assert (got > 0) == fits
    assert (L.spx_rankmap_bytes(len(shape), batch, _lib.ints(shape)) > 0) == fits     # the same gate as the rank map's


def test_ws_bytes_grows_with_rows_and_refuses_bad_operand_counts():
    L = _lib.load()
    sp = _lib.ints([12, 14, 16])
    assert L.spx_union_ws_bytes(3, 2, sp, 8, 100000) > L.spx_union_ws_bytes(3, 2, sp, 2, 100)
    assert L.spx_union_ws_bytes(3, 2, sp, 0, 100) == 0
    assert L.spx_union_ws_bytes(3, 2, sp, 9, 100) == 0


def test_launch_count_keys():
    L = _lib.load()
    for key in ("union/mark", "union/prefix", "union/claim", "union/fill", "union/add_fwd", "union/add_bwd"):
        assert L.spx_launch_count(key.encode()) >= 0, key
    for key in ("union", "union/", "union/add", "union/add_fwd/", "union/mark/f16"):
        assert L.spx_launch_count(key.encode()) == -1, key


@pytest.mark.parametrize("T", [0, 9])
def test_operand_count_is_refused(T):
    """The checks run before any pointer is looked at: no device is needed to be told no."""
    L = _lib.load()
    sp = _lib.ints([4, 5, 6])
    n = _lib.ints([0] * max(T, 1))
    p = _lib.ptrs([None] * max(T, 1))
    result = (ctypes.c_int * 12)()
    calls = {
        "count": lambda: L.spx_union_count(p, n, None, T, 3, 1, sp, None, 0, None, 0, result, None),
        "fill": lambda: L.spx_union_fill(p, n, None, T, 3, 1, sp, 0, -1, None, p, None, None, 0, None, 0, None),
        "static": lambda: L.spx_union_static(p, n, None, T, 3, 1, sp, 4, None, p, None, None, None, 0, None, 0, None),
        "add_fwd": lambda: L.spx_union_add_fwd(p, n, T, None, 0, 4, _lib.DTYPE_F16, None, None, None),
        "add_bwd": lambda: L.spx_union_add_bwd(None, 0, p, p, n, T, 4, 2, None),
    }
    for name, call in calls.items():
        assert call() != 0, name
        with pytest.raises(RuntimeError, match="operands"):
            _lib.check(-1)
        assert "1 to 8" in L.spx_last_error().decode(), name


def test_bad_arguments_are_refused():
    L = _lib.load()
    p, n = _lib.ptrs([None]), _lib.ints([0])
    assert L.spx_union_add_fwd(p, n, 1, None, 4, 4, _lib.DTYPE_I8, None, None, None) != 0
    assert "dtype" in L.spx_last_error().decode()
    assert L.spx_union_add_bwd(None, 0, p, p, n, 1, 4, 1, None) != 0
    assert "element size" in L.spx_last_error().decode()
    assert L.spx_union_add_fwd(p, n, 1, None, 4, 0, _lib.DTYPE_F16, None, None, None) != 0     # C >= 1
