"""The sparse-class hint in a gather-GEMM call's `tile_order` word (SPX_SPARSE_ROWS_HINT, include/spconv_amd.h): a flag
and the exact appendix row count in the bits above the table form and SPX_DENSE_HINT.  Pure Python: the encoding the
drivers use, its limits, and the header's constants."""
import os
import re

import pytest

from spconv_amd.pytorch import _rulebook as R


def _header_constants():
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "spconv_amd.h")
    text = open(path).read()
    return {k: int(v, 0) for k, v in re.findall(r"#define (SPX_[A-Z_]+) (0x[0-9a-fA-F]+|\d+)\s", text)}


def test_constants_match_the_header():
    h = _header_constants()
    assert R._SPARSE_ROWS_HINT == h["SPX_SPARSE_ROWS_HINT"] and R._SPARSE_ROWS_SHIFT == h["SPX_SPARSE_ROWS_SHIFT"]
    assert R._SPARSE_ROWS_MAX == h["SPX_SPARSE_ROWS_MAX"] and R._DENSE_HINT == h["SPX_DENSE_HINT"]
    assert R._ROWS_LAYOUT == h["SPX_ROWS_LAYOUT"]
    # the flag, the count and the dense hint share no bit with each other or with the table forms 0 / 1 / 2, and the
    # word stays a non-negative C int
    count_bits = R._SPARSE_ROWS_MAX << R._SPARSE_ROWS_SHIFT
    assert count_bits & (R._SPARSE_ROWS_HINT | R._DENSE_HINT | 0xff) == 0
    assert R._SPARSE_ROWS_HINT & (R._DENSE_HINT | 0xff) == 0
    assert (count_bits | R._SPARSE_ROWS_HINT | R._DENSE_HINT | 0xff) < 2 ** 31


@pytest.mark.parametrize("m", [0, 1, 15, 561, 8191, 8192, 8193, 0x7fffe, 0x7ffff])
def test_round_trip(m):
    word = R.sparse_rows_hint(R._ROWS_LAYOUT, m)
    assert word & R._SPARSE_ROWS_HINT and 0 <= word < 2 ** 31
    assert R.split_tile_order(word) == (R._ROWS_LAYOUT, False, m)
    # next to the dense hint (the drivers never give both; the word can carry both)
    assert R.split_tile_order(word | R._DENSE_HINT) == (R._ROWS_LAYOUT, True, m)


@pytest.mark.parametrize("m", [None, -1, 0x80000, 2 ** 31])
def test_a_count_that_does_not_fit_is_no_hint(m):
    assert R.sparse_rows_hint(R._ROWS_LAYOUT, m) == R._ROWS_LAYOUT


@pytest.mark.parametrize("order", [0, 1])
def test_only_a_rows_layout_takes_the_hint(order):
    assert R.sparse_rows_hint(order, 100) == order
    assert R.split_tile_order(order) == (order, False, None)
    assert R.split_tile_order(order | R._DENSE_HINT) == (order, True, None)


class _Blob:
    """Stands for a layout tensor: what the drivers look at are its attributes."""


def test_the_hint_needs_a_read_of_class_1():
    b = _Blob()
    assert R._with_sparse_hint(R._ROWS_LAYOUT, b) == R._ROWS_LAYOUT            # nothing read
    assert R._with_hints(R._ROWS_LAYOUT, b) == R._ROWS_LAYOUT
    b._spx_dense, b._spx_heavy = False, 700                                     # a count without a class: no hint
    assert R._with_sparse_hint(R._ROWS_LAYOUT, b) == R._ROWS_LAYOUT
    b._spx_class = 0                                                            # class 0 read
    assert R._with_sparse_hint(R._ROWS_LAYOUT, b) == R._ROWS_LAYOUT
    b._spx_class = 1                                                            # class 1 and M read
    assert R.split_tile_order(R._with_sparse_hint(R._ROWS_LAYOUT, b)) == (R._ROWS_LAYOUT, False, 700)
    assert R.split_tile_order(R._with_hints(R._ROWS_LAYOUT, b)) == (R._ROWS_LAYOUT, False, 700)
    assert R._with_dense_hint(R._ROWS_LAYOUT, b) == R._ROWS_LAYOUT              # (the dense hint alone stays what it was)
    assert R._with_sparse_hint(0, b) == 0 and R._with_sparse_hint(1, b) == 1
    b._spx_heavy = R._SPARSE_ROWS_MAX + 1                                       # beyond the bits
    assert R._with_sparse_hint(R._ROWS_LAYOUT, b) == R._ROWS_LAYOUT
    d = _Blob()
    d._spx_dense, d._spx_class, d._spx_heavy = True, 0, 90_000                  # a dense rulebook keeps its own hint
    assert R.split_tile_order(R._with_hints(R._ROWS_LAYOUT, d)) == (R._ROWS_LAYOUT, True, None)
