"""Expected result of a row filter (RowFilter::evaluate), from the oracle's canonical values (checker only).

`expected(preds)`: preds is a list of (tree, op, scalar); row i is kept where EVERY conjunct is
true and its column is valid in row i -- the AND of the row masks of compare_expected.expected
(primitive columns) and compare_bytes_expected.expected (utf8/binary columns), which already hold
0 at null rows: arrow's boolean::and is not Kleene, and null_as_false then drops the validity.
The bitmap is laid out by compare_expected.bitmap, as vxg_row_filter lays out its buffer.
"""
import numpy as np

import compare_bytes_expected
import compare_expected
import vortex_amd._lib as L
from compare_expected import bitmap


def row_mask(tree, op: str, scalar) -> np.ndarray:
    """The row mask of one conjunct."""
    if tree.dtype in (L.DTYPE["UTF8"], L.DTYPE["BINARY"]):
        return compare_bytes_expected.expected(tree, op, scalar)[2]
    return compare_expected.expected(tree, op, scalar)[2]


def expected(preds):
    """-> (bitmap bytes, row mask, true count) of the conjunction of `preds`."""
    preds = list(preds)
    n = preds[0][0].len
    m = np.ones(n, dtype=bool)
    for tree, op, scalar in preds:
        assert tree.len == n, "columns of a row filter have one length"
        m &= row_mask(tree, op, scalar)
    return bitmap(m), m, int(m.sum())
