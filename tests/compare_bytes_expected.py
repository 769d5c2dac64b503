"""Expected result of a string compare-with-a-scalar, from the oracle's canonical views (checker only).

`expected(tree, op, scalar)`: bit i = op(bytes of row i, scalar) AND valid i, where the rows are
the oracle walk's (oracle_tree.canon + view_bytes) and the comparison is Python's `bytes` order:
unsigned, lexicographic, a proper prefix is smaller -- arrow's order for Utf8 and Binary.  The
bitmaps are laid out by compare_expected.bitmap, as vxg_compare_bytes lays out its buffers.
"""
import numpy as np

from compare_expected import OPS, bitmap
from oracle_tree import canon, view_bytes


def as_bytes(scalar) -> bytes:
    return scalar.encode("utf-8") if isinstance(scalar, str) else bytes(scalar)


def rows_of(tree):
    """-> (list of the rows' bytes, valid bool array | None); a null row's bytes are b""."""
    (views, heap), valid = canon(tree)
    rows = [view_bytes(views, heap, i) if valid is None or valid[i] else b"" for i in range(tree.len)]
    return rows, valid


def compare_rows(rows, valid, op: str, scalar) -> np.ndarray:
    s = as_bytes(scalar)
    f = OPS[op]
    m = np.fromiter((f(r, s) for r in rows), dtype=bool, count=len(rows))
    return m if valid is None else m & np.asarray(valid, dtype=bool)


def expected(tree, op: str, scalar, rows=None):
    """-> (values bitmap bytes, validity bitmap bytes | None, row mask) of compare(tree, op, scalar).
    `rows`: a rows_of(tree) computed once for several scalars."""
    r, valid = rows if rows is not None else rows_of(tree)
    m = compare_rows(r, valid, op, scalar)
    return bitmap(m), (None if valid is None else bitmap(valid)), m
