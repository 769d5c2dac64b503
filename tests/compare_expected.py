"""Expected result of compare-with-a-scalar, from the oracle's canonical values (checker only).

`expected(a, op, rhs)`: bit i = op(decoded value i, rhs) AND valid i, where the decoded values and
the validity are the oracle walk's (oracle_tree.canon) and the comparison is numpy's, which is
IEEE for floats (ordered compares with NaN false, != true, -0.0 == +0.0) and the dtype's
signedness for integers.  `bitmap(mask)` packs a row mask the way vxg_compare_scalar lays out its
buffers: LSB first, ((n + 63) // 64) * 8 bytes, zero past n.
"""
import operator

import numpy as np

from oracle_tree import canon

OPS = {"==": operator.eq, "!=": operator.ne, ">": operator.gt, ">=": operator.ge, "<": operator.lt,
       "<=": operator.le}


def bitmap(mask) -> bytes:
    m = np.asarray(mask, dtype=bool)
    out = np.zeros(((m.size + 63) // 64) * 8, dtype=np.uint8)
    bits = np.packbits(m, bitorder="little")
    out[: bits.size] = bits
    return out.tobytes()


def compare_values(vals: np.ndarray, valid, op: str, rhs) -> np.ndarray:
    """Row mask of op(vals, rhs) AND valid; rhs (a scalar or an array) is taken in vals' dtype."""
    r = np.asarray(rhs).astype(vals.dtype)
    with np.errstate(invalid="ignore"):
        m = OPS[op](vals, r)
    m = np.asarray(m, dtype=bool)
    return m if valid is None else m & np.asarray(valid, dtype=bool)


def expected(a, op: str, rhs):
    """-> (values bitmap bytes, validity bitmap bytes | None, row mask) of compare(a, op, rhs)."""
    vals, valid = canon(a)
    m = compare_values(np.asarray(vals), valid, op, rhs)
    return bitmap(m), (None if valid is None else bitmap(valid)), m
