"""compute::take on the CPU: what vxg_take_array_ex must return, for every dtype it serves.

The reference takes a string array row by row into a VarBinBuilder (varbin/compute/take.rs:11-83;
FSST takes its codes, fsst/src/compute.rs:114-126; Dict its codes, dict/compute.rs:44-52), a null
row as an empty value; the canonical of that VarBin (varbin/flatten.rs) is one heap of the taken
rows in index order with the views vxo_make_views writes over it.  `take_canon` builds exactly
that from the oracle's canonical of the array, as oracle_tree.filter_canon does for a predicate."""
from __future__ import annotations

import numpy as np

from oracle_tree import O, _validity, canon, canon_bool, view_bytes  # (oracle_tree puts the repository on sys.path)
from vortex_amd._lib import DTYPE
from vortex_amd.arrays import Array


def take_canon(a: Array, indices, canonical=None):
    """-> ((views u8[k,16], heap u8[]), valid bool[k] | None) for utf8/binary, (values, valid) for
    primitive and bool (a bool mask).  An index outside [0, len) raises IndexError.  `canonical`:
    `oracle_tree.canon(a)` of a string array computed earlier (tests that take from one array many
    times canonicalize it once)."""
    idx = np.asarray(indices).astype(np.int64).reshape(-1)
    if idx.size and (idx.min() < 0 or idx.max() >= a.len):
        raise IndexError("take: index out of bounds")
    if a.dtype in (DTYPE["PRIMITIVE"], DTYPE["BOOL"]):
        vals, valid = canon(a) if a.dtype == DTYPE["PRIMITIVE"] else (canon_bool(a), _validity(a))
        return np.ascontiguousarray(vals[idx]), (None if valid is None else valid[idx])
    (views, heap), valid = canon(a) if canonical is None else canonical
    tvalid = None if valid is None else valid[idx]
    strs = [b"" if (tvalid is not None and not tvalid[j]) else bytes(view_bytes(views, heap, int(i)))
            for j, i in enumerate(idx)]
    offs = np.zeros(len(strs) + 1, dtype=np.int64)
    if strs:
        offs[1:] = np.cumsum([len(s) for s in strs])
    new_heap = np.frombuffer(b"".join(strs), dtype=np.uint8).copy()
    vbits = None if tvalid is None else np.packbits(tvalid, bitorder="little")
    out = np.zeros((len(strs), 16), dtype=np.uint8)
    O.lib().vxo_make_views(O.p(new_heap), O.p(offs), len(strs), O.p(vbits) if vbits is not None else None, 0,
                           O.p(out))
    return (out, new_heap), tvalid
