"""Seeded trees and scan batches as Vortex files: what the file reader is given, per seed.

Plain module: numpy, the file writer (tools/vxfile.py), tree_cases, batch_cases and the CPU oracle --
no GPU, no torch.  The seeded trees of tests/tree_cases.py are built by the array constructors, which
type every child more freely than a file can: in a file only the column's dtype is written, and
every child's dtype, nullability and length follow from its parent's metadata through the
reference's accessors.  `as_file(tree)` is the smallest change that makes a seeded tree legal content
of a file column; `tree_file` / `batch_file` write the result with tools.vxfile.write_file, and
`chunk_ranges` names the chunk ranges a reader is asked for.  tests/test_file_cases.py holds all of
it on the CPU; tests/test_gpu_file_trees.py sends the reader's trees through the engine.

How a child is typed (`child_nullability`), restated from the reference's accessors:
  validity child of any array            Validity::DTYPE = Bool, non-nullable (validity.rs:39-49;
                                         primitive/mod.rs:95-101, bool/mod.rs:51-57, bytebool/src/array.rs:31-37,
                                         varbin/mod.rs:120-126, varbinview/mod.rs:348-358, bitpacking/mod.rs:183-187,
                                         delta/mod.rs:193-199, runend/src/array.rs:128-134, runend-bool/src/array.rs:108-114)
  VarBin offsets, bytes                  Primitive(offsets_ptype, NonNullable), DType::BYTES (varbin/mod.rs:87-118)
  VarBinView views, buffers              DType::BYTES (varbinview/mod.rs:303-325)
  Sparse indices, values                 DType::IDX = u64 non-nullable; self.dtype() (sparse/mod.rs:98-110)
  Chunked offsets, chunks                u64 non-nullable; self.dtype() (chunked/mod.rs:82-104)
  ALP encoded, patches                   i32 / i64 of self's nullability; self.dtype().as_nullable()
                                         (alp/src/alp/array.rs:87-129)
  ALP-RD left, right, exceptions         left_parts_ptype of self's nullability; u32 / u64 non-nullable;
                                         left_parts_ptype nullable (alp/src/alp_rd/array.rs:118-165)
  Dict values, codes                     self.dtype(); codes_ptype non-nullable (dict/src/array.rs:52-63)
  BitPacked patches                      self.dtype() made nullable (bitpacking/mod.rs:163-172)
  Delta bases, deltas                    self.dtype() (delta/mod.rs:160-171)
  FoR encoded                            the unsigned ptype of self's nullability (for/mod.rs:56-66)
  ZigZag encoded                         the unsigned ptype of self's nullability (zigzag/src/array.rs:56-64)
  FSST symbols, lengths, codes, lengths  u64, u8 non-nullable; Binary(codes_nullability) from the metadata;
                                         uncompressed_lengths_ptype non-nullable (fsst/src/array.rs:108-140)
  RunEnd ends, values                    ends_ptype non-nullable; self.dtype() (runend/src/array.rs:149-167)
  RunEndBool ends                        ends_ptype non-nullable (runend-bool/src/array.rs:98-106)
"""
from __future__ import annotations

import functools
from dataclasses import dataclass

import numpy as np

import batch_cases as BC
import tree_cases as TC
import vortex_amd.arrays as A
from oracle_tree import canon
from tools import vxfile as X
from vortex_amd._lib import ENC, VALIDITY
from vortex_amd.arrays import Array

OWN_VALIDITY = {ENC[k] for k in ("PRIMITIVE", "BOOL", "BYTE_BOOL", "RUN_END_BOOL", "FL_BITPACKED", "FL_DELTA", "RUN_END",
                                 "VARBIN", "VARBINVIEW")}
NN = VALIDITY["NON_NULLABLE"]


# ---------------------------------------------------------------------------- as_file
def shared_children(a: Array) -> list:
    """The child slots whose dtype is the node's own (up to the ptype): their nulls are the node's."""
    e = a.encoding
    if e in (ENC["FL_FOR"], ENC["ZIGZAG"], ENC["ALP"], ENC["ALP_RD"], ENC["DICT"]):
        return [0]
    if e in (ENC["SPARSE"], ENC["RUN_END"]):
        return [1]
    if e == ENC["FL_DELTA"]:
        return [0, 1]
    if e == ENC["CHUNKED"]:
        return list(range(1, len(a.children)))
    return []


def needs_nullable(a: Array) -> bool:
    """Bottom-up: the node carries nulls or a validity itself (its flag: a null Constant, a Sparse with
    a null fill, an FSST over nullable codes; or a validity other than NonNullable), or a child that
    shares its dtype does."""
    if a.nullable or (a.encoding in OWN_VALIDITY and a.validity != NN):
        return True
    return any(needs_nullable(a.children[i]) for i in shared_children(a))


def child_nullability(a: Array, nullable: bool) -> list:
    """Top-down: the nullability the reference's accessors give each child of `a`, whose own dtype is
    `nullable` (the table in the module's docstring)."""
    e, n = a.encoding, len(a.children)
    own = [False] if (e in OWN_VALIDITY and a.validity == VALIDITY["ARRAY"]) else []
    if e in (ENC["PRIMITIVE"], ENC["BOOL"], ENC["BYTE_BOOL"]):
        kids = []
    elif e == ENC["VARBIN"]:
        kids = [False, False]
    elif e == ENC["VARBINVIEW"]:
        kids = [False] * (1 + a.meta["n_buffers"])
    elif e == ENC["SPARSE"]:
        kids = [False, nullable]
    elif e in (ENC["CONSTANT"], ENC["ROARING_BOOL"]):
        kids = []
    elif e == ENC["CHUNKED"]:
        kids = [False] + [nullable] * (n - 1)
    elif e == ENC["ALP"]:
        kids = [nullable] + [True] * (n - 1)
    elif e == ENC["ALP_RD"]:
        kids = [nullable, False] + [True] * (n - 2)
    elif e == ENC["DICT"]:
        kids = [nullable, False]
    elif e == ENC["FL_BITPACKED"]:
        kids = [True] if a.meta["has_patches"] else []
    elif e == ENC["FL_DELTA"]:
        kids = [nullable, nullable]
    elif e in (ENC["FL_FOR"], ENC["ZIGZAG"]):
        kids = [nullable]
    elif e == ENC["FSST"]:
        kids = [False, False, bool(a.meta["codes_nullable"]), False]
    elif e == ENC["RUN_END"]:
        kids = [False, nullable]
    elif e == ENC["RUN_END_BOOL"]:
        kids = [False]
    else:
        raise NotImplementedError(f"no file typing for encoding {e}")
    kids += own
    assert len(kids) == n, (TC.ENC_NAME[e], len(kids), n)
    return kids


def _typed(a: Array, nullable: bool) -> Array:
    """`a` as the reader types it when its dtype's nullability is `nullable`; `a` itself where nothing changes."""
    e = a.encoding
    if not nullable and needs_nullable(a):
        raise ValueError(f"{TC.describe(a)} carries nulls where the file types it non-nullable")
    kids = [_typed(c, k) for c, k in zip(a.children, child_nullability(a, nullable))]
    if e == ENC["SPARSE"] and kids[0].ptype != "u64":  # DType::IDX (sparse/mod.rs:54, 108)
        kids[0] = A.primitive(np.ascontiguousarray(canon(a.children[0])[0]).astype(np.uint64))
    validity = a.validity
    if nullable and e in OWN_VALIDITY and validity == NN:
        validity = VALIDITY["ALL_VALID"]
    if nullable == bool(a.nullable) and validity == a.validity and all(k is c for k, c in zip(kids, a.children)):
        return a
    return Array(e, a.len, a.dtype, a.ptype, nullable, validity, a.meta, a.buffers, kids)


def as_file(tree: Array) -> Array:
    """The smallest change that makes a seeded tree legal content of a reference file column: the
    column's nullability computed bottom-up (`needs_nullable`) and pushed down the way the reference's
    accessors type each child (`child_nullability`); a node typed nullable whose own validity is
    NonNullable becomes AllValid; every chunk of a root ChunkedArray gets the column's one dtype; a
    Sparse indices child (patches included) that is not u64 becomes a Primitive u64 of its canonical
    values.  Nothing else changes: a tree that is legal already comes back as the same object."""
    return _typed(tree, needs_nullable(tree))


def changes(tree: Array) -> set:
    """What as_file changes in `tree`: a subset of {"nullable", "sparse-indices"}."""
    out = set()

    def walk(a, b):
        if a is b:
            return
        if bool(a.nullable) != bool(b.nullable) or a.validity != b.validity:
            out.add("nullable")
        for i, (c, d) in enumerate(zip(a.children, b.children)):
            if a.encoding == ENC["SPARSE"] and i == 0 and c.ptype != "u64":
                out.add("sparse-indices")
            else:
                walk(c, d)

    walk(tree, as_file(tree))
    return out


# ---------------------------------------------------------------------------- files
def pieces(tree: Array) -> list:
    """The chunks a column is written as: the children of a root ChunkedArray, else the tree itself.
    (A root ChunkedArray without chunks would be written as one zero-length chunk; no seed builds one:
    arrays.chunked refuses an empty list and the slices of a root keep at least one chunk.)"""
    if tree.encoding != ENC["CHUNKED"]:
        return [tree]
    chunks = list(tree.children[1:])
    if not chunks:
        raise ValueError("a root ChunkedArray without chunks")
    return chunks


@dataclass
class FileColumn:
    name: str
    tree: Array          # as_file(the seeded tree)
    chunks: list         # pieces(tree): what was written, one Batch message each
    words: tuple         # the seed words chunk_ranges draws from


@dataclass
class TreeFile:
    seed: int
    data: bytes          # a one-column file
    column: FileColumn
    case: TC.TreeCase    # the truth (values, valid, kind) and the compute inputs

    @property
    def chunks(self):
        return self.column.chunks

    @property
    def tree(self):
        return self.column.tree


@dataclass
class BatchFile:
    seed: object
    data: bytes
    columns: list        # FileColumn, in the batch's column order
    case: BC.BatchCase


def _column(name: str, tree: Array, words) -> FileColumn:
    t = as_file(tree)
    return FileColumn(name, t, pieces(t), tuple(int(w) for w in words))


@functools.lru_cache(maxsize=None)
def _tree_file(seed: int, typed: bool) -> TreeFile:
    case = TC.build(seed)
    col = _column("c", case.tree, [seed])
    return TreeFile(seed, X.write_file([(col.name, col.chunks)]), col, case)


def tree_file(seed: int) -> TreeFile:
    """The one-column file of a tree seed (under the current tools.vxfile.TYPED_VECTORS), the chunks
    that were written and the TreeCase that holds the truth."""
    return _tree_file(seed, bool(X.TYPED_VECTORS))


@functools.lru_cache(maxsize=None)
def _batch_file(seed, typed: bool) -> BatchFile:
    case = BC.build(seed)
    words = [0xBA7C] + (list(seed) if isinstance(seed, tuple) else [seed])
    cols = [_column(f"c{i}", c.tree, words + [i]) for i, c in enumerate(case.columns)]
    return BatchFile(seed, X.write_file([(c.name, c.chunks) for c in cols], row_count=case.n), cols, case)


def batch_file(seed) -> BatchFile:
    """One file per BatchCase: its columns in order, each through as_file and written as its own
    chunks (so the columns of one file are chunked differently); n = 0 gives a file of zero rows."""
    return _batch_file(seed, bool(X.TYPED_VECTORS))


def chunk_ranges(col) -> list:
    """The chunk ranges [c0, c1) a reader is asked for, of a column (FileColumn or TreeFile) of k >= 2
    chunks: all of it, the first chunk, the last chunk, one interior range where k >= 3, and a range
    that begins or ends at a zero-length chunk where the column has one.  [] for a one-chunk column."""
    col = getattr(col, "column", col)
    k = len(col.chunks)
    if k < 2:
        return []
    rng = np.random.default_rng([0xF11E] + list(col.words))
    out = [(0, k), (0, 1), (k - 1, k)]
    if k >= 3:
        c0 = int(rng.integers(1, k - 1))
        out.append((c0, int(rng.integers(c0 + 1, k))))
    zeros = [i for i, c in enumerate(col.chunks) if c.len == 0]
    if zeros:
        z = zeros[int(rng.integers(0, len(zeros)))]
        begins = (z, min(z + 2, k))          # begins at the zero-length chunk
        ends = (max(z - 1, 0), z + 1)        # ends at it
        out.append(begins if rng.random() < 0.5 else ends)
    seen, uniq = set(), []
    for r in out:
        if r not in seen:
            seen.add(r)
            uniq.append(r)
    return uniq


def range_tree(col, c0: int, c1: int) -> Array:
    """The ChunkedArray of chunks [c0, c1) of a column, as the reader's root states it (its dtype is
    the column's): what the oracle canonicalizes for that range."""
    col = getattr(col, "column", col)
    t = A.chunked(col.chunks[c0:c1])
    t.nullable = bool(col.tree.nullable)
    return t


TREE_SEEDS = list(TC.SEEDS)
BATCH_SEEDS = list(BC.BATCH_SEEDS)
