"""CPU: the seeded trees and scan batches as files (tests/file_cases.py), the writer and the reader
held against each other -- for EVERY tree seed and EVERY batch seed, none left out.

`as_file` keeps the truth (the oracle's canonical of the file tree is bit-exact with the plain truth
the seed was encoded from, so it can serve as the GPU expectation) and changes nothing in a tree that
is legal file content already; the reader (vortex_amd/csrc/serde.cpp), given region = NULL, rebuilds
`as_file`'s tree node for node -- per chunk, per chunk range of `chunk_ranges`, and for both settings
of tools.vxfile.TYPED_VECTORS -- and reports the file's geometry; with a region base every leaf buffer
lies inside the region; the generated files cover what tests/test_gpu_file_trees.py relies on; and a
batch's file columns take the routes of its in-memory columns.  Where reader and `as_file` disagree
the reference's accessor decides (file_cases cites them); `as_file` is never bent to match serde.cpp.
"""
import collections

import numpy as np
import pytest

import batch_cases as BC
import file_cases as FC
import tree_cases as TC
import vortex_amd._lib as L
from file_tree_check import check_tree, leaf_buffers
from oracle_tree import canon
from test_tree_cases import assert_canonical_is_truth
from tools import vxfile as X
from vortex_amd._lib import DTYPE, ENC
from vortex_amd.file import VortexFile

BATCH_IDS = [BC.seed_id(s) for s in FC.BATCH_SEEDS]

# what as_file does to the 72 seeded trees (derived below, pinned here)
UNCHANGED_TREES = 50        # as_file(tree) is the tree itself
NULLABLE_TREES = 20         # nullable flags / NonNullable -> AllValid differ
NARROW_SPARSE_TREES = 13    # a Sparse indices child narrower than u64 is widened
BOTH_TREES = 11


# ---------------------------------------------------------------------------- as_file
@pytest.mark.parametrize("seed", FC.TREE_SEEDS)
def test_as_file_preserves_the_truth(seed):
    case = TC.build(seed)
    got, gvalid = canon(FC.as_file(case.tree))
    assert_canonical_is_truth(case, got, gvalid, "oracle of as_file")


@pytest.mark.parametrize("seed", FC.BATCH_SEEDS, ids=BATCH_IDS)
def test_as_file_preserves_the_truth_of_batch_columns(seed):
    for c in BC.build(seed).columns:
        got, gvalid = canon(FC.as_file(c.tree))
        assert_canonical_is_truth(c, got, gvalid, f"oracle of as_file, batch {seed}")


def test_as_file_changes_only_what_a_file_cannot_hold():
    what = {s: FC.changes(TC.build(s).tree) for s in FC.TREE_SEEDS}
    unchanged = [s for s in FC.TREE_SEEDS if not what[s]]
    for s in FC.TREE_SEEDS:
        tree = TC.build(s).tree
        filed = FC.as_file(tree)
        if s in unchanged:  # the tree itself, buffer for buffer
            assert filed is tree and TC.tree_bytes(filed, []) == TC.tree_bytes(tree, []), s
        else:
            assert filed is not tree and TC.tree_bytes(filed, []) != TC.tree_bytes(tree, []), s
        assert FC.as_file(filed) is filed, f"seed {s}: as_file of a file tree changes it again"
        assert what[s] <= {"nullable", "sparse-indices"}, (s, what[s])
    assert len(unchanged) == UNCHANGED_TREES, unchanged
    assert sum("nullable" in w for w in what.values()) == NULLABLE_TREES
    assert sum("sparse-indices" in w for w in what.values()) == NARROW_SPARSE_TREES
    assert sum(len(w) == 2 for w in what.values()) == BOTH_TREES


def test_as_file_leaves_the_seeds_alone():
    """as_file builds new nodes and never writes into the seeded tree: the digests still hold."""
    import json
    from pathlib import Path
    want = json.loads((Path(__file__).parent / "golden" / "tree_digests.json").read_text())
    for s in FC.TREE_SEEDS:
        FC.tree_file(s)
        assert TC.digest(TC.build(s)) == want[str(s)], s


def test_sparse_indices_are_u64_in_every_file_tree():
    for s in FC.TREE_SEEDS:
        for node, _, _ in TC.walk(FC.tree_file(s).tree):
            if node.encoding == ENC["SPARSE"]:
                idx = node.children[0]
                assert idx.ptype == "u64" and not idx.nullable and idx.len == node.meta["indices_len"], s


# ---------------------------------------------------------------------------- the reader
def check_file(data: bytes, columns: list, rows: int, at: str):
    """One file against the columns that were written: the file's geometry, then every chunk range of
    every column node for node (region = NULL) and rebased into a region."""
    raw = np.frombuffer(data, np.uint8)
    f = VortexFile(data)
    try:
        assert f.row_count == rows, at
        assert [c.name for c in f.columns] == [c.name for c in columns], at
        taken = []
        for ci, col in enumerate(columns):
            where = f"{at}, column {ci}"
            k = len(col.chunks)
            info = f.columns[ci]
            t = col.tree
            assert (info.n_chunks, info.rows, info.dtype, info.nullable, info.is_extension) == \
                (k, rows, t.dtype, bool(t.nullable), False), (info, where)
            if t.dtype == DTYPE["PRIMITIVE"]:
                assert info.ptype == t.ptype, where
            row, end = 0, None
            for i, ch in enumerate(col.chunks):
                c = f.chunk(ci, i)
                assert (c.row_offset, c.rows) == (row, ch.len), (c, where)
                assert c.message_begin % 64 == 0 and c.buffers_begin % 64 == 0 and c.message_end % 64 == 0, (c, where)
                assert c.message_begin < c.buffers_begin <= c.message_end, (c, where)
                assert end is None or c.message_begin == end, (c, where)  # contiguous messages
                row, end = row + ch.len, c.message_end
            taken.append((f.chunk(ci, 0).message_begin, end))
            for c0, c1 in [(0, k)] + FC.chunk_ranges(col):
                rwhere = f"{where}, chunks [{c0}, {c1})"
                lens = [ch.len for ch in col.chunks[c0:c1]]
                assert list(f.chunk_offsets(ci, c0, c1)) == [0] + list(np.cumsum(lens)), rwhere
                b, e = f.byte_range(ci, c0, c1)
                assert (b, e) == (f.chunk(ci, c0).message_begin, f.chunk(ci, c1 - 1).message_end), rwhere
                node = f.column_tree(ci, c0, c1)
                assert node.encoding == ENC["CHUNKED"] and node.len == sum(lens), rwhere
                assert node.meta.chunked.nchunks == c1 - c0 and node.n_children == c1 - c0 + 1, rwhere
                assert (node.dtype, bool(node.nullable)) == (t.dtype, bool(t.nullable)), rwhere
                offs = node.children[0]
                assert (offs.encoding, offs.len, L.PTYPES[offs.ptype], offs.n_buffers) == \
                    (ENC["PRIMITIVE"], c1 - c0 + 1, "u64", 0), rwhere
                for i in range(c0, c1):
                    check_tree(node.children[1 + i - c0], col.chunks[i], raw, f"{rwhere}, chunk {i}")
                # rebased: every leaf buffer inside the region the chunks' messages are copied to
                base = 1 << 40
                node = f.column_tree(ci, c0, c1, region=base, region_offset=b, region_len=e - b)
                for ptr, n in leaf_buffers(node):
                    assert base <= ptr and ptr + n <= base + (e - b), (ptr, n, rwhere)
                    assert (ptr - base + b) % 64 == 0, rwhere
        # the columns' message ranges follow one another in column order and do not overlap
        for (b0, e0), (b1, e1) in zip(taken, taken[1:]):
            assert e0 <= b1, at
    finally:
        f.close()


@pytest.mark.parametrize("typed", [True, False])
@pytest.mark.parametrize("seed", FC.TREE_SEEDS)
def test_reader_rebuilds_the_tree(seed, typed, monkeypatch):
    monkeypatch.setattr(X, "TYPED_VECTORS", typed)
    tf = FC.tree_file(seed)
    check_file(tf.data, [tf.column], tf.case.tree.len, f"seed {seed} typed={typed}: {tf.case.describe}")


@pytest.mark.parametrize("typed", [True, False])
@pytest.mark.parametrize("seed", FC.BATCH_SEEDS, ids=BATCH_IDS)
def test_reader_rebuilds_the_batch(seed, typed, monkeypatch):
    monkeypatch.setattr(X, "TYPED_VECTORS", typed)
    bf = FC.batch_file(seed)
    assert len(bf.columns) == len(bf.case.columns)
    check_file(bf.data, bf.columns, bf.case.n, f"typed={typed}: {bf.case.describe}")


def test_typed_vectors_change_the_bytes():
    """The two settings write different files for some seed (else the second run above shows nothing)."""
    differ = 0
    for s in FC.TREE_SEEDS:
        a, b = FC._tree_file.__wrapped__(s, True).data, None
        old = X.TYPED_VECTORS
        try:
            X.TYPED_VECTORS = not old
            b = FC._tree_file.__wrapped__(s, False).data
        finally:
            X.TYPED_VECTORS = old
        differ += a != b
    assert differ >= 3, differ


@pytest.mark.parametrize("seed", FC.BATCH_SEEDS, ids=BATCH_IDS)
def test_file_columns_take_the_routes_of_the_batch(seed):
    bf = FC.batch_file(seed)
    for col, c in zip(bf.columns, bf.case.columns):
        assert BC.expected_route(col.tree) == c.route, f"{c.describe} in {bf.case.describe}"
        assert [ch.len for ch in col.chunks] == [p.len for p in BC.pieces(c.tree)]
    if bf.case.n == 0:
        assert all(len(col.chunks) >= 1 and sum(ch.len for ch in col.chunks) == 0 for col in bf.columns)


# ---------------------------------------------------------------------------- chunk ranges
def test_chunk_ranges():
    for s in FC.TREE_SEEDS:
        tf = FC.tree_file(s)
        k = len(tf.chunks)
        r = FC.chunk_ranges(tf)
        assert r == FC.chunk_ranges(tf), s  # from the seed alone
        if k < 2:
            assert r == []
            continue
        assert r[:3] == [(0, k), (0, 1), (k - 1, k)] and len(set(r)) == len(r), (s, r)
        assert all(0 <= a < b <= k for a, b in r), (s, r)
        if k >= 3:
            assert any(0 < a and b < k for a, b in r), (s, r)
        zeros = {i for i, c in enumerate(tf.chunks) if c.len == 0}
        if zeros:
            assert any(a in zeros or b - 1 in zeros for a, b in r), (s, r)


# ---------------------------------------------------------------------------- coverage conditions
def _survey():
    chunk_roots, below, inside, kinds = (collections.Counter() for _ in range(4))
    nested = zero_chunk = max_chunks = fsst = zero_ranges = 0
    offsets = set()
    for s in FC.TREE_SEEDS:
        tf = FC.tree_file(s)
        max_chunks = max(max_chunks, len(tf.chunks))
        zero_chunk += any(c.len == 0 for c in tf.chunks)
        zeros = {i for i, c in enumerate(tf.chunks) if c.len == 0}
        zero_ranges += any(a in zeros or b - 1 in zeros for a, b in FC.chunk_ranges(tf)[3:])
        for ch in tf.chunks:
            for node, parent, _ in TC.walk(ch):
                name = TC.ENC_NAME[node.encoding]
                below[name] += 1
                (chunk_roots if parent is None else inside)[name] += 1
                k = TC.validity_kind(node)
                if k is not None:
                    kinds[k] += 1
                nested += node.encoding == ENC["CHUNKED"]
                fsst += node.encoding == ENC["FSST"]
                if node.encoding == ENC["VARBIN"]:
                    offsets.add(L.PTYPES[node.meta["offsets_ptype"]])
    return dict(chunk_roots=chunk_roots, below=below, inside=inside, kinds=kinds, nested=nested, zero_chunk=zero_chunk,
                max_chunks=max_chunks, fsst=fsst, offsets=offsets, zero_ranges=zero_ranges)


def test_coverage_conditions():
    """Over all tree files.  The reader's root of every column is the ChunkedArray of its chunks, so
    Chunked is no chunk's root (a root ChunkedArray's chunks become the column's chunks): it is the
    root of every column and occurs nested inside chunks.  "Non-root" is meant of the reader's column
    tree: a chunk's root is one.  RoaringBool, Constant and VarBinView have no position below a
    chunk's root in the seeded trees; the others occur there too."""
    s = _survey()
    for name in TC.CONSTRUCTIBLE:
        if name != "CHUNKED":
            assert s["chunk_roots"][name] >= 3, f"{name} is the root of {s['chunk_roots'][name]} chunks"
        assert s["below"][name] >= 3, f"{name} is a non-root node of a column {s['below'][name]} times"
    for name in ("PRIMITIVE", "BOOL", "BYTE_BOOL", "RUN_END_BOOL", "FL_BITPACKED", "SPARSE", "FL_FOR", "ZIGZAG", "ALP_RD",
                 "FL_DELTA", "CHUNKED", "VARBIN", "FSST"):
        assert s["inside"][name] >= 1, f"{name} never occurs below a chunk's root"
    for kind in TC.VALIDITY_KINDS:
        assert s["kinds"][kind] >= 3, f"validity kind {kind} appears {s['kinds'][kind]} times"
    assert s["nested"] >= 5, f"{s['nested']} ChunkedArrays nested inside a chunk"
    nested_seeds = [x for x in FC.TREE_SEEDS
                    if any(n.encoding == ENC["CHUNKED"] for ch in FC.tree_file(x).chunks for n, _, _ in TC.walk(ch))]
    assert nested_seeds == [2, 21, 38, 39, 42, 56, 58, 60, 61, 62]
    assert s["zero_chunk"] >= 5, f"{s['zero_chunk']} columns contain a zero-length chunk"
    assert s["zero_ranges"] >= 3, f"{s['zero_ranges']} columns have a range that begins or ends at a zero-length chunk"
    assert s["max_chunks"] >= 6, f"the longest column has {s['max_chunks']} chunks"
    assert s["offsets"] >= {"i32", "i64"}, f"VarBin offset widths {s['offsets']}"
    assert s["fsst"] >= 3, f"FSST occurs {s['fsst']} times"
