"""CPU: the seeded tree generator (tests/tree_cases.py) and the oracle held against each other.

Before any GPU is involved: build(seed) is deterministic; the oracle's canonical of every tree is
bit-exact with the plain truth the tree was encoded from (values as bytes, so NaN payloads and
-0.0 count; strings row by row; validity as masks) -- for EVERY seed, none left out; the seed list
covers the encodings, positions and validity kinds the GPU test relies on (conditions on the
generator's output, asserted); and the new metadata-only slices agree with slicing the canonical.
"""
import collections

import numpy as np
import pytest

import tree_cases as TC
import vortex_amd.arrays as A
import vortex_amd.encode as E
from oracle_tree import canon, slice_any, view_bytes
from vortex_amd._lib import DTYPE, ENC


def _buffers(a, out):
    out.append((a.encoding, a.len, a.dtype, a.ptype, a.nullable, a.validity,
                sorted((k, bytes(v) if isinstance(v, (bytes, bytearray)) else v) for k, v in a.meta.items())))
    out.extend(np.ascontiguousarray(b).tobytes() for b in a.buffers)
    for c in a.children:
        _buffers(c, out)
    return out


def full(mask, n):
    return np.ones(n, bool) if mask is None else np.asarray(mask, bool)


def assert_canonical_is_truth(case, got, gvalid, what="oracle"):
    """`got`, `gvalid`: a canonical of case.tree as oracle_tree.canon returns it."""
    at = f"seed {case.seed} ({what}): {case.describe}"
    n = case.tree.len
    assert np.array_equal(full(gvalid, n), full(case.valid, n)), "validity differs, " + at
    if case.kind == "str":
        views, heap = got
        assert len(case.values) == n == views.shape[0], "length differs, " + at
        valid = full(case.valid, n)
        for i, s in enumerate(case.values):
            if valid[i]:
                assert view_bytes(views, heap, i) == s, f"row {i} differs, " + at
        return
    want = np.asarray(case.values)
    got = np.asarray(got)
    assert got.dtype == want.dtype and got.size == want.size == n, "dtype or length differs, " + at
    if got.tobytes() != want.tobytes():
        bad = np.flatnonzero(got.view(np.uint8).reshape(n, -1) != want.view(np.uint8).reshape(n, -1))
        raise AssertionError(f"values differ first at byte {int(bad[0])}, " + at)


@pytest.mark.parametrize("seed", TC.SEEDS)
def test_build_is_deterministic(seed):
    a, b = TC.build.__wrapped__(seed), TC.build.__wrapped__(seed)
    assert a.describe == b.describe
    assert _buffers(a.tree, []) == _buffers(b.tree, [])
    assert [(n, i.dtype, i.tobytes()) for n, i in a.take_sets] == [(n, i.dtype, i.tobytes()) for n, i in b.take_sets]
    assert [(n, _buffers(p, [])) for n, p in a.predicates] == [(n, _buffers(p, [])) for n, p in b.predicates]
    assert repr(a.scalars) == repr(b.scalars) and repr(a.range) == repr(b.range)


def test_generator_has_not_drifted():
    """tests/golden/tree_digests.json: a sha256 per seed over `describe`, every buffer of the tree and the
    compute inputs, recorded before Gen was extended for tests/batch_cases.py.  A seed that builds other
    bytes changes what the GPU suite covers: add seeds, do not change what the existing ones build."""
    import json
    from pathlib import Path
    want = json.loads((Path(__file__).parent / "golden" / "tree_digests.json").read_text())
    assert sorted(want) == sorted(str(s) for s in TC.SEEDS)
    drifted = [s for s in TC.SEEDS if TC.digest(TC.build.__wrapped__(s)) != want[str(s)]]
    assert not drifted, f"seeds {drifted} no longer build the recorded bytes"


@pytest.mark.parametrize("seed", TC.SEEDS)
def test_oracle_canonical_is_the_truth(seed):
    case = TC.build(seed)
    got, gvalid = canon(case.tree)
    assert_canonical_is_truth(case, got, gvalid)


def test_compute_inputs():
    for seed in TC.SEEDS:
        c = TC.build(seed)
        n = c.tree.len
        names = [k for k, _ in c.take_sets]
        assert names == (["empty", "one", "few", "many"] if n else ["empty"]), seed
        for name, ix in c.take_sets:
            assert ix.dtype.kind in "iu" and (ix.size == 0 or (0 <= int(ix.min()) and int(ix.max()) < n)), (seed, name)
        if n:
            sets = dict(c.take_sets)
            assert sets["one"].size == 1 and 1 <= sets["few"].size <= 16 and sets["many"].size * 4 > n
            assert {0, n - 1} <= set(sets["few"].tolist()) | set(sets["many"].tolist())
        assert all(p.len == n and p.dtype == DTYPE["BOOL"] and not p.nullable for _, p in c.predicates), seed
        assert {p.encoding for _, p in c.predicates} >= {ENC["BOOL"], ENC["CONSTANT"]}
        if c.kind != "bool":
            assert len(c.scalars) >= 2 and len(c.range) == 4


# ---------------------------------------------------------------------------- coverage conditions
def _survey():
    roots, inner, kinds = collections.Counter(), collections.Counter(), collections.Counter()
    nested = zero_chunk = one_chunk = offsets = mixed = 0
    for seed in TC.SEEDS:
        tree = TC.build(seed).tree
        has0 = has1 = False
        for node, parent, slot in TC.walk(tree):
            name = TC.ENC_NAME[node.encoding]
            (roots if parent is None else inner)[name] += 1
            k = TC.validity_kind(node)
            if k is not None:
                kinds[k] += 1
            if TC.node_offset(node):
                offsets += 1
            if node.encoding == ENC["CHUNKED"]:
                has0 |= any(c.len == 0 for c in node.children[1:])
                has1 |= any(c.len == 1 for c in node.children[1:])
                if parent is not None and slot == 0 and TC.ENC_NAME[parent.encoding] in ("DICT", "FL_FOR", "ZIGZAG", "ALP"):
                    nested += 1
        zero_chunk += has0
        one_chunk += has1
        if tree.encoding == ENC["CHUNKED"]:
            k1 = [TC.has_patches(c) for c in tree.children[1:] if TC.k1_fusable(c)]
            mixed += any(k1) and not all(k1)
    return dict(roots=roots, inner=inner, kinds=kinds, nested=nested, zero_chunk=zero_chunk, one_chunk=one_chunk,
                offsets=offsets, mixed=mixed)


def test_coverage_conditions():
    s = _survey()
    for name in TC.CONSTRUCTIBLE:
        assert s["roots"][name] >= 3, f"{name} is the root of {s['roots'][name]} trees"
        assert s["inner"][name] >= 3, f"{name} is a non-root node {s['inner'][name]} times"
    assert set(TC.CONSTRUCTIBLE) == {k for k in ENC if k != "STRUCT"}
    for kind in TC.VALIDITY_KINDS:
        assert s["kinds"][kind] >= 3, f"validity kind {kind} appears {s['kinds'][kind]} times"
    assert s["nested"] >= 5, f"{s['nested']} nested ChunkedArrays under Dict values or a FoR / ZigZag / ALP child"
    assert s["zero_chunk"] >= 5, f"{s['zero_chunk']} roots contain a zero-length chunk"
    assert s["one_chunk"] >= 5, f"{s['one_chunk']} roots contain a one-row chunk"
    assert s["offsets"] >= 8, f"{s['offsets']} sliced nodes have a non-zero offset"
    assert s["mixed"] >= 5, f"{s['mixed']} ChunkedArray roots mix patched and patch-free K1 chunks"


# ---------------------------------------------------------------------------- the new slices
def _slice_subjects():
    rng = np.random.default_rng(7)
    n = 5000
    u = rng.integers(0, 1 << 9, n).astype(np.uint32)
    u[rng.choice(n, 60, replace=False)] = rng.integers(1 << 20, 1 << 30, 60).astype(np.uint32)
    m = rng.random(n) < 0.8
    yield "for", E.encode_for_bitpacked(rng.integers(-(1 << 40), 1 << 40, n).astype(np.int64))
    yield "for-shift", E.encode_for_bitpacked((rng.integers(0, 900, n).astype(np.int32) << 3) - 777 * 8)
    yield "for-nullable", A.frame_of_reference(E.encode_bitpacked(u, bit_width=9, validity=m), -5, 0, "i32")
    yield "zigzag", E.encode_zigzag(rng.integers(-3000, 3000, n).astype(np.int16))
    prices = np.round(rng.uniform(1, 1000, n), 2)
    prices[rng.choice(n, 40, replace=False)] = rng.standard_normal(40) * np.pi
    yield "alp-patched", E.encode_alp(prices)
    yield "alp-f32", E.encode_alp(np.round(rng.uniform(0, 100, n), 1).astype(np.float32))
    yield "dict", E.encode_dict(rng.integers(0, 40, n).astype(np.uint64) * 3)
    yield "dict-nullable", E.encode_dict_nullable(rng.integers(0, 9, n).astype(np.int16), m)
    yield "dict-strings", E.encode_dict_strings([[b"alpha", b"a-much-longer-value", b"z"][i] for i in
                                                 rng.integers(0, 3, n).tolist()])
    chunks = [E.encode_bitpacked(u[:1024], bit_width=9), A.primitive(u[1024:1024]), A.primitive(u[1024:2049]),
              E.encode_bitpacked(u[2049:4000], bit_width=9, validity=m[2049:4000]), A.primitive(u[4000:4000]),
              E.encode_bitpacked(u[4000:], bit_width=9)]
    yield "chunked", A.chunked(chunks)
    yield "for-chunked", A.frame_of_reference(A.chunked(chunks), 12345, 1, "u32")


EDGES = [(0, 0), (0, 1), (0, 5000), (1, 1023), (1023, 1025), (1024, 2048), (1024, 1024), (1025, 4097), (2049, 4000),
         (4000, 5000), (4999, 5000), (5000, 5000), (63, 4096)]


SLICE_SUBJECTS = ["for", "for-shift", "for-nullable", "zigzag", "alp-patched", "alp-f32", "dict", "dict-nullable",
                  "dict-strings", "chunked", "for-chunked"]


@pytest.mark.parametrize("name", SLICE_SUBJECTS)
def test_slices_are_the_canonical_slices(name):
    """canon(slice_any(a, i, j)) == canon(a)[i:j] at block edges (values as bytes, validity as masks)."""
    subjects = dict(_slice_subjects())
    assert list(subjects) == SLICE_SUBJECTS
    a = subjects[name]
    vals, valid = canon(a)
    for i, j in EDGES:
        s = slice_any(a, i, j)
        assert s.len == j - i and (s.dtype, s.ptype) == (a.dtype, a.ptype), (name, i, j)
        got, gvalid = canon(s)
        assert np.array_equal(full(gvalid, j - i), full(valid, a.len)[i:j]), (name, i, j)
        if a.dtype in (DTYPE["UTF8"], DTYPE["BINARY"]):
            assert [view_bytes(got[0], got[1], k) for k in range(j - i)] == \
                   [view_bytes(vals[0], vals[1], k) for k in range(i, j)], (name, i, j)
        else:
            assert got.tobytes() == vals[i:j].tobytes(), (name, i, j)


def test_chunked_slice_drops_what_the_reference_drops():
    """chunked/compute/slice.rs: a stop at a chunk's first row drops that chunk; empty chunks before
    the start are skipped (find_chunk_idx searches from the right); one chunk holding both ends is
    sliced once."""
    c = A.chunked([A.primitive(np.arange(3, dtype=np.uint64)), A.primitive(np.zeros(0, np.uint64)),
                   A.primitive(np.arange(3, 6, dtype=np.uint64)), A.primitive(np.arange(6, 9, dtype=np.uint64))])
    assert [k.len for k in slice_any(c, 0, 3).children[1:]] == [3, 0]  # only the chunk holding `stop` is dropped
    assert [k.len for k in slice_any(c, 3, 6).children[1:]] == [3]   # starts in chunk 2, not in the empty one
    assert [k.len for k in slice_any(c, 2, 7).children[1:]] == [1, 0, 3, 1]
    assert [k.len for k in slice_any(c, 4, 5).children[1:]] == [1]
    assert [k.len for k in slice_any(c, 0, 9).children[1:]] == [3, 0, 3, 3]
