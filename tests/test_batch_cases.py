"""CPU: the seeded batches (tests/batch_cases.py) held against the oracle, and the comparer held against itself.

Before any GPU is involved: build(seed) is deterministic; the oracle's canonical of every column is
bit-exact with the plain truth; oracle_tree.filter_canon of every column under every mask equals
values[mask] / valid[mask] taken from the plain truth with numpy alone; row_filter_expected of every
conjunction equals the AND of numpy compares on the truth with nulls false; the batches cover the
shapes the GPU test relies on (conditions on the generator's output, asserted); and
filter_batch_run.check_outputs raises for one wrong byte, bit, guard byte, view offset or heap size.
"""
import collections
import copy

import numpy as np
import pytest

import batch_cases as BC
import row_filter_expected
import tree_cases as TC
import vortex_amd as V
import vortex_amd.arrays as A
import vortex_amd.encode as E
from filter_batch_run import GUARD, HostBuffer, HostOut, buffer_sizes, check_outputs, mask_bytes
from oracle_tree import canon, filter_canon, view_bytes
from test_tree_cases import assert_canonical_is_truth, full
from vortex_amd._lib import DTYPE, ENC

SEEDS = BC.BATCH_SEEDS
IDS = [BC.seed_id(s) for s in SEEDS]


def test_seed_list():
    assert BC.GENERATED_SEEDS == list(range(24)) and len(SEEDS) == len(set(SEEDS))
    groups = [s for s in SEEDS if isinstance(s, tuple)]
    assert sorted(len(g) for g in groups)[-2:] == [7, 10]  # the 2047-row and the 1025-row trees
    assert {BC.build(g).n for g in groups} >= {64, 1023, 1025, 2047, 4096, 4097, 20011}
    assert sorted({BC.build(s).n for s in BC.GENERATED_SEEDS}) == sorted(BC.LENS)
    for s in SEEDS:
        b = BC.build(s)
        assert all(c.tree.len == b.n for c in b.columns), b.describe
        if not isinstance(s, tuple):
            assert b.n <= BC.MAX_ROWS and 6 <= len(b.columns) <= BC.MAX_COLUMNS, b.describe
            made = collections.Counter(c.made_as for c in b.columns)
            assert made["packed-chunked"] >= (1 if b.n >= 2 else 0) and made["inplace"] and made["inplace-chunked"]
            assert {"str", "bool"} <= {c.kind for c in b.columns}, b.describe
            assert 2 <= len(b.conjunctions) <= 4, b.describe
            conj = {name: c for name, c, _ in b.conjunctions}
            assert {"range+others", "one-column-thrice", "nullable+string"} <= set(conj), b.describe
            assert all(1 <= len(c) <= 5 or len(c) == 17 for c in conj.values()), b.describe
            assert len({i for i, _, _ in conj["one-column-thrice"]}) == 1 and len(conj["one-column-thrice"]) == 3
            ranged = conj["range+others"]
            assert len({i for i, _, _ in ranged}) >= 2 and ranged[0][0] == ranged[1][0], b.describe
            assert any(b.columns[i].kind == "str" for i, _, _ in ranged), b.describe
            if any(c.valid is not None and c.valid.any() for c in b.columns if c.kind != "bool"):
                assert b.columns[conj["nullable+string"][0][0]].valid is not None, b.describe
            names = [m[0] for m in b.masks]
            assert names[:8] == ["zero", "all", "first", "last", "50%", "2%", "words", "runs"] and "dirty-tail" in names
            assert ("hole" in names) == (b.n >= 3072)
            assert len([m for m in names if m.startswith("conjunction-")]) == len(b.conjunctions)
    long_one = BC.build(BC.LONG_CONJUNCTION_SEED)
    assert long_one.n >= 1025 and max(len(c[1]) for c in long_one.conjunctions) == 17


def _column_bytes(c):
    vals = b"\0".join(c.values) if c.kind == "str" else np.asarray(c.values).tobytes()
    return (TC.tree_bytes(c.tree, []), vals, None if c.valid is None else c.valid.tobytes(), c.describe, c.route,
            repr(c.scalars), repr(c.range))


@pytest.mark.parametrize("seed", SEEDS, ids=IDS)
def test_build_is_deterministic(seed):
    a, b = BC.build.__wrapped__(seed), BC.build.__wrapped__(seed)
    assert a.describe == b.describe and a.n == b.n
    assert [_column_bytes(c) for c in a.columns] == [_column_bytes(c) for c in b.columns]
    assert [(n, m.tobytes(), d) for n, m, d in a.masks] == [(n, m.tobytes(), d) for n, m, d in b.masks]
    assert repr([(n, c) for n, c, _ in a.conjunctions]) == repr([(n, c) for n, c, _ in b.conjunctions])


@pytest.mark.parametrize("seed", SEEDS, ids=IDS)
def test_oracle_canonical_is_the_truth(seed):
    b = BC.build(seed)
    for c in b.columns:
        got, gvalid = canon(c.tree)
        assert_canonical_is_truth(c, got, gvalid, what=f"batch {BC.seed_id(seed)}, oracle")


@pytest.mark.parametrize("seed", SEEDS, ids=IDS)
def test_filter_canon_is_the_truth_under_the_mask(seed):
    """filter_canon(column, mask) == values[mask] / valid[mask] of the plain truth, by numpy alone."""
    b = BC.build(seed)
    for name, mask, _ in b.masks:
        pred = A.bool_array(mask)
        idx = np.flatnonzero(mask)
        for c in b.columns:
            at = f"batch {BC.seed_id(seed)} mask {name}: {c.describe}"
            got, gvalid = filter_canon(c.tree, pred)
            wvalid = full(c.valid, b.n)[mask]
            assert np.array_equal(full(gvalid, idx.size), wvalid), "validity differs, " + at
            if c.kind == "str":
                views, heap = got
                assert views.shape[0] == idx.size, "length differs, " + at
                for j, i in enumerate(idx):
                    if wvalid[j]:
                        assert view_bytes(views, heap, j) == c.values[int(i)], f"row {int(i)} differs, " + at
            else:
                want = np.asarray(c.values)[mask]
                assert np.asarray(got).dtype == want.dtype and np.asarray(got).tobytes() == want.tobytes(), \
                    "values differ, " + at


@pytest.mark.parametrize("seed", SEEDS, ids=IDS)
def test_row_filter_expected_is_the_truth(seed):
    """row_filter_expected.expected == the AND of numpy compares on the plain truth, nulls false."""
    b = BC.build(seed)
    for name, conj, mask in b.conjunctions:
        at = f"batch {BC.seed_id(seed)} conjunction {name} {[(i, op, s) for i, op, s in conj]!r}: {b.describe}"
        want = np.ones(b.n, bool)
        for i, op, s in conj:
            want &= BC.truth_mask(b.columns[i], op, s)
        assert np.array_equal(want, mask), at
        bits, got, count = row_filter_expected.expected([(b.columns[i].tree, op, s) for i, op, s in conj])
        assert np.array_equal(got, want) and count == int(want.sum()), at
        assert bits == mask_bytes(want).tobytes(), at
        assert all(b.columns[i].kind != "bool" for i, _, _ in conj), at


def test_route_predictor_on_the_existing_trees():
    """The 72 trees of tree_cases by the header's rule: what the batch filter's newer routes see of them."""
    routes = collections.Counter()
    for s in TC.SEEDS:
        tree = TC.build(s).tree
        kind, count = BC.expected_route(tree)
        routes[kind + ("-chunked" if tree.encoding == ENC["CHUNKED"] and kind != "fallback" else "")] += 1
    assert dict(routes) == {"fallback": 60, "packed": 7, "packed-chunked": 2, "inplace": 3}, routes
    # hand-made: every sentence of the rule
    rng = np.random.default_rng(5)
    u = rng.integers(0, 100, 300).astype(np.uint32)
    bp = E.encode_bitpacked(u, bit_width=7, allow_patches=False)
    fr = E.encode_for_bitpacked(u.astype(np.int32) - 50, allow_patches=False)
    zz = E.encode_zigzag(u.astype(np.int32) - 50)
    alp = E.encode_alp(np.round(rng.uniform(1, 100, 300), 1))
    prim, empty = A.primitive(u), A.primitive(u[:0])
    for t in (bp, A.frame_of_reference(bp, 5, 0, "u32"), zz, alp):
        assert BC.expected_route(t) == ("packed", 1)
    assert BC.expected_route(A.chunked([bp, empty, A.frame_of_reference(bp, 5, 0, "u32")])) == ("packed", 2)
    assert BC.expected_route(A.chunked([fr, A.primitive(u[:0].astype(np.int32)), zz])) == ("packed", 2)
    assert BC.expected_route(prim) == ("inplace", 1)
    assert BC.expected_route(A.chunked([prim, empty, prim])) == ("inplace", 2)
    assert BC.expected_route(A.chunked([bp, prim])) == ("fallback", 1)
    assert BC.expected_route(A.chunked([bp, E.encode_dict(u)])) == ("fallback", 1)
    assert BC.expected_route(A.zigzag(A.primitive(u))) == ("fallback", 1)
    assert BC.expected_route(A.frame_of_reference(prim, 5, 0, "u32")) == ("fallback", 1)
    for t in (E.encode_dict(u), E.encode_runend(u), A.bool_array(u > 50), E.encode_fsst([b"a", b"bc"])):
        assert BC.expected_route(t) == ("fallback", 1)


# ---------------------------------------------------------------------------- coverage conditions
def survey():
    """What the batches hold, counted over BATCH_SEEDS."""
    s = dict(routes=collections.Counter(), cells=collections.Counter(), kinds_packed=collections.Counter(),
             kinds_inplace=collections.Counter(), kinds_fallback=collections.Counter(), fallback_encs=collections.Counter(),
             mixed_epilogues=0, mixed_widths=0, whole_slices=0, inner_cuts=0, zero_chunk=0, one_chunk=0,
             conj_total=0, conj_partial=0)
    for seed in SEEDS:
        b = BC.build(seed)
        for c in b.columns:
            tree = c.tree
            chunked = tree.encoding == ENC["CHUNKED"]
            s["routes"][c.route[0] + ("-chunked" if chunked and c.route[0] != "fallback" else "")] += 1
            live = [p for p in BC.pieces(tree) if p.len]
            if c.route[0] == "packed":
                for p in live:
                    s["kinds_packed"][TC.validity_kind(BC.packed_leaf_of(p))] += 1
            if c.route[0] == "packed" and chunked:
                epis = [BC.epilogue_of(p) for p in live]
                for p, e in zip(live, epis):
                    s["cells"][(8 * A.ptype_width(p.ptype), e, TC.has_patches(p))] += 1
                s["mixed_epilogues"] += len(set(epis)) >= 2
                widths = collections.defaultdict(set)
                for p, e in zip(live, epis):
                    widths[e].add(BC.packed_leaf_of(p).meta["bit_width"])
                s["mixed_widths"] += any(len(w) >= 2 for w in widths.values())
                s["whole_slices"] += c.whole_slice % 64 != 0
                offs = np.cumsum([p.len for p in BC.pieces(tree)])[:-1]
                s["inner_cuts"] += any(0 < o < b.n and o % 4096 and o % 64 for o in offs.tolist())
                s["zero_chunk"] += any(p.len == 0 for p in BC.pieces(tree))
                s["one_chunk"] += any(p.len == 1 for p in BC.pieces(tree))
            if c.route[0] == "inplace":
                for p in live:
                    s["kinds_inplace"][TC.validity_kind(p)] += 1
            if c.route[0] == "fallback":
                for node, _, _ in TC.walk(tree):
                    k = TC.validity_kind(node)
                    if k is not None and node.len == tree.len:
                        s["kinds_fallback"][k] += 1
                name = TC.ENC_NAME[tree.encoding]
                if name == "DICT" and c.kind == "str":
                    name = "DICT-strings"
                s["fallback_encs"][(c.kind, name)] += 1
        if b.n >= 64:
            for _, _, m in b.conjunctions:
                s["conj_total"] += 1
                s["conj_partial"] += 0 < int(m.sum()) < b.n
    return s


def allowed_cells():
    """Every T x epilogue the ptype rules allow (Gen.packed_epilogues), with and without patches."""
    out = set()
    for pt in TC.UNSIGNED + TC.SIGNED + TC.FLOATS:
        for e in TC.Gen.packed_epilogues(pt):
            out |= {(8 * A.ptype_width(pt), e, False), (8 * A.ptype_width(pt), e, True)}
    return out


def test_coverage_conditions():
    s = survey()
    cells = allowed_cells()
    assert len(cells) == 44 and {e for _, e, _ in cells} == set(TC.PACKED_EPILOGUES)
    for cell in sorted(cells):
        assert s["cells"][cell] >= 2, f"(T, epilogue, patched) = {cell} is a packed chunk {s['cells'][cell]} times"
    assert s["mixed_epilogues"] >= 6, f"{s['mixed_epilogues']} packed Chunked columns hold two or more epilogues"
    assert s["mixed_widths"] >= 1, f"{s['mixed_widths']} packed Chunked columns hold two bit widths under one epilogue"
    assert s["whole_slices"] >= 6, f"{s['whole_slices']} packed Chunked columns are slices that start off a 64-row boundary"
    assert s["inner_cuts"] >= 6, f"{s['inner_cuts']} packed Chunked columns have a chunk boundary inside a tile and a mask word"
    assert s["zero_chunk"] >= 4, f"{s['zero_chunk']} packed Chunked columns have a zero-length chunk"
    assert s["one_chunk"] >= 4, f"{s['one_chunk']} packed Chunked columns have a one-row chunk"
    for kind in TC.VALIDITY_KINDS:
        for where in ("kinds_packed", "kinds_inplace", "kinds_fallback"):
            assert s[where][kind] >= 2, f"validity kind {kind} occurs {s[where][kind]} times in {where}"
    want = [("prim", e) for e in BC.FALLBACK_PRIM] + [("bool", e) for e in BC.FALLBACK_BOOL] + \
           [("str", "VARBIN"), ("str", "VARBINVIEW"), ("str", "FSST"), ("str", "DICT-strings")]
    for enc in want:
        assert s["fallback_encs"][enc] >= 1, f"fallback encoding {enc} occurs {s['fallback_encs'][enc]} times"
    assert s["routes"]["fallback"] and s["routes"]["inplace-chunked"] >= 6 and s["routes"]["inplace"] >= 6
    assert 4 * s["conj_partial"] >= 3 * s["conj_total"], \
        f"{s['conj_partial']} of {s['conj_total']} conjunction masks have 0 < k < n"


# ---------------------------------------------------------------------------- the comparer can fail
def _fabricated():
    """Three columns (i32 nullable, bool, nullable strings) and the buffers a correct call would return."""
    rng = np.random.default_rng(11)
    n = 300
    strs = [None if i % 5 == 2 else (b"row %d " % i) * (1 + i % 3) for i in range(n)]
    heap, offs, valid = E.strings_to_heap(strs)
    trees = [A.primitive(rng.integers(-1000, 1000, n).astype(np.int32), validity=rng.random(n) < 0.7),
             A.bool_array(rng.random(n) < 0.5),
             A.varbin(A.primitive(offs.astype(np.int32)), A.primitive(heap), validity=valid)]
    mask = rng.random(n) < 0.4
    mask[n - 1] = True
    k = int(mask.sum())
    want = [filter_canon(t, A.bool_array(mask)) for t in trees]
    host, outs = [], []
    for t, (wvals, wvalid), sizes in zip(trees, want, buffer_sizes(trees, want, k)):
        payload = {}
        if t.dtype == DTYPE["PRIMITIVE"]:
            payload["values"] = wvals.tobytes()
        elif t.dtype == DTYPE["BOOL"]:
            payload["values"] = mask_bytes(wvals).tobytes()[: sizes["values"]]
        else:
            payload["views"], payload["data"] = wvals[0].tobytes(), wvals[1].tobytes()
        if "validity" in sizes:
            payload["validity"] = mask_bytes(wvalid).tobytes()[: sizes["validity"]]
        b = {}
        for j, (name, nbytes) in enumerate(sizes.items()):
            raw = np.full(nbytes + GUARD, 0xFF, np.uint8)
            raw[:nbytes] = np.frombuffer(payload[name].ljust(nbytes, b"\0"), np.uint8)
            b[name] = HostBuffer(raw, nbytes, 0x1000 * (j + 1))
        host.append(b)
        is_str = "views" in sizes
        outs.append(HostOut(k, t.dtype, {DTYPE["PRIMITIVE"]: V.ENC["PRIMITIVE"], DTYPE["BOOL"]: V.ENC["BOOL"]}.get(
            t.dtype, V.ENC["VARBINVIEW"]), sizes.get("values", 0), sizes.get("data", 0), 1 if is_str else 0,
            [(0, sizes["data"])] if is_str else [], b["validity"].ptr if "validity" in b else 0))
    return trees, mask, k, want, host, outs


def test_check_outputs_can_fail():
    trees, mask, k, want, host, outs = _fabricated()
    n = mask.size
    check_outputs(host, outs, want, trees, n, k)  # the fabricated buffers are right

    def broken(edit):
        h, o = copy.deepcopy(host), copy.deepcopy(outs)
        edit(h, o)
        with pytest.raises(AssertionError):
            check_outputs(h, o, want, trees, n, k)

    def last_value_byte(h, o):
        h[0]["values"].bytes[4 * k - 1] ^= 1

    def validity_bit(h, o):
        h[0]["validity"].bytes[(k - 1) // 8] ^= 1 << ((k - 1) % 8)

    def guard_byte(h, o):
        h[1]["values"].bytes[h[1]["values"].nbytes + GUARD - 1] = 0xFE

    def view_offset(h, o):
        long_rows = [j for j in range(k) if int(h[2]["views"].bytes[16 * j: 16 * j + 4].view(np.uint32)[0]) > 12]
        at = 16 * long_rows[-1] + 12
        h[2]["views"].bytes[at: at + 4] = (h[2]["views"].bytes[at: at + 4].view(np.uint32) + 1).view(np.uint8)

    def short_heap(h, o):
        o[2].data_bytes -= 1
        o[2].data_buffers = [(0, o[2].data_bytes)]

    for edit in (last_value_byte, validity_bit, guard_byte, view_offset, short_heap):
        broken(edit)
    # ... and each of the other fields it reads
    broken(lambda h, o: setattr(o[0], "len", k - 1))
    broken(lambda h, o: setattr(o[0], "validity", 0))
    broken(lambda h, o: setattr(o[0], "validity", 0x7777))
    broken(lambda h, o: setattr(o[1], "validity", 0x7777))
    last = (k - 1) // 8
    broken(lambda h, o: h[1]["values"].bytes.__setitem__(last, h[1]["values"].bytes[last] ^ (1 << ((k - 1) % 8))))
    broken(lambda h, o: h[2]["data"].bytes.__setitem__(h[2]["data"].nbytes - 1, 0))
    broken(lambda h, o: h[2]["validity"].bytes.__setitem__(0, h[2]["validity"].bytes[0] ^ 1))
