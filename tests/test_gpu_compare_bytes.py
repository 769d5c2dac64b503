"""GPU: vxg_compare_bytes against the oracle's canonical rows compared as Python bytes, byte for byte.

Every call writes into buffers of the exact size + 64 guard bytes filled with 0xFF: the tail bits
past len must be zero and the guard untouched.  `info` says which path ran, and the tests assert
it: the truth-table + lookup kernels for Dict, the row kernel in place for VarBin / VarBinView /
FSST, the canonicalize fallback elsewhere."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import vortex_amd as V
import vortex_amd._lib as L
import vortex_amd.arrays as A
import vortex_amd.encode as E
from compare_bytes_expected import expected, rows_of
from compare_expected import OPS
from oracle_tree import bad_bitpacked, misaligned_bitpacked, slice_bitpacked

pytestmark = pytest.mark.gpu

GUARD = 64
ALL_OPS = list(OPS)
ZERO = dict(dict_launches=0, dict_chunks=0, table_launches=0, direct_launches=0, direct_chunks=0, fallback_arrays=0)


def _dev():
    import torch
    return torch.device("cuda", 0)


def run(ctx, tree, op, scalar, null_as_false=False):
    """compare on the GPU into guarded buffers -> (Canonical, values bytes, validity bytes | None)."""
    import torch
    nb = ((tree.len + 63) // 64) * 8
    vals = torch.full((nb + GUARD,), 0xFF, dtype=torch.uint8, device=_dev())
    valid = torch.full((nb + GUARD,), 0xFF, dtype=torch.uint8, device=_dev())
    res = V.compare(tree.to(_dev()), op, scalar, ctx, null_as_false=null_as_false, out_values=vals,
                    out_validity=valid)
    hv, hm = vals.cpu().numpy(), valid.cpu().numpy()
    assert (hv[nb:] == 0xFF).all(), "values guard bytes written"
    assert (hm[nb:] == 0xFF).all(), "validity guard bytes written"
    if res.validity is None:
        assert (hm == 0xFF).all(), "validity written although none is returned"
    assert res.kind == "bool" and res.len == tree.len
    return res, hv[:nb].tobytes(), (None if res.validity is None else hm[:nb].tobytes())


def check(ctx, tree, op, scalar, rows=None, null_as_false=False, info=None):
    """One compare checked against the oracle; `info`: the counters that must match exactly."""
    want, want_valid, mask = expected(tree, op, scalar, rows)
    res, got, got_valid = run(ctx, tree, op, scalar, null_as_false)
    assert got == want, (op, scalar[:16], tree.len, np.flatnonzero(
        np.frombuffer(got, np.uint8) != np.frombuffer(want, np.uint8))[:8])
    assert got_valid == (None if null_as_false else want_valid)
    for k, v in (info or {}).items():
        assert res.info[k] == v, (k, res.info)
    return res, mask


def check_dict(ctx, tree, op, scalar, rows=None, **kw):
    res, mask = check(ctx, tree, op, scalar, rows, **kw)
    if tree.len:
        assert res.info["dict_launches"] >= 1 and res.info["table_launches"] >= 1, res.info
    assert res.info["fallback_arrays"] == 0 and res.info["direct_launches"] == 0, res.info
    return res, mask


def check_direct(ctx, tree, op, scalar, rows=None, **kw):
    res, mask = check(ctx, tree, op, scalar, rows, **kw)
    if tree.len:
        assert res.info["direct_launches"] >= 1, res.info
    assert res.info["fallback_arrays"] == 0 and res.info["dict_launches"] == 0 and res.info["table_launches"] == 0, res.info
    return res, mask


# ---- trees -----------------------------------------------------------------------------------
def varbin_of(rows, offs_dtype=np.int32, packed_offsets=False, utf8=True):
    heap, offs, valid = E.strings_to_heap(rows)
    o = E.encode_for_bitpacked(offs.astype(offs_dtype), allow_patches=False) if packed_offsets \
        else A.primitive(offs.astype(offs_dtype))
    return A.varbin(o, A.primitive(heap), utf8=utf8, validity=None if valid.all() else valid)


def codes_tree(T, W, codes):
    """BitPacked u<T> codes of exactly W bits."""
    dt, p = np.dtype(f"u{T // 8}"), f"u{T}"
    c = np.asarray(codes).astype(dt)
    if W == 0:
        return A.bitpacked(np.zeros(0, np.uint8), p, 0, c.size)
    if W == T:
        return A.bitpacked(E.bitpack_buffer(c, T), p, T, c.size)
    return E.encode_bitpacked(c, bit_width=W, allow_patches=False)


def distinct(k):
    """k distinct strings whose lengths straddle the 12/13-byte view boundary."""
    return [b"v%05d" % i + b"-" * (i % 11) for i in range(k)]


def views_tree(rows, n_buffers=2, utf8=True):
    """A VarBinView whose non-inlined rows are spread round-robin over n_buffers data buffers."""
    views = np.zeros((len(rows), 16), dtype=np.uint8)
    parts = [[] for _ in range(n_buffers)]
    sizes = [0] * n_buffers
    k = 0
    for i, st in enumerate(rows):
        if st is None:
            continue
        views[i, :4] = np.frombuffer(np.uint32(len(st)).tobytes(), np.uint8)
        if len(st) <= 12:
            views[i, 4: 4 + len(st)] = np.frombuffer(st, np.uint8)
            continue
        b = k % n_buffers
        k += 1
        views[i, 4:8] = np.frombuffer(st[:4], np.uint8)
        views[i, 8:12] = np.frombuffer(np.uint32(b).tobytes(), np.uint8)
        views[i, 12:16] = np.frombuffer(np.uint32(sizes[b]).tobytes(), np.uint8)
        parts[b].append(st)
        sizes[b] += len(st)
    bufs = [np.frombuffer(b"".join(p), dtype=np.uint8).copy() for p in parts]
    valid = [s is not None for s in rows]
    return A.varbinview(views, bufs, utf8=utf8, validity=None if all(valid) else valid)


BASE = [b"a", b"ab", b"abc", b"AIR", b"MAIL", b"abcd", b"abcde", b"twelve bytes", b"thirteen byte", b"thirteen bytf",
        b"\x80\xff\x00z", b"\xff", b"\x01", b"x" * 64, b"x" * 65, b"x" * 64 + b"y", b"q" * 300, b"q" * 299 + b"r",
        "héllo wörld".encode(), b"thirteen byte and more", b"prefix-tie-0001-aaaa", b"prefix-tie-0001-aaab"]
# present / absent / empty / a proper prefix of a row / a row plus one byte / below the minimum /
# above the maximum / bytes >= 0x80 / lengths 0, 1, 4, 5, 12, 13, 64, 65, 300
SCALARS = [b"abc", b"zzz-absent", b"", b"thirteen", b"thirteen byte\x00", b"\x00", b"\xff\xff", b"\x80\xff\x00z",
           b"a", b"MAIL", b"abcde", b"twelve bytes", b"thirteen byte", b"x" * 64, b"x" * 65, b"q" * 300,
           b"prefix-tie-0001-aaab", b"\x80"]


def corpus(n, seed, empties=False, binary=False):
    rng = np.random.default_rng(seed)
    pool = BASE + ([b""] if empties else [])
    if binary:  # random binary strings among the text: FSST escapes
        pool = pool + [rng.integers(0, 256, int(rng.integers(1, 30)), dtype=np.uint8).tobytes() for _ in range(12)]
    return pool + [pool[int(i)] for i in rng.integers(0, len(pool), n - len(pool))]


KINDS = {
    "dict": lambda rows: E.encode_dict_strings(rows),
    "varbin": lambda rows: varbin_of(rows),
    "varbinview": lambda rows: E.encode_varbinview(rows),
    "fsst": lambda rows: E.encode_fsst(rows),
}
CHECK = {"dict": check_dict, "varbin": check_direct, "varbinview": check_direct, "fsst": check_direct}


# ---- Dict geometry -----------------------------------------------------------------------------
LENS = [0, 1, 63, 64, 65, 1023, 1024, 1025, 2085, 3073]
OFFSETS = [0, 1, 63, 1000, 1023]


@pytest.mark.parametrize("T", [8, 16, 32, 64])
def test_dict_geometry(ctx, T):
    rng = np.random.default_rng(300 + T)
    total = max(LENS) + max(OFFSETS)
    k = 0
    for W, nd in ((0, 1), (1, 2), (3, 7), (5, 20) if T == 8 else (9, 300), (T, 200 if T == 8 else 300)):
        values = distinct(nd)
        codes = rng.integers(0, nd, total)
        codes[rng.integers(0, total, 4)] = nd - 1
        full = A.dict_array(varbin_of(values), codes_tree(T, W, codes))
        assert full.children[1].meta["bit_width"] == W
        full_rows = rows_of(full)  # the oracle walk, once; a slice's rows are a slice of these
        assert full_rows[0] == [values[c] for c in codes]
        scalar = values[nd // 2]
        for n in LENS:
            for off in OFFSETS:
                tree = A.dict_array(full.children[0], slice_bitpacked(full.children[1], off, off + n))
                assert tree.children[1].meta["offset"] == off and tree.len == n
                if n == 65:  # a slice's rows are that slice of the whole array's rows
                    assert rows_of(tree)[0] == full_rows[0][off: off + n]
                op = ALL_OPS[k % 6]
                k += 1
                check_dict(ctx, tree, op, scalar, (full_rows[0][off: off + n], None),
                           info=dict(dict_chunks=1, direct_chunks=0))


@pytest.mark.parametrize("nd", [8191, 8192, 8193])
def test_dict_lds_table_bound(ctx, nd):
    """Dictionaries just below, at and just above the bound up to which the lookup kernel keeps the
    truth table in LDS (8192 entries)."""
    rng = np.random.default_rng(nd)
    values = [b"k%05d" % i for i in range(nd)]
    codes = rng.integers(0, nd, 3000)
    codes[:3] = [nd - 1, 0, nd - 2]
    tree = A.dict_array(varbin_of(values), codes_tree(16, 14, codes))
    rows = rows_of(tree)
    for op, s in (("==", values[nd - 1]), ("<", values[nd // 2]), (">=", values[nd - 2])):
        check_dict(ctx, tree, op, s, rows)


def test_dict_other_codes(ctx):
    """Primitive codes are read in place; FoR(BitPacked) codes and BitPacked codes with patches go
    through a temporary."""
    rng = np.random.default_rng(7)
    values = distinct(40)
    codes = rng.integers(0, 40, 1500)
    vb = varbin_of(values, np.int64)
    for ct in (A.primitive(codes.astype(np.uint8)), A.primitive(codes.astype(np.uint16)), A.primitive(codes.astype(np.uint32)),
               A.primitive(codes.astype(np.uint64)), E.encode_for_bitpacked(codes.astype(np.uint32), allow_patches=False),
               E.encode_bitpacked(codes.astype(np.uint32), bit_width=4, allow_patches=True)):  # patched
        tree = A.dict_array(vb, ct)
        rows = rows_of(tree)
        for op in ("==", ">"):
            check_dict(ctx, tree, op, values[17], rows)
    # a dictionary held as VarBinView or FSST is compared by the same row kernels
    for vals in (E.encode_varbinview(values), E.encode_fsst(values)):
        tree = A.dict_array(vals, codes_tree(32, 6, codes))
        check_dict(ctx, tree, "<=", values[17], rows_of(tree))


# ---- operators and scalars ---------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(KINDS))
def test_operators_and_scalars(ctx, kind):
    for empties in (False, True):
        tree = KINDS[kind](corpus(200, 5, empties=empties, binary=True))
        rows = rows_of(tree)
        for i, s in enumerate(SCALARS):
            for op in (ALL_OPS if not empties else ALL_OPS[i % 3::3]):
                CHECK[kind](ctx, tree, op, s, rows)
    # a str scalar is compared as its UTF-8 bytes
    CHECK[kind](ctx, tree, "==", "héllo wörld", rows)


def test_long_scalars(ctx):
    """Scalars beyond the kernel-argument form, up to 64 KiB, against rows that tie with them."""
    big = bytes(np.random.default_rng(1).integers(0, 256, 65536, dtype=np.uint8))
    rows = [big, big[:-1], big[:-1] + b"\xff", big + b"\x00", b"", big[:65], big[:66]]
    for kind in KINDS:
        tree = KINDS[kind](rows)
        r = rows_of(tree)
        for s in (big, big[:66], big[:65], big[:300]):
            for op in ("==", "<"):
                CHECK[kind](ctx, tree, op, s, r)


# ---- nulls ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("null_as_false", [False, True])
def test_nulls(ctx, null_as_false):
    rows = corpus(300, 9, empties=True)
    rows = [None if i % 7 == 3 else r for i, r in enumerate(rows)]
    trees = [(E.encode_dict_strings_nullable(rows), check_dict), (varbin_of(rows), check_direct),
             (E.encode_fsst(rows), check_direct), (E.encode_varbinview(rows), check_direct)]
    for tree, chk in trees:
        assert tree.nullable
        r = rows_of(tree)
        for op, s in (("==", b"AIR"), ("!=", b"AIR"), ("<", b"b"), (">=", b"")):
            chk(ctx, tree, op, s, r, null_as_false=null_as_false)


# ---- VarBin / VarBinView -----------------------------------------------------------------------
def test_varbin_offsets(ctx):
    rows = corpus(700, 12, empties=True)
    for dt in (np.int32, np.int64, np.uint32):
        for packed in (False, True):
            tree = varbin_of(rows, dt, packed)
            assert (tree.children[0].encoding != A.ENC["PRIMITIVE"]) == packed
            r = rows_of(tree)
            for op, s in (("==", b"abcde"), ("<", b"thirteen byte"), (">", b"x" * 64)):
                check_direct(ctx, tree, op, s, r, info=dict(direct_chunks=1, direct_launches=1))
    # a sliced VarBin: the first offset is not 0
    heap, offs, _ = E.strings_to_heap(rows)
    tree = A.varbin(A.primitive(offs[5:].astype(np.int32)), A.primitive(heap))
    assert int(offs[5]) != 0
    r = rows_of(tree)
    assert r[0] == rows[5:]
    for op in ALL_OPS:
        check_direct(ctx, tree, op, b"abcd", r)


def test_varbinview_buffers(ctx):
    rows = corpus(500, 13, empties=True)
    for nb in (2, 3):
        tree = views_tree(rows, nb)
        assert tree.meta["n_buffers"] == nb
        r = rows_of(tree)
        assert r[0] == rows
        for op, s in (("==", b"prefix-tie-0001-aaab"), ("<", b"prefix-tie-0001-aaab"), (">=", b"thirteen byte"),
                      ("!=", b"q" * 300), ("<=", b"thir")):
            check_direct(ctx, tree, op, s, r, info=dict(direct_chunks=1, direct_launches=1))


# ---- FSST ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("compress_children", [True, False])
def test_fsst(ctx, compress_children):
    for n in (0, 1, 63, 64, 65, 1000, 2085):
        rows = corpus(max(n, 40), 20 + n, empties=True, binary=True)[:n]
        if n:
            tree = E.encode_fsst(rows, compress_children=compress_children)
        else:  # an empty FSST array: empty codes, offsets [0]
            tree = A.fsst(A.primitive(np.zeros(0, np.uint64)), A.primitive(np.zeros(0, np.uint8)),
                          A.varbin(A.primitive(np.zeros(1, np.int32)), A.primitive(np.zeros(0, np.uint8))),
                          A.primitive(np.zeros(0, np.int32)))
        r = rows_of(tree)
        # rows equal to the scalar, rows that are a prefix of it and the reverse; escapes
        for op, s in (("==", b"thirteen byte"), ("!=", b"thirteen byte"), ("<", b"thirteen byte and"), (">", b"thirteen"),
                      ("<=", b"\x80\xff\x00z"), (">=", b"")):
            check_direct(ctx, tree, op, s, r, info=dict(direct_chunks=1, direct_launches=1 if n else 0))


def test_fsst_codes_that_are_not_the_greedy_choice(ctx):
    """Symbols "a", "b", "ab"; row 0 is stored as the codes for "a","b": it still equals b"ab"."""
    syms = np.array([ord("a"), ord("b"), ord("a") | ord("b") << 8], dtype=np.uint64)
    codes = np.array([0, 1, 2, 0, 255, ord("z")], dtype=np.uint8)
    tree = A.fsst(A.primitive(syms), A.primitive(np.array([1, 1, 2], np.uint8)),
                  A.varbin(A.primitive(np.array([0, 2, 3, 4, 6, 6], np.int32)), A.primitive(codes)),
                  A.primitive(np.array([2, 2, 1, 1, 0], np.int32)))
    r = rows_of(tree)
    assert r[0] == [b"ab", b"ab", b"a", b"z", b""]
    res, mask = check_direct(ctx, tree, "==", b"ab", r)
    assert mask.tolist() == [True, True, False, False, False]
    for op in ALL_OPS:
        for s in (b"ab", b"a", b"z", b"", b"abc"):
            check_direct(ctx, tree, op, s, r)


# ---- Chunked ---------------------------------------------------------------------------------------
def test_chunked_dict_column_is_two_launches(ctx):
    """92 Dict chunks with different dictionaries and odd lengths (chunks start inside a word): one
    truth-table launch and one lookup launch, nothing uploaded."""
    rng = np.random.default_rng(92)
    modes = [b"AIR", b"MAIL", b"SHIP", b"TRUCK", b"RAIL", b"REG AIR", b"FOB"]
    chunks = []
    for i in range(92):
        k = 3 + i % 5
        pool = [modes[(i + j) % 7] for j in range(k)]
        chunks.append(E.encode_dict_strings([pool[int(c)] for c in rng.integers(0, k, 37 + (i * 13) % 50)]))
    tree = A.chunked(chunks)
    r = rows_of(tree)
    for op, s in (("==", b"AIR"), ("<", b"REG AIR"), ("!=", "MAIL")):
        check(ctx, tree, op, s, r, info=dict(ZERO, table_launches=1, dict_launches=1, dict_chunks=92))


def test_chunked_mixed(ctx):
    rows = corpus(120, 33, empties=True, binary=True)
    empty_vb = A.varbin(A.primitive(np.zeros(1, np.int32)), A.primitive(np.zeros(0, np.uint8)))
    empty_dict = A.dict_array(varbin_of([b"x"]), codes_tree(64, 0, np.zeros(0, np.uint64)))
    tree = A.chunked([KINDS["dict"](rows[:33]), empty_dict, KINDS["fsst"](rows[33:70]), KINDS["varbin"](rows[70:99]), empty_vb,
                      KINDS["varbinview"](rows[99:]), A.chunked([KINDS["varbin"](rows[:10]), KINDS["fsst"](rows[10:31])])])
    r = rows_of(tree)
    for op, s in (("==", b"abcde"), (">", b"abcde"), ("<=", b"thirteen byte")):
        # the VarBinView chunk and the canonicalized nested Chunked share the view kernel's launch
        check(ctx, tree, op, s, r, info=dict(dict_launches=1, dict_chunks=2, table_launches=1, direct_launches=3,
                                             direct_chunks=4, fallback_arrays=1))


def test_fallback(ctx):
    """An encoding with no in-place path (a nested Chunked, also as a dictionary) is canonicalized
    into a temporary VarBinView and compared.  (Constant and Sparse string arrays are not part of the
    engine's array model -- vxg_canonicalize answers NotImplemented for them -- so none is built here.)"""
    rows = corpus(150, 34, empties=True)
    nested = A.chunked([A.chunked([KINDS["dict"](rows[:70]), KINDS["varbinview"](rows[70:])])])
    r = rows_of(nested)
    for op in ("==", "<"):
        res, _ = check(ctx, nested, op, b"abcd", r, info=dict(ZERO, fallback_arrays=1, direct_launches=1))
    values = distinct(9)
    tree = A.dict_array(A.chunked([varbin_of(values[:4]), varbin_of(values[4:])]), codes_tree(8, 4, np.arange(300) % 9))
    check(ctx, tree, ">=", values[4], info=dict(ZERO, fallback_arrays=1, table_launches=1, dict_launches=1, dict_chunks=1))


# ---- errors ------------------------------------------------------------------------------------------
def _status(ctx, tree, op_code=0, flags=0, scalar=b"AIR"):
    keep = []
    node = A.flatten(tree.to(_dev()), keep)
    out = L.VxgCanonical()
    sc = (C.c_uint8 * max(len(scalar), 1)).from_buffer_copy(scalar.ljust(1, b"\0"))
    st = ctx.lib.vxg_compare_bytes(ctx.handle, C.byref(node), op_code, sc, len(scalar), flags, C.byref(out), None,
                                   ctx.stream_ptr())
    assert not out.values or st == 0
    if out.values:
        ctx.sync()
        L.check(ctx.lib.vxg_free(ctx.handle, C.c_void_p(out.values)))
    return L.STATUS[st]


def test_errors(ctx):
    ok = E.encode_dict_strings([b"AIR", b"MAIL"] * 600)
    assert _status(ctx, ok) == "OK"
    assert _status(ctx, A.primitive(np.arange(10, dtype=np.int32))) == "MismatchedTypes"
    assert _status(ctx, A.bool_array(np.ones(10, bool))) == "MismatchedTypes"
    assert _status(ctx, ok, op_code=6) == "InvalidArgument"
    assert _status(ctx, ok, op_code=-1) == "InvalidArgument"
    assert _status(ctx, ok, flags=2) == "InvalidArgument"
    codes = ok.children[1]
    short = dataclasses.replace(ok, children=[ok.children[0], dataclasses.replace(
        codes, buffers=[np.asarray(codes.buffers[0])[:-128]])])
    assert _status(ctx, short) == "InvalidArgument"
    assert "Expected 256 packed bytes, got 128" in ctx.lib.vxg_last_error().decode()
    # the BitPacked codes of a Dict, malformed: rejected before anything is launched
    block = E.encode_dict_strings([b"AIR", b"MAIL"] * 512)
    values, codes = block.children
    for bad, text in bad_bitpacked(codes) + [(misaligned_bitpacked(codes, _dev()), "16-byte aligned")]:
        assert _status(ctx, dataclasses.replace(block, children=[values, bad])) == "InvalidArgument"
        assert text in ctx.lib.vxg_last_error().decode()
    with pytest.raises(V.VortexGpuError, match="unknown operator"):
        V.compare(ok.to(_dev()), "~", b"AIR", ctx)


def test_code_out_of_bounds(ctx):
    """A code >= values_len: the call returns OK, the next sync reports OutOfBounds, the row's bit is
    0, and a following compare on a good array is clean."""
    values = varbin_of([b"AIR", b"MAIL", b"SHIP"])
    good_codes = np.arange(2000) % 3
    bad_codes = good_codes.copy()
    bad_codes[1234] = 3
    for make in (lambda c: codes_tree(16, 2, c), lambda c: A.primitive(c.astype(np.uint8))):
        with pytest.raises(V.VortexGpuError) as ei:
            V.compare(A.dict_array(values, make(bad_codes)).to(_dev()), "!=", b"zz", ctx)
        assert ei.value.kind == "OutOfBounds"
        res = V.compare(A.dict_array(values, make(bad_codes)).to(_dev()), "!=", b"zz", ctx, sync=False)
        with pytest.raises(V.VortexGpuError):
            ctx.sync()
        got = res.numpy()
        assert not got[1234] and got.sum() == 1999
        check_dict(ctx, A.dict_array(values, make(good_codes)), "!=", b"zz")
    # an empty dictionary makes every code out of bounds
    empty = A.dict_array(A.varbin(A.primitive(np.zeros(1, np.int32)), A.primitive(np.zeros(0, np.uint8))),
                         codes_tree(8, 0, np.zeros(100, np.uint8)))
    with pytest.raises(V.VortexGpuError) as ei:
        V.compare(empty.to(_dev()), "==", b"", ctx)
    assert ei.value.kind == "OutOfBounds"


# ---- compare then filter -----------------------------------------------------------------------------
def test_compare_then_filter(ctx):
    """filter(col, predicate_from(compare(col, "==", b"AIR", null_as_false=True))) == the selected rows."""
    rng = np.random.default_rng(11)
    modes = [b"AIR", b"MAIL", b"SHIP", b"TRUCK", b"RAIL", b"REG AIR", b"FOB"]
    rows = [None if rng.random() < 0.2 else modes[int(rng.integers(0, 7))] for _ in range(5000)]
    tree = E.encode_dict_strings_nullable(rows)
    dev_tree = tree.to(_dev())
    pred = V.compare(dev_tree, "==", b"AIR", ctx, null_as_false=True)
    assert pred.info["dict_launches"] == 1 and pred.info["table_launches"] == 1 and pred.info["fallback_arrays"] == 0
    got = A.filter(dev_tree, V.predicate_from(pred), ctx)
    want = [r for r in rows if r == b"AIR"]
    assert got.len == len(want) > 0
    from oracle_tree import view_bytes
    views, data = got.numpy()
    assert [view_bytes(views, data, i) for i in range(got.len)] == want
    assert got.validity is None or got.validity_mask().all()
