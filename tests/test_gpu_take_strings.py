"""vxg_take_array_ex on the GPU: string, bool and primitive rows taken from compressed arrays, byte
for byte against take_expected.take_canon (views, heap, data buffer table, validity), with the
info counters that say which path ran."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import vortex_amd as V
import vortex_amd._lib as L
import vortex_amd.arrays as A
import vortex_amd.encode as E
from oracle_tree import canon
from take_expected import take_canon

pytestmark = pytest.mark.gpu

N = 20_000
# wave (64) and heap-rebuild tile (4096) edges, and the FSST kernels' own 1024-row tile
COUNTS = [0, 1, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097, 10_001]


def _dev():
    import torch
    return torch.device("cuda", 0)


# ---- the base rows and their trees, built once -------------------------------------------------
def base_rows():
    """20 000 rows from a pool of 300 strings: lengths 0, 1, 12, 13, about 40 and 300, some with
    bytes >= 0x80 (escapes under an FSST table trained mostly on ASCII); every 7th row null."""
    rng = np.random.default_rng(2024)
    words = [b"the", b"quick", b"brown", b"fox", b"jumps", b"over", b"lazy", b"dog", b"MAIL", b"TRUCK", b"deliver in person"]
    pool = [b"", b"x", b"twelve bytes", b"thirteen byte", b"\x80\xff\x00\xfe high bytes \xc3\xa9", b"q" * 300,
            (b"long row " * 34)[:300]]
    while len(pool) < 300:
        ln = int(rng.choice([1, 12, 13, 40, 40, 40, 41, 38, 300]))
        s = b" ".join(words[int(i)] for i in rng.integers(0, len(words), 80))[:ln]
        if len(pool) % 9 == 0:
            s = bytes([0x80 + len(pool) % 100]) + s[1:]
        pool.append(s)
    rows = [pool[int(i)] for i in rng.integers(0, len(pool), N)]
    rows[:len(pool)] = pool
    return [None if i % 7 == 3 else r for i, r in enumerate(rows)]


def varbin_of(rows, offs_dtype=np.int32, packed_offsets=False):
    heap, offs, valid = E.strings_to_heap(rows)
    o = E.encode_for_bitpacked(offs.astype(offs_dtype), allow_patches=False) if packed_offsets \
        else A.primitive(offs.astype(offs_dtype))
    return A.varbin(o, A.primitive(heap), validity=None if valid.all() else valid)


KINDS = {
    "varbin": lambda rows: varbin_of(rows),
    "fsst": lambda rows: E.encode_fsst(rows),
    "dict": lambda rows: E.encode_dict_strings_nullable(rows),
    "varbinview": lambda rows: E.encode_varbinview(rows),
}
_CACHE: dict = {}


def cached(key, make):
    """(tree, its device copy, oracle canonical) built once per session."""
    if key not in _CACHE:
        tree = make()
        _CACHE[key] = (tree, tree.to(_dev()), canon(tree))
    return _CACHE[key]


def base(kind):
    if "rows" not in _CACHE:
        _CACHE["rows"] = base_rows()
    return cached(("base", kind), lambda: KINDS[kind](_CACHE["rows"]))


def check(ctx, entry, idx, force=False, info=None):
    """One take checked byte for byte against the oracle; `info`: counters that must match."""
    tree, dev_tree, canonical = entry
    idx = np.asarray(idx)
    (wviews, wheap), wvalid = take_canon(tree, idx, canonical)
    res = A.take(dev_tree, idx, ctx, force_canonical=force)
    assert res.kind == "varbinview" and res.len == idx.size
    views, heap = res.numpy()
    assert heap.tobytes() == wheap.tobytes(), (idx.size, heap.size, wheap.size)
    bad = np.flatnonzero((views != wviews).any(axis=1))
    assert bad.size == 0, (bad[:8], views[bad[:2]], wviews[bad[:2]])
    assert res.data_buffers == [(0, wheap.size)]
    gvalid = res.validity_mask()
    if wvalid is None or gvalid is None:
        assert (wvalid is None or wvalid.all()) and (gvalid is None or gvalid.all())
    else:
        assert gvalid.tolist() == wvalid.tolist()
    for k, v in (info or {}).items():
        assert res.info[k] == v, (k, res.info)
    if force:
        assert res.info["fallback_arrays"] == 1 and res.info["direct_arrays"] == 0 and res.info["dict_arrays"] == 0, res.info
    return res


def in_place(kind):
    return dict(fallback_arrays=0, **({"dict_arrays": 1} if kind == "dict" else {"direct_arrays": 1}))


# ---- 1. index counts -----------------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(KINDS))
def test_index_counts(ctx, kind):
    rng = np.random.default_rng(1)
    for k in COUNTS:
        idx = rng.integers(0, N, k).astype(np.int32)
        if k > 10:
            idx[5] = idx[2]  # a repeat for certain
        check(ctx, base(kind), idx, info=in_place(kind))


# ---- 2. index patterns ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(KINDS))
def test_index_patterns(ctx, kind):
    rng = np.random.default_rng(2)
    k = 5000
    idx = np.sort(rng.integers(0, N, k)).astype(np.int64)
    check(ctx, base(kind), idx, info=in_place(kind))
    check(ctx, base(kind), idx[::-1].copy(), info=in_place(kind))
    check(ctx, base(kind), np.full(k, 5, np.uint32), info=in_place(kind))  # row 5: 300 bytes, k copies
    assert base(kind)[0].len == N and len(_CACHE["rows"][5]) == 300
    check(ctx, base(kind), np.array([0, N - 1, N - 1, 0], np.uint64), info=in_place(kind))


@pytest.mark.parametrize("dt", [np.uint8, np.uint16, np.uint32, np.uint64, np.int8, np.int16, np.int32, np.int64])
def test_index_dtypes(ctx, dt):
    if "rows" not in _CACHE:
        _CACHE["rows"] = base_rows()
    rng = np.random.default_rng(3)
    idx = rng.integers(0, 120, 100).astype(dt)  # (fewer than len: a Dict stays on its in-place path)
    for kind in KINDS:
        check(ctx, cached(("short", kind), lambda: KINDS[kind](_CACHE["rows"][:120])), idx, info=in_place(kind))


# ---- 3. offsets forms ------------------------------------------------------------------------------
def test_varbin_offsets(ctx):
    if "rows" not in _CACHE:
        _CACHE["rows"] = base_rows()
    rows = _CACHE["rows"][:3000]
    rng = np.random.default_rng(4)
    idx = rng.integers(0, len(rows), 700).astype(np.int32)
    for dt in (np.int64, np.uint32):
        check(ctx, cached(("vb", dt), lambda: varbin_of(rows, dt)), idx, info=in_place("varbin"))
    # FoR(BitPacked) offsets are read in place, element by element: no decode of the offsets
    entry = cached(("vb", "packed"), lambda: varbin_of(rows, np.int32, packed_offsets=True))
    assert entry[0].children[0].encoding != A.ENC["PRIMITIVE"]
    check(ctx, entry, idx, info=in_place("varbin"))
    # a sliced VarBin: the first offset is not 0
    heap, offs, _ = E.strings_to_heap([r or b"" for r in rows])
    sliced = A.varbin(A.primitive(offs[5:].astype(np.int32)), A.primitive(heap))
    assert int(offs[5]) != 0
    check(ctx, cached(("vb", "sliced"), lambda: sliced), idx[idx < len(rows) - 5], info=in_place("varbin"))


# ---- 4. Dict ---------------------------------------------------------------------------------------
def test_dict_codes(ctx):
    if "rows" not in _CACHE:
        _CACHE["rows"] = base_rows()
    rows = [r or b"" for r in _CACHE["rows"]]
    rng = np.random.default_rng(5)
    packed = cached(("dict", "packed"), lambda: E.encode_dict_strings(rows))
    assert packed[0].children[1].encoding == A.ENC["FL_BITPACKED"]
    plain_codes = A.primitive(canon(packed[0].children[1])[0].astype(np.uint16))
    plain = cached(("dict", "plain"), lambda: A.dict_array(packed[0].children[0], plain_codes))
    few = rng.integers(0, N, N // 8).astype(np.uint32)
    res = check(ctx, packed, few, info=dict(dict_arrays=1, fallback_arrays=0, direct_arrays=0))
    assert res.info["packed_launches"] >= 1
    # above len / 8 the codes go through their canonical values, not the packed-domain kernel
    check(ctx, packed, rng.integers(0, N, N // 2).astype(np.uint32), info=dict(dict_arrays=1, fallback_arrays=0, packed_launches=0))
    # from n = len the planner's density rule canonicalizes the Dict whole ("String take")
    check(ctx, packed, rng.integers(0, N, N).astype(np.uint32), info=dict(dict_arrays=0, fallback_arrays=1, packed_launches=0))
    check(ctx, plain, few, info=dict(dict_arrays=1, fallback_arrays=0, packed_launches=0))
    # the nullable dictionary (slot 0 null) is the base "dict" tree
    res = check(ctx, base("dict"), few, info=dict(dict_arrays=1, fallback_arrays=0))
    assert res.info["packed_launches"] >= 1 and res.validity is not None


def test_dict_code_past_the_dictionary(ctx):
    values = varbin_of([b"AIR", b"MAIL", b"a value past twelve bytes"])
    codes = (np.arange(2000) % 3).astype(np.uint64)
    codes[1234] = 3
    for make in (lambda c: E.encode_bitpacked(c, bit_width=2, allow_patches=False), lambda c: A.primitive(c.astype(np.uint8))):
        tree = A.dict_array(values, make(codes)).to(_dev())
        for idx in (np.array([7, 1234, 9], np.int32), np.arange(2000, dtype=np.int32)):
            with pytest.raises(V.VortexGpuError) as ei:
                A.take(tree, idx, ctx)
            assert ei.value.kind == "OutOfBounds"
        good = A.take(tree, np.array([7, 1235, 9], np.int32), ctx)
        assert good.info["dict_arrays"] == 1 and good.numpy()[1].tobytes() == b"MAILa value past twelve bytesAIR"


# ---- 5. FSST ---------------------------------------------------------------------------------------
def fsst_literal(symbols, rows_codes, ulens, lens_dtype=np.int32, offs_dtype=np.int32):
    syms = np.array([int.from_bytes(s, "little") for s in symbols], dtype=np.uint64)
    slen = np.array([len(s) for s in symbols], dtype=np.uint8)
    codes = np.array([c for r in rows_codes for c in r], dtype=np.uint8)
    offs = np.cumsum([0] + [len(r) for r in rows_codes]).astype(offs_dtype)
    return A.fsst(A.primitive(syms), A.primitive(slen), A.varbin(A.primitive(offs), A.primitive(codes), utf8=False),
                  A.primitive(np.asarray(ulens).astype(lens_dtype)))


def decode_literal(symbols, codes):
    out, it = b"", iter(codes)
    for c in it:
        out += bytes([next(it)]) if c == 255 else symbols[c]
    return out


SYMS = [b"ABCDEFGH", b"12345678", b"a", b"bc", b"xyz"]
SHAPES = [[255, 0x80, 255, 0xFF, 255, 0x00], [255, 7] * 13, [0, 1, 0, 1], [0], [1] * 40, [], [2], [3, 2, 4], [0, 255, 9, 1, 2],
          [4, 4, 4, 4, 3], [2] * 12, [2] * 13, [0, 3, 2, 2], [0, 4, 2, 2]]


@pytest.mark.parametrize("lens_dtype", [np.int32, np.uint16, np.int64])
def test_fsst_literals(ctx, lens_dtype):
    """Rows made only of escapes, rows of 8-byte symbols (the one-store path and the byte tail), empty
    rows, rows that end exactly on 12 and 13 bytes -- 10 copies, so rows cross waves."""
    rows_codes = SHAPES * 10
    want = [decode_literal(SYMS, r) for r in rows_codes]
    entry = cached(("fsst-lit", lens_dtype), lambda: fsst_literal(SYMS, rows_codes, [len(w) for w in want], lens_dtype))
    rng = np.random.default_rng(6)
    idx = np.concatenate([np.arange(len(rows_codes)), rng.integers(0, len(rows_codes), 200)]).astype(np.int32)
    res = check(ctx, entry, idx, info=in_place("fsst"))
    views, heap = res.numpy()
    assert heap.tobytes() == b"".join(want[i] for i in idx)


def test_fsst_uncompressed_children(ctx):
    if "rows" not in _CACHE:
        _CACHE["rows"] = base_rows()
    rows = _CACHE["rows"][:3000]
    entry = cached(("fsst", "plain"), lambda: E.encode_fsst(rows, compress_children=False))
    assert entry[0].children[3].encoding == A.ENC["PRIMITIVE"] and entry[0].children[3].ptype == "i32"
    assert base("fsst")[0].children[3].encoding != A.ENC["PRIMITIVE"]  # the base tree's are compressed
    rng = np.random.default_rng(7)
    check(ctx, entry, rng.integers(0, len(rows), 1500).astype(np.int64), info=in_place("fsst"))


# row 1 of each: a code >= n_symbols / an escape with no byte after it / a decode that does not match
# uncompressed_lengths (too short, too long); every other row is well formed
GOOD = dict(codes=[[2, 3], [2, 2], [255, ord("z")], [], [0, 1]], ulens=[3, 2, 1, 0, 16])
MALFORMED = {"code past the table": ([2, 7], 2), "dangling escape": ([2, 255], 2), "decodes short": ([2, 2], 3),
             "decodes long": ([0, 0], 2)}


@pytest.mark.parametrize("what", list(MALFORMED))
def test_fsst_malformed_rows(ctx, what):
    codes, ulen = MALFORMED[what]
    rows_codes = [list(r) for r in GOOD["codes"]]
    ulens = list(GOOD["ulens"])
    rows_codes[1], ulens[1] = codes, ulen
    bad = fsst_literal(SYMS, rows_codes, ulens).to(_dev())
    for idx in ([1], [0, 1, 2], [4, 4, 1]):
        with pytest.raises(V.VortexGpuError) as ei:
            A.take(bad, np.array(idx, np.int32), ctx)
        assert ei.value.kind == "InvalidArgument", (what, idx)
    # the good rows of the same tree are right and raise nothing (a malformed row that is not taken
    # is not looked at): checked against the well-formed twin's oracle canonical
    twin = fsst_literal(SYMS, GOOD["codes"], GOOD["ulens"])
    check(ctx, (twin, bad, canon(twin)), np.array([0, 2, 3, 4, 0, 4], np.int32), info=in_place("fsst"))


def test_fsst_code_offsets_out_of_range(ctx):
    tree = fsst_literal(SYMS, GOOD["codes"], GOOD["ulens"])
    vb = tree.children[2]
    offs = np.asarray(vb.children[0].buffers[0]).view(np.int32).copy()
    offs[-1] += 5  # the last row's codes end past the code bytes
    broken = dataclasses.replace(tree, children=[tree.children[0], tree.children[1], dataclasses.replace(
        vb, children=[A.primitive(offs)] + list(vb.children[1:])), tree.children[3]]).to(_dev())
    with pytest.raises(V.VortexGpuError) as ei:
        A.take(broken, np.array([4], np.int32), ctx)
    assert ei.value.kind == "InvalidArgument"
    check(ctx, (tree, broken, canon(tree)), np.array([0, 1, 2, 3], np.int32), info=in_place("fsst"))


# ---- 6. forced fallback ----------------------------------------------------------------------------
def test_forced_fallback_gives_the_same_bytes(ctx):
    """Every tree of the cases above through VXG_TAKE_CANONICALIZE: the new kernels against the
    existing decoders on the device, as well as against the oracle."""
    test_varbin_offsets(ctx), test_dict_codes(ctx), test_fsst_uncompressed_children(ctx)  # (fills the cache)
    for dt in (np.int32, np.uint16, np.int64):
        test_fsst_literals(ctx, dt)
    for kind in KINDS:
        base(kind)
    rng = np.random.default_rng(8)
    for key, entry in list(_CACHE.items()):
        if key == "rows":
            continue
        n = entry[0].len
        idx = rng.integers(0, n, min(n, 2085)).astype(np.int32)
        want = A.take(entry[1], idx, ctx)
        got = check(ctx, entry, idx, force=True)
        assert got.numpy()[0].tobytes() == want.numpy()[0].tobytes()
        assert got.numpy()[1].tobytes() == want.numpy()[1].tobytes()


# ---- 7. chunked ------------------------------------------------------------------------------------
def test_chunked_strings_fall_back(ctx):
    if "rows" not in _CACHE:
        _CACHE["rows"] = base_rows()
    rows = _CACHE["rows"]
    idx = np.array([0, 1499, 1500, 1501, 2999, 1500, 1499, 7], np.int32)  # across the chunk boundary
    fs = cached(("chunked", "fsst"), lambda: A.chunked([E.encode_fsst(rows[:1500]), E.encode_fsst(rows[1500:3000])]))
    check(ctx, fs, idx, info=dict(fallback_arrays=1, direct_arrays=0, dict_arrays=0))
    dc = cached(("chunked", "dict"), lambda: A.chunked([E.encode_dict_strings_nullable(rows[:1500]),
                                                       E.encode_dict_strings_nullable(rows[1500:3000])]))
    check(ctx, dc, idx, info=dict(fallback_arrays=1, direct_arrays=0, dict_arrays=0))
    # a dictionary whose values are chunked
    vals = [b"v%03d" % i + b"-" * (i % 14) for i in range(9)]
    dv = cached(("dict", "chunked values"), lambda: A.dict_array(
        A.chunked([varbin_of(vals[:4]), varbin_of(vals[4:])]),
        E.encode_bitpacked((np.arange(300) % 9).astype(np.uint8), bit_width=4, allow_patches=False)))
    check(ctx, dv, np.array([8, 299, 0, 13], np.int32), info=dict(fallback_arrays=1, direct_arrays=0, dict_arrays=0))


# ---- 8. errors -------------------------------------------------------------------------------------
def raw_take(ctx, dev_tree, idx, flags=0, data_cap=None, table_cap=1, fn="vxg_take_array_ex"):
    """A direct C call -> (status name, VxgCanonical, keep-alive list); engine allocations are freed."""
    import torch
    keep: list = []
    node = A.flatten(dev_tree, keep)
    idx = np.ascontiguousarray(idx)
    it = torch.from_numpy(idx.view(np.uint8).copy()).to(_dev())
    out = L.VxgCanonical()
    table = (L.VxgDataBuffer * 1)()
    out.data_buffers, out.data_buffers_cap = table, table_cap
    if data_cap is not None:
        data = torch.zeros(max(data_cap, 1) + 16, dtype=torch.uint8, device=_dev())
        out.data, out.data_bytes = data.data_ptr(), data_cap
        keep.append(data)
    provided = out.data
    ip = A.PTYPE[A.PTYPE_OF_NP[idx.dtype]]
    if fn == "vxg_take_array_ex":
        st = ctx.lib.vxg_take_array_ex(ctx.handle, C.byref(node), ip, C.c_void_p(it.data_ptr()), idx.size, flags,
                                       C.byref(out), None, ctx.stream_ptr())
    else:
        st = ctx.lib.vxg_take_array(ctx.handle, C.byref(node), ip, C.c_void_p(it.data_ptr()), idx.size, C.byref(out),
                                    ctx.stream_ptr())
    result = dict(status=L.STATUS[st], heap=int(out.data_bytes), n_buffers=int(out.n_data_buffers),
                  table=(int(table[0].offset), int(table[0].len)))
    try:
        ctx.sync()
    except V.VortexGpuError as e:
        result["sync"] = e.kind
    for name in ("values", "validity", "views", "data"):
        p = getattr(out, name)
        if p and p != (provided if name == "data" else None):
            if st != 0:
                raise AssertionError(f"{name} handed back with status {L.STATUS[st]}")
            L.check(ctx.lib.vxg_free(ctx.handle, C.c_void_p(p)))
    return result


@pytest.mark.parametrize("kind", list(KINDS) + ["bool"])
def test_index_out_of_bounds(ctx, kind):
    if kind == "bool":
        tree = A.bool_array(np.arange(N) % 3 == 0, validity=np.arange(N) % 5 != 0).to(_dev())
    else:
        tree = base(kind)[1]
    for idx in (np.array([1, N, 2], np.int64), np.array([N], np.uint32), np.array([3, -1, 5], np.int8),
                np.concatenate([np.arange(5000), [N]]).astype(np.int32)):
        with pytest.raises(V.VortexGpuError) as ei:
            A.take(tree, idx, ctx)
        assert ei.value.kind == "OutOfBounds", (kind, idx[:3])
    # the context is usable afterwards
    if kind != "bool":
        check(ctx, base(kind), np.array([3, 2, 1], np.int32), info=in_place(kind))


def test_arguments(ctx):
    entry = base("fsst")
    idx = np.array([5, 0, 5, 4], np.int32)
    (_, wheap), _ = take_canon(entry[0], idx, entry[2])
    ok = raw_take(ctx, entry[1], idx)
    assert ok == dict(status="OK", heap=wheap.size, n_buffers=1, table=(0, wheap.size))
    for kind in KINDS:
        assert raw_take(ctx, base(kind)[1], idx, flags=2)["status"] == "InvalidArgument"
        assert raw_take(ctx, base(kind)[1], idx, flags=3)["status"] == "InvalidArgument"
        assert raw_take(ctx, base(kind)[1], idx, data_cap=wheap.size - 1)["status"] == "InvalidArgument"
        fit = raw_take(ctx, base(kind)[1], idx, data_cap=wheap.size)
        assert fit["status"] == "OK" and fit["heap"] == wheap.size
        none = raw_take(ctx, base(kind)[1], idx, table_cap=0)  # data_buffers_cap == 0: the table is not written
        assert none["status"] == "OK" and none["n_buffers"] == 1 and none["table"] == (0, 0)
    assert raw_take(ctx, A.primitive(np.arange(10, dtype=np.int32)).to(_dev()), idx, flags=4)["status"] == "InvalidArgument"


# ---- 9. bool ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [0, 31, 32, 33, 4097])
def test_bool(ctx, k):
    rng = np.random.default_rng(9)
    n = 5000
    m = rng.random(n) < 0.4
    runs = np.repeat(rng.random(n // 20) < 0.5, 20)
    trees = [A.bool_array(m, validity=rng.random(n) < 0.8), E.encode_runend_bool(runs), A.constant_bool(True, n)]
    idx = rng.integers(0, n, k).astype(np.int32)
    for tree in trees:
        want, wvalid = take_canon(tree, idx)
        for force in (False, True):
            res = A.take(tree.to(_dev()), idx, ctx, force_canonical=force)
            assert res.kind == "bool" and res.len == k
            bits = np.packbits(want, bitorder="little")
            assert res.values.cpu().numpy().tobytes() == bits.tobytes().ljust(((k + 31) // 32) * 4, b"\0")
            gvalid = res.validity_mask()
            assert (gvalid is None) == (wvalid is None)
            if wvalid is not None:
                assert gvalid.tolist() == wvalid.tolist()


# ---- 10. primitive ---------------------------------------------------------------------------------
def test_primitive_ex_matches_take_array(ctx):
    import torch
    rng = np.random.default_rng(10)
    n = 40_000
    v = rng.integers(0, 1 << 11, n).astype(np.uint32)
    trees = {"bitpacked": E.encode_bitpacked(v, bit_width=11, allow_patches=False, validity=rng.random(n) < 0.9),
             "dict": E.encode_dict((v % 300) * 7)}
    for name, tree in trees.items():
        dev_tree = tree.to(_dev())
        for k in (n // 16, n):
            idx = rng.integers(0, n, k).astype(np.uint32)
            want, wvalid = take_canon(tree, idx)
            outs = []
            for force in (False, True):
                res = A.take(dev_tree, idx, ctx, force_canonical=force)
                assert res.numpy().tobytes() == want.tobytes()
                assert (res.validity_mask() is None) == (wvalid is None)
                if wvalid is not None:
                    assert res.validity_mask().tolist() == wvalid.tolist()
                outs.append(res)
            info = outs[0].info
            if name == "bitpacked":
                assert info == (dict(packed_launches=1, dict_arrays=0, direct_arrays=0, fallback_arrays=0) if k * 8 <= n
                                else dict(packed_launches=0, dict_arrays=0, direct_arrays=0, fallback_arrays=1))
            else:
                assert info == dict(packed_launches=1 if k * 8 <= n else 0, dict_arrays=1, direct_arrays=0, fallback_arrays=0)
            assert outs[1].info == dict(packed_launches=0, dict_arrays=0, direct_arrays=0, fallback_arrays=1)
            # vxg_take_array is vxg_take_array_ex with flags 0: the same bytes through the old symbol
            keep: list = []
            node = A.flatten(dev_tree, keep)
            it = torch.from_numpy(idx.view(np.uint8).copy()).to(_dev())
            out = L.VxgCanonical()
            vals = torch.zeros(k * 4, dtype=torch.uint8, device=_dev())
            out.values = vals.data_ptr()
            vt = torch.zeros(((k + 31) // 32) * 4, dtype=torch.uint8, device=_dev())
            if tree.nullable:
                out.validity = vt.data_ptr()
            L.check(ctx.lib.vxg_take_array(ctx.handle, C.byref(node), A.PTYPE["u32"], C.c_void_p(it.data_ptr()), k,
                                           C.byref(out), ctx.stream_ptr()))
            ctx.sync()
            assert vals.cpu().numpy().tobytes() == outs[0].values.cpu().numpy().tobytes()
            if tree.nullable:
                assert vt.cpu().numpy()[: (k + 7) // 8].tobytes() == outs[0].validity.cpu().numpy().tobytes()
