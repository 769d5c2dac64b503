"""GPU: vxg_row_filter against row_filter_expected (the AND of the oracle's one-sided compares),
byte for byte.

Every call writes into a bitmap of the exact size + 64 guard bytes of 0xFF and a count of 8 bytes +
64 guard bytes: the tail bits past len must be zero and the guards untouched.  Wherever a test
asserts counters it forces the pairing flag, so it holds whatever the engine's default is."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import vortex_amd as V
import vortex_amd._lib as L
import vortex_amd.arrays as A
import vortex_amd.encode as E
from oracle_tree import canon, slice_bitpacked
from row_filter_expected import expected

pytestmark = pytest.mark.gpu

GUARD = 64
FUSE, NO_FUSE = L.ROWF_FUSE_RANGES, L.ROWF_NO_FUSE_RANGES
PAIRS = [(">", "<"), (">", "<="), (">=", "<"), (">=", "<=")]


def _dev():
    import torch
    return torch.device("cuda", 0)


def run(ctx, preds, flags=0, count=True):
    """The filter on the GPU into guarded buffers -> (Canonical, bitmap bytes).  A tree OBJECT that
    occurs in several conjuncts is moved to the device once, so they share one node."""
    import torch
    n = preds[0][0].len
    nb = ((n + 63) // 64) * 8
    vals = torch.full((nb + GUARD,), 0xFF, dtype=torch.uint8, device=_dev())
    cnt = torch.full((8 + GUARD,), 0xFF, dtype=torch.uint8, device=_dev())
    on_dev = {}
    for t, _, _ in preds:
        if id(t) not in on_dev:
            on_dev[id(t)] = t.to(_dev())
    res = V.row_filter([(on_dev[id(t)], op, s) for t, op, s in preds], ctx, flags=flags, out_values=vals,
                       count=cnt if count else False)
    hv, hc = vals.cpu().numpy(), cnt.cpu().numpy()
    assert (hv[nb:] == 0xFF).all(), "bitmap guard bytes written"
    assert (hc[8:] == 0xFF).all(), "count guard bytes written"
    if not count:
        assert (hc == 0xFF).all() and res.true_count is None
    assert res.kind == "bool" and res.len == n and res.validity is None
    assert res.info["predicates"] == len(preds)
    assert res.info["compare_passes"] == len(preds) - res.info["range_pairs"]
    return res, hv[:nb].tobytes()


def check(ctx, preds, flags=0, count=True):
    want, mask, want_count = expected(preds)
    res, got = run(ctx, preds, flags, count)
    assert got == want, (flags, [(op, s) for _, op, s in preds], preds[0][0].len, np.flatnonzero(
        np.frombuffer(got, np.uint8) != np.frombuffer(want, np.uint8))[:8])
    if count:
        assert res.true_count == want_count
    return res, mask


def check_range(ctx, tree, lo_op, lo, hi_op, hi, fallback=0):
    """One range, paired and unpaired: identical bytes, and the counters say which ran."""
    preds = [(tree, lo_op, lo), (tree, hi_op, hi)]
    res, mask = check(ctx, preds, FUSE)
    assert res.info["range_pairs"] == 1 and res.info["compare_passes"] == 1, res.info
    if fallback is not None:
        assert res.info["range_launches"] >= 1 and res.info["fallback_arrays"] == fallback, res.info
    res2, _ = check(ctx, preds, NO_FUSE)
    assert res2.info["range_pairs"] == 0 and res2.info["compare_passes"] == 2 and res2.info["range_launches"] == 0
    assert res2.info["combine_launches"] == (1 if tree.len else 0)
    return res, mask


def packed_tree(T: int, W: int, n: int, offset: int, rng) -> A.Array:
    """A BitPacked u<T> array of n values of W bits at slice offset `offset`."""
    dt = np.dtype(f"u{T // 8}")
    hi = (1 << W) - 1
    full = rng.integers(0, hi + 1, n + offset, dtype=np.uint64, endpoint=False).astype(dt)
    if full.size:
        full[rng.integers(0, full.size, 3)] = hi  # the width's extremes are present
        full[rng.integers(0, full.size, 3)] = 0
    if W == T:
        a = A.bitpacked(E.bitpack_buffer(full, T), f"u{T}", T, n + offset)
    else:
        a = E.encode_bitpacked(full, bit_width=W, allow_patches=False)
    return slice_bitpacked(a, offset, offset + n) if offset else a


LENS = [0, 1, 63, 64, 65, 1023, 1024, 1025, 2085, 3073]
OFFSETS = [0, 1, 63, 1000]


@pytest.mark.parametrize("T,W", [(32, 1), (32, 7), (32, 32), (8, 5), (16, 11), (64, 37)])
def test_range_geometry(ctx, T, W):
    rng = np.random.default_rng(1000 + 64 * T + W)
    for n in LENS:
        for off in OFFSETS:
            tree = packed_tree(T, W, n, off, rng)
            assert tree.meta["offset"] == off and tree.len == n
            vals = np.sort(canon(tree)[0])
            lo, hi = (int(vals[n // 4]), int(vals[(3 * n) // 4])) if n else (0, 0)
            for lo_op, hi_op in PAIRS:
                check_range(ctx, tree, lo_op, lo, hi_op, hi)


@pytest.mark.parametrize("dt", [np.int32, np.int64])
def test_range_for_bounds_at_the_extremes(ctx, dt):
    rng = np.random.default_rng(11)
    info = np.iinfo(dt)
    vals = (rng.integers(0, 3000, 1300) - 2990).astype(dt)  # a negative reference
    tree = E.encode_for_bitpacked(vals, allow_patches=False)
    assert tree.encoding == V.ENC["FL_FOR"] and tree.children[0].encoding == V.ENC["FL_BITPACKED"]
    lo, hi = int(vals.min()), int(vals.max())
    for lo_op, hi_op in PAIRS:
        _, m = check_range(ctx, tree, lo_op, info.min, hi_op, info.max)
        assert m.all()
        check_range(ctx, tree, lo_op, lo, hi_op, hi)
        check_range(ctx, tree, lo_op, info.min, hi_op, -100)
        check_range(ctx, tree, lo_op, -100, hi_op, info.max)
        _, m = check_range(ctx, tree, lo_op, info.max, hi_op, info.min)
        assert not m.any()
    # unsigned: a wrapped reference near the top of the type, bounds across the wrap
    T = 8 * np.dtype(dt).itemsize
    child = E.encode_bitpacked(rng.integers(0, 100, 1100, dtype=np.uint64).astype(f"u{T // 8}"), bit_width=7,
                               allow_patches=False)
    utree = A.frame_of_reference(child, (1 << T) - 40, 0, f"u{T}")
    for lo_op, hi_op in PAIRS:
        check_range(ctx, utree, lo_op, 0, hi_op, (1 << T) - 1)
        check_range(ctx, utree, lo_op, 30, hi_op, (1 << T) - 20)


def test_range_zigzag(ctx):
    rng = np.random.default_rng(12)
    vals = rng.integers(-500, 500, 1400).astype(np.int32)
    tree = E.encode_zigzag(vals)
    for lo_op, hi_op in PAIRS:
        check_range(ctx, tree, lo_op, -250, hi_op, 250)
        check_range(ctx, tree, lo_op, int(vals.min()), hi_op, int(vals.max()))


def _alp_values(dt, rng, n=3000):
    vals = (np.round(rng.uniform(1, 1000, n) * 100) / 100).astype(dt)
    vals[::211] = dt(65536.5)                      # encodable, far above the rest: BitPacked patches
    vals[::97] = (rng.standard_normal(vals[::97].size) * 1e9 + 0.123456789).astype(dt)  # ALP exceptions
    vals[5], vals[6], vals[7] = np.nan, 0.0, -0.0
    return vals


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_range_alp_with_patches_nan_and_zeros(ctx, dt):
    vals = _alp_values(dt, np.random.default_rng(13))
    tree = E.encode_alp(vals)
    bp = tree.children[0].children[0]
    assert tree.meta["has_patches"] and bp.encoding == V.ENC["FL_BITPACKED"] and bp.meta["has_patches"]
    for lo_op, hi_op in PAIRS:
        res, _ = check_range(ctx, tree, lo_op, 250.0, hi_op, 750.0)
        check_range(ctx, tree, lo_op, float(vals[3]), hi_op, 1e8)      # exceptions and patches inside
        _, m = check_range(ctx, tree, lo_op, float("nan"), hi_op, 750.0)
        assert not m.any()
        _, m = check_range(ctx, tree, lo_op, 250.0, hi_op, float("nan"))
        assert not m.any()
        _, m = check_range(ctx, tree, lo_op, -0.0, hi_op, 0.0)
        assert m.sum() == (2 if (lo_op, hi_op) == (">=", "<=") else 0)  # -0.0 == +0.0


def test_range_nullable_column(ctx):
    rng = np.random.default_rng(14)
    n = 1500
    vals = rng.integers(0, 128, n, dtype=np.uint32)
    valid = rng.random(n) < 0.7
    packed = E.bitpack_buffer(vals, 7)
    for tree in (A.bitpacked(packed, "u32", 7, n, validity=A.bool_array(valid, bit_offset=3)),
                 A.frame_of_reference(A.bitpacked(packed, "u32", 7, n, validity=valid), 1000, 0, "u32")):
        ref = 1000 if tree.encoding == V.ENC["FL_FOR"] else 0
        _, m = check_range(ctx, tree, ">=", ref + 32, "<", ref + 96)
        assert not m[~valid].any() and m[valid].any()
    _, m = check_range(ctx, A.bitpacked(packed, "u32", 7, n, validity="ALL_INVALID"), ">=", 0, "<=", 127)
    assert not m.any()


def _for_chunk(vals):
    if vals.size == 0:  # FoR(BitPacked) of no rows, by hand (for_compress needs a row)
        return A.frame_of_reference(A.bitpacked(np.zeros(0, np.uint8), "u32", 5, 0), -50, 0, "i32")
    return A.frame_of_reference(E.encode_bitpacked((vals + 50).astype(np.uint32), bit_width=8, allow_patches=False),
                                -50, 0, "i32")


def test_range_chunked(ctx):
    """Chunks that begin mid-word, an empty one and word-aligned ones; one fused launch."""
    rng = np.random.default_rng(15)
    chunks = [_for_chunk((rng.integers(0, 200, n) - 50).astype(np.int32)) for n in (1000, 24, 0, 1025, 64)]
    tree = A.chunked(chunks)
    for lo_op, hi_op in PAIRS:
        res, _ = check_range(ctx, tree, lo_op, 0, hi_op, 100)
        assert res.info["range_launches"] == 1 and res.info["fused_launches"] == 1


def test_range_chunked_fused_and_fallback_in_one_call(ctx):
    rng = np.random.default_rng(16)
    v = [(rng.integers(0, 200, n) - 50).astype(np.int32) for n in (1100, 77, 900)]
    tree = A.chunked([_for_chunk(v[0]), A.primitive(v[1]), E.encode_dict(v[2])])
    for lo_op, hi_op in PAIRS:
        res, _ = check_range(ctx, tree, lo_op, -10, hi_op, 90, fallback=2)
        assert res.info["range_launches"] == 1
    # a column with no packed chunk at all: the pair still runs as one pass, through the plain twin
    res, _ = check_range(ctx, E.encode_dict(v[2]), ">", -10, "<=", 90, fallback=None)
    assert res.info["range_launches"] == 0 and res.info["fallback_arrays"] == 1


def test_lower_bound_above_upper_bound(ctx):
    tree = E.encode_bitpacked(np.arange(2085, dtype=np.uint32) % 128, bit_width=7, allow_patches=False)
    for lo_op, hi_op in PAIRS:
        res, m = check_range(ctx, tree, lo_op, 90, hi_op, 30)
        assert not m.any() and res.true_count == 0


def test_pairing_rule(ctx):
    rng = np.random.default_rng(17)
    tree = E.encode_bitpacked(rng.integers(0, 128, 1500, dtype=np.uint32), bit_width=7, allow_patches=False)
    preds = [(tree, ">=", 20), (tree, ">=", 40), (tree, "<", 100)]
    res, m = check(ctx, preds, FUSE)
    assert res.info["range_pairs"] == 1 and res.info["compare_passes"] == 2 and res.info["combine_launches"] == 1
    assert m.any()
    res, _ = check(ctx, preds, NO_FUSE)
    assert res.info["range_pairs"] == 0 and res.info["compare_passes"] == 3
    # ==, != and strings never pair; two ranges on one node pair in list order
    preds = [(tree, "<=", 110), (tree, "!=", 50), (tree, ">", 10), (tree, "<", 100), (tree, "==", 60), (tree, ">=", 30)]
    res, _ = check(ctx, preds, FUSE)
    assert res.info["range_pairs"] == 2 and res.info["compare_passes"] == 4
    # the same data flattened twice is two nodes: nothing to pair, whatever the flag
    copy = dataclasses.replace(tree)
    res, _ = check(ctx, [(tree, ">=", 20), (copy, "<", 100)], FUSE)
    assert res.info["range_pairs"] == 0 and res.info["compare_passes"] == 2 and res.info["range_launches"] == 0


def test_flags_give_identical_bytes(ctx):
    rng = np.random.default_rng(18)
    tree = E.encode_for_bitpacked((rng.integers(0, 5000, 3073) - 100).astype(np.int64), allow_patches=False)
    preds = [(tree, ">", 700), (tree, "<=", 3100), (tree, "!=", 1000)]
    got = [run(ctx, preds, f)[1] for f in (0, FUSE, NO_FUSE)]
    assert got[0] == got[1] == got[2] == expected(preds)[0]


def test_q6_conjunction_then_filter(ctx):
    """A Q6-shaped filter: two ranges, a packed <, a Dict-of-strings == and an FSST >=; then the
    mask selects the rows of a sixth column."""
    rng = np.random.default_rng(19)
    n = 3073
    date = (rng.integers(0, 2500, n) + 8000).astype(np.int32)
    date_valid = rng.random(n) < 0.9
    date_t = A.frame_of_reference(
        A.bitpacked(E.bitpack_buffer((date - 8000).astype(np.uint32), 12), "u32", 12, n, validity=date_valid), 8000, 0, "i32")
    disc = np.round(rng.uniform(0.0, 0.1, n) * 100) / 100
    disc_t = E.encode_alp(disc)
    qty = rng.integers(1, 51, n, dtype=np.uint32)
    qty_t = E.encode_bitpacked(qty, bit_width=6, allow_patches=False)
    flags_rows = [None if rng.random() < 0.1 else bytes([b"ANR"[int(rng.integers(0, 3))]]) for _ in range(n)]
    flag_t = E.encode_dict_strings_nullable(flags_rows)
    modes = [b"AIR", b"MAIL", b"RAIL", b"SHIP", b"TRUCK", b"REG AIR", b"FOB"]
    mode_rows = [modes[int(i)] for i in rng.integers(0, len(modes), n)]
    mode_t = E.encode_fsst(mode_rows)
    assert date_t.nullable and flag_t.nullable
    assert disc_t.encoding == V.ENC["ALP"] and flag_t.encoding == V.ENC["DICT"] and mode_t.encoding == V.ENC["FSST"]
    preds = [(date_t, ">=", 8400), (date_t, "<", 9800), (disc_t, ">=", 0.02), (disc_t, "<=", 0.08), (qty_t, "<", 40),
             (flag_t, "==", b"N"), (mode_t, ">=", b"MAIL")]
    keep = (date >= 8400) & (date < 9800) & date_valid & (disc >= 0.02) & (disc <= 0.08) & (qty < 40) & \
        np.array([r == b"N" for r in flags_rows]) & np.array([r >= b"MAIL" for r in mode_rows])
    res, mask = check(ctx, preds, FUSE)
    assert (mask == keep).all() and 0 < keep.sum() < n
    assert res.info["range_pairs"] == 2 and res.info["compare_passes"] == 5 and res.info["range_launches"] == 2
    assert res.info["combine_launches"] == 1
    res2, _ = check(ctx, preds, NO_FUSE)
    assert res2.info["compare_passes"] == 7 and res2.info["range_launches"] == 0

    price = rng.uniform(900, 105000, n)
    got = A.filter(A.primitive(price).to(_dev()), V.predicate_from(res), ctx)
    assert got.len == res.true_count == int(keep.sum())
    assert (got.numpy() == price[keep]).all()


@pytest.mark.parametrize("k", [1, 2, 16, 17, 33])
def test_combine_boundaries(ctx, k):
    """k single conjuncts: one AND launch per 16 bitmaps (15 after the first), and the count is
    taken once -- counting in an earlier launch would count rows a later bitmap clears."""
    launches = {1: 1, 2: 1, 16: 1, 17: 2, 33: 3}[k]
    for n in (1, 64, 65, 4097):
        rng = np.random.default_rng(2000 + 10 * k + n % 7)
        hi = 3 if k <= 2 else 40  # many conjuncts: each clears few rows, so rows survive the AND
        cols = [A.primitive(rng.integers(0, hi, n, dtype=np.uint8)) for _ in range(k)]
        preds = [(c, "!=", i % hi) for i, c in enumerate(cols)]
        res, mask = check(ctx, preds, FUSE)
        assert res.info["combine_launches"] == launches and res.info["compare_passes"] == k
        assert res.info["fallback_arrays"] == k
        if n == 4097:
            assert 0 < mask.sum() < n
        res, _ = check(ctx, preds, 0, count=False)
        assert res.info["combine_launches"] == (launches if k > 1 else 0)


def test_single_range_without_count_writes_straight_out(ctx):
    tree = E.encode_bitpacked(np.arange(1025, dtype=np.uint32) % 128, bit_width=7, allow_patches=False)
    res, _ = check(ctx, [(tree, ">=", 10), (tree, "<", 90)], FUSE, count=False)
    assert res.info["compare_passes"] == 1 and res.info["combine_launches"] == 0
    res, _ = check(ctx, [(tree, ">=", 10), (tree, "<", 90)], FUSE, count=True)
    assert res.info["combine_launches"] == 1  # in place over the one bitmap, for the count


# ---- the C entry point: engine allocation and arguments -----------------------------------
def _pred_array(nodes_ops_scalars):
    keep = []
    arr = (L.VxgPredicate * max(len(nodes_ops_scalars), 1))()
    for i, (node, op, scalar) in enumerate(nodes_ops_scalars):
        arr[i].column = C.pointer(node) if node is not None else None
        arr[i].op = op
        if scalar is not None:
            buf = (C.c_uint8 * 8).from_buffer_copy(scalar)
            keep.append(buf)
            arr[i].scalar_host = C.cast(buf, C.c_void_p)
    return arr, keep


def test_engine_allocates_the_bitmap(ctx):
    rng = np.random.default_rng(20)
    n = 2085
    tree = E.encode_bitpacked(rng.integers(0, 128, n, dtype=np.uint32), bit_width=7, allow_patches=False)
    keep = []
    node = A.flatten(tree.to(_dev()), keep)
    arr, k2 = _pred_array([(node, L.CMP_OP[">="], np.uint32(30).tobytes().ljust(8, b"\0")),
                           (node, L.CMP_OP["<"], np.uint32(90).tobytes().ljust(8, b"\0"))])
    out = L.VxgCanonical()
    info = L.VxgRowFilterInfo()
    L.check(ctx.lib.vxg_row_filter(ctx.handle, arr, 2, FUSE, C.byref(out), None, C.byref(info), ctx.stream_ptr()))
    nb = ((n + 63) // 64) * 8
    assert out.values and not out.validity and out.kind == V.ENC["BOOL"] and out.len == n and out.values_bytes == nb
    host = np.zeros(nb, np.uint8)
    L.check(ctx.lib.vxg_memcpy_d2h(ctx.handle, host.ctypes.data_as(C.c_void_p), C.c_void_p(out.values), nb,
                                   ctx.stream_ptr()))
    ctx.sync()
    assert host.tobytes() == expected([(tree, ">=", 30), (tree, "<", 90)])[0]
    assert info.range_pairs == 1 and info.combine_launches == 0
    L.check(ctx.lib.vxg_free(ctx.handle, C.c_void_p(out.values)))


def test_arguments(ctx):
    import torch
    keep = []
    flat = lambda t: A.flatten(t.to(_dev()), keep)  # noqa: E731
    ok = flat(E.encode_bitpacked(np.arange(100, dtype=np.uint32), bit_width=7, allow_patches=False))
    longer = flat(A.primitive(np.arange(101, dtype=np.uint32)))
    boolean = flat(A.bool_array(np.ones(100, bool)))
    half = flat(A.primitive(np.ones(100, np.float16)))
    string = flat(E.encode_varbinview([b"a"] * 100))
    null_dtype = flat(A.primitive(np.arange(100, dtype=np.uint32)))
    null_dtype.dtype = L.DTYPE["NULL"]
    sc = bytes(8)
    LT, GT = L.CMP_OP["<"], L.CMP_OP[">"]
    vals = torch.full((16 + GUARD,), 0xFF, dtype=torch.uint8, device=_dev())
    cnt = torch.full((16 + GUARD,), 0xFF, dtype=torch.uint8, device=_dev())

    def status(preds, n_preds=None, flags=0, null_preds=False, null_out=False, values=True, count_off=0, reserved=0):
        arr, k = _pred_array(preds)
        if reserved:
            arr[0].reserved = reserved
        out = L.VxgCanonical()
        if values:
            out.values = vals.data_ptr()
        st = ctx.lib.vxg_row_filter(ctx.handle, None if null_preds else arr, len(preds) if n_preds is None else n_preds,
                                    flags, None if null_out else C.byref(out), C.c_void_p(cnt.data_ptr() + count_off),
                                    None, ctx.stream_ptr())
        ctx.sync()
        assert st != 0
        assert out.values == (vals.data_ptr() if values else None) and not out.validity, "an engine pointer came back"
        assert (vals.cpu().numpy() == 0xFF).all() and (cnt.cpu().numpy() == 0xFF).all(), "an output was written"
        return L.STATUS[st]

    good = (ok, LT, sc)
    for values in (True, False):
        assert status([], values=values) == "InvalidArgument"                       # n_preds == 0
        assert status([good], null_preds=True, values=values) == "InvalidArgument"
        assert status([good, (None, LT, sc)], values=values) == "InvalidArgument"   # a null column
        assert status([good, (ok, GT, None)], values=values) == "InvalidArgument"   # a null primitive scalar
        assert status([good], reserved=1, values=values) == "InvalidArgument"
        assert status([good, (longer, LT, sc)], values=values) == "InvalidArgument"
        assert "different lengths" in ctx.lib.vxg_last_error().decode()
        assert status([good, (ok, 6, sc)], values=values) == "InvalidArgument"
        assert status([(ok, -1, sc)], values=values) == "InvalidArgument"
        assert status([good], flags=4, values=values) == "InvalidArgument"
        assert status([good], flags=FUSE | NO_FUSE, values=values) == "InvalidArgument"
        assert status([good], count_off=4, values=values) == "InvalidArgument"      # a misaligned count
        assert status([good, (boolean, LT, sc)], values=values) == "NotImplemented"
        assert status([good, (half, LT, sc)], values=values) == "NotImplemented"
        assert status([good, (null_dtype, LT, sc)], values=values) == "MismatchedTypes"
    assert status([good], null_out=True) == "InvalidArgument"
    # a string conjunct of the same length is fine, and so is the call after all those errors
    arr, k = _pred_array([good, (string, L.CMP_OP["=="], b"a".ljust(8, b"\0"))])
    arr[1].scalar_len = 1
    out = L.VxgCanonical()
    out.values = vals.data_ptr()
    L.check(ctx.lib.vxg_row_filter(ctx.handle, arr, 2, 0, C.byref(out), C.c_void_p(cnt.data_ptr()), None, ctx.stream_ptr()))
    ctx.sync()
    assert int(cnt[:8].cpu().numpy().view(np.uint64)[0]) == 0  # no value of 0..99 is < 0
    with pytest.raises(V.VortexGpuError, match="unknown operator"):
        V.row_filter([(E.encode_varbinview([b"a"]).to(_dev()), "~", b"a")], ctx)
