"""GPU: vxg_filter_batch against oracle_tree.filter_canon, byte for byte.

Every call goes through the C ABI with caller-provided outputs sized exactly for the k selected rows
plus 64 guard bytes of 0xFF: the guards must come back untouched, k must be the mask's popcount and
each out must equal what filter(column, mask) gives.  The counters of vxg_filter_batch_info say
which route ran."""
import ctypes as C

import numpy as np
import pytest

import vortex_amd as V
import vortex_amd._lib as L
import vortex_amd.arrays as A
import vortex_amd.encode as E
from filter_batch_run import _guarded, mask_tensor, run  # the call and its comparison with filter_canon
from oracle_tree import bad_bitpacked, filter_canon, slice_bitpacked

pytestmark = pytest.mark.gpu

CANON = L.FILTB_CANONICALIZE


def _dev():
    import torch
    return torch.device("cuda", 0)


def masks_for(n: int, rng):
    """The masks of the geometry cases."""
    first, last = np.zeros(n, bool), np.zeros(n, bool)
    first[:1] = True
    last[n - 1:] = True
    hole = np.ones(n, bool)  # one whole 1024-row block empty between two full ones
    hole[1024:2048] = False
    words = (np.arange(n) // 64) % 2 == 0  # every other 64-bit word
    return {"zero": np.zeros(n, bool), "one": np.ones(n, bool), "first": first, "last": last,
            "half": rng.random(n) < 0.5, "sparse": rng.random(n) < 0.02, "hole": hole, "words": words}


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


LENS = [0, 1, 63, 64, 65, 1023, 1024, 1025, 2085, 4095, 4096, 4097, 8200]
OFFSETS = [0, 1, 63, 1000]


@pytest.mark.parametrize("T,W", [(32, 0), (32, 1), (32, 7), (32, 32), (8, 5), (16, 11), (64, 37)])
def test_geometry(ctx, T, W):
    """Every length x slice offset x mask; the four offsets of one length are one batch."""
    rng = np.random.default_rng(3000 + 64 * T + W)
    for n in LENS:
        trees = [packed_tree(T, W, n, off, rng) for off in OFFSETS]
        for t, off in zip(trees, OFFSETS):
            assert t.meta["offset"] == off and t.len == n
        for name, mask in masks_for(n, rng).items():
            info = run(ctx, trees, mask)
            assert info["fallback_arrays"] == 0 and info["inplace_arrays"] == 0, (n, name, info)
            assert info["syncs"] == (1 if n else 0), (n, name, info)
            if mask.any():
                assert info["packed_launches"] >= 1 and info["packed_chunks"] == len(trees), (n, name, info)
            else:  # k == 0: nothing is launched after the count
                assert info["packed_launches"] == 0, (n, name, info)


def _rand_mask(n, rng, p=0.4):
    return rng.random(n) < p


def packed_only(ctx, tree, mask, patch_launches=None):
    info = run(ctx, [tree], mask)
    assert info["packed_launches"] >= 1 and info["fallback_arrays"] == 0 and info["mask_scans"] == 1, info
    if patch_launches is not None:
        assert info["patch_launches"] == patch_launches, info
    return info


def test_epilogues(ctx):
    rng = np.random.default_rng(31)
    n = 2085
    mask = _rand_mask(n, rng)
    for dt in (np.int32, np.int64):  # FoR with a negative reference
        vals = (rng.integers(0, 3000, n) - 2993).astype(dt)
        tree = E.encode_for_bitpacked(vals, allow_patches=False)
        assert tree.encoding == V.ENC["FL_FOR"] and tree.children[0].encoding == V.ENC["FL_BITPACKED"]
        assert np.array([tree.meta["reference"]], np.uint64).astype(f"u{vals.itemsize}").view(dt)[0] < 0
        packed_only(ctx, tree, mask)
    for T in (8, 64):  # unsigned FoR whose add wraps at the top of the type
        enc = rng.integers(0, 100, n, dtype=np.uint64).astype(f"u{T // 8}")
        tree = A.frame_of_reference(E.encode_bitpacked(enc, bit_width=7, allow_patches=False), (1 << T) - 40, 0, f"u{T}")
        packed_only(ctx, tree, mask)
    shifted = E.encode_for_bitpacked(np.arange(0, n * 8, 8, dtype=np.int32) - 4000, allow_patches=False)
    assert shifted.meta["shift"] == 3
    packed_only(ctx, shifted, mask)
    for dt in (np.int16, np.int32):  # ZigZag
        packed_only(ctx, E.encode_zigzag(rng.integers(-500, 500, n).astype(dt)), mask)
    zz = E.zigzag_encode(rng.integers(-500, 500, n).astype(np.int16))  # ZigZag over FoR(BitPacked)
    child = E.encode_bitpacked((zz - zz.min()).astype(np.uint16), allow_patches=False)
    packed_only(ctx, A.zigzag(A.frame_of_reference(child, int(zz.min()), 0, "u16")), mask)
    for dt in (np.float32, np.float64):  # ALP over FoR(BitPacked) (test_patches has the exceptions)
        tree = E.encode_alp(np.round(rng.uniform(1, 1000, n), 1).astype(dt))
        assert tree.children[0].encoding == V.ENC["FL_FOR"]
        assert tree.children[0].children[0].encoding == V.ENC["FL_BITPACKED"]
        packed_only(ctx, tree, mask)


def test_patches(ctx):
    rng = np.random.default_rng(32)
    n = 2500
    vals = rng.integers(0, 128, n, dtype=np.uint32)
    rows = np.array([0, 63, 64, 1023, 1024, 2499])  # row 0 and the last row among them
    vals[rows] = 1024 + np.arange(rows.size, dtype=np.uint32) * 128 + 5
    tree = E.encode_bitpacked(vals, bit_width=7)
    assert tree.meta["has_patches"]
    on = np.zeros(n, bool)
    on[rows] = True
    half = _rand_mask(n, rng, 0.5)
    for mask in (on, ~on, half, half | on, half & ~on, np.ones(n, bool)):  # patches on selected and unselected rows
        packed_only(ctx, tree, mask, patch_launches=1)
    # FoR over patched BitPacked: the patch values go through the epilogue
    f = E.encode_for_bitpacked(vals.astype(np.int64) - 300, allow_patches=True)
    assert f.children[0].meta["has_patches"]
    packed_only(ctx, f, half | on, patch_launches=1)
    # a slice at offset 1000 that keeps patches: its first and last rows are patched
    big = rng.integers(0, 128, 4000, dtype=np.uint32)
    big[[1000, 1500, 2047, 2048, 3499]] = 70_000
    sl = slice_bitpacked(E.encode_bitpacked(big, bit_width=7), 1000, 3500)
    assert sl.meta["offset"] == 1000 and sl.meta["has_patches"] and sl.len == 2500
    for mask in (half, half | on, np.ones(2500, bool)):
        packed_only(ctx, sl, mask, patch_launches=1)
    # ALP with exceptions: BitPacked's patches first, then ALP's values as they are
    for dt in (np.float32, np.float64):
        fv = (np.round(rng.uniform(1, 1000, n) * 100) / 100).astype(dt)
        fv[::97] = (rng.standard_normal(fv[::97].size) * 1e9 + 0.123456789).astype(dt)
        fv[0], fv[n - 1], fv[5] = np.pi, np.e, np.nan
        a = E.encode_alp(fv)
        assert a.meta["has_patches"]
        for mask in (half, ~half, np.ones(n, bool)):
            info = packed_only(ctx, a, mask)
            assert info["patch_launches"] >= 1, info


CHUNK_LENS = [1000, 0, 1, 2085, 64, 5000]


def _for_chunks(rng, lens):
    return [E.encode_for_bitpacked((rng.integers(0, 500, m) - 250 + 10 * i).astype(np.int32), allow_patches=False)
            if m else A.frame_of_reference(E.encode_bitpacked(np.zeros(0, np.uint32), bit_width=3, allow_patches=False),
                                           0, 0, "i32")
            for i, m in enumerate(lens)]


def test_chunked(ctx):
    rng = np.random.default_rng(33)
    chunks = _for_chunks(rng, CHUNK_LENS)
    n = sum(CHUNK_LENS)
    col = A.chunked(chunks)
    for name, mask in masks_for(n, rng).items():
        info = run(ctx, [col], mask)
        if mask.any():
            assert info["packed_launches"] == 1 and info["packed_chunks"] == 5 and info["fallback_arrays"] == 0, (name, info)
    # one Dict chunk: the whole column falls back, the bytes stay
    mixed = list(chunks)
    mixed[3] = E.encode_dict((rng.integers(0, 50, CHUNK_LENS[3]) * 3).astype(np.int32))
    for mask in (_rand_mask(n, rng), np.ones(n, bool)):
        info = run(ctx, [A.chunked(mixed)], mask)
        assert info["fallback_arrays"] == 1 and info["packed_launches"] == 0, info
    # BitPacked and FoR(BitPacked) chunks in one column: one launch per epilogue
    two = [E.encode_bitpacked(rng.integers(0, 99, 700, dtype=np.uint32), bit_width=7, allow_patches=False),
           E.encode_for_bitpacked(rng.integers(1000, 1099, 900, dtype=np.uint32), allow_patches=False)] * 2
    info = run(ctx, [A.chunked(two)], _rand_mask(3200, rng))
    assert info["packed_launches"] == 2 and info["packed_chunks"] == 4, info


def test_more_chunks_than_one_table(ctx):
    """kCmpArgChunks = 100 chunks ride in one kernel argument: 130 chunks take two launches."""
    rng = np.random.default_rng(34)
    lens = [int(x) for x in rng.integers(1, 200, 130)]
    col = A.chunked([E.encode_bitpacked(rng.integers(0, 31, m, dtype=np.uint16), bit_width=5, allow_patches=False)
                     for m in lens])
    info = run(ctx, [col], _rand_mask(sum(lens), rng))
    assert info["packed_launches"] == 2 and info["packed_chunks"] == 130 and info["fallback_arrays"] == 0, info


def test_in_place(ctx):
    rng = np.random.default_rng(35)
    n = 8200
    for name, mask in masks_for(n, rng).items():
        trees = [A.primitive(rng.integers(0, 255, n).astype(np.uint8)),
                 A.primitive(rng.standard_normal(n).astype(np.float32)),
                 A.primitive(rng.integers(-(1 << 40), 1 << 40, n).astype(np.int64), validity=rng.random(n) < 0.7)]
        info = run(ctx, trees, mask)
        assert info["fallback_arrays"] == 0 and info["packed_launches"] == 0, (name, info)
        assert info["inplace_arrays"] == (3 if mask.any() else 0), (name, info)
    # a Chunked of Primitive chunks: every chunk from its own buffer, first rows anywhere
    col = A.chunked([A.primitive(rng.integers(0, 1 << 30, m).astype(np.uint32)) for m in CHUNK_LENS])
    info = run(ctx, [col], _rand_mask(sum(CHUNK_LENS), rng))
    assert info["inplace_arrays"] == 5 and info["fallback_arrays"] == 0, info


def _strings(n):
    strs = [None if i % 7 == 3 else (b"comment %d " % i) * (1 + i % 4) for i in range(n)]
    strs[5], strs[6], strs[8] = b"", b"x" * 12, b"y" * 13
    return strs


def test_fallbacks(ctx):
    rng = np.random.default_rng(36)
    n = 4097
    mask = _rand_mask(n, rng)
    v = rng.integers(0, 1 << 12, n).astype(np.uint32)
    heap, offs, valid = E.strings_to_heap(_strings(n))
    trees = [E.encode_dict((rng.integers(0, 50, n) * 3).astype(np.uint8)),
             E.encode_runend(np.repeat(np.arange(n // 8 + 1, dtype=np.int64), 8)[:n]),
             E.encode_delta(np.cumsum(rng.integers(0, 5, n)).astype(np.uint64)),
             A.bool_array(rng.random(n) < 0.5, validity=E.encode_runend_bool(rng.random(n) < 0.7)),
             A.varbin(A.primitive(offs.astype(np.int32)), A.primitive(heap), validity=valid),
             E.encode_fsst(_strings(n))]
    for t in trees:
        is_str = t.dtype in (A.DTYPE["UTF8"], A.DTYPE["BINARY"])
        for m in (mask, np.ones(n, bool), np.zeros(n, bool)):
            info = run(ctx, [t], m)
            assert info["packed_launches"] == 0 and info["inplace_arrays"] == 0, (t.encoding, info)
            assert info["fallback_arrays"] == (1 if m.any() else 0), (t.encoding, info)
            assert info["syncs"] == (1 + (1 if is_str and m.any() else 0)), (t.encoding, info)
    # a nullable packed column stays packed: its validity is compacted by the same tile offsets
    nullable = [E.encode_bitpacked(v, bit_width=12, allow_patches=False, validity=rng.random(n) < 0.7),
                A.frame_of_reference(A.bitpacked(E.bitpack_buffer(v & 127, 7), "u32", 7, n, validity=rng.random(n) < 0.5),
                                     1000, 0, "u32"),
                A.bitpacked(E.bitpack_buffer(v & 127, 7), "u32", 7, n, validity="ALL_INVALID"),
                A.bitpacked(E.bitpack_buffer(v & 127, 7), "u32", 7, n, validity="ALL_VALID")]
    for m in (mask, np.ones(n, bool)):
        info = run(ctx, nullable, m)
        assert info["packed_launches"] == 4 and info["fallback_arrays"] == 0, info


def _batch(rng, n):
    heap, offs, valid = E.strings_to_heap(_strings(n))
    prices = np.round(rng.uniform(1, 100_000, n) * 100) / 100
    prices[::501] = rng.standard_normal(prices[::501].size) * 1e9
    return [E.encode_for_bitpacked(rng.integers(-3000, 3000, n).astype(np.int32), allow_patches=False),   # packed
            E.encode_alp(prices),                                                                          # packed + patches
            A.chunked(_for_chunks(rng, [1000, 0, 1, 2085, 64, n - 3150])),                                 # packed, chunked
            A.primitive(rng.standard_normal(n)),                                                           # in place
            E.encode_dict((rng.integers(0, 50, n) * 3).astype(np.uint16)),                                 # fallback
            A.bool_array(rng.random(n) < 0.5),                                                             # fallback
            E.encode_bitpacked(rng.integers(0, 4096, n, dtype=np.uint32), bit_width=12, allow_patches=False,
                               validity=rng.random(n) < 0.8),                                              # packed, nullable
            E.encode_runend(np.repeat(np.arange(n // 16 + 1, dtype=np.int16), 16)[:n]),                    # fallback
            A.varbin(A.primitive(offs.astype(np.int32)), A.primitive(heap), validity=valid),               # string
            E.encode_fsst(_strings(n))]                                                                    # string


def test_whole_batch(ctx):
    """Ten columns of mixed routes under one mask: one count, one wait (+ one per string column), and
    the bytes of A.filter per column; VXG_FILTB_CANONICALIZE gives the same bytes by the fallback."""
    import torch
    rng = np.random.default_rng(37)
    n = 8200
    batch = _batch(rng, n)
    mask = _rand_mask(n, rng, 0.3)
    pred = A.bool_array(mask)
    want = [filter_canon(t, pred) for t in batch]
    info = run(ctx, batch[:8], mask, want=want[:8])
    assert info["mask_scans"] == 1 and info["syncs"] == 1, info
    assert info["packed_launches"] == 4 and info["packed_chunks"] == 8 and info["inplace_arrays"] == 1, info
    assert info["fallback_arrays"] == 3 and info["patch_launches"] >= 1, info
    info = run(ctx, batch, mask, want=want)
    assert info["mask_scans"] == 1 and info["syncs"] == 3 and info["fallback_arrays"] == 5, info
    forced = run(ctx, batch, mask, flags=CANON, want=want)
    assert forced["packed_launches"] == 0 and forced["inplace_arrays"] == 0 and forced["patch_launches"] == 0, forced
    assert forced["fallback_arrays"] == len(batch) and forced["mask_scans"] == 1 and forced["syncs"] == 3, forced
    # the binding: the same Canonicals A.filter gives, column by column
    dev_batch = [t.to(_dev()) for t in batch]
    mt = mask_tensor(mask)
    outs, k, binfo = V.filter_batch(dev_batch, mt, ctx, length=n)
    assert k == int(mask.sum()) and binfo == info
    dpred = pred.to(_dev())
    for t, got in zip(dev_batch, outs):
        ref = A.filter(t, dpred, ctx)
        assert (got.kind, got.len, got.ptype) == (ref.kind, ref.len, ref.ptype)
        for f in ("values", "views", "data", "validity"):
            a, b = getattr(got, f), getattr(ref, f)
            assert (a is None) == (b is None), (t.encoding, f)
            assert a is None or torch.equal(a, b), (t.encoding, f)
        assert got.data_buffers == ref.data_buffers


def test_row_filter_result_goes_straight_in(ctx):
    """A range plus a string conjunct: row_filter's Canonical is the mask as it stands."""
    rng = np.random.default_rng(38)
    n = 5000
    qty = E.encode_for_bitpacked(rng.integers(1, 51, n).astype(np.int32), allow_patches=False)
    mode = E.encode_dict_strings([[b"AIR", b"MAIL", b"SHIP", b"TRUCK"][i] for i in rng.integers(0, 4, n)])
    price = E.encode_alp(np.round(rng.uniform(900, 105_000, n) * 100) / 100)
    dq, dm, dp = (t.to(_dev()) for t in (qty, mode, price))
    res = V.row_filter([(dq, ">=", 10), (dq, "<", 24), (dm, "==", b"AIR")], ctx)
    assert res.true_count is not None and 0 < res.true_count < n
    outs, k, info = V.filter_batch([dq, dp, dm], res, ctx)
    assert k == res.true_count and info["mask_scans"] == 1 and info["packed_launches"] == 2, info
    mask = res.numpy()
    for t, got in zip((qty, price), outs):
        assert got.numpy().tobytes() == filter_canon(t, A.bool_array(mask))[0].tobytes()
    (wv, wh), _ = filter_canon(mode, A.bool_array(mask))
    gv, gh = outs[2].numpy()
    assert gv.tobytes() == wv.tobytes() and gh.tobytes() == wh.tobytes()


@pytest.mark.parametrize("n", [65, 1025])
def test_tail_bits_past_len_are_ignored(ctx, n):
    rng = np.random.default_rng(39 + n)
    trees = [packed_tree(32, 7, n, 1, rng), A.primitive(rng.integers(0, 9, n).astype(np.int16)),
             E.encode_dict((rng.integers(0, 5, n) * 3).astype(np.uint8)), A.bool_array(rng.random(n) < 0.5)]
    for mask in (_rand_mask(n, rng), np.ones(n, bool), np.zeros(n, bool)):
        clean = run(ctx, trees, mask)
        dirty = run(ctx, trees, mask, dirty_tail=True)  # the expectation is the clean mask's
        assert clean == dirty


# ---- errors: found before anything is launched or allocated ---------------------------------
def _call(ctx, nodes, mask_ptr, n, flags=0, n_columns=None, null_columns=False, null_outs=False):
    """One call with NULL value pointers (the engine would allocate) -> (status, outs, guard)."""
    m = len(nodes)
    cols = (C.POINTER(L.VxgArray) * max(m, 1))(*[C.pointer(nd) if nd is not None else None for nd in nodes])
    outs = (L.VxgCanonical * max(m, 1))()
    guard = _guarded(0)
    if m:
        outs[m - 1].validity = guard.data_ptr()  # a caller's pointer: must come back as it went in
    k = C.c_uint64(77)
    info = L.VxgFilterBatchInfo()
    st = ctx.lib.vxg_filter_batch(ctx.handle, None if null_columns else cols, m if n_columns is None else n_columns,
                                  mask_ptr, n, flags, None if null_outs else outs, C.byref(k), C.byref(info),
                                  ctx.stream_ptr())
    ctx.sync()
    assert (guard.cpu().numpy() == 0xFF).all()
    for i in range(m):  # nothing engine-allocated is handed back
        assert not outs[i].values and not outs[i].views and not outs[i].data
        assert outs[i].validity == (guard.data_ptr() if i == m - 1 else None)
    assert info.packed_launches == 0 and info.fallback_arrays == 0 and info.inplace_arrays == 0
    return st


def test_errors(ctx):
    rng = np.random.default_rng(40)
    n = 2085
    keep: list = []
    good = A.flatten(packed_tree(32, 7, n, 0, rng).to(_dev()), keep)
    prim = A.flatten(A.primitive(np.arange(n, dtype=np.uint32)).to(_dev()), keep)
    short = A.flatten(A.primitive(np.arange(n - 1, dtype=np.uint32)).to(_dev()), keep)
    mt = mask_tensor(np.ones(n, bool))
    mp = C.c_void_p(mt.data_ptr())
    INVALID, NOT_IMPL = 3, 5
    assert _call(ctx, [], mp, n) == INVALID                                      # n_columns == 0
    assert _call(ctx, [good], mp, n, null_columns=True) == INVALID               # null columns
    assert _call(ctx, [good, None, prim], mp, n) == INVALID                      # null columns[i]
    assert _call(ctx, [good], mp, n, null_outs=True) == INVALID                  # null outs
    assert _call(ctx, [good], None, n) == INVALID                                # null mask with len > 0
    assert _call(ctx, [good], C.c_void_p(mt.data_ptr() + 4), n) == INVALID       # misaligned mask
    assert _call(ctx, [good, short], mp, n) == INVALID                           # a column of another length
    assert "does not equal array.len() of " + str(n - 1) in ctx.lib.vxg_last_error().decode()
    assert _call(ctx, [good], mp, n, flags=2) == INVALID                         # unknown flags
    assert _call(ctx, [good], mp, n, flags=CANON | 4) == INVALID
    null_dtype = A.flatten(A.primitive(np.arange(n, dtype=np.uint32)).to(_dev()), keep)
    null_dtype.dtype = A.DTYPE["NULL"]
    assert _call(ctx, [good, null_dtype], mp, n) == NOT_IMPL                     # an unsupported dtype
    # compare_shape's checks, at a later column: the packed byte count and its alignment
    bad_bytes = A.flatten(packed_tree(32, 7, n, 0, rng).to(_dev()), keep)
    bad_bytes.buffers[0].len -= 16
    assert _call(ctx, [good, prim, bad_bytes], mp, n) == INVALID
    assert "packed bytes" in ctx.lib.vxg_last_error().decode()
    bad_align = A.flatten(packed_tree(32, 7, n + 1024, 0, rng).to(_dev()), keep)
    bad_align.len = n
    bad_align.buffers[0].ptr += 4
    bad_align.buffers[0].len -= 128 * 7
    assert _call(ctx, [good, bad_align], mp, n) == INVALID
    assert "16-byte aligned" in ctx.lib.vxg_last_error().decode()
    # ... and under VXG_FILTB_CANONICALIZE too
    assert _call(ctx, [good, bad_bytes], mp, n, flags=CANON) == INVALID
    # every rejection of a BitPacked buffer, on the leaf of a FoR of one block
    block = E.encode_bitpacked(np.arange(1024, dtype=np.uint32) % 128, bit_width=7, allow_patches=False)
    for bad, text in bad_bitpacked(block):
        node = A.flatten(A.frame_of_reference(bad, 5, 0, "u32").to(_dev()), keep)
        assert _call(ctx, [node], mp, 1024) == INVALID
        assert text in ctx.lib.vxg_last_error().decode()


def test_good_call_allocates_what_is_null(ctx):
    """NULL pointers in an out are engine-allocated (vxg_free) and hold the filtered rows."""
    import torch
    rng = np.random.default_rng(41)
    n = 2085
    tree = E.encode_bitpacked(rng.integers(0, 128, n, dtype=np.uint32), bit_width=7, allow_patches=False,
                              validity=rng.random(n) < 0.6)
    mask = _rand_mask(n, rng)
    k = int(mask.sum())
    keep: list = []
    node = A.flatten(tree.to(_dev()), keep)
    cols = (C.POINTER(L.VxgArray) * 1)(C.pointer(node))
    outs = (L.VxgCanonical * 1)()
    mt = mask_tensor(mask)
    L.check(ctx.lib.vxg_filter_batch(ctx.handle, cols, 1, C.c_void_p(mt.data_ptr()), n, 0, outs, None, None,
                                     ctx.stream_ptr()))
    assert outs[0].values and outs[0].validity and outs[0].len == k
    got = torch.empty(4 * k, dtype=torch.uint8, device=_dev())
    gv = torch.empty(((k + 31) // 32) * 4, dtype=torch.uint8, device=_dev())
    L.check(ctx.lib.vxg_memcpy_d2d(ctx.handle, C.c_void_p(got.data_ptr()), C.c_void_p(outs[0].values), 4 * k, ctx.stream_ptr()))
    L.check(ctx.lib.vxg_memcpy_d2d(ctx.handle, C.c_void_p(gv.data_ptr()), C.c_void_p(outs[0].validity), gv.numel(),
                                   ctx.stream_ptr()))
    ctx.sync()
    L.check(ctx.lib.vxg_free(ctx.handle, C.c_void_p(outs[0].values)))
    L.check(ctx.lib.vxg_free(ctx.handle, C.c_void_p(outs[0].validity)))
    wvals, wvalid = filter_canon(tree, A.bool_array(mask))
    assert got.cpu().numpy().tobytes() == wvals.tobytes()
    assert np.array_equal(np.unpackbits(gv.cpu().numpy(), bitorder="little")[:k].astype(bool), wvalid)


def test_patch_position_outside_the_array_is_reported_at_sync(ctx):
    """A device-side error: the patch writes nothing and the next sync says OutOfBounds."""
    rng = np.random.default_rng(42)
    n = 1500
    vals = rng.integers(0, 128, n, dtype=np.uint32)
    patches = A.sparse(A.primitive(np.array([3, n + 5], np.uint64)),
                       A.primitive(np.array([70_000, 80_000], np.uint32), validity="ALL_VALID"), n)
    tree = A.bitpacked(E.bitpack_buffer(vals, 7), "u32", 7, n, patches=patches)
    keep: list = []
    node = A.flatten(tree.to(_dev()), keep)
    cols = (C.POINTER(L.VxgArray) * 1)(C.pointer(node))
    outs = (L.VxgCanonical * 1)()
    buf = _guarded(4 * n)
    outs[0].values = buf.data_ptr()
    mt = mask_tensor(np.ones(n, bool))
    L.check(ctx.lib.vxg_filter_batch(ctx.handle, cols, 1, C.c_void_p(mt.data_ptr()), n, 0, outs, None, None,
                                     ctx.stream_ptr()))
    with pytest.raises(V.VortexGpuError) as ei:
        ctx.sync()
    assert ei.value.kind == "OutOfBounds"
    host = buf.cpu().numpy()
    assert (host[4 * n:] == 0xFF).all()
    want = vals.copy()
    want[3] = 70_000
    assert host[: 4 * n].tobytes() == want.tobytes()
