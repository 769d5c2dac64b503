"""GPU: vxg_compare_scalar against the oracle's canonical values compared by numpy, byte for byte.

Every call writes into buffers of the exact size + 64 guard bytes filled with 0xFF: the tail bits
past len must be zero and the guard untouched.  `info` says which path ran, and the tests assert
it: the packed-domain kernel where it is claimed, the canonicalize fallback elsewhere."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import vortex_amd as V
import vortex_amd._lib as L
import vortex_amd.arrays as A
import vortex_amd.encode as E
from compare_expected import OPS, bitmap, expected
from oracle_tree import bad_bitpacked, canon, misaligned_bitpacked, slice_bitpacked

pytestmark = pytest.mark.gpu

GUARD = 64
ALL_OPS = list(OPS)


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


def check(ctx, tree, op, scalar, null_as_false=False, fused=None):
    """One compare checked against the oracle; `fused`: True = the packed-domain kernel ran and
    nothing fell back, False = only the fallback ran."""
    want, want_valid, mask = expected(tree, op, scalar)
    res, got, got_valid = run(ctx, tree, op, scalar, null_as_false)
    assert got == want, (op, scalar, tree.len, np.flatnonzero(
        np.frombuffer(got, np.uint8) != np.frombuffer(want, np.uint8))[:8])
    assert got_valid == (None if null_as_false else want_valid)
    if fused is True:
        assert res.info["fused_launches"] >= 1 and res.info["fallback_arrays"] == 0, res.info
    elif fused is False:
        assert res.info["fused_launches"] == 0 and res.info["fallback_arrays"] >= 1, res.info
    return res, mask


def packed_tree(T: int, W: int, n: int, offset: int, rng) -> A.Array:
    """A BitPacked u<T> array of n values of W bits whose slice offset is `offset` (a slice of a
    longer array, bitpacking/compute/slice.rs)."""
    dt = np.dtype(f"u{T // 8}")
    hi = (1 << W) - 1
    full = rng.integers(0, hi + 1, n + offset, dtype=np.uint64, endpoint=False).astype(dt) if W else np.zeros(n + offset, dt)
    if W and full.size:
        full[rng.integers(0, full.size, 3)] = hi  # the width's extremes are present
        full[rng.integers(0, full.size, 3)] = 0
    p = f"u{T}"
    if W == 0:
        a = A.bitpacked(np.zeros(0, np.uint8), p, 0, n + offset)
    elif W == T:
        a = A.bitpacked(E.bitpack_buffer(full, T), p, T, n + offset)
    else:
        a = E.encode_bitpacked(full, bit_width=W, allow_patches=False)
    return slice_bitpacked(a, offset, offset + n) if offset else a


LENS = [0, 1, 63, 64, 65, 1023, 1024, 1025, 2085, 3073]
OFFSETS = [0, 1, 63, 1000, 1023]


@pytest.mark.parametrize("W", [0, 1, 7, 31, 32])
def test_geometry_t32(ctx, W):
    rng = np.random.default_rng(100 + W)
    for n in LENS:
        for off in OFFSETS:
            tree = packed_tree(32, W, n, off, rng)
            assert tree.meta["offset"] == off and tree.len == n
            vals = canon(tree)[0]
            s = int(np.median(vals)) if n else 0
            check(ctx, tree, "<", s, fused=True)   # W >= 1: a random pattern, about half the rows
            check(ctx, tree, ">=", s, fused=True)  # its complement (W = 0: every row, so the tail must stay 0)
            check(ctx, tree, "==", s, fused=True)


@pytest.mark.parametrize("T", [8, 16, 64])
def test_geometry_other_widths(ctx, T):
    rng = np.random.default_rng(200 + T)
    for W in (0, 1, {8: 5, 16: 11, 64: 37}[T], T - 1, T):
        for n in (0, 1, 65, 1025, 2085):
            for off in (0, 63, 1000):
                tree = packed_tree(T, W, n, off, rng)
                vals = canon(tree)[0]
                s = int(np.median(vals)) if n else 0
                check(ctx, tree, "<=", s, fused=True)
                check(ctx, tree, "!=", s, fused=True)


def scalars_for(vals: np.ndarray):
    """A present value, the column's min and max and their neighbours where representable, and
    the ptype's own min and max."""
    info = np.iinfo(vals.dtype)
    lo, hi = int(vals.min()), int(vals.max())
    out = {int(vals[vals.size // 3]), lo, hi, info.min, info.max}
    if lo > info.min:
        out.add(lo - 1)
    if hi < info.max:
        out.add(hi + 1)
    return sorted(out)


def all_ops_and_scalars(ctx, tree, fused=True):
    vals = canon(tree)[0]
    for s in scalars_for(vals):
        for op in ALL_OPS:
            check(ctx, tree, op, s, fused=fused)


def test_ops_bitpacked_u32(ctx):
    rng = np.random.default_rng(1)
    tree = E.encode_bitpacked(rng.integers(3, 120, 1500, dtype=np.uint32), bit_width=7, allow_patches=False)
    all_ops_and_scalars(ctx, tree)


@pytest.mark.parametrize("dt", [np.int8, np.int16, np.int32, np.int64])
def test_ops_signed_for_negative_reference(ctx, dt):
    rng = np.random.default_rng(2)
    span = 100 if dt == np.int8 else 3000
    vals = (rng.integers(0, span, 1300) - span + 7).astype(dt)  # reference = the negative minimum
    tree = E.encode_for_bitpacked(vals, allow_patches=False)
    assert tree.encoding == V.ENC["FL_FOR"] and tree.children[0].encoding == V.ENC["FL_BITPACKED"]
    assert np.array([tree.meta["reference"]], np.uint64).astype(f"u{vals.itemsize}").view(dt)[0] < 0
    all_ops_and_scalars(ctx, tree)


@pytest.mark.parametrize("T", [8, 64])
def test_ops_unsigned_for_whose_add_wraps(ctx, T):
    """for/compress.rs:100-117 adds with wrapping_add: reference near the type's maximum."""
    rng = np.random.default_rng(3)
    dt = np.dtype(f"u{T // 8}")
    enc = rng.integers(0, 100, 1100, dtype=np.uint64).astype(dt)
    child = E.encode_bitpacked(enc, bit_width=7, allow_patches=False)
    ref = (1 << T) - 40  # values 0..59 wrap to 0..59, the rest stay near the top
    tree = A.frame_of_reference(child, ref, 0, f"u{T}")
    vals = canon(tree)[0]
    assert vals.min() < 60 and vals.max() > (1 << T) - 41
    all_ops_and_scalars(ctx, tree)


def test_ops_for_with_shift(ctx):
    vals = (np.arange(0, 1200 * 8, 8, dtype=np.int32) - 4000)
    tree = E.encode_for_bitpacked(vals, allow_patches=False)
    assert tree.meta["shift"] == 3
    all_ops_and_scalars(ctx, tree)


def test_ops_zigzag(ctx):
    rng = np.random.default_rng(4)
    vals = rng.integers(-500, 500, 1400).astype(np.int32)
    all_ops_and_scalars(ctx, E.encode_zigzag(vals))
    # ZigZag over FoR(BitPacked): FoR on the unsigned encoded words
    zz = E.zigzag_encode(vals.astype(np.int16))
    child = E.encode_bitpacked((zz - zz.min()).astype(np.uint16), allow_patches=False)
    tree = A.zigzag(A.frame_of_reference(child, int(zz.min()), 0, "u16"))
    assert (canon(tree)[0] == vals).all()
    all_ops_and_scalars(ctx, tree)


def test_bitpacked_patches(ctx):
    rng = np.random.default_rng(5)
    vals = rng.integers(0, 128, 2500, dtype=np.uint32)
    rows = np.array([0, 63, 64, 1023, 1024, 2499])
    vals[rows] = 1024 + np.arange(rows.size, dtype=np.uint32) * 128 + 5  # low 7 bits = 5
    tree = E.encode_bitpacked(vals, bit_width=7)
    assert tree.meta["has_patches"]
    res, mask = check(ctx, tree, "==", 1029, fused=True)       # a patch value: true at its row
    assert res.info["patch_launches"] == 1 and mask[0] and mask.sum() == 1
    _, mask = check(ctx, tree, "==", 5, fused=True)             # the truncated low bits: false there
    assert not mask[rows].any()
    for op in ALL_OPS:
        check(ctx, tree, op, 127, fused=True)
    # FoR over patched BitPacked: the patch values go through the epilogue
    f = E.encode_for_bitpacked((vals.astype(np.int64) - 300), allow_patches=True)
    assert f.children[0].meta["has_patches"]
    for op in ALL_OPS:
        check(ctx, f, op, 729, fused=True)


def test_alp_reference_literals_f32(ctx):
    a = E.encode_alp(np.full(1025, 1.234, dtype=np.float32))
    _, mask = check(ctx, a, "==", 1.3, fused=True)
    assert not mask.any()
    _, mask = check(ctx, a, "==", 1.234, fused=True)
    assert mask.all()
    b = E.encode_alp(np.array([1.234, 1.5, 19.0, np.e, 1_000_000.9], dtype=np.float32))
    assert b.meta["has_patches"]
    _, mask = check(ctx, b, "==", 1_000_000.9, fused=True)
    assert mask.tolist() == [False, False, False, False, True]
    # the documented divergence: exception slots compare their decoded values, so == 1.234 is row
    # 0 only (the reference compares the slots' fill value 1234 and also reports rows 3 and 4)
    _, mask = check(ctx, b, "==", 1.234, fused=True)
    assert mask.tolist() == [True, False, False, False, False]


def test_alp_f64_with_patches(ctx):
    rng = np.random.default_rng(6)
    vals = np.round(rng.uniform(1, 1000, 3000) * 100) / 100
    vals[::97] = rng.standard_normal(vals[::97].size) * 1e9 + 0.123456789
    vals[5] = np.nan
    tree = E.encode_alp(vals)
    assert tree.meta["has_patches"] and tree.children[0].encoding == V.ENC["FL_FOR"]
    for op in ALL_OPS:
        res, _ = check(ctx, tree, op, float(vals[1]), fused=True)
        assert res.info["patch_launches"] >= 1
        check(ctx, tree, op, float(vals[97]), fused=True)
        check(ctx, tree, op, float("nan"), fused=True)


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_primitive_floats_ieee(ctx, dt):
    base = np.array([np.nan, -0.0, 0.0, np.inf, -np.inf, 1.5, -2.25, np.finfo(dt).max, np.finfo(dt).tiny], dtype=dt)
    vals = np.tile(base, 9)[:70]
    tree = A.primitive(vals)
    for s in (float("nan"), 0.0, -0.0, float("inf"), float("-inf"), 1.5):
        for op in ALL_OPS:
            check(ctx, tree, op, s, fused=False)


def test_validity(ctx):
    rng = np.random.default_rng(7)
    n = 1500
    vals = rng.integers(0, 128, n, dtype=np.uint32)
    mask = rng.random(n) < 0.7
    packed = E.bitpack_buffer(vals, 7)
    trees = [A.bitpacked(packed, "u32", 7, n, validity=A.bool_array(mask, bit_offset=3)),  # a sliced Bool child
             A.bitpacked(packed, "u32", 7, n, validity="ALL_INVALID"),
             A.frame_of_reference(A.bitpacked(packed, "u32", 7, n, validity=mask), 1000, 0, "u32"),
             A.primitive(vals, validity=mask)]
    for i, tree in enumerate(trees):
        for op in ("<", "!="):
            res, m = check(ctx, tree, op, 64, fused=i < 3)
            assert res.validity is not None
            res, m2 = check(ctx, tree, op, 64, null_as_false=True, fused=i < 3)
            assert res.validity is None and (m == m2).all()
    # nullable but all valid: no validity comes back
    res, _ = check(ctx, A.bitpacked(packed, "u32", 7, n, validity="ALL_VALID"), "<", 64, fused=True)
    assert res.validity is None


def _mixed_chunks(rng, lens):
    kinds, chunks = [], []
    for i, n in enumerate(lens):
        vals = (rng.integers(0, 200, n) - 50).astype(np.int32)
        kind = ["for", "primitive", "for", "for", "constant", "runend"][i % 6]
        if kind == "for" and n == 0:  # FoR(BitPacked) of no rows, by hand (for_compress needs a row)
            c = A.frame_of_reference(A.bitpacked(np.zeros(0, np.uint8), "u32", 5, 0), -3, 0, "i32")
        elif kind == "for":
            c = A.frame_of_reference(E.encode_bitpacked((vals + 50).astype(np.uint32), bit_width=8, allow_patches=False),
                                     -50, 0, "i32")
        elif kind == "primitive":
            c = A.primitive(vals)
        elif kind == "constant":
            c = A.constant(17, n, "i32")
        else:
            c = E.encode_runend(np.repeat(vals[:: 8], 8)[:n])
        kinds.append(kind)
        chunks.append(c)
    return kinds, chunks


def test_chunked_mixed(ctx):
    rng = np.random.default_rng(8)
    lens = [1, 63, 1024, 0, 65, 2049]  # boundaries inside words, one empty chunk
    kinds, chunks = _mixed_chunks(rng, lens)
    assert kinds == ["for", "primitive", "for", "for", "constant", "runend"]
    tree = A.chunked(chunks)
    for op in ALL_OPS:
        res, _ = check(ctx, tree, op, 17)
        assert res.info["fused_chunks"] == kinds.count("for")
        assert res.info["fallback_arrays"] == len(kinds) - kinds.count("for")
        assert res.info["fused_launches"] == 1  # one distinct fused shape: FoR(BitPacked) i32


def test_chunked_launches_do_not_grow_with_chunks(ctx):
    """The chunks of one shape share launches: one per 100 chunks, whatever their bit widths."""
    rng = np.random.default_rng(9)
    chunks = []
    for i in range(70):
        n = int(rng.integers(1, 300))
        w = 3 + i % 5  # the bit width differs between the chunks of one launch
        vals = rng.integers(0, 1 << w, n, dtype=np.uint64)
        vals[0] = (1 << w) - 1
        if i % 2:
            chunks.append(A.frame_of_reference(E.encode_bitpacked(vals.astype(np.uint64), bit_width=w, allow_patches=False),
                                               -7, 0, "i64"))
        else:
            chunks.append(A.frame_of_reference(A.primitive(vals.astype(np.uint64)), -7, 0, "i64"))
    tree = A.chunked(chunks)
    for op in ("<", "=="):
        res, _ = check(ctx, tree, op, 2)
        assert res.info == {"fused_launches": 1, "fused_chunks": 35, "fallback_arrays": 35, "patch_launches": 0}
    all_fused = A.chunked(chunks[1::2] + chunks[1::2])
    res, _ = check(ctx, all_fused, ">=", 5, fused=True)
    assert res.info["fused_launches"] == 1 and res.info["fused_chunks"] == 70
    # a C5 column's 92 chunks are one launch; the kernel-argument table holds 100, then it repeats
    res, _ = check(ctx, A.chunked((chunks[1::2] * 3)[:92]), "<", 5, fused=True)
    assert res.info["fused_launches"] == 1 and res.info["fused_chunks"] == 92
    res, _ = check(ctx, A.chunked(chunks[1::2] * 6), "!=", 3, fused=True)
    assert res.info["fused_launches"] == 3 and res.info["fused_chunks"] == 210


def test_fallback_encodings(ctx):
    rng = np.random.default_rng(10)
    ints = rng.integers(0, 50, 700).astype(np.int32)
    floats = rng.standard_normal(700) * 1e-7 + 1.0
    idx = np.sort(rng.choice(700, 40, replace=False)).astype(np.uint64)
    trees = [E.encode_dict(ints), E.encode_delta(np.cumsum(ints).astype(np.uint32)),
             E.encode_runend(np.repeat(ints[:100], 7)), E.encode_alprd(floats),
             A.sparse(A.primitive(idx), A.primitive(ints[:40]), 700, fill=9),
             A.constant(25, 700, "i32")]
    for tree in trees:
        vals = canon(tree)[0]
        for op in ("<", "=="):
            check(ctx, tree, op, vals[vals.size // 2].item(), fused=False)


def _status(ctx, tree, op_code=4):
    keep = []
    node = A.flatten(tree.to(_dev()), keep)
    out = L.VxgCanonical()
    sc = (C.c_uint8 * 8)()
    st = ctx.lib.vxg_compare_scalar(ctx.handle, C.byref(node), op_code, sc, 0, C.byref(out), None, ctx.stream_ptr())
    assert not out.values or st == 0
    return L.STATUS[st]


def test_errors(ctx):
    ok = E.encode_bitpacked(np.arange(100, dtype=np.uint32), bit_width=7, allow_patches=False)
    assert _status(ctx, A.bool_array(np.ones(10, bool))) == "NotImplemented"
    assert _status(ctx, E.encode_varbinview([b"a", b"bc"])) == "NotImplemented"
    assert _status(ctx, A.primitive(np.ones(10, np.float16))) == "NotImplemented"
    assert _status(ctx, ok, op_code=6) == "InvalidArgument"
    assert _status(ctx, ok, op_code=-1) == "InvalidArgument"
    short = dataclasses.replace(ok, buffers=[np.asarray(ok.buffers[0])[:-128]])
    assert _status(ctx, short) == "InvalidArgument"
    assert "Expected 896 packed bytes, got 768" in ctx.lib.vxg_last_error().decode()
    # the BitPacked leaf of a FoR, malformed: rejected before anything is launched
    block = E.encode_bitpacked(np.arange(1024, dtype=np.uint32) % 128, bit_width=7, allow_patches=False)
    for bad, text in bad_bitpacked(block) + [(misaligned_bitpacked(block, _dev()), "16-byte aligned")]:
        assert _status(ctx, A.frame_of_reference(bad, 5, 0, "u32")) == "InvalidArgument"
        assert text in ctx.lib.vxg_last_error().decode()
    with pytest.raises(V.VortexGpuError, match="unknown operator"):
        V.compare(ok.to(_dev()), "~", 1, ctx)


def test_compare_then_filter(ctx):
    """filter(a, predicate_from(compare(a, "<", s, null_as_false=True))) == vals[(vals < s) & valid]."""
    rng = np.random.default_rng(11)
    n = 5000
    vals = (rng.integers(0, 1000, n) - 400).astype(np.int32)
    valid = rng.random(n) < 0.8
    tree = A.frame_of_reference(
        A.bitpacked(E.bitpack_buffer((vals + 400).astype(np.uint32), 10), "u32", 10, n, validity=valid), -400, 0, "i32")
    assert (canon(tree)[0] == vals).all()
    dev_tree = tree.to(_dev())
    pred = V.compare(dev_tree, "<", 24, ctx, null_as_false=True)
    assert pred.info["fused_launches"] == 1 and pred.info["fallback_arrays"] == 0
    got = A.filter(dev_tree, V.predicate_from(pred), ctx)
    keep = (vals < 24) & valid
    assert got.len == int(keep.sum())
    assert (got.numpy() == vals[keep]).all()
    assert got.validity_mask() is None or got.validity_mask().all()
