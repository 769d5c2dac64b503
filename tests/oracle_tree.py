"""CPU canonicalize of a vortex_amd Array tree through the oracle (TEST INFRASTRUCTURE).

Walks the same tree the GPU engine receives and decodes it the way the reference does:
child-first, one materialised buffer per cascade level, patches applied after the level that
owns them (canonical.rs:353-357 recursion; per-encoding IntoCanonical impls cited below).
Every arithmetic step is a call into oracle/liboracle.so (vx_oracle.c).
"""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

from oracle import oracle as O  # noqa: E402
from vortex_amd._lib import DTYPE, ENC, VALIDITY  # noqa: E402
from vortex_amd.arrays import NP_OF_PTYPE, Array, ptype_width, unsigned_of  # noqa: E402


def _buf(b) -> np.ndarray:
    if hasattr(b, "cpu"):
        return b.cpu().numpy().view(np.uint8)
    return np.ascontiguousarray(b).view(np.uint8).reshape(-1)


def _validity(a: Array):
    """Bool mask or None (no nulls) following the reference's validity() accessors."""
    e = a.encoding

    def from_meta(idx):
        if a.validity in (VALIDITY["NON_NULLABLE"], VALIDITY["ALL_VALID"]):
            return None
        if a.validity == VALIDITY["ALL_INVALID"]:
            return np.zeros(a.len, dtype=bool)
        v = a.children[idx]
        if v.encoding != ENC["BOOL"]:  # a compressed Bool array: its canonical bits
            return canon_bool(v)
        bits = _buf(v.buffers[0])
        off = v.meta.get("first_byte_bit_offset", 0)
        return np.unpackbits(bits, bitorder="little")[off: off + a.len].astype(bool)

    if e in (ENC["PRIMITIVE"], ENC["BOOL"], ENC["BYTE_BOOL"]):
        return from_meta(0)
    if e == ENC["RUN_END_BOOL"]:
        return from_meta(1)
    if e == ENC["FL_BITPACKED"]:
        return from_meta(1 if a.meta["has_patches"] else 0)
    if e in (ENC["FL_DELTA"], ENC["RUN_END"], ENC["VARBIN"]):
        return from_meta(2)
    if e == ENC["VARBINVIEW"]:
        return from_meta(1 + a.meta["n_buffers"])
    if e in (ENC["FL_FOR"], ENC["ZIGZAG"], ENC["ALP"], ENC["ALP_RD"]):
        return _validity(a.children[0])
    if e == ENC["FSST"]:
        return _validity(a.children[2])
    if e == ENC["CONSTANT"]:
        return np.zeros(a.len, dtype=bool) if a.meta["is_null"] else None
    if e == ENC["DICT"]:
        # take(values, codes): values.validity().take(codes) (primitive/compute/take.rs:58-67)
        vv = _validity(a.children[0])
        if vv is None:
            return None
        return vv[canon(a.children[1])[0].astype(np.int64)]
    if e == ENC["SPARSE"]:
        # primitives: validity only with a null fill; bools: always the indices
        # (sparse/flatten.rs:41-61 vs :72-96)
        if not a.meta["fill_is_null"] and a.dtype != DTYPE["BOOL"]:
            return None
        m = np.zeros(a.len, dtype=bool)
        idx = canon(a.children[0])[0].astype(np.int64) - a.meta["indices_offset"]
        m[idx] = True
        return m
    if e == ENC["CHUNKED"]:
        parts = [_validity(c) for c in a.children[1:]]
        if all(p is None for p in parts):
            return None
        return np.concatenate([np.ones(c.len, bool) if p is None else p
                               for p, c in zip(parts, a.children[1:])])
    return None


def _patch(out: np.ndarray, sp: Array) -> None:
    # SparseArray::resolved_indices + PrimitiveArray::patch
    idx = canon(sp.children[0])[0]
    vals = np.ascontiguousarray(canon(sp.children[1])[0]).astype(out.dtype, copy=False)
    ipt = sp.children[0].ptype
    rc = O.lib().vxo_patch(O.PT[_pt(out)], O.p(out), out.size, O.PT[ipt], O.p(np.ascontiguousarray(idx)),
                           sp.meta["indices_offset"], O.p(vals), idx.size)
    if rc != 0:
        raise IndexError("patch index out of bounds")


def _pt(arr: np.ndarray) -> str:
    for k, v in NP_OF_PTYPE.items():
        if np.dtype(v) == arr.dtype:
            return k
    raise KeyError(arr.dtype)


def canon(a: Array):
    """-> (values ndarray, validity mask|None) for primitives;
          ((views u8[n,16], heap u8[]), validity) for utf8/binary."""
    L = O.lib()
    e = a.encoding
    if a.dtype in (DTYPE["UTF8"], DTYPE["BINARY"]):
        return _canon_string(a), _validity(a)
    if a.dtype == DTYPE["BOOL"]:
        return canon_bool(a), _validity(a)
    dt = NP_OF_PTYPE[a.ptype]
    val = _validity(a)
    if e == ENC["PRIMITIVE"]:
        return _buf(a.buffers[0])[: a.len * np.dtype(dt).itemsize].view(dt).copy(), val
    if e == ENC["FL_BITPACKED"]:
        # bitpacking/compress.rs:167-189
        out = np.zeros(a.len, dtype=NP_OF_PTYPE[unsigned_of(a.ptype)])
        packed = _buf(a.buffers[0])
        rc = L.vxo_unpack(O.PT[unsigned_of(a.ptype)], a.meta["bit_width"], a.meta["offset"], a.len,
                          O.p(packed), packed.size, O.p(out))
        if rc:
            raise ValueError("Invalid packed length")
        out = out.view(dt)
        if a.meta["has_patches"]:
            _patch(out, a.children[0])
        return out, val
    if e == ENC["FL_FOR"]:
        # for/compress.rs:86-98
        child = np.ascontiguousarray(canon(a.children[0])[0]).view(dt).copy()
        L.vxo_for_decode(O.PT[a.ptype], O.p(child), child.size, a.meta["reference"], a.meta["shift"], O.p(child))
        return child, val
    if e == ENC["ZIGZAG"]:
        child = np.ascontiguousarray(canon(a.children[0])[0])
        out = np.zeros(a.len, dtype=dt)
        L.vxo_zigzag_decode(O.PT[a.ptype], O.p(child), child.size, O.p(out))
        return out, val
    if e == ENC["ALP"]:
        # alp/compress.rs:61-96
        enc = np.ascontiguousarray(canon(a.children[0])[0])
        out = np.zeros(a.len, dtype=dt)
        fn = L.vxo_alp_decode_f32 if a.ptype == "f32" else L.vxo_alp_decode_f64
        fn(O.p(enc), enc.size, a.meta["e"], a.meta["f"], O.p(out))
        if a.meta["has_patches"]:
            _patch(out, a.children[1])
        return out, val
    if e == ENC["ALP_RD"]:
        # alp_rd/array.rs:179-235
        left = np.ascontiguousarray(canon(a.children[0])[0]).astype(np.uint16)
        right = np.ascontiguousarray(canon(a.children[1])[0])
        d = np.array(a.meta["dict"], dtype=np.uint16)
        pos = np.zeros(0, np.uint64)
        exc = np.zeros(0, np.uint16)
        if a.meta["has_exceptions"]:
            sp = a.children[2]
            pos = (canon(sp.children[0])[0].astype(np.int64) - sp.meta["indices_offset"]).astype(np.uint64)
            exc = np.ascontiguousarray(canon(sp.children[1])[0]).astype(np.uint16)
        out = np.zeros(a.len, dtype=dt)
        fn = L.vxo_alprd_decode_checked_f32 if a.ptype == "f32" else L.vxo_alprd_decode_checked_f64
        if fn(O.p(left), O.p(d), d.size, a.meta["right_bit_width"], O.p(right), a.len, O.p(pos), O.p(exc), pos.size,
              O.p(out)):
            raise IndexError("ALP-RD left code or exception position out of bounds")
        return out, val
    if e == ENC["DICT"]:
        values = np.ascontiguousarray(canon(a.children[0])[0])
        codes = np.ascontiguousarray(canon(a.children[1])[0])
        out = np.zeros(a.len, dtype=dt)
        rc = L.vxo_take(values.dtype.itemsize, O.p(values), values.size, O.PT[a.children[1].ptype],
                        O.p(codes), codes.size, O.p(out))
        if rc:
            raise IndexError("take: index out of bounds")
        return out, val
    if e == ENC["FL_DELTA"]:
        bases = np.ascontiguousarray(canon(a.children[0])[0])
        deltas = np.ascontiguousarray(canon(a.children[1])[0])
        out = np.zeros(a.len, dtype=dt)
        rc = L.vxo_delta_decode(O.PT[a.ptype], O.p(bases), bases.size, O.p(deltas), deltas.size,
                                a.meta["offset"], a.len, O.p(out))
        if rc:
            raise ValueError("delta decode failed")
        return out, val
    if e == ENC["RUN_END"]:
        ends = np.ascontiguousarray(canon(a.children[0])[0])
        values = np.ascontiguousarray(canon(a.children[1])[0])
        out = np.zeros(a.len, dtype=dt)
        rc = L.vxo_runend_decode(values.dtype.itemsize, O.p(values), O.PT[a.children[0].ptype], O.p(ends),
                                 ends.size, a.meta["offset"], a.len, O.p(out))
        if rc:
            raise ValueError("runend decode failed")
        return out, val
    if e == ENC["SPARSE"]:
        fill = np.frombuffer(bytes(a.meta["fill"])[: np.dtype(dt).itemsize], dtype=dt)
        out = np.full(a.len, 0 if a.meta["fill_is_null"] else fill[0], dtype=dt)
        _patch(out, a)
        return out, val
    if e == ENC["CONSTANT"]:
        sc = np.frombuffer(bytes(a.meta["scalar"])[: np.dtype(dt).itemsize], dtype=dt)
        return np.full(a.len, 0 if a.meta["is_null"] else sc[0], dtype=dt), val
    if e == ENC["CHUNKED"]:
        # chunked/canonical.rs:170-187 pack_primitives
        parts = [canon(c)[0] for c in a.children[1:]]
        return (np.concatenate(parts).astype(dt) if parts else np.zeros(0, dt)), val
    raise NotImplementedError(f"oracle canonicalize for encoding {e}")


def canon_bool(a: Array) -> np.ndarray:
    """Canonical::Bool values of a Bool-dtype tree as a bool mask."""
    L = O.lib()
    e, n = a.encoding, a.len
    if e == ENC["BOOL"]:  # array/bool/mod.rs: bits from first_byte_bit_offset
        off = a.meta.get("first_byte_bit_offset", 0)
        return np.unpackbits(_buf(a.buffers[0]), bitorder="little")[off: off + n].astype(bool)
    if e == ENC["BYTE_BOOL"]:  # bytebool/src/array.rs:138-146
        out = np.zeros((n + 7) // 8 + 1, np.uint8)
        L.vxo_bytebool_to_bits(O.p(np.ascontiguousarray(_buf(a.buffers[0])[:n])), n, O.p(out))
        return np.unpackbits(out, bitorder="little")[:n].astype(bool)
    if e == ENC["RUN_END_BOOL"]:  # runend-bool/src/array.rs:152-163 -> compress.rs:46-93
        ends = np.ascontiguousarray(canon(a.children[0])[0])
        out = np.zeros((n + 7) // 8 + 1, np.uint8)
        rc = L.vxo_runend_bool_decode(O.PT[a.children[0].ptype], O.p(ends), ends.size, a.meta["offset"],
                                      int(a.meta["start"]), n, O.p(out))
        if rc:
            raise ValueError("runend bool decode failed")
        return np.unpackbits(out, bitorder="little")[:n].astype(bool)
    if e == ENC["ROARING_BOOL"]:  # roaring/src/boolean/mod.rs:127-147 (croaring Native)
        raw = np.ascontiguousarray(_buf(a.buffers[0]))
        out = np.zeros((n + 7) // 8 + 1, np.uint8)
        if L.vxo_roaring_bool_decode(O.p(raw), raw.size, n, O.p(out)):
            raise ValueError("malformed croaring Native bitmap")
        return np.unpackbits(out, bitorder="little")[:n].astype(bool)
    if e == ENC["CONSTANT"]:  # constant/canonical.rs:26-33
        return np.full(n, (not a.meta["is_null"]) and bytes(a.meta["scalar"])[0] != 0, dtype=bool)
    if e == ENC["SPARSE"]:  # sparse/flatten.rs:41-61
        out = np.full(n, (not a.meta["fill_is_null"]) and bytes(a.meta["fill"])[0] != 0, dtype=bool)
        idx = canon(a.children[0])[0].astype(np.int64) - a.meta["indices_offset"]
        out[idx] = canon_bool(a.children[1])
        return out
    if e == ENC["CHUNKED"]:  # chunked/canonical.rs:154-163 pack_bools
        parts = [canon_bool(c) for c in a.children[1:]]
        return np.concatenate(parts) if parts else np.zeros(0, bool)
    raise NotImplementedError(f"oracle bool canonicalize for encoding {e}")


def _canon_string(a: Array):
    L = O.lib()
    e = a.encoding
    val = _validity(a)
    vbits = None if val is None else np.packbits(val, bitorder="little")
    if e == ENC["VARBIN"]:
        offs = canon(a.children[0])[0].astype(np.int64)
        heap = np.ascontiguousarray(canon(a.children[1])[0]).astype(np.uint8)
        views = np.zeros((a.len, 16), dtype=np.uint8)
        L.vxo_make_views(O.p(heap), O.p(offs), a.len, O.p(vbits) if vbits is not None else None, 0, O.p(views))
        return views, heap
    if e == ENC["FSST"]:
        syms = np.ascontiguousarray(canon(a.children[0])[0]).astype(np.uint64)
        slen = np.ascontiguousarray(canon(a.children[1])[0]).astype(np.uint8)
        codes = a.children[2]
        coffs = np.ascontiguousarray(canon(codes.children[0])[0])
        cbytes = np.ascontiguousarray(canon(codes.children[1])[0]).astype(np.uint8)
        lens = np.ascontiguousarray(canon(a.children[3])[0])
        total = int(lens.astype(np.int64).sum())
        heap = np.zeros(total + 16, dtype=np.uint8)
        views = np.zeros((a.len, 16), dtype=np.uint8)
        import ctypes as C
        hl = C.c_size_t()
        rc = L.vxo_fsst_canonicalize(O.p(syms), O.p(slen), O.p(cbytes), O.PT[codes.children[0].ptype], O.p(coffs),
                                     O.PT[a.children[3].ptype], O.p(lens), a.len,
                                     O.p(vbits) if vbits is not None else None, O.p(heap), C.byref(hl), O.p(views))
        if rc:
            raise ValueError("fsst canonicalize: decoded length mismatch")
        return views, heap[: hl.value]
    if e == ENC["VARBINVIEW"]:
        # already canonical: views + data buffers (varbinview/mod.rs:217-262)
        views = np.ascontiguousarray(canon(a.children[0])[0]).astype(np.uint8).reshape(-1, 16).copy()
        bufs = [np.ascontiguousarray(canon(c)[0]).astype(np.uint8) for c in a.children[1: 1 + a.meta["n_buffers"]]]
        return views, bufs
    if e == ENC["DICT"]:
        (vviews, vheap), _ = canon(a.children[0])
        codes = canon(a.children[1])[0].astype(np.int64)
        return vviews[codes], vheap
    if e == ENC["CHUNKED"]:
        # pack_views (chunked/canonical.rs:194-236): buffers concatenated in chunk order, each
        # chunk's non-inlined views rebased by the number of buffers before it
        all_views, bufs = [], []
        for c in a.children[1:]:
            (v, b), _ = canon(c)
            b = b if isinstance(b, list) else [b]
            v = np.ascontiguousarray(v).copy()
            L.vxo_rebase_views(O.p(v), v.shape[0], len(bufs))
            all_views.append(v)
            bufs.extend(b)
        return (np.concatenate(all_views) if all_views else np.zeros((0, 16), np.uint8)), bufs
    raise NotImplementedError(f"oracle string canonicalize for encoding {e}")


def view_bytes(views: np.ndarray, heap, i: int):
    """Logical string of view i (None-safe caller) — Appendix C decoding.  `heap` is the data
    buffer, or the list of data buffers indexed by the view's buffer_index."""
    v = views[i]
    n = int(np.frombuffer(v[:4].tobytes(), dtype=np.uint32)[0])
    if n <= 12:
        return v[4: 4 + n].tobytes()
    bi = int(np.frombuffer(v[8:12].tobytes(), dtype=np.uint32)[0])
    off = int(np.frombuffer(v[12:16].tobytes(), dtype=np.uint32)[0])
    buf = heap[bi] if isinstance(heap, list) else heap
    return buf[off: off + n].tobytes()


def filter_canon(a: Array, predicate: Array):
    """compute::filter (compute/filter.rs:23-52) on the CPU: canonical of the selected rows.

    Primitive / Bool: `filter_primitive_slice` (primitive/compute/filter.rs:32-48) and
    bool/compute/filter.rs:15-60 keep the set rows in order; validity.filter the same way.
    Strings: VarBin's filter (varbin/compute/filter.rs:135-200, by index; the by-slice path
    builds the same bytes) appends each selected value to a VarBinBuilder — a null row as an
    empty value — and the result canonicalizes through varbin/flatten.rs (one heap, views by
    vxo_make_views).  FSST's filter (fsst/compute.rs:147-160) filters codes and lengths, whose
    canonical is the same single heap of the selected strings."""
    mask = canon_bool(predicate).astype(bool)
    if predicate.nullable:
        raise ValueError("predicate must be non-nullable bool")
    if len(mask) != a.len:
        raise ValueError("predicate length mismatch")
    if a.dtype in (DTYPE["PRIMITIVE"], DTYPE["BOOL"]):
        vals, valid = canon(a) if a.dtype == DTYPE["PRIMITIVE"] else (canon_bool(a), _validity(a))
        return np.ascontiguousarray(vals[mask]), (None if valid is None else valid[mask])
    (views, heap), valid = canon(a)
    idx = np.nonzero(mask)[0]
    fvalid = None if valid is None else valid[mask]
    strs = []
    for j, i in enumerate(idx):
        strs.append(b"" if (fvalid is not None and not fvalid[j]) else view_bytes(views, heap, int(i)))
    offs = np.zeros(len(strs) + 1, dtype=np.int64)
    if strs:
        offs[1:] = np.cumsum([len(s) for s in strs])
    new_heap = np.frombuffer(b"".join(strs), dtype=np.uint8).copy()
    vbits = None if fvalid is None else np.packbits(fvalid, bitorder="little")
    out = np.zeros((len(strs), 16), dtype=np.uint8)
    O.lib().vxo_make_views(O.p(new_heap), O.p(offs), len(strs), O.p(vbits) if vbits is not None else None, 0,
                           O.p(out))
    return (out, new_heap), fvalid


# ---- slice (SliceFn) of the arrays the reference's slice KATs build: metadata-only, as the
# reference does it (no decode), so the sliced trees exercise the engine's offset handling.
def slice_primitive(a: Array, start: int, stop: int) -> Array:
    """primitive/compute/slice.rs:8-16 (buffer sub-range; validity sliced likewise)."""
    from vortex_amd import arrays as A
    vals = np.ascontiguousarray(a.buffers[0]).view(NP_OF_PTYPE[a.ptype])[start:stop]
    return A.primitive(vals, a.ptype, validity=_slice_validity(a, start, stop))


def slice_sparse(sp: Array, start: int, stop: int) -> Array:
    """sparse/compute/slice.rs:7-21: the indices in [start, stop) found by search_sorted(Left) of
    indices_offset + start / + stop (sparse/mod.rs:123-129); new indices_offset = old + start."""
    from vortex_amd import arrays as A
    off = sp.meta["indices_offset"]
    idx = canon(sp.children[0])[0].astype(np.uint64)
    i0 = int(np.searchsorted(idx, np.uint64(off + start), side="left"))
    i1 = int(np.searchsorted(idx, np.uint64(off + stop), side="left"))
    ind = slice_any(sp.children[0], i0, i1)
    vals = slice_any(sp.children[1], i0, i1)
    fill = None if sp.meta["fill_is_null"] else np.frombuffer(
        sp.meta["fill"][: ptype_width(sp.ptype)], NP_OF_PTYPE[sp.ptype])[0]
    return A.sparse(ind, vals, stop - start, indices_offset=off + start, fill=fill, ptype=sp.ptype)


def slice_bitpacked(a: Array, start: int, stop: int) -> Array:
    """bitpacking/compute/slice.rs:10-43: whole blocks of packed words around [start, stop) of the
    physical positions (offset included), the new offset = physical start % 1024, patches sliced
    and dropped when the slice holds none."""
    from vortex_amd import arrays as A
    W, off0 = a.meta["bit_width"], a.meta["offset"]
    s, e = start + off0, stop + off0
    offset = s % 1024
    block_start, block_stop = s - offset, ((e + 1023) // 1024) * 1024
    packed = np.ascontiguousarray(a.buffers[0]).view(np.uint8)[(block_start // 8) * W: (block_stop // 8) * W]
    patches = None
    if a.meta["has_patches"]:
        sp = slice_sparse(a.children[0], start, stop)
        if sp.children[0].len:
            patches = sp
    return A.bitpacked(packed, a.ptype, W, stop - start, offset, patches, validity=_slice_validity(a, start, stop))


def bad_bitpacked(bp: Array):
    """The three rejections of BitPackedArray::try_new_from_offset (bitpacking/mod.rs:54-130) on a
    one-block (1024-row) BitPacked array -> [(malformed copy, a substring of the error text)]: offset
    1024, a bit width one above the type's, a packed buffer one block short."""
    import dataclasses
    T, W = 8 * ptype_width(bp.ptype), bp.meta["bit_width"]
    assert bp.encoding == ENC["FL_BITPACKED"] and bp.len == 1024 and bp.meta["offset"] == 0 and W > 0
    return [
        (dataclasses.replace(bp, meta=dict(bp.meta, offset=1024)), "Offset must be less than full block"),
        (dataclasses.replace(bp, meta=dict(bp.meta, bit_width=T + 1)), "Unsupported bit width"),
        (dataclasses.replace(bp, buffers=[np.asarray(bp.buffers[0])[:-128 * W]]),
         f"Expected {128 * W} packed bytes, got 0"),
    ]


def misaligned_bitpacked(bp: Array, device) -> Array:
    """`bp` with its packed bytes in device memory 4 bytes past a 16-byte boundary (Array.to keeps a
    device tensor where it lies)."""
    import dataclasses

    import torch
    src = torch.from_numpy(np.ascontiguousarray(bp.buffers[0]).view(np.uint8).copy())
    t = torch.zeros(src.numel() + 16, dtype=torch.uint8, device=device)
    assert t.data_ptr() % 16 == 0
    t[4:4 + src.numel()].copy_(src)
    return dataclasses.replace(bp, buffers=[t[4:4 + src.numel()]])


def _slice_validity(a: Array, start: int, stop: int):
    """Validity::slice (validity.rs): the metadata kinds stay, an Array child is sliced -- a
    BoolArray child by slice_bool (its bit offset moves), any other Bool encoding as its bits."""
    if a.validity == VALIDITY["NON_NULLABLE"]:
        return None
    if a.validity == VALIDITY["ALL_VALID"]:
        return "ALL_VALID"
    if a.validity == VALIDITY["ALL_INVALID"]:
        return "ALL_INVALID"
    child = a.children[-1]
    if child.dtype == DTYPE["BOOL"] and child.encoding == ENC["BOOL"] and child.validity == VALIDITY["NON_NULLABLE"]:
        return slice_bool(child, start, stop)
    return _validity(a)[start:stop]


def slice_bool(a: Array, start: int, stop: int) -> Array:
    """bool/compute/slice.rs:7-15 + BoolArray::try_new (bool/mod.rs:59-82): the bit buffer
    sliced, first_byte_bit_offset = the buffer's bit offset % 8."""
    from vortex_amd import arrays as A
    off = a.meta.get("first_byte_bit_offset", 0)
    bits = canon_bool(a)[start:stop]
    return A.bool_array(bits, validity=_slice_validity(a, start, stop), bit_offset=(off + start) % 8)


def slice_delta(a: Array, start: int, stop: int) -> Array:
    """delta/compute.rs:36-73 (SliceFn::slice, no bounds check -- the reference's jagged "empty"
    KAT slices past the end): whole 1024-value chunks of bases (LANES per chunk, one for the
    remainder) and deltas around the physical range, offset = physical start % 1024."""
    from vortex_amd import arrays as A
    lanes = 1024 // (8 * ptype_width(a.ptype))
    bases, deltas = a.children[0], a.children[1]
    ps, pe = start + a.meta["offset"], stop + a.meta["offset"]
    c0, c1 = ps // 1024, (pe + 1023) // 1024
    nb = bases.len
    nd = a.meta["deltas_len"]
    new_bases = slice_any(bases, min(c0 * lanes, nb), min(c1 * lanes, nb))
    new_deltas = slice_any(deltas, min(c0 * 1024, nd), min(c1 * 1024, nd))
    v = _slice_validity(a, start, stop)
    return A.delta(new_bases, new_deltas, offset=ps % 1024, length=stop - start, validity=v)


def find_physical_index(a: Array, index: int) -> int:
    """RunEndArray::find_physical_index (runend/array.rs:95-98): search_sorted(ends, index +
    offset, Right).to_ends_index(len) (search_sorted.rs:78-85)."""
    ends = canon(a.children[0])[0].astype(np.uint64)
    i = int(np.searchsorted(ends, np.uint64(index + a.meta["offset"]), side="right"))
    return i - 1 if i == ends.size else i


def slice_runend(a: Array, start: int, stop: int) -> Array:
    """runend/compute.rs:104-119: ends and values [begin, end + 1) of the runs holding start and
    stop, validity sliced, offset = start + old offset, len = stop - start."""
    from vortex_amd import arrays as A
    b, e = find_physical_index(a, start), find_physical_index(a, stop)
    return A.run_end(slice_any(a.children[0], b, e + 1), slice_any(a.children[1], b, e + 1),
                     length=stop - start, offset=start + a.meta["offset"],
                     validity=_slice_validity(a, start, stop))


def slice_varbinview(a: Array, start: int, stop: int) -> Array:
    """varbinview/compute.rs:49-65: views [start, stop) (16 bytes each), every data buffer kept,
    validity sliced."""
    from vortex_amd import arrays as A
    views = _buf(a.children[0].buffers[0])[16 * start: 16 * stop]
    bufs = [_buf(c.buffers[0]) for c in a.children[1: 1 + a.meta["n_buffers"]]]
    return A.varbinview(views, bufs, utf8=a.dtype == DTYPE["UTF8"], validity=_slice_validity(a, start, stop))


def slice_for(a: Array, start: int, stop: int) -> Array:
    """fastlanes/src/for/compute.rs:87-96: the encoded child sliced, reference and shift kept."""
    from vortex_amd import arrays as A
    ref = int(np.array([a.meta["reference"]], dtype=NP_OF_PTYPE[unsigned_of(a.ptype)]).view(NP_OF_PTYPE[a.ptype])[0])
    return A.frame_of_reference(slice_any(a.children[0], start, stop), ref, a.meta["shift"], a.ptype)


def slice_zigzag(a: Array, start: int, stop: int) -> Array:
    """zigzag/src/compute.rs:68-72: the encoded child sliced."""
    from vortex_amd import arrays as A
    return A.zigzag(slice_any(a.children[0], start, stop))


def slice_alp(a: Array, start: int, stop: int) -> Array:
    """alp/src/alp/compute.rs:73-82: the encoded child sliced, the exponents kept, the patches
    sliced as a SparseArray (kept even when the slice holds none of them)."""
    from vortex_amd import arrays as A
    patches = slice_any(a.children[1], start, stop) if a.meta["has_patches"] else None
    return A.alp(slice_any(a.children[0], start, stop), a.meta["e"], a.meta["f"], patches)


def slice_dict(a: Array, start: int, stop: int) -> Array:
    """dict/src/compute.rs:60-65: the codes sliced, the values kept whole."""
    from vortex_amd import arrays as A
    return A.dict_array(a.children[0], slice_any(a.children[1], start, stop))


def find_chunk_idx(a: Array, index: int) -> tuple[int, int]:
    """ChunkedArray::find_chunk_idx (array/chunked/mod.rs:106-121): search_sorted(chunk_offsets,
    index, Right).to_ends_index(nchunks + 1) - 1 (saturating): of several chunks that start at
    `index` (empty ones before it) the last."""
    offs = np.ascontiguousarray(a.children[0].buffers[0]).view(np.uint64)
    i = int(np.searchsorted(offs, np.uint64(index), side="right"))
    i = max((i - 1 if i == offs.size else i) - 1, 0)
    return i, index - int(offs[i])


def slice_chunked(a: Array, start: int, stop: int) -> Array:
    """array/chunked/compute/slice.rs:7-36: the chunks holding start and stop and those between;
    the first sliced from start to its end, the last up to stop -- or dropped when stop is its
    first row; one chunk holding both is sliced once."""
    from vortex_amd import arrays as A
    c0, in0 = find_chunk_idx(a, start)
    c1, in1 = find_chunk_idx(a, stop)
    chunks = a.children[1:]
    if c0 == c1:
        return A.chunked([slice_any(chunks[c0], in0, in1)])
    out = list(chunks[c0: c1 + 1])
    out[0] = slice_any(out[0], in0, out[0].len)
    if in1 == 0:
        out.pop()
    else:
        out[-1] = slice_any(out[-1], 0, in1)
    return A.chunked(out)


def slice_any(a: Array, start: int, stop: int) -> Array:
    """SliceFn restatements: the encodings the reference's slice KATs build, and FoR, ZigZag, ALP,
    Dict and Chunked for the seeded trees of tests/tree_cases.py -- metadata only, nothing decoded."""
    if a.encoding == ENC["FL_FOR"]:
        return slice_for(a, start, stop)
    if a.encoding == ENC["ZIGZAG"]:
        return slice_zigzag(a, start, stop)
    if a.encoding == ENC["ALP"]:
        return slice_alp(a, start, stop)
    if a.encoding == ENC["DICT"]:
        return slice_dict(a, start, stop)
    if a.encoding == ENC["CHUNKED"]:
        return slice_chunked(a, start, stop)
    if a.encoding == ENC["FL_BITPACKED"]:
        return slice_bitpacked(a, start, stop)
    if a.encoding == ENC["PRIMITIVE"]:
        return slice_primitive(a, start, stop)
    if a.encoding == ENC["SPARSE"]:
        return slice_sparse(a, start, stop)
    if a.encoding == ENC["FL_DELTA"]:
        return slice_delta(a, start, stop)
    if a.encoding == ENC["RUN_END"]:
        return slice_runend(a, start, stop)
    if a.encoding == ENC["VARBINVIEW"]:
        return slice_varbinview(a, start, stop)
    if a.encoding == ENC["BOOL"]:
        return slice_bool(a, start, stop)
    raise NotImplementedError(f"slice of encoding {a.encoding}")


def slice_checked(a: Array, start: int, stop: int) -> Array:
    """compute::slice (compute/slice.rs:21-48): bounds checked, then SliceFn."""
    if start > a.len or stop > a.len:
        raise IndexError(f"OutOfBounds: {max(start, stop)} not in [0, {a.len}]")
    if start > stop:
        raise ValueError(f"start ({start}) must be <= stop ({stop})")
    return slice_any(a, start, stop)


def sparse_take(sp: Array, indices) -> Array:
    """SparseArray's TakeFn (sparse/compute/take.rs:13-86): positions of the taken indices that
    hit a patch and the patch values at them, as a new SparseArray of len(indices) with the same
    fill (take_search_sorted; take_map gives the same pairs above 128 indices)."""
    from vortex_amd import arrays as A
    off = sp.meta["indices_offset"]
    resolved = canon(sp.children[0])[0].astype(np.int64) - off
    vals, vvalid = canon(sp.children[1])
    pos, phys = [], []
    lo = int(resolved.min()) if resolved.size else 0
    hi = int(resolved.max()) if resolved.size else 0
    for p, i in enumerate(np.asarray(indices, dtype=np.int64).tolist()):
        if i < lo or i > hi:
            continue
        j = int(np.searchsorted(resolved, i, side="left"))
        if j < resolved.size and resolved[j] == i:
            pos.append(p)
            phys.append(j)
    pv = vals[np.array(phys, dtype=np.int64)]
    pvalid = None if vvalid is None else vvalid[np.array(phys, dtype=np.int64)]
    fill = None if sp.meta["fill_is_null"] else np.frombuffer(
        sp.meta["fill"][: ptype_width(sp.ptype)], NP_OF_PTYPE[sp.ptype])[0]
    return A.sparse(A.primitive(np.array(pos, dtype=np.uint64)),
                    A.primitive(pv, sp.children[1].ptype,
                                validity=None if not sp.children[1].nullable else
                                ("ALL_VALID" if pvalid is None else pvalid)),
                    len(np.asarray(indices)), fill=fill, ptype=sp.ptype)
