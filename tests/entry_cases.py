"""Cases for the per-encoding C entry points (include/vortex_gpu.h, "per-encoding kernels").

Plain module: numpy, the host encoders (vortex_amd.encode) and the CPU oracle -- no GPU, no torch.
For every entry point `cases(entry)` yields named cases.  A case holds

  bufs    the device inputs as numpy arrays (uploaded as they are),
  args    the scalar arguments,
  outs    the caller-allocated outputs: size, initial contents, and the bytes the matching vxo_*
          function of the oracle wrote (`want`),
  plain   per output, an independent plain-numpy statement of the same operation (what
          tests/test_entry_cases.py holds the oracle's bytes against),
  error   where the call must be rejected: the status name, and whether the call itself returns
          it ("call") or the next vxg_stream_sync ("sync"); `oracle_rc` is what the oracle
          returned for the same arguments (-1 = its own error) where it has an equivalent.

tests/test_gpu_entry_points.py uploads, calls and compares byte for byte.
"""
from __future__ import annotations

import ctypes as C
import functools
import itertools
from dataclasses import dataclass, field
from typing import Optional

import numpy as np

import vortex_amd.encode as E
from oracle import oracle as O
from vortex_amd._lib import VxeFsstTable

INT_PTYPES = ["u8", "u16", "u32", "u64", "i8", "i16", "i32", "i64"]
UNSIGNED = ["u8", "u16", "u32", "u64"]
SIGNED = ["i8", "i16", "i32", "i64"]
U_OF_BITS = {8: "u8", 16: "u16", 32: "u32", 64: "u64"}
VALUE_WIDTHS = [1, 2, 4, 8, 16]
FILL = 0xCD  # what an output holds before the call unless a case says otherwise


def width(pt: str) -> int:
    return np.dtype(O.NP[pt]).itemsize


def unsigned_of(pt: str) -> str:
    return U_OF_BITS[8 * width(pt)]


def n_set(elem_bytes: int) -> list[int]:
    """Vector body, scalar tail and workgroup edge of the 16-byte-per-lane elementwise kernels."""
    v = max(16 // elem_bytes, 1)
    return sorted({0, 1, v - 1, v, v + 1, 255, 256, 257, 1023, 1024, 1025, 4097})


@dataclass
class Out:
    nbytes: int
    want: Optional[bytes] = None   # the oracle's bytes (None: only the guards are checked)
    init: Optional[bytes] = None   # contents before the call (None: FILL)
    slack: int = 0                 # bytes after nbytes the entry point may scribble on (FSST heap)
    shift: int = 0                 # byte offset of the pointer from a 16-byte boundary


@dataclass
class Case:
    entry: str
    name: str
    bufs: dict = field(default_factory=dict)
    args: dict = field(default_factory=dict)
    outs: dict = field(default_factory=dict)
    plain: dict = field(default_factory=dict)
    error: Optional[str] = None
    at: str = "call"
    oracle_rc: Optional[int] = None
    shift_in: dict = field(default_factory=dict)  # input name -> byte offset from a 16-byte boundary
    inplace: Optional[str] = None                 # the input that IS the output "out"


def _seed(*key) -> np.random.Generator:
    # (hash() of a str changes between interpreter runs: seed from the characters instead)
    flat = []
    for k in key:
        flat += [ord(c) for c in k] if isinstance(k, str) else [int(k)]
    return np.random.default_rng(flat or [0])


def rand_bits(r, n: int, bits: int, dtype) -> np.ndarray:
    if bits == 0:
        return np.zeros(n, dtype=dtype)
    return r.integers(0, 1 << bits, n, dtype=np.uint64).astype(dtype)


def pack(vals: np.ndarray, W: int, offset: int, r) -> np.ndarray:
    """The FastLanes buffer of a BitPacked array sliced at `offset`: `offset` other values of
    the same width, then vals (vortex_amd.encode.bitpack_buffer = bitpack_primitive)."""
    bits = 8 * vals.dtype.itemsize
    full = np.concatenate([rand_bits(r, offset, W, vals.dtype), vals]) if offset else vals
    assert full.dtype == vals.dtype and (W == bits or W == 0 or int(full.max(initial=0)) < (1 << W))
    return E.bitpack_buffer(full, W).copy() if W else np.zeros(0, np.uint8)


def o_unpack(upt: str, W: int, offset: int, n: int, packed: np.ndarray, packed_bytes=None):
    out = np.zeros(n, dtype=O.NP[upt])
    rc = O.lib().vxo_unpack(O.PT[upt], W, offset, n, O.p(packed), packed.size if packed_bytes is None else packed_bytes,
                            O.p(out))
    return rc, out


def o_for(pt: str, x: np.ndarray, ref: int, shift: int) -> np.ndarray:
    out = np.zeros_like(x)
    O.lib().vxo_for_decode(O.PT[pt], O.p(x), x.size, ref, shift, O.p(out))
    return out


def o_zigzag(spt: str, x: np.ndarray) -> np.ndarray:
    out = np.zeros_like(x)
    O.lib().vxo_zigzag_decode(O.PT[spt], O.p(x), x.size, O.p(out))
    return out


def np_for(x: np.ndarray, ref: int, shift: int) -> np.ndarray:
    u = x.dtype.type
    return (x << u(shift)) + u(ref)  # uint arrays wrap


def np_zigzag(x: np.ndarray) -> np.ndarray:
    u = x.dtype.type
    return (x >> u(1)) ^ (u(0) - (x & u(1)))


def wrap_ref(bits: int) -> int:
    return (1 << bits) - 3  # -3: every value >= 3 wraps


# ------------------------------------------------------------------ BitPacked family
def _w_set(T: int) -> list[int]:
    return [0, 1, T // 2 + 1, T - 1, T]


def cases_bitunpack():
    for pt in INT_PTYPES:
        T, upt = 8 * width(pt), unsigned_of(pt)
        for W, offset, n in itertools.product(_w_set(T), [0, 1023], [1, 1025, 2049]):
            r = _seed("bitunpack", pt, W, offset, n)
            x = rand_bits(r, n, W, O.NP[upt])
            packed = pack(x, W, offset, r)
            rc, got = o_unpack(upt, W, offset, n, packed)
            yield Case("vxg_bitunpack", f"{pt}-W{W}-o{offset}-n{n}", {"packed": packed},
                       dict(ptype=pt, W=W, offset=offset, len=n, packed_bytes=packed.size),
                       {"out": Out(n * width(pt), got.tobytes())}, {"out": x.tobytes()}, oracle_rc=rc)
    r = _seed("bitunpack-bad")
    x = rand_bits(r, 1025, 7, np.uint32)
    packed = pack(x, 7, 0, r)
    rc, _ = o_unpack("u32", 7, 0, 3000, packed)  # three blocks wanted, two given
    yield Case("vxg_bitunpack", "packed-length", {"packed": packed},
               dict(ptype="u32", W=7, offset=0, len=3000, packed_bytes=packed.size),
               {"out": Out(3000 * 4)}, error="InvalidArgument", oracle_rc=rc)
    yield Case("vxg_bitunpack", "float-ptype", {"packed": packed},
               dict(ptype="f32", W=7, offset=0, len=1025, packed_bytes=packed.size),
               {"out": Out(1025 * 4)}, error="MismatchedTypes")


def cases_bitunpack_for():
    for pt in INT_PTYPES:
        T, upt = 8 * width(pt), unsigned_of(pt)
        for zz in ([0, 1] if pt in SIGNED else [0]):
            for W, offset, shift, n in itertools.product(_w_set(T), [0, 1, 1023], [0, 1, T - 1], [1, 1024, 1025, 2049]):
                r = _seed("bitunpack_for", pt, zz, W, offset, shift, n)
                x = rand_bits(r, n, W, O.NP[upt])
                packed = pack(x, W, offset, r)
                ref = wrap_ref(T)
                rc, u = o_unpack(upt, W, offset, n, packed)
                got = o_for(pt, u, ref, shift)
                plain = np_for(x, ref, shift)
                if zz:
                    got, plain = o_zigzag(pt, got), np_zigzag(plain)
                yield Case("vxg_bitunpack_for", f"{pt}-zz{zz}-W{W}-o{offset}-s{shift}-n{n}", {"packed": packed},
                           dict(ptype=pt, W=W, offset=offset, len=n, packed_bytes=packed.size, reference=ref,
                                shift=shift, zigzag=zz),
                           {"out": Out(n * width(pt), got.tobytes())}, {"out": plain.tobytes()}, oracle_rc=rc)
    for pt in INT_PTYPES:  # shift >= bits of the type: undefined in `e << shift`
        T = 8 * width(pt)
        r = _seed("bitunpack_for-shift", pt)
        packed = pack(rand_bits(r, 5, 3, O.NP[unsigned_of(pt)]), 3, 0, r)
        for shift in (T, T + 1, 255):
            yield Case("vxg_bitunpack_for", f"{pt}-shift{shift}", {"packed": packed},
                       dict(ptype=pt, W=3, offset=0, len=5, packed_bytes=packed.size, reference=1, shift=shift,
                            zigzag=0), {"out": Out(5 * width(pt))}, error="InvalidArgument")
    yield Case("vxg_bitunpack_for", "offset-1024", {"packed": packed},
               dict(ptype="i64", W=3, offset=1024, len=5, packed_bytes=packed.size, reference=1, shift=0, zigzag=0),
               {"out": Out(40)}, error="InvalidArgument")


_IF10 = {"f32": [np.float32(f"1e-{i}") for i in range(11)], "f64": [np.float64(f"1e-{i}") for i in range(24)]}
_F10 = {"f32": [np.float32(f"1e{i}") for i in range(11)], "f64": [np.float64(f"1e{i}") for i in range(24)]}


def o_alp(fpt: str, enc: np.ndarray, e: int, f: int) -> np.ndarray:
    out = np.zeros(enc.size, dtype=O.NP[fpt])
    fn = O.lib().vxo_alp_decode_f32 if fpt == "f32" else O.lib().vxo_alp_decode_f64
    fn(O.p(enc), enc.size, e, f, O.p(out))
    return out


def np_alp(fpt: str, enc: np.ndarray, e: int, f: int) -> np.ndarray:
    """decode_single (alp/mod.rs:161-163): (v as F) * F10[f] * IF10[e], each product rounded."""
    ft = O.NP[fpt]
    return (enc.astype(ft) * _F10[fpt][f]) * _IF10[fpt][e]


_ALP_EF = {"f32": [(0, 0), (5, 2), (10, 10), (10, 0)], "f64": [(0, 0), (14, 3), (23, 23), (23, 0)]}


def cases_bitunpack_alp():
    for fpt, ipt in (("f32", "i32"), ("f64", "i64")):
        T, upt = 8 * width(fpt), unsigned_of(fpt)
        for (e, f), shift, offset, n in itertools.product(_ALP_EF[fpt], [0, 1], [0, 7], [1, 1025, 2049]):
            r = _seed("bitunpack_alp", fpt, e, f, shift, offset, n)
            v = (r.integers(-5000, 5000, n, dtype=np.int64) << shift).astype(O.NP[ipt])  # the ALP-encoded values
            v[0] = -5000 << shift
            ref = int(v.min())  # negative: the FoR reference's add wraps back below zero
            x = ((v - O.NP[ipt](ref)).view(O.NP[upt])) >> O.NP[upt](shift)
            W = int(x.max()).bit_length()
            packed = pack(x, W, offset, r)
            rc, u = o_unpack(upt, W, offset, n, packed)
            dec = o_for(ipt, u, ref & ((1 << T) - 1), shift).view(O.NP[ipt])
            got = o_alp(fpt, dec, e, f)
            yield Case("vxg_bitunpack_alp", f"{fpt}-e{e}-f{f}-s{shift}-o{offset}-n{n}", {"packed": packed},
                       dict(ptype=fpt, W=W, offset=offset, len=n, packed_bytes=packed.size,
                            reference=ref & ((1 << T) - 1), shift=shift, e=e, f=f),
                       {"out": Out(n * width(fpt), got.tobytes())}, {"out": np_alp(fpt, v, e, f).tobytes()},
                       oracle_rc=rc)
    r = _seed("bitunpack_alp-bad")
    packed = pack(rand_bits(r, 9, 5, np.uint32), 5, 0, r)
    base = dict(ptype="f32", W=5, offset=0, len=9, packed_bytes=packed.size, reference=0, shift=0, e=3, f=1)
    for name, over, err in (("shift32", dict(shift=32), "InvalidArgument"), ("e11", dict(e=11), "InvalidArgument"),
                            ("f11", dict(f=11), "InvalidArgument"), ("int-ptype", dict(ptype="i32"), "MismatchedTypes")):
        yield Case("vxg_bitunpack_alp", name, {"packed": packed}, {**base, **over}, {"out": Out(36)}, error=err)
    packed64 = pack(rand_bits(r, 9, 5, np.uint64), 5, 0, r)
    yield Case("vxg_bitunpack_alp", "f64-shift64", {"packed": packed64},
               {**base, "ptype": "f64", "packed_bytes": packed64.size, "shift": 64}, {"out": Out(72)},
               error="InvalidArgument")
    yield Case("vxg_bitunpack_alp", "f64-e24", {"packed": packed64},
               {**base, "ptype": "f64", "packed_bytes": packed64.size, "e": 24}, {"out": Out(72)},
               error="InvalidArgument")


def o_take(vw: int, values: np.ndarray, n_values: int, cpt: str, codes: np.ndarray):
    out = np.zeros(codes.size * vw, dtype=np.uint8)
    rc = O.lib().vxo_take(vw, O.p(values), n_values, O.PT[cpt], O.p(codes), codes.size, O.p(out))
    return rc, out


def np_take(vw: int, values: np.ndarray, codes: np.ndarray) -> np.ndarray:
    return values.reshape(-1, vw)[codes.astype(np.int64)]


def cases_bitunpack_dict():
    for cpt, W in itertools.product(["u8", "u16", "u32"], [1, 8, 16]):
        if W > 8 * width(cpt):
            continue
        for vw, dlen, n, offset in itertools.product(VALUE_WIDTHS, sorted({1, 2, 1 << W}), [1, 2049], [0, 5]):
            r = _seed("bitunpack_dict", cpt, W, vw, dlen, n, offset)
            codes = r.integers(0, dlen, n, dtype=np.uint64).astype(O.NP[cpt])
            codes[-1] = dlen - 1
            values = r.integers(0, 256, dlen * vw, dtype=np.uint8)
            packed = pack(codes, W, offset, r)
            rc, u = o_unpack(cpt, W, offset, n, packed)
            rc2, got = o_take(vw, values, dlen, cpt, u)
            yield Case("vxg_bitunpack_dict", f"{cpt}-W{W}-vw{vw}-d{dlen}-n{n}-o{offset}",
                       {"packed": packed, "dict": values},
                       dict(ptype=cpt, W=W, offset=offset, len=n, packed_bytes=packed.size, dict_len=dlen, vw=vw),
                       {"out": Out(n * vw, got.tobytes())}, {"out": np_take(vw, values, codes).tobytes()},
                       oracle_rc=rc | rc2)
    r = _seed("bitunpack_dict-bad")
    codes = r.integers(0, 2, 1500, dtype=np.uint16)
    values = r.integers(0, 256, 2 * 4, dtype=np.uint8)
    packed = pack(codes, 8, 0, r)
    base = dict(ptype="u16", W=8, offset=0, len=1500, packed_bytes=packed.size, dict_len=2, vw=4)
    bufs = {"packed": packed, "dict": values}
    for vw in (0, 3, 32):  # 0 divided by zero in the output alignment check
        yield Case("vxg_bitunpack_dict", f"value-width-{vw}", bufs, {**base, "vw": vw}, {"out": Out(1500 * 16)},
                   error="InvalidArgument")
    yield Case("vxg_bitunpack_dict", "empty-dict", bufs, {**base, "dict_len": 0}, {"out": Out(6000)},
               error="OutOfBounds", oracle_rc=o_take(4, values, 0, "u16", codes)[0])
    yield Case("vxg_bitunpack_dict", "signed-codes", bufs, {**base, "ptype": "i16"}, {"out": Out(6000)},
               error="MismatchedTypes")
    p17 = pack(rand_bits(r, 10, 17, np.uint32), 17, 0, r)
    yield Case("vxg_bitunpack_dict", "W17", {"packed": p17, "dict": values},
               dict(ptype="u32", W=17, offset=0, len=10, packed_bytes=p17.size, dict_len=2, vw=4), {"out": Out(40)},
               error="NotImplemented")
    bad = codes.copy()
    bad[777] = 2  # == dict_len
    pbad = pack(bad, 8, 0, r)
    yield Case("vxg_bitunpack_dict", "code-eq-dict-len", {"packed": pbad, "dict": values}, base, {"out": Out(6000)},
               error="OutOfBounds", at="sync", oracle_rc=o_take(4, values, 2, "u16", bad)[0])


def cases_bitunpack_dict_chunks():
    lens = [1, 1023, 1024, 1025, 3000]
    for vw, cpt, W in ((1, "u8", 3), (4, "u16", 9), (16, "u32", 16)):
        for nch in (0, 1, 5):
            r = _seed("dict_chunks", vw, nch)
            bufs, chunks, want, plain, pos = {}, [], [], [], 0
            for i in range(nch):
                n = lens[(i + (nch == 1) * 3) % 5]  # a single chunk: 1025
                dlen = [1, 2, 1 << W, 300, 7][i] if (1 << W) >= 300 else [1, 2, 1 << W, 5, 7][i]
                codes = r.integers(0, dlen, n, dtype=np.uint64).astype(O.NP[cpt])
                values = r.integers(0, 256, dlen * vw, dtype=np.uint8)
                bufs[f"packed{i}"], bufs[f"dict{i}"] = pack(codes, W, 0, r), values
                rc, u = o_unpack(cpt, W, 0, n, bufs[f"packed{i}"])
                rc2, got = o_take(vw, values, dlen, cpt, u)
                assert rc == 0 and rc2 == 0
                want.append(got.tobytes())
                plain.append(np_take(vw, values, codes).tobytes())
                chunks.append(dict(len=n, dict_len=dlen, out_offset=pos, n_blocks=(n + 1023) // 1024))
                pos += n * vw
            yield Case("vxg_bitunpack_dict_chunks", f"vw{vw}-{cpt}-W{W}-chunks{nch}", bufs,
                       dict(ptype=cpt, W=W, vw=vw, chunks=chunks), {"out": Out(pos, b"".join(want))},
                       {"out": b"".join(plain)}, oracle_rc=0)
    r = _seed("dict_chunks-bad")
    codes = r.integers(0, 4, 1500, dtype=np.uint16)
    bufs = {"packed0": pack(codes, 9, 0, r), "dict0": r.integers(0, 256, 16, dtype=np.uint8)}
    ch = dict(len=1500, dict_len=4, out_offset=0, n_blocks=2)
    base = dict(ptype="u16", W=9, vw=4, chunks=[ch])
    yield Case("vxg_bitunpack_dict_chunks", "n-blocks", bufs, {**base, "chunks": [{**ch, "n_blocks": 3}]},
               {"out": Out(6000)}, error="InvalidArgument")
    for vw in (0, 3):
        yield Case("vxg_bitunpack_dict_chunks", f"value-width-{vw}", bufs, {**base, "vw": vw}, {"out": Out(6000)},
                   error="InvalidArgument")
    yield Case("vxg_bitunpack_dict_chunks", "W17", bufs, {**base, "ptype": "u32", "W": 17}, {"out": Out(6000)},
               error="NotImplemented")


# ------------------------------------------------------------------ patch
def cases_patch():
    for vpt, ipt, ioff, npatch, order in itertools.product(["u8", "i16", "f32", "f64"], INT_PTYPES, [0, 7], [0, 1, 257],
                                                          ["sorted", "unsorted"]):
        r = _seed("patch", vpt, ipt, ioff, npatch, order)
        imax = int(np.iinfo(O.NP[ipt]).max)
        out_len = min(300, imax + 1 - ioff)   # every position must be reachable by an index of ipt
        npt = min(npatch, out_len)            # (no duplicates: 8-bit index types hold fewer than 257)
        pos = r.permutation(out_len)[:npt]
        if order == "sorted":
            pos = np.sort(pos)
        idx = (pos + ioff).astype(O.NP[ipt])
        w = width(vpt)
        vals = r.integers(0, 256, npt * w, dtype=np.uint8)
        init = r.integers(0, 256, out_len * w, dtype=np.uint8)
        got = init.copy()
        rc = O.lib().vxo_patch(O.PT[vpt], O.p(got), out_len, O.PT[ipt], O.p(idx), ioff, O.p(vals), npt)
        plain = init.copy().reshape(out_len, w)
        plain[pos] = vals.reshape(npt, w)
        yield Case("vxg_patch", f"{vpt}-{ipt}-off{ioff}-n{npatch}-{order}", {"indices": idx, "values": vals},
                   dict(ptype=vpt, out_len=out_len, indices_ptype=ipt, indices_offset=ioff, n_patches=npt),
                   {"out": Out(out_len * w, got.tobytes(), init.tobytes())}, {"out": plain.tobytes()}, oracle_rc=rc)
    for ipt, bad in itertools.product(["u16", "i16", "u64", "i64"], ["below-offset", "at-end"]):
        r = _seed("patch-oob", ipt, bad)
        out_len, ioff = 300, 7
        idx = (np.sort(r.permutation(out_len)[:40]) + ioff).astype(O.NP[ipt])
        idx[11] = 3 if bad == "below-offset" else out_len + ioff
        vals = r.integers(0, 256, 40 * 4, dtype=np.uint8)
        init = np.zeros(out_len * 4, np.uint8)
        tmp = init.copy()
        rc = O.lib().vxo_patch(O.PT["u32"], O.p(tmp), out_len, O.PT[ipt], O.p(idx), ioff, O.p(vals), 40)
        yield Case("vxg_patch", f"{ipt}-{bad}", {"indices": idx, "values": vals},
                   dict(ptype="u32", out_len=out_len, indices_ptype=ipt, indices_offset=ioff, n_patches=40),
                   {"out": Out(out_len * 4, None, init.tobytes())}, error="OutOfBounds", at="sync", oracle_rc=rc)
    # a negative index is a huge usize (sparse/mod.rs:132-144 `as usize`): out of bounds, although its
    # bits read as unsigned (255, 65535) are a position of this output.  It comes last, so the
    # oracle has applied every other patch when it stops, as the kernel does in any order.
    for ipt, out_len in (("i8", 300), ("i16", 70_000)):
        r = _seed("patch-neg", ipt)
        idx = np.array([5, 100, 9, -1], dtype=O.NP[ipt])
        vals = r.integers(1, 256, 4, dtype=np.uint8)
        got = np.zeros(out_len, np.uint8)
        rc = O.lib().vxo_patch(O.PT["u8"], O.p(got), out_len, O.PT[ipt], O.p(idx), 0, O.p(vals), 4)
        assert rc == -1 and np.count_nonzero(got) == 3
        yield Case("vxg_patch", f"{ipt}-negative", {"indices": idx, "values": vals},
                   dict(ptype="u8", out_len=out_len, indices_ptype=ipt, indices_offset=0, n_patches=4),
                   {"out": Out(out_len, got.tobytes(), bytes(out_len))}, error="OutOfBounds", at="sync", oracle_rc=rc)
    yield Case("vxg_patch", "float-indices", {"indices": np.zeros(3, np.float32), "values": vals},
               dict(ptype="u8", out_len=100, indices_ptype="f32", indices_offset=0, n_patches=3),
               {"out": Out(100, None, bytes(100))}, error="InvalidArgument")


# ------------------------------------------------------------------ FoR / ZigZag / ALP (standalone)
def cases_for_decode():
    for pt in INT_PTYPES:
        T, upt = 8 * width(pt), unsigned_of(pt)
        for k, (n, inplace) in enumerate(itertools.product(n_set(width(pt)), [False, True])):
            shift = [0, 1, T - 1][k % 3]
            r = _seed("for_decode", pt, n, inplace)
            x = rand_bits(r, n, T, O.NP[upt])
            ref = wrap_ref(T)
            got = o_for(pt, x, ref, shift)
            yield Case("vxg_for_decode", f"{pt}-n{n}-s{shift}-{'inplace' if inplace else 'copy'}", {"in": x},
                       dict(ptype=pt, n=n, reference=ref, shift=shift),
                       {"out": Out(n * width(pt), got.tobytes(), x.tobytes() if inplace else None)},
                       {"out": np_for(x, ref, shift).tobytes()}, oracle_rc=0, inplace="in" if inplace else None)
    for pt in INT_PTYPES:
        T, w = 8 * width(pt), width(pt)
        x = np.arange(40, dtype=O.NP[unsigned_of(pt)])
        base = dict(ptype=pt, n=40, reference=1, shift=0)
        for shift in (T, 200):
            yield Case("vxg_for_decode", f"{pt}-shift{shift}", {"in": x}, {**base, "shift": shift}, {"out": Out(40 * w)},
                       error="InvalidArgument")
        if w < 16:  # a tensor sliced by one element
            yield Case("vxg_for_decode", f"{pt}-misaligned-in", {"in": x}, base, {"out": Out(40 * w)},
                       error="InvalidArgument", shift_in={"in": w})
            yield Case("vxg_for_decode", f"{pt}-misaligned-out", {"in": x}, base, {"out": Out(40 * w, shift=w)},
                       error="InvalidArgument")
    yield Case("vxg_for_decode", "float-ptype", {"in": np.zeros(8, np.uint32)}, dict(ptype="f32", n=8, reference=1, shift=0),
               {"out": Out(32)}, error="MismatchedTypes")


def cases_zigzag_decode():
    for pt in SIGNED:
        T, upt = 8 * width(pt), unsigned_of(pt)
        for n in n_set(width(pt)):
            r = _seed("zigzag", pt, n)
            x = rand_bits(r, n, T, O.NP[upt])
            ext = np.array([0, 1, (1 << T) - 1, (1 << T) - 2], dtype=np.uint64).astype(O.NP[upt])
            x[: min(n, 4)] = ext[: min(n, 4)]
            if n >= 8:
                x[n - 4:] = ext  # the extremes in the scalar tail as well
            got = o_zigzag(pt, x)
            plain = np_zigzag(x)
            if n >= 4:  # 0 -> 0, 1 -> -1, max -> min, max - 1 -> max (zigzag 0.1.0)
                info = np.iinfo(O.NP[pt])
                assert plain.view(O.NP[pt])[:4].tolist() == [0, -1, info.min, info.max]
            yield Case("vxg_zigzag_decode", f"{pt}-n{n}", {"in": x}, dict(ptype=pt, n=n),
                       {"out": Out(n * width(pt), got.tobytes())}, {"out": plain.tobytes()}, oracle_rc=0)
    for pt in UNSIGNED + ["f32"]:
        yield Case("vxg_zigzag_decode", f"{pt}-out-ptype", {"in": np.zeros(16, O.NP[pt])}, dict(ptype=pt, n=16),
                   {"out": Out(16 * width(pt))}, error="MismatchedTypes")
    yield Case("vxg_zigzag_decode", "misaligned-in", {"in": np.zeros(16, np.uint32)}, dict(ptype="i32", n=16),
               {"out": Out(64)}, error="InvalidArgument", shift_in={"in": 4})


def cases_alp_decode():
    for fpt, ipt in (("f32", "i32"), ("f64", "i64")):
        for k, n in enumerate(n_set(width(fpt))):
            for e, f in _ALP_EF[fpt]:
                r = _seed("alp", fpt, n, e, f)
                info = np.iinfo(O.NP[ipt])
                enc = r.integers(-(10 ** 7), 10 ** 7, n, dtype=np.int64).astype(O.NP[ipt])
                ext = np.array([0, -1, info.min, info.max], dtype=np.int64).astype(O.NP[ipt])
                enc[: min(n, 4)] = ext[: min(n, 4)]
                got = o_alp(fpt, enc, e, f)
                yield Case("vxg_alp_decode", f"{fpt}-n{n}-e{e}-f{f}", {"encoded": enc}, dict(ptype=fpt, n=n, e=e, f=f),
                           {"out": Out(n * width(fpt), got.tobytes())}, {"out": np_alp(fpt, enc, e, f).tobytes()},
                           oracle_rc=0)
    enc = np.arange(8, dtype=np.int32)
    enc64 = np.arange(8, dtype=np.int64)
    for name, bufs, args, err in (
            ("f32-e11", enc, dict(ptype="f32", n=8, e=11, f=0), "InvalidArgument"),
            ("f32-f11", enc, dict(ptype="f32", n=8, e=3, f=11), "InvalidArgument"),
            ("f64-e24", enc64, dict(ptype="f64", n=8, e=24, f=0), "InvalidArgument"),
            ("f64-f24", enc64, dict(ptype="f64", n=8, e=3, f=24), "InvalidArgument"),
            ("i32-ptype", enc, dict(ptype="i32", n=8, e=3, f=1), "MismatchedTypes"),
            ("f16-ptype", enc, dict(ptype="f16", n=8, e=3, f=1), "MismatchedTypes"),
            ("i64-ptype-n0", enc64, dict(ptype="i64", n=0, e=3, f=1), "MismatchedTypes")):
        yield Case("vxg_alp_decode", name, {"encoded": bufs}, args, {"out": Out(64)}, error=err)
    yield Case("vxg_alp_decode", "misaligned-in", {"encoded": enc}, dict(ptype="f32", n=8, e=3, f=1), {"out": Out(32)},
               error="InvalidArgument", shift_in={"encoded": 4})
    yield Case("vxg_alp_decode", "misaligned-out", {"encoded": enc64}, dict(ptype="f64", n=8, e=3, f=1),
               {"out": Out(64, shift=8)}, error="InvalidArgument")


# ------------------------------------------------------------------ ALP-RD
def o_alprd(fpt, left, d, rbw, right, pos, exc):
    out = np.zeros(left.size, dtype=O.NP[fpt])
    fn = O.lib().vxo_alprd_decode_checked_f32 if fpt == "f32" else O.lib().vxo_alprd_decode_checked_f64
    rc = fn(O.p(left), O.p(d), d.size, rbw, O.p(right), left.size, O.p(pos), O.p(exc), pos.size, O.p(out))
    return rc, out


def _alprd_inputs(r, fpt, rbw, dlen, nexc, n):
    ut = O.NP[unsigned_of(fpt)]
    left = r.integers(0, dlen, n, dtype=np.uint16)
    d = r.integers(0, 1 << 16, dlen, dtype=np.uint16)
    right = rand_bits(r, n, rbw, ut)
    pos = np.sort(r.permutation(n)[:nexc]).astype(np.uint64)
    exc = r.integers(0, 1 << 16, pos.size, dtype=np.uint16)
    return left, d, right, pos, exc


def cases_alprd_decode():
    for fpt, rbws in (("f32", [1, 16, 31]), ("f64", [1, 48, 63])):
        ut = O.NP[unsigned_of(fpt)]
        for rbw, dlen, nexc, n in itertools.product(rbws, [1, 8], [0, 1, 300], n_set(width(fpt))):
            r = _seed("alprd", fpt, rbw, dlen, nexc, n)
            left, d, right, pos, exc = _alprd_inputs(r, fpt, rbw, dlen, min(nexc, n), n)
            rc, got = o_alprd(fpt, left, d, rbw, right, pos, exc)
            lp = d[left].astype(ut)
            lp[pos.astype(np.int64)] = exc.astype(ut)
            plain = (lp << ut(rbw)) | right
            yield Case("vxg_alprd_decode", f"{fpt}-rbw{rbw}-d{dlen}-exc{nexc}-n{n}",
                       {"left": left, "right": right, "exc_pos": pos, "exc_vals": exc},
                       dict(ptype=fpt, dict=d, right_bw=rbw, n=n, n_exc=pos.size),
                       {"out": Out(n * width(fpt), got.tobytes())}, {"out": plain.tobytes()}, oracle_rc=rc)
    for fpt, rbw in (("f32", 16), ("f64", 48)):
        r = _seed("alprd-bad", fpt)
        n = 1500
        left, d, right, pos, exc = _alprd_inputs(r, fpt, rbw, 5, 20, n)
        bufs = {"left": left, "right": right, "exc_pos": pos, "exc_vals": exc}
        base = dict(ptype=fpt, dict=d, right_bw=rbw, n=n, n_exc=pos.size)
        out = {"out": Out(n * width(fpt))}
        # dict[*code as usize] (alp_rd/mod.rs:287) panics for a code >= dict_len, even under an exception
        bl = left.copy()
        bl[700] = 5
        yield Case("vxg_alprd_decode", f"{fpt}-left-code-eq-dict-len", {**bufs, "left": bl}, base, out,
                   error="OutOfBounds", at="sync", oracle_rc=o_alprd(fpt, bl, d, rbw, right, pos, exc)[0])
        bp = pos.copy()
        bp[-1] = n
        yield Case("vxg_alprd_decode", f"{fpt}-exception-position-eq-n", {**bufs, "exc_pos": bp}, base, out,
                   error="OutOfBounds", at="sync", oracle_rc=o_alprd(fpt, left, d, rbw, right, bp, exc)[0])
        d9 = r.integers(0, 1 << 16, 9, dtype=np.uint16)
        yield Case("vxg_alprd_decode", f"{fpt}-dict-len-9", bufs, {**base, "dict": d9}, out, error="InvalidArgument")
        for bw in (0, 8 * width(fpt), 8 * width(fpt) + 1):
            yield Case("vxg_alprd_decode", f"{fpt}-right-bw-{bw}", bufs, {**base, "right_bw": bw}, out,
                       error="InvalidArgument")
    yield Case("vxg_alprd_decode", "int-ptype", bufs, {**base, "ptype": "u64"}, out, error="MismatchedTypes")


# ------------------------------------------------------------------ take
def cases_take():
    for vw, cpt, nv in itertools.product(VALUE_WIDTHS, UNSIGNED, [1, 255, 70_000]):
        for n in n_set(vw):
            r = _seed("take", vw, cpt, nv, n)
            hi = min(nv, 1 << (8 * width(cpt)))
            codes = r.integers(0, hi, n, dtype=np.uint64).astype(O.NP[cpt])
            if n:
                codes[-1] = hi - 1
            values = r.integers(0, 256, nv * vw, dtype=np.uint8)
            rc, got = o_take(vw, values, nv, cpt, codes)
            yield Case("vxg_take", f"vw{vw}-{cpt}-nv{nv}-n{n}", {"values": values, "codes": codes},
                       dict(vw=vw, n_values=nv, codes_ptype=cpt, n=n), {"out": Out(n * vw, got.tobytes())},
                       {"out": np_take(vw, values, codes).tobytes()}, oracle_rc=rc)
    r = _seed("take-bad")
    values = r.integers(0, 256, 255 * 4, dtype=np.uint8)
    for cpt in UNSIGNED:
        codes = r.integers(0, 255, 1025, dtype=np.uint64).astype(O.NP[cpt])
        codes[1024] = 255  # == n_values, in the last element
        yield Case("vxg_take", f"{cpt}-code-eq-n-values", {"values": values, "codes": codes},
                   dict(vw=4, n_values=255, codes_ptype=cpt, n=1025), {"out": Out(4100)}, error="OutOfBounds", at="sync",
                   oracle_rc=o_take(4, values, 255, cpt, codes)[0])
    codes = r.integers(0, 255, 100, dtype=np.uint16)
    bufs = {"values": values, "codes": codes}
    base = dict(vw=4, n_values=255, codes_ptype="u16", n=100)
    yield Case("vxg_take", "no-values", bufs, {**base, "n_values": 0}, {"out": Out(400)}, error="OutOfBounds",
               oracle_rc=o_take(4, values, 0, "u16", codes)[0])
    for cpt in SIGNED + ["f32"]:
        yield Case("vxg_take", f"{cpt}-codes", bufs, {**base, "codes_ptype": cpt}, {"out": Out(400)},
                   error="MismatchedTypes")
    for vw in (0, 3, 32):
        yield Case("vxg_take", f"value-width-{vw}", bufs, {**base, "vw": vw}, {"out": Out(3200)}, error="InvalidArgument")


# ------------------------------------------------------------------ Delta
def delta_encode(x: np.ndarray):
    """delta_compress (delta/compress.rs:14-98) -> (bases, deltas)."""
    pt = E.PTYPE_OF_NP[x.dtype]
    lanes = 1024 // (8 * x.dtype.itemsize)
    nb = (x.size // 1024) * lanes + (1 if x.size % 1024 else 0)
    bases = np.zeros(max(nb, 1), dtype=x.dtype)
    deltas = np.zeros(max(x.size, 1), dtype=x.dtype)
    E._lib_enc().vxe_delta_compress(E.PTYPE[pt], E._p(x), x.size, E._p(bases), E._p(deltas))
    return bases[:nb].copy(), deltas[: x.size].copy()


def o_delta(pt, bases, n_bases, deltas, n_deltas, offset, n):
    out = np.zeros(n, dtype=O.NP[pt])
    rc = O.lib().vxo_delta_decode(O.PT[pt], O.p(bases), n_bases, O.p(deltas), n_deltas, offset, n, O.p(out))
    return rc, out


def cases_delta_decode():
    for pt in UNSIGNED:
        T = 8 * width(pt)
        for nd, offset in itertools.product([1024, 2048, 1025, 3 * 1024 + 500], [0, 1, 1023, 1500]):
            if offset >= nd:
                continue
            for n in sorted({nd - offset, max((nd - offset) // 2, 1), 1}):  # to the end, inside, one value
                r = _seed("delta", pt, nd, offset, n)
                x = rand_bits(r, nd, T, O.NP[pt])
                bases, deltas = delta_encode(x)
                rc, got = o_delta(pt, bases, bases.size, deltas, nd, offset, n)
                yield Case("vxg_delta_decode", f"{pt}-nd{nd}-o{offset}-n{n}", {"bases": bases, "deltas": deltas},
                           dict(ptype=pt, n_bases=bases.size, n_deltas=nd, offset=offset, len=n),
                           {"out": Out(n * width(pt), got.tobytes())}, {"out": x[offset: offset + n].tobytes()},
                           oracle_rc=rc)
    r = _seed("delta-bad")
    x = rand_bits(r, 2500, 32, np.uint32)
    bases, deltas = delta_encode(x)
    bufs = {"bases": bases, "deltas": deltas}
    base = dict(ptype="u32", n_bases=bases.size, n_deltas=2500, offset=10, len=100)
    for name, over, err in (("n-bases-less", dict(n_bases=bases.size - 1), "InvalidArgument"),
                            ("n-bases-more", dict(n_bases=bases.size + 1), "InvalidArgument"),
                            ("past-the-end", dict(offset=2401), "InvalidArgument"),
                            ("offset-past-the-end", dict(offset=2501, len=0), "InvalidArgument"),
                            ("len-wraps", dict(offset=10, len=(1 << 64) - 5), "InvalidArgument"),
                            ("signed", dict(ptype="i32"), "MismatchedTypes"), ("float", dict(ptype="f32"), "MismatchedTypes")):
        a = {**base, **over}
        rc = None
        if err == "InvalidArgument" and a["len"] < (1 << 32):
            rc = o_delta("u32", bases, a["n_bases"], deltas, 2500, a["offset"], a["len"])[0]
        yield Case("vxg_delta_decode", name, bufs, a, {"out": Out(400)}, error=err, oracle_rc=rc)


# ------------------------------------------------------------------ RunEnd
def sliced_runs(r, mean: int, offset: int, n: int):
    """Ends of a run-end array of offset + n + 9 rows with runs of mean length `mean`, sliced to
    [offset, offset + n) the way RunEndArray::slice leaves them (runend/compute.rs:104-119): the runs
    holding the first and the last row kept whole, ends untouched, `offset` in the metadata."""
    total = offset + n + 9
    lens = np.ones(total, np.int64) if mean == 1 else r.integers(1, 2 * mean, total)
    ends = np.cumsum(lens)
    ends = ends[: int(np.searchsorted(ends, total, side="left")) + 1]
    ends[-1] = total

    def phys(i):  # find_physical_index (runend/array.rs:95-98)
        k = int(np.searchsorted(ends, i + 0, side="right"))
        return k - 1 if k == ends.size else k

    b, e = phys(offset), phys(offset + n)
    return ends[b: e + 1].astype(np.uint64)


def o_runend(vw, values, ept, ends, n_runs, offset, n):
    out = np.zeros(n * vw, dtype=np.uint8)
    rc = O.lib().vxo_runend_decode(vw, O.p(values), O.PT[ept], O.p(ends), n_runs, offset, n, O.p(out))
    return rc, out


def run_lengths(ends: np.ndarray, offset: int, n: int) -> np.ndarray:
    t = np.minimum(ends.astype(np.int64) - offset, n)  # trimmed ends (runend/compress.rs:140)
    return np.diff(np.concatenate([[0], t]))


def cases_runend_decode():
    eps = UNSIGNED + ["i32", "i64"]
    for vw, ept, mean, offset, n in itertools.product([1, 2, 4, 8], eps, [1, 16, 17, 300], [0, 5],
                                                      [1, 2047, 2048, 2049, 4097, 10_000]):
        if offset + n + 9 > int(np.iinfo(O.NP[ept]).max):
            continue
        r = _seed("runend", vw, ept, mean, offset, n)
        ends = sliced_runs(r, mean, offset, n).astype(O.NP[ept])
        values = r.integers(0, 256, ends.size * vw, dtype=np.uint8)
        rc, got = o_runend(vw, values, ept, ends, ends.size, offset, n)
        plain = np.repeat(values.reshape(-1, vw), run_lengths(ends, offset, n), axis=0)
        yield Case("vxg_runend_decode", f"vw{vw}-{ept}-mean{mean}-o{offset}-n{n}", {"values": values, "ends": ends},
                   dict(vw=vw, ends_ptype=ept, n_runs=ends.size, offset=offset, len=n),
                   {"out": Out(n * vw, got.tobytes())}, {"out": plain.tobytes()}, oracle_rc=rc)
    for mean in (1, 300):  # the thread-per-run kernel and the span kernel
        r = _seed("runend-short", mean)
        n = 5000
        ends = sliced_runs(r, mean, 5, n).astype(np.uint32)
        ends = ends[ends < 5 + n - 40]  # the last 40 rows have no run
        values = r.integers(0, 256, ends.size * 4, dtype=np.uint8)
        yield Case("vxg_runend_decode", f"ends-stop-short-mean{mean}", {"values": values, "ends": ends},
                   dict(vw=4, ends_ptype="u32", n_runs=ends.size, offset=5, len=n), {"out": Out(n * 4)},
                   error="InvalidArgument", at="sync", oracle_rc=o_runend(4, values, "u32", ends, ends.size, 5, n)[0])
    bufs = {"values": values, "ends": ends}
    base = dict(vw=4, ends_ptype="u32", n_runs=ends.size, offset=5, len=100)
    yield Case("vxg_runend_decode", "no-runs", bufs, {**base, "n_runs": 0}, {"out": Out(400)}, error="InvalidArgument",
               oracle_rc=o_runend(4, values, "u32", ends, 0, 5, 100)[0])
    for vw in (0, 3, 32):
        yield Case("vxg_runend_decode", f"value-width-{vw}", bufs, {**base, "vw": vw}, {"out": Out(3200)},
                   error="InvalidArgument")
    yield Case("vxg_runend_decode", "float-ends", bufs, {**base, "ends_ptype": "f32"}, {"out": Out(400)},
               error="MismatchedTypes")


# ------------------------------------------------------------------ Bool encodings
BOOL_LENS = [1, 31, 32, 33, 8191, 8192, 8193]
BIT_OFFSETS = [0, 1, 31, 32, 37]


def bits_at(mask: np.ndarray, bit_offset: int) -> bytes:
    """`mask` as LSB bits starting at bit `bit_offset` of a zeroed buffer of whole 32-bit words."""
    nbytes = ((bit_offset + mask.size + 31) // 32) * 4
    full = np.zeros(nbytes * 8, dtype=np.uint8)
    full[bit_offset: bit_offset + mask.size] = mask
    return np.packbits(full, bitorder="little").tobytes()


def oracle_bits(buf: np.ndarray, n: int) -> np.ndarray:
    return np.unpackbits(buf, bitorder="little")[:n]


def cases_runend_bool_decode():
    for n, boff, ept, start, offset in itertools.product(BOOL_LENS, BIT_OFFSETS, UNSIGNED, [0, 1], [0, 5]):
        if offset + n + 9 > int(np.iinfo(O.NP[ept]).max):
            continue
        r = _seed("runend_bool", n, boff, ept, start, offset)
        ends = sliced_runs(r, [1, 3, 40, 3000][(n + boff + start) % 4], offset, n).astype(O.NP[ept])
        ob = np.zeros((n + 7) // 8 + 1, np.uint8)
        rc = O.lib().vxo_runend_bool_decode(O.PT[ept], O.p(ends), ends.size, offset, start, n, O.p(ob))
        vals = (np.arange(ends.size) % 2 == 0) == bool(start)  # value_at_index: start ^ (run odd)
        plain = np.repeat(vals, run_lengths(ends, offset, n)).astype(np.uint8)
        want = bits_at(oracle_bits(ob, n), boff)
        yield Case("vxg_runend_bool_decode", f"n{n}-bit{boff}-{ept}-start{start}-o{offset}", {"ends": ends},
                   dict(ends_ptype=ept, n_runs=ends.size, offset=offset, start=start, len=n, out_bit_offset=boff),
                   {"out": Out(len(want), want, bytes(len(want)))}, {"out": bits_at(plain, boff)}, oracle_rc=rc)
    r = _seed("runend_bool-bad")
    ends = sliced_runs(r, 40, 0, 9000).astype(np.uint32)
    base = dict(ends_ptype="u32", n_runs=ends.size, offset=0, start=1, len=9000, out_bit_offset=0)
    zero = {"out": Out(1128, None, bytes(1128))}
    tmp = np.zeros(1200, np.uint8)
    for ept in SIGNED:
        yield Case("vxg_runend_bool_decode", f"{ept}-ends", {"ends": ends}, {**base, "ends_ptype": ept}, zero,
                   error="InvalidArgument")
    yield Case("vxg_runend_bool_decode", "no-runs", {"ends": ends}, {**base, "n_runs": 0}, zero, error="InvalidArgument",
               oracle_rc=O.lib().vxo_runend_bool_decode(O.PT["u32"], O.p(ends), 0, 0, 1, 9000, O.p(tmp)))
    short = ends[ends < 8900]
    yield Case("vxg_runend_bool_decode", "ends-stop-short", {"ends": short}, {**base, "n_runs": short.size}, zero,
               error="InvalidArgument", at="sync",
               oracle_rc=O.lib().vxo_runend_bool_decode(O.PT["u32"], O.p(short), short.size, 0, 1, 9000,
                                                        O.p(tmp)))


def cases_bytebool_to_bits():
    for n, boff, mis in itertools.product(BOOL_LENS, BIT_OFFSETS, [0, 1]):
        r = _seed("bytebool", n, boff, mis)
        src = r.choice(np.array([0, 0, 0, 1, 2, 0x80, 0xFF], dtype=np.uint8), n)
        src[: min(n, 4)] = np.array([2, 0x80, 0xFF, 0], np.uint8)[: min(n, 4)]  # non-zero is true
        ob = np.zeros((n + 7) // 8 + 1, np.uint8)
        O.lib().vxo_bytebool_to_bits(O.p(src), n, O.p(ob))
        want = bits_at(oracle_bits(ob, n), boff)
        yield Case("vxg_bytebool_to_bits", f"n{n}-bit{boff}-src+{mis}", {"bytes": src}, dict(n=n, out_bit_offset=boff),
                   {"out": Out(len(want), want, bytes(len(want)))}, {"out": bits_at((src != 0).astype(np.uint8), boff)},
                   oracle_rc=0, shift_in={"bytes": mis})


# ------------------------------------------------------------------ fill
def cases_fill():
    pattern = np.arange(0x10, 0x20, dtype=np.uint8)  # 16 distinct bytes
    for vw in VALUE_WIDTHS:
        for n in n_set(vw):
            got = np.zeros(n * vw, dtype=np.uint8)
            O.lib().vxo_fill(vw, O.p(pattern), n, O.p(got))
            plain = np.full(n, pattern[:vw].view(f"V{vw}")[0], dtype=f"V{vw}")
            yield Case("vxg_fill", f"vw{vw}-n{n}", {}, dict(vw=vw, scalar=pattern[:vw].tobytes(), n=n),
                       {"out": Out(n * vw, got.tobytes())}, {"out": plain.tobytes()}, oracle_rc=0)
    for vw in (0, 3, 17, 32, 1 << 31):
        yield Case("vxg_fill", f"value-width-{vw}", {}, dict(vw=vw, scalar=pattern.tobytes(), n=64), {"out": Out(2048)},
                   error="InvalidArgument")


# ------------------------------------------------------------------ FSST
def fsst_encode(strings, offs_pt: str, lens_pt: str):
    """fsst_compress (fsst/compress.rs:83-129) with a table trained on the strings themselves."""
    heap, offs, valid = E.strings_to_heap(strings)
    n = len(strings)
    t = VxeFsstTable()
    lib = E._lib_enc()
    h = heap if heap.size else np.zeros(1, np.uint8)
    lib.vxe_fsst_train(E._p(h), E._p(offs), n, C.byref(t))
    cap = 2 * int(heap.size) + 16
    codes = np.zeros(cap, dtype=np.uint8)
    coffs = np.zeros(n + 1, dtype=np.int32)
    nc = lib.vxe_fsst_compress(C.byref(t), E._p(h), E._p(offs), n, E._p(codes), cap, E._p(coffs))
    assert nc != 2 ** 64 - 1
    syms = np.array(list(t.symbols)[: t.n_symbols], dtype=np.uint64)
    slen = np.array(list(t.lens)[: t.n_symbols], dtype=np.uint8)
    return (syms, slen, codes[:nc].copy(), coffs.astype(O.NP[offs_pt]), np.diff(offs).astype(O.NP[lens_pt]),
            None if valid.all() else np.packbits(valid, bitorder="little"))


def o_fsst(syms, slen, codes, offs_pt, coffs, lens_pt, lens, vbits):
    n = lens.size
    heap = np.zeros(int(lens.astype(np.int64).sum()) + 16, dtype=np.uint8)
    views = np.zeros(16 * n, dtype=np.uint8)
    hl = C.c_size_t()
    rc = O.lib().vxo_fsst_canonicalize(O.p(syms), O.p(slen), O.p(codes), O.PT[offs_pt], O.p(coffs), O.PT[lens_pt],
                                       O.p(lens), n, O.p(vbits) if vbits is not None else None, O.p(heap),
                                       C.byref(hl), O.p(views))
    return rc, heap[: hl.value], views


def np_views(strings) -> tuple[bytes, bytes]:
    """The canonical VarBinView of `strings` with one data buffer holding every string in order
    (arrow make_view: len <= 12 inline, else len, 4-byte prefix, buffer 0, offset; null = zeros)."""
    views = np.zeros((len(strings), 16), dtype=np.uint8)
    off = 0
    for i, s in enumerate(strings):
        if s is None:
            continue
        views[i, :4] = np.frombuffer(np.uint32(len(s)).tobytes(), np.uint8)
        if len(s) <= 12:
            views[i, 4: 4 + len(s)] = np.frombuffer(s, np.uint8)
        else:
            views[i, 4:8] = np.frombuffer(s[:4], np.uint8)
            views[i, 12:16] = np.frombuffer(np.uint32(off).tobytes(), np.uint8)
        off += len(s)
    return b"".join(s for s in strings if s is not None), views.tobytes()


def fsst_strings(r, n: int, nulls: bool):
    text = b"the quick brown fox jumps over the lazy dog, carefully final deposits sleep furiously; "
    edge = [b"", text[:12], text[:13], (text * 4)[:300],
            bytes(r.integers(128, 256, 40, dtype=np.uint8))]  # bytes outside the table: an escape-heavy row
    out = []
    for i in range(n):
        if n <= 3:
            s = [edge[3], edge[0], edge[4]][i] if n == 3 else edge[2]
        elif i < len(edge):
            s = edge[i]
        else:
            a = int(r.integers(0, len(text)))
            s = (text[a:] + text)[: int(r.integers(0, 40))]
        out.append(None if nulls and i % 7 == 3 else s)
    return out


def cases_fsst_decode():
    for n, offs_pt, lens_pt, nulls in itertools.product([1, 3, 1000], ["i32", "i64"], ["i32", "u32"], [False, True]):
        r = _seed("fsst", n, offs_pt, lens_pt, nulls)
        strings = fsst_strings(r, n, nulls and n > 1) if n > 1 or not nulls else [None]
        syms, slen, codes, coffs, lens, vbits = fsst_encode(strings, offs_pt, lens_pt)
        rc, heap, views = o_fsst(syms, slen, codes, offs_pt, coffs, lens_pt, lens, vbits)
        pheap, pviews = np_views(strings)
        bufs = {"symbols": syms, "sym_lens": slen, "codes": codes, "offsets": coffs, "lens": lens}
        if vbits is not None:
            bufs["validity"] = vbits
        yield Case("vxg_fsst_decode", f"n{n}-offs-{offs_pt}-lens-{lens_pt}-{'nulls' if nulls else 'valid'}", bufs,
                   dict(n_symbols=syms.size, offs_ptype=offs_pt, lens_ptype=lens_pt, n=n),
                   {"heap": Out(heap.size, heap.tobytes(), slack=8), "views": Out(16 * n, views.tobytes())},
                   {"heap": pheap, "views": pviews}, oracle_rc=rc)
    r = _seed("fsst-bad")
    strings = [b"carefully final deposits"] * 600
    syms, slen, codes, coffs, lens, _ = fsst_encode(strings, "i32", "i32")
    lens[5] += 3  # the codes no longer decode to uncompressed_lengths
    rc, _, _ = o_fsst(syms, slen, codes, "i32", coffs, "i32", lens, None)
    bufs = {"symbols": syms, "sym_lens": slen, "codes": codes, "offsets": coffs, "lens": lens}
    total = int(lens.sum())
    yield Case("vxg_fsst_decode", "inconsistent-lengths", bufs, dict(n_symbols=syms.size, offs_ptype="i32", lens_ptype="i32", n=600),
               {"heap": Out(total, None, slack=8), "views": Out(16 * 600)}, error="InvalidArgument", at="sync",
               oracle_rc=rc)
    base = dict(n_symbols=syms.size, offs_ptype="i32", lens_ptype="i32", n=600)
    outs = {"heap": Out(total, None, slack=8), "views": Out(16 * 600)}
    yield Case("vxg_fsst_decode", "float-offsets", bufs, {**base, "offs_ptype": "f32"}, outs, error="MismatchedTypes")
    yield Case("vxg_fsst_decode", "float-lengths", bufs, {**base, "lens_ptype": "f64"}, outs, error="MismatchedTypes")
    yield Case("vxg_fsst_decode", "256-symbols", bufs, {**base, "n_symbols": 256}, outs, error="InvalidArgument")


# ------------------------------------------------------------------ grid-stride cases
GRID_CAP_THREADS = 32768 * 256  # grid_for caps a launch at 32768 workgroups of 256 threads


def grid_stride_case(entry: str) -> Case:
    """One case in which some thread makes a second trip of its grid-stride loop.  Built on demand
    (8 MiB for vxg_take / vxg_fill, 128 MiB for vxg_for_decode)."""
    n = GRID_CAP_THREADS + 257
    r = _seed("grid-stride", entry)
    if entry == "vxg_take":
        values = r.integers(0, 256, 255, dtype=np.uint8)
        codes = r.integers(0, 255, n, dtype=np.uint8)
        rc, got = o_take(1, values, 255, "u8", codes)
        return Case("vxg_take", "grid-stride", {"values": values, "codes": codes},
                    dict(vw=1, n_values=255, codes_ptype="u8", n=n), {"out": Out(n, got.tobytes())},
                    {"out": values[codes].tobytes()}, oracle_rc=rc)
    if entry == "vxg_fill":
        got = np.zeros(n, dtype=np.uint8)
        scalar = np.array([0xA7], np.uint8)
        O.lib().vxo_fill(1, O.p(scalar), n, O.p(got))
        return Case("vxg_fill", "grid-stride", {}, dict(vw=1, scalar=b"\xa7", n=n), {"out": Out(n, got.tobytes())},
                    {"out": np.full(n, 0xA7, np.uint8).tobytes()}, oracle_rc=0)
    assert entry == "vxg_for_decode"
    n = 2 * GRID_CAP_THREADS + 3  # two u64 per thread of the vector body
    x = r.integers(0, 1 << 64, n, dtype=np.uint64)
    ref = wrap_ref(64)
    got = o_for("u64", x, ref, 1)
    return Case("vxg_for_decode", "grid-stride", {"in": x}, dict(ptype="u64", n=n, reference=ref, shift=1),
                {"out": Out(n * 8, got.tobytes())}, {"out": np_for(x, ref, 1).tobytes()}, oracle_rc=0)


GENERATORS = {
    "vxg_bitunpack": cases_bitunpack,
    "vxg_bitunpack_for": cases_bitunpack_for,
    "vxg_bitunpack_alp": cases_bitunpack_alp,
    "vxg_bitunpack_dict": cases_bitunpack_dict,
    "vxg_bitunpack_dict_chunks": cases_bitunpack_dict_chunks,
    "vxg_patch": cases_patch,
    "vxg_for_decode": cases_for_decode,
    "vxg_zigzag_decode": cases_zigzag_decode,
    "vxg_alp_decode": cases_alp_decode,
    "vxg_alprd_decode": cases_alprd_decode,
    "vxg_take": cases_take,
    "vxg_delta_decode": cases_delta_decode,
    "vxg_runend_decode": cases_runend_decode,
    "vxg_fsst_decode": cases_fsst_decode,
    "vxg_runend_bool_decode": cases_runend_bool_decode,
    "vxg_bytebool_to_bits": cases_bytebool_to_bits,
    "vxg_fill": cases_fill,
}
ENTRY_POINTS = list(GENERATORS)


@functools.lru_cache(maxsize=None)
def cases(entry: str) -> tuple:
    """Every case of one entry point; names are unique."""
    out = tuple(GENERATORS[entry]())
    assert len({c.name for c in out}) == len(out), f"duplicate case names for {entry}"
    assert all(c.entry == entry for c in out)
    return out
