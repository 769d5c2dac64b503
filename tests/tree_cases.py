"""Seeded random encoding trees: one tree per seed, with its plain truth and its compute inputs.

Plain module: numpy, the host encoders (vortex_amd.encode), the array constructors
(vortex_amd.arrays) and the CPU oracle's metadata-only slices (oracle_tree.slice_any) -- no GPU,
no torch.  `build(seed)` composes the encodings by POSITION, the way the planner decides what to
launch: a root, a chunk of a root ChunkedArray, the child of FoR / ZigZag / ALP, the codes and the
values of a Dict, the ends and the values of a RunEnd, patch indices, a validity child.  Every tree
is valid (malformed input belongs to the error tests and the file fuzzer).

A TreeCase holds the tree, the plain numpy truth it was encoded from, a one-line `describe`, and
the inputs of the compute routes (take index sets, filter predicates, compare scalars, one
two-sided range).  tests/test_tree_cases.py holds the oracle's canonical of every tree against the
truth on the CPU; tests/test_gpu_trees.py sends every tree through every route of the engine.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass, field
from typing import Optional

import numpy as np

import vortex_amd.arrays as A
import vortex_amd.encode as E
from oracle_tree import slice_any
from vortex_amd._lib import DTYPE, ENC, VALIDITY
from vortex_amd.arrays import NP_OF_PTYPE, Array

ENC_NAME = {v: k for k, v in ENC.items()}
CONSTRUCTIBLE = ["PRIMITIVE", "BOOL", "BYTE_BOOL", "ROARING_BOOL", "RUN_END_BOOL", "FL_BITPACKED", "SPARSE", "FL_FOR",
                 "ZIGZAG", "ALP", "ALP_RD", "DICT", "FL_DELTA", "RUN_END", "CONSTANT", "CHUNKED", "VARBIN",
                 "VARBINVIEW", "FSST"]  # what vortex_amd.arrays can construct
VALIDITY_KINDS = ["NON_NULLABLE", "ALL_VALID", "ALL_INVALID", "BOOL", "BOOL_OFFSET", "RUN_END_BOOL"]

# the block (1024), tile (4096) and word (64) edges the kernels are built around
CHUNK_LENS = [0, 1, 63, 64, 65, 1023, 1024, 1025, 2047, 4095, 4096, 4097, 8193]
CHUNK_LEN_WEIGHTS = [4, 4, 1, 1, 1, 2, 2, 2, 1, 1, 1, 1, 1]
SINGLE_LENS = CHUNK_LENS + [20_011]
ROW_CAP = 40_000
STRING_ROW_CAP = 9_000  # the string expectations walk the rows in Python

UNSIGNED = ["u8", "u16", "u32", "u64"]
SIGNED = ["i8", "i16", "i32", "i64"]
FLOATS = ["f32", "f64"]
PTYPES_OF = {"PRIMITIVE": UNSIGNED + SIGNED + FLOATS, "FL_BITPACKED": UNSIGNED, "FL_FOR": UNSIGNED + SIGNED,
             "ZIGZAG": SIGNED, "ALP": FLOATS, "ALP_RD": FLOATS, "DICT": UNSIGNED + SIGNED + FLOATS,
             "FL_DELTA": UNSIGNED, "RUN_END": UNSIGNED + SIGNED + FLOATS, "SPARSE": UNSIGNED + SIGNED + FLOATS,
             "CONSTANT": UNSIGNED + SIGNED + FLOATS}
PRIM_ENCS = list(PTYPES_OF)
BOOL_ENCS = ["BOOL", "BYTE_BOOL", "RUN_END_BOOL", "ROARING_BOOL", "SPARSE", "CONSTANT"]
STR_ENCS = ["VARBIN", "VARBINVIEW", "FSST", "DICT"]
EMPTY_OK = {"PRIMITIVE", "FL_BITPACKED", "FL_FOR", "ZIGZAG", "DICT", "CONSTANT", "SPARSE", "FL_DELTA",
            "BOOL", "BYTE_BOOL", "VARBIN", "VARBINVIEW"}  # encodings built at length 0

# the root of seed s is ROOTS[s % 72]: every encoding three times, ChunkedArray eighteen times
ROOTS = ([(e, "prim") for e in PRIM_ENCS] + [(e, "bool") for e in BOOL_ENCS[:4]] +
         [(e, "str") for e in STR_ENCS[:3]]) * 3 + [("CHUNKED", "prim")] * 10 + [("CHUNKED", "bool")] * 4 + \
        [("CHUNKED", "str")] * 4
assert len(ROOTS) == 72

# the packed shapes (vxg_compare_scalar's and vxg_filter_batch's packed route) and where chunks are cut
PACKED_EPILOGUES = ["bp", "for", "for-shift", "zz", "zz-for", "alp-for"]
CUT_EDGES = [1, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097]


@dataclass
class TreeCase:
    seed: int
    tree: Array
    values: object                 # ndarray (primitive), bool mask (bool), list of bytes | None (strings)
    valid: Optional[np.ndarray]    # bool mask, or None = every row valid
    describe: str
    kind: str                      # "prim" | "bool" | "str"
    take_sets: list = field(default_factory=list)    # (name, indices ndarray)
    predicates: list = field(default_factory=list)   # (name, non-nullable Bool Array)
    scalars: list = field(default_factory=list)      # compare scalars (numbers, or bytes for strings)
    range: Optional[tuple] = None                    # (lo_op, lo, hi_op, hi)


# ---------------------------------------------------------------------------- describe / walk
def validity_kind(a: Array) -> Optional[str]:
    """The validity kind of a node that carries its own validity, else None."""
    own = ("PRIMITIVE", "BOOL", "BYTE_BOOL", "RUN_END_BOOL", "FL_BITPACKED", "FL_DELTA", "RUN_END", "VARBIN",
           "VARBINVIEW")
    if ENC_NAME[a.encoding] not in own:
        return None
    if a.validity != VALIDITY["ARRAY"]:
        return {v: k for k, v in VALIDITY.items()}[a.validity]
    v = a.children[-1]
    if v.encoding == ENC["BOOL"]:
        return "BOOL_OFFSET" if v.meta.get("first_byte_bit_offset", 0) else "BOOL"
    return ENC_NAME[v.encoding]


def node_offset(a: Array) -> int:
    """The slice offset a node's metadata carries (0: not sliced, or sliced at a multiple)."""
    m = a.meta
    if a.encoding == ENC["SPARSE"]:
        return m["indices_offset"]
    if a.encoding == ENC["BOOL"]:
        return m.get("first_byte_bit_offset", 0)
    return m.get("offset", 0)


def describe(a: Array) -> str:
    name = ENC_NAME[a.encoding]
    dt = {DTYPE["PRIMITIVE"]: a.ptype, DTYPE["BOOL"]: "bool", DTYPE["UTF8"]: "utf8", DTYPE["BINARY"]: "binary"}[a.dtype]
    s = f"{name}<{dt}>[{a.len}]"
    bits = []
    if node_offset(a):
        bits.append(f"off={node_offset(a)}")
    if a.encoding == ENC["FL_BITPACKED"]:
        bits.append(f"W={a.meta['bit_width']}")
    if a.encoding == ENC["FL_FOR"] and a.meta["shift"]:
        bits.append(f"shift={a.meta['shift']}")
    vk = validity_kind(a)
    if vk and vk != "NON_NULLABLE":
        bits.append(f"v={vk}")
    if a.encoding in (ENC["SPARSE"], ENC["CONSTANT"]) and a.nullable:
        bits.append("null")
    if bits:
        s += "{" + ",".join(bits) + "}"
    kids = a.children
    if a.encoding == ENC["CHUNKED"]:
        kids = kids[1:]
    elif vk in ("BOOL", "BOOL_OFFSET"):
        kids = kids[:-1]
    if a.encoding == ENC["VARBINVIEW"]:
        kids = []
    if kids:
        s += "(" + ", ".join(describe(c) for c in kids) + ")"
    return s


def walk(a: Array, parent: Optional[Array] = None, slot: int = 0):
    """Every node of the tree as (node, parent, child slot)."""
    yield a, parent, slot
    for i, c in enumerate(a.children):
        yield from walk(c, a, i)


def k1_fusable(c: Array) -> bool:
    """planner.hpp's rule for a chunk whose whole decode is one K1 launch (+ patch scatters)."""
    def bp_of(x, w):
        return x is not None and x.encoding == ENC["FL_BITPACKED"] and A.ptype_width(x.ptype) == w

    w = A.ptype_width(c.ptype)
    kid = c.children[0] if c.children else None
    if c.dtype != DTYPE["PRIMITIVE"]:
        return False
    if c.encoding == ENC["FL_BITPACKED"]:
        return True
    if c.encoding in (ENC["FL_FOR"], ENC["ZIGZAG"]):
        return bp_of(kid, w)
    if c.encoding == ENC["ALP"]:
        if kid is not None and kid.encoding == ENC["FL_FOR"]:
            kid = kid.children[0]
        return bp_of(kid, w)
    if c.encoding == ENC["DICT"]:
        v, k = c.children
        return v.encoding == ENC["PRIMITIVE"] and k.encoding == ENC["FL_BITPACKED"] and k.meta["bit_width"] <= 16
    return False


def has_patches(c: Array) -> bool:
    return any(n.encoding in (ENC["FL_BITPACKED"], ENC["ALP"]) and n.meta["has_patches"] for n, _, _ in walk(c))


# ---------------------------------------------------------------------------- the generator
TEXT = (b"the quick brown fox jumps over the lazy dog, carefully final deposits sleep furiously; "
        b"DELIVER IN PERSON, TAKE BACK RETURN, COLLECT COD, NONE. ")


class Gen:
    def __init__(self, seed: int):
        self.rng = np.random.default_rng([0x7EE5, int(seed)])  # from the integer alone
        self.to_be_sliced = 0  # > 0 while building a node that slice_any will slice: restated encodings only

    # -- small draws
    def chance(self, p: float) -> bool:
        return bool(self.rng.random() < p)

    def pick(self, xs):
        return xs[int(self.rng.integers(0, len(xs)))]

    def slice_window(self, n: int):
        """(start, total): a window [start, start + n) of a longer array, start no multiple of 1024."""
        start = int(self.pick([1, 7, 63, 64, 1000, 1023, 1025, 1500]))
        return start, start + n + int(self.pick([0, 1, 9, 1024]))

    # -- validity
    def mask(self, n: int) -> np.ndarray:
        if self.chance(0.5):
            return self.rng.random(n) < self.pick([0.1, 0.7, 0.97])
        lens = self.rng.integers(1, self.pick([3, 40, 900]) + 1, n + 1)
        m = np.repeat(np.arange(lens.size) % 2 == 0, lens)[:n]
        return m if self.chance(0.5) else ~m

    def validity(self, n: int, kinds=None):
        """-> (the constructors' validity argument, the mask | None)."""
        k = self.pick(kinds or ["NON_NULLABLE", "NON_NULLABLE", "ALL_VALID", "ALL_INVALID", "BOOL", "BOOL_OFFSET",
                                "RUN_END_BOOL"])
        if k == "NON_NULLABLE":
            return None, None
        if k == "ALL_VALID":
            return "ALL_VALID", None
        if k == "ALL_INVALID":
            return "ALL_INVALID", np.zeros(n, bool)
        m = self.mask(n)
        if k == "BOOL":
            return m, m
        if k == "BOOL_OFFSET":
            return A.bool_array(m, bit_offset=int(self.rng.integers(1, 8))), m
        if n == 0:
            return m, m
        return E.encode_runend_bool(m, bitpack_ends=self.chance(0.5) and n < (1 << 62)), m

    # -- integer leaves: a given array in one of the child positions' encodings
    def leaf(self, vals: np.ndarray, kinds, validity=None, mask=None, sliced=None) -> Array:
        """`vals` as a primitive ("prim"), BitPacked ("bp", patch-free; "bpp", with patches),
        FoR(BitPacked) ("for"), ZigZag ("zz", signed values), Delta ("delta", unsigned), ALP-RD ("alprd",
        floats) or a nested ChunkedArray of those ("chunked").  `validity`/`mask`: the
        leaf's own validity.  With some probability the leaf is a slice of a longer array."""
        vals = np.ascontiguousarray(vals)
        n, kind = vals.size, self.pick(kinds)
        if kind == "alprd" and self.to_be_sliced:
            kind = "prim"
        isint = vals.dtype.kind in "iu"
        bits = 8 * vals.dtype.itemsize
        if kind == "chunked":
            cuts = sorted(int(c) for c in self.rng.integers(0, n + 1, int(self.rng.integers(1, 4))))
            cuts = [0] + cuts + [n]
            sub = [k for k in kinds if k != "chunked"] or ["prim"]
            parts = []
            for a, b in zip(cuts, cuts[1:]):
                pm = None if mask is None else mask[a:b]
                parts.append(self.leaf(vals[a:b], sub, pm if validity is not None else None, pm, sliced=False))
            return A.chunked(parts)
        if sliced is None:
            sliced = self.chance(0.25)
        if sliced and n:
            start, total = self.slice_window(n)
            ext = vals[self.rng.integers(0, n, total)]
            ext[start: start + n] = vals
            emask = None
            if validity is not None and mask is not None and not isinstance(validity, str):
                emask = self.rng.random(total) < 0.5
                emask[start: start + n] = mask
                validity = emask if not isinstance(validity, Array) or validity.encoding != ENC["BOOL"] else \
                    A.bool_array(emask, bit_offset=validity.meta["first_byte_bit_offset"])
            return slice_any(self.leaf(ext, [kind], validity, emask, sliced=False), start, start + n)
        if isinstance(validity, np.ndarray):
            validity = np.asarray(validity, bool)
        if kind == "alprd" and not isint and n and validity is None:
            return E.encode_alprd(vals)
        if kind == "delta" and vals.dtype.kind == "u" and n:
            d = E.encode_delta(vals, bitpack_deltas=self.chance(0.5))
            return A.delta(d.children[0], d.children[1], 0, n, validity=validity)
        if not isint or kind == "prim":
            return A.primitive(vals, validity=validity)
        if kind == "for":
            u, ref, shift = self.for_parts(vals)
            return A.frame_of_reference(self.leaf(u, ["bp", "bpp"], validity, mask, sliced=False), ref, shift,
                                        A.PTYPE_OF_NP[vals.dtype])
        if kind == "zz" and vals.dtype.kind == "i":
            return A.zigzag(self.leaf(E.zigzag_encode(vals), ["bp", "prim"], validity, mask, sliced=False))
        if vals.dtype.kind != "u":
            return A.primitive(vals, validity=validity)
        need = int(vals.max(initial=0)).bit_length()
        W = max(need, 1)
        if kind == "bpp" and n > 8:
            W = max(min(int(np.sort(vals)[int(0.97 * (n - 1))]).bit_length(), bits - 1), 1)
        if W >= bits:
            return A.primitive(vals, validity=validity)
        bp = E.encode_bitpacked(vals, bit_width=W)
        patches = None
        if bp.meta["has_patches"]:
            idx = np.flatnonzero(vals >> vals.dtype.type(W)).astype(np.uint64)  # the values too wide for W bits
            patches = A.sparse(self.index_array(idx), bp.children[0].children[1], n)
        return A.bitpacked(bp.buffers[0], bp.ptype, W, n, 0, patches, validity=validity)

    def index_array(self, idx: np.ndarray) -> Array:
        """Sorted positions as u16, u32 or u64, packed or plain."""
        mx = int(idx.max(initial=0))
        dt = self.pick([d for d in (np.uint16, np.uint32, np.uint64) if mx <= np.iinfo(d).max])
        v = idx.astype(dt)
        W = max(mx.bit_length(), 1)
        if self.chance(0.5) and W < 8 * v.dtype.itemsize:
            return E.encode_bitpacked(v, bit_width=W, allow_patches=False)
        return A.primitive(v)

    @staticmethod
    def for_parts(vals: np.ndarray):
        """for_compress (for/compress.rs:13-85) -> (encoded unsigned, reference, shift)."""
        ut = NP_OF_PTYPE[A.unsigned_of(A.PTYPE_OF_NP[vals.dtype])]
        if vals.size == 0:
            return np.zeros(0, ut), 0, 0
        u, ref, shift = E.for_compress(vals)
        if shift >= 8 * vals.dtype.itemsize:  # every value equals the reference
            shift = 0
        return u, ref, shift

    # -- value families
    def ints(self, pt: str, n: int, family: str) -> np.ndarray:
        dt = np.dtype(NP_OF_PTYPE[pt])
        info = np.iinfo(dt)
        bits = 8 * dt.itemsize
        r = self.rng
        if family == "narrow":  # narrow values with a few wide outliers
            W = int(r.integers(1, bits - 2))
            v = r.integers(0, 1 << W, n, dtype=np.uint64)
            k = max(n // 50, 1 if n > 8 else 0)
            if k:
                v[r.choice(n, k, replace=False)] = r.integers(1 << W, (1 << (bits - 1)) - 1, k, dtype=np.uint64)
            return v.astype(dt)
        if family == "offset":  # values around a large offset, multiples of 2^shift or not
            shift = int(self.pick([0, 0, 1, 3]))
            span = int(r.integers(2, max(3, min(1 << (bits - 3 - shift), 1 << 20))))
            base = int(r.integers(info.min // 2, info.max // 2)) if bits > 8 else int(info.min // 2)
            base -= base % (1 << shift)
            off = r.integers(0, span, n).astype(np.int64) << shift
            if info.min == 0:
                return (np.uint64(base) + off.astype(np.uint64)).astype(dt)
            return (np.int64(base) + off).astype(dt)
        if family == "small":  # small signed values
            lim = int(self.pick([1, 50, min(5000, info.max // 2)]))
            return r.integers(-lim, lim + 1, n).astype(dt)
        if family == "lowcard":
            card = int(self.pick([1, 2, 7, 200]))
            pool = r.integers(info.min, info.max, card, dtype=np.int64 if info.min < 0 else np.uint64, endpoint=True)
            return pool[r.integers(0, card, n)].astype(dt)
        if family == "monotone":
            step = int(self.pick([1, 3, 200]))
            room = max(int(info.max) // max(n, 1), 1)
            return np.cumsum(r.integers(0, min(step, room) + 1, n).astype(np.uint64)).astype(dt)
        return r.integers(info.min, info.max, n, dtype=np.int64 if info.min < 0 else np.uint64, endpoint=True).astype(dt)

    def floats(self, pt: str, n: int, family: str) -> np.ndarray:
        dt = NP_OF_PTYPE[pt]
        r = self.rng
        if family == "decimal":  # decimals with (or without) a few irrational exceptions
            digits = int(self.pick([0, 1, 2])) if pt == "f32" else int(self.pick([1, 2, 4]))
            v = np.round(r.uniform(-1000, 1000, n), digits).astype(dt)
            if self.chance(0.7) and n > 4:
                k = max(n // 60, 1)
                v[r.choice(n, k, replace=False)] = (r.standard_normal(k) * np.pi * 1e3).astype(dt)
            return v
        if family == "lowcard":  # NaN payloads and -0.0 count: values are compared as bytes
            ut = np.uint32 if pt == "f32" else np.uint64
            nan = np.array([0x7FC00001 if pt == "f32" else 0x7FF8000000000001], ut).view(dt)
            pool = np.concatenate([r.standard_normal(5).astype(dt), np.array([-0.0, 0.0, np.inf], dt), nan])
            return pool[r.integers(0, pool.size, n)]
        return (r.standard_normal(n) * 10.0 ** r.integers(-3, 6, n)).astype(dt)  # arbitrary

    def values_for(self, enc: str, pt: str, n: int) -> np.ndarray:
        if pt in FLOATS:
            fam = {"ALP": "decimal", "ALP_RD": "arbitrary", "PRIMITIVE": "arbitrary"}.get(enc, "lowcard")
            return self.floats(pt, n, fam)
        fam = {"FL_BITPACKED": "narrow", "FL_FOR": "offset", "ZIGZAG": "small", "DICT": "lowcard", "FL_DELTA": "monotone",
               "RUN_END": "lowcard", "SPARSE": "lowcard"}.get(enc, "any")
        if fam == "offset" and pt in UNSIGNED and self.chance(0.5):
            fam = "narrow"
        return self.ints(pt, n, fam)

    # -- primitive nodes: (Array, values, valid mask | None)
    def prim_node(self, enc: str, pt: str, n: int, sliced=None):
        if n == 0 and enc not in EMPTY_OK:
            enc = "PRIMITIVE"
        if sliced is None:
            sliced = self.chance(0.3)
        can_slice = enc in ("PRIMITIVE", "FL_BITPACKED", "FL_FOR", "ZIGZAG", "ALP", "DICT", "FL_DELTA", "RUN_END", "SPARSE")
        if sliced and can_slice and n:
            start, total = self.slice_window(n)
            self.to_be_sliced += 1
            node, vals, valid = self.prim_node(enc, pt, total, sliced=False)
            self.to_be_sliced -= 1
            return (slice_any(node, start, start + n), vals[start: start + n].copy(),
                    None if valid is None else valid[start: start + n].copy())
        return getattr(self, "_" + enc.lower())(pt, n)

    def _primitive(self, pt, n):
        vals = self.values_for("PRIMITIVE", pt, n)
        varg, m = self.validity(n)
        return A.primitive(vals, validity=varg), vals, m

    def _fl_bitpacked(self, pt, n):
        vals = self.values_for("FL_BITPACKED", pt, n)
        varg, m = self.validity(n)
        node = self.leaf(vals, ["bp", "bpp"], varg, m, sliced=False)
        if node.encoding != ENC["FL_BITPACKED"]:  # too wide to pack: narrow it
            vals = vals >> vals.dtype.type(1)
            node = self.leaf(vals, ["bp", "bpp"], varg, m, sliced=False)
        return node, vals, m

    def _fl_for(self, pt, n):
        vals = self.values_for("FL_FOR", pt, n)
        varg, m = self.validity(n)
        u, ref, shift = self.for_parts(vals)
        child = self.leaf(u, ["bp", "bpp", "prim", "chunked", "chunked"], varg, m)
        return A.frame_of_reference(child, ref, shift, pt), vals, m

    def _zigzag(self, pt, n):
        vals = self.values_for("ZIGZAG", pt, n)
        varg, m = self.validity(n)
        u = E.zigzag_encode(vals) if n else np.zeros(0, NP_OF_PTYPE[A.unsigned_of(pt)])
        return A.zigzag(self.leaf(u, ["bp", "bpp", "prim", "chunked", "chunked"], varg, m)), vals, m

    def _alp(self, pt, n):
        vals = self.values_for("ALP", pt, n)
        varg, m = self.validity(n)
        e, f, enc, idx, pv = E.alp_encode(vals)
        patches = None
        if idx.size:
            patches = A.sparse(self.index_array(idx), A.primitive(pv, validity="ALL_VALID"), n)
        child = self.leaf(enc, ["for", "for", "prim", "chunked", "chunked"], varg, m)
        return A.alp(child, e, f, patches), vals, m

    def _alp_rd(self, pt, n):
        vals = self.values_for("ALP_RD", pt, n)
        return E.encode_alprd(vals), vals, None

    def _dict(self, pt, n):
        vals = self.values_for("DICT", pt, n)
        m = None
        if self.chance(0.4) and n:  # nullable values: slot 0 is the null entry
            m = self.mask(n)
            codes, dv, vvalid = E.dict_encode_nullable(vals, m)
            vals = np.where(m, vals, vals.dtype.type(0))
            values = self.leaf(dv, ["prim", "bp"], self.pick([vvalid, A.bool_array(vvalid, bit_offset=3)]), vvalid,
                               sliced=False)
        else:
            codes, dv = E.dict_encode(vals) if n else (np.zeros(0, np.uint64), vals[:0])
            if dv.size == 0:
                dv = self.values_for("DICT", pt, 2)
            values = self.leaf(dv, ["prim", "bp", "zz", "alprd", "chunked", "chunked"], sliced=False)
        cdt = self.pick([d for d in (np.uint8, np.uint16, np.uint32, np.uint64) if dv.size - 1 <= np.iinfo(d).max])
        return A.dict_array(values, self.leaf(codes.astype(cdt), ["prim", "bp", "bp", "for"])), vals, m

    def _fl_delta(self, pt, n):
        vals = self.values_for("FL_DELTA", pt, n)
        varg, m = self.validity(n)
        d = E.encode_delta(vals, bitpack_deltas=self.chance(0.6))
        return A.delta(d.children[0], d.children[1], 0, n, validity=varg), vals, m

    def runs(self, pool: np.ndarray, n: int) -> np.ndarray:
        mean = int(self.pick([1, 4, 17, 300]))
        lens = np.ones(n + 1, np.int64) if mean == 1 else self.rng.integers(1, 2 * mean, n // mean + 2)
        lens = np.concatenate([lens, [n]])  # (the drawn runs may stop short of n)
        return np.repeat(pool[self.rng.integers(0, pool.size, lens.size)], lens)[:n]

    def _run_end(self, pt, n):
        pool = self.values_for("RUN_END", pt, 50)
        vals = self.runs(pool, n)
        varg, m = self.validity(n)
        ends, rv = E.runend_encode(vals)
        edt = self.pick([d for d in (np.uint16, np.uint32, np.uint64, np.int32, np.int64) if n <= np.iinfo(d).max])
        e = self.leaf(ends.astype(edt), ["prim", "bp", "delta"], sliced=False)
        v = self.leaf(rv, ["prim", "for", "bp", "zz", "zz"] if pt not in FLOATS else ["prim", "alprd"], sliced=False)
        return A.run_end(e, v, length=n, validity=varg), vals, m

    def _sparse(self, pt, n):
        pool = self.values_for("SPARSE", pt, 20)
        k = 0 if (n == 0 or self.chance(0.1)) else int(self.rng.integers(1, max(n // 20, 1) + 1))
        idx = np.sort(self.rng.choice(n, k, replace=False)).astype(np.uint64) if k else np.zeros(0, np.uint64)
        pv = pool[self.rng.integers(0, pool.size, k)]
        null_fill = self.chance(0.5)
        fill = pool[0]
        vals = np.full(n, 0 if null_fill else fill, dtype=pool.dtype)
        vals[idx.astype(np.int64)] = pv
        m = None
        if null_fill:
            m = np.zeros(n, bool)
            m[idx.astype(np.int64)] = True
        node = A.sparse(self.index_array(idx), self.leaf(pv, ["prim", "bp", "zz"], sliced=False), n,
                        fill=None if null_fill else fill, ptype=pt)
        return node, vals, m

    def _constant(self, pt, n):
        v = self.values_for("CONSTANT", pt, 1)[0]
        if self.chance(0.3):
            return A.constant(None, n, pt), np.zeros(n, NP_OF_PTYPE[pt]), np.zeros(n, bool)
        return A.constant(v, n, pt), np.full(n, v, NP_OF_PTYPE[pt]), None

    # -- bool nodes
    def bool_node(self, enc: str, n: int, sliced=None):
        if n == 0 and enc not in EMPTY_OK:
            enc = "BOOL"
        if sliced is None:
            sliced = self.chance(0.3)
        if sliced and enc == "BOOL" and n:
            start, total = self.slice_window(n)
            node, vals, valid = self.bool_node(enc, total, sliced=False)
            return slice_any(node, start, start + n), vals[start: start + n], None if valid is None else valid[start: start + n]
        bits = self.mask(n)
        if enc == "BOOL":
            varg, m = self.validity(n)
            return A.bool_array(bits, validity=varg, bit_offset=int(self.pick([0, 0, 1, 5, 7]))), bits, m
        if enc == "BYTE_BOOL":  # any non-zero byte is true
            varg, m = self.validity(n)
            raw = np.where(bits, self.rng.choice(np.array([1, 2, 0x80, 0xFF], np.uint8), n), 0).astype(np.uint8)
            return A.byte_bool(raw, validity=varg), bits, m
        if enc == "RUN_END_BOOL":
            varg, m = self.validity(n, ["NON_NULLABLE", "ALL_VALID", "BOOL", "BOOL_OFFSET", "ALL_INVALID"])
            return E.encode_runend_bool(bits, bitpack_ends=self.chance(0.5), validity=varg), bits, m
        if enc == "ROARING_BOOL":
            return E.encode_roaring_bool(bits), bits, None
        if enc == "CONSTANT":
            v = self.pick([True, False, None])
            return A.constant_bool(v, n), np.full(n, bool(v), bool), (np.zeros(n, bool) if v is None else None)
        # sparse bools: valid exactly at the indices, whatever the fill
        k = 0 if n == 0 else int(self.rng.integers(1, max(n // 10, 1) + 1))
        idx = np.sort(self.rng.choice(n, k, replace=False)).astype(np.uint64) if k else np.zeros(0, np.uint64)
        pv = self.rng.random(k) < 0.5
        fill = self.pick([True, False, None])
        vals = np.full(n, bool(fill), bool)
        vals[idx.astype(np.int64)] = pv
        m = np.zeros(n, bool)
        m[idx.astype(np.int64)] = True
        pvals = A.byte_bool(pv) if self.chance(0.5) else A.bool_array(pv, bit_offset=int(self.pick([0, 3])))
        return A.sparse_bool(self.index_array(idx), pvals, n, fill=fill), vals, m

    # -- string nodes
    def strings(self, n: int, utf8: bool) -> list:
        r = self.rng
        edge = [b"", TEXT[:12], TEXT[:13], (TEXT * 3)[:300]]
        if not utf8:
            edge.append(bytes(r.integers(128, 256, 40, dtype=np.uint8)))
        card = int(self.pick([3, 40, 100_000]))
        out = []
        for i in range(n):
            j = int(r.integers(0, card))
            if j < len(edge) and r.random() < 0.3:
                out.append(edge[j])
            else:
                a = (j * 7919) % len(TEXT)
                out.append((TEXT[a:] + TEXT)[: 1 + (j * 31) % 45])
        return out

    def fsst_node(self, strs: list, utf8: bool, varg=None) -> Array:
        """FSST over `strs` (None = a null row, no bytes), its codes' validity `varg`."""
        heap, offs, _ = E.strings_to_heap(strs)
        fs = E.encode_fsst_from_heap(heap, offs, None, compress_children=self.chance(0.5))
        syms, slen, codes, ulen = fs.children
        codes = A.varbin(codes.children[0], codes.children[1], utf8=False, validity=varg)
        return A.fsst(syms, slen, codes, ulen, utf8=utf8)

    def str_node(self, enc: str, n: int, utf8: bool, sliced=None):
        if n == 0 and enc not in ("VARBIN", "VARBINVIEW"):
            enc = "VARBIN"
        if sliced is None:
            sliced = self.chance(0.3)
        if sliced and enc in ("VARBINVIEW", "DICT") and n:
            start, total = self.slice_window(n)
            node, vals, valid = self.str_node(enc, total, utf8, sliced=False)
            return slice_any(node, start, start + n), vals[start: start + n], None if valid is None else valid[start: start + n]
        strs = self.strings(n, utf8)
        if enc == "DICT":  # dict_encode_varbin (dict/compress.rs:88-143); nullable: slot 0 is the null entry
            m = self.mask(n) if self.chance(0.5) else None
            pos = {}
            for i, s in enumerate(strs):
                if m is None or m[i]:
                    pos.setdefault(s, len(pos))
            uniq = list(pos)
            base = 0 if m is None else 1
            craw = np.array([pos[s] + base if (m is None or m[i]) else 0 for i, s in enumerate(strs)], np.uint64)
            dstr = uniq if m is None else [None] + uniq
            heap, offs, vvalid = E.strings_to_heap(dstr)
            if m is None and heap.size and self.chance(0.4):
                values = self.fsst_node(dstr, utf8)
            else:
                values = A.varbin(A.primitive(offs.astype(self.pick([np.int32, np.uint32, np.int64]))), A.primitive(heap),
                                  utf8=utf8, validity=None if m is None else vvalid)
            cdt = self.pick([d for d in (np.uint8, np.uint16, np.uint32) if len(dstr) - 1 <= np.iinfo(d).max])
            return A.dict_array(values, self.leaf(craw.astype(cdt), ["prim", "bp", "bp"])), strs, m
        varg, m = self.validity(n)
        enc_strs = [s if (m is None or m[i]) else None for i, s in enumerate(strs)]  # null rows hold no bytes
        heap, offs, _ = E.strings_to_heap(enc_strs)
        if enc == "VARBIN" or (enc == "FSST" and heap.size == 0):  # (FSST trains on the bytes: none here)
            odt = self.pick([np.int32, np.int64])
            return A.varbin(A.primitive(offs.astype(odt)), A.primitive(heap), utf8=utf8, validity=varg), strs, m
        if enc == "VARBINVIEW":
            v = E.encode_varbinview(enc_strs, utf8=utf8)
            bufs = [np.ascontiguousarray(c.buffers[0]) for c in v.children[1: 1 + v.meta["n_buffers"]]]
            return A.varbinview(np.ascontiguousarray(v.children[0].buffers[0]), bufs, utf8=utf8, validity=varg), strs, m
        return self.fsst_node(enc_strs, utf8, varg), strs, m

    # -- ChunkedArray roots
    def chunk_lens(self, cap: int) -> list:
        k = int(self.rng.integers(1, 10))
        w = np.array(CHUNK_LEN_WEIGHTS, float)
        lens = [int(x) for x in self.rng.choice(CHUNK_LENS, k, p=w / w.sum())]
        while sum(lens) > cap:
            lens[int(np.argmax(lens))] = int(self.pick([1, 64, 1023, 1025]))
        return lens

    def k1_chunk(self, pt: str, n: int, patched: bool):
        """A chunk that is one K1 decode, with or without patches (n > 8)."""
        dt = NP_OF_PTYPE[pt]
        if pt in FLOATS:
            digits = 1 if pt == "f32" else 2
            vals = np.round(self.rng.uniform(-1000, 1000, n), digits).astype(dt)
            if patched:
                k = max(n // 60, 1)
                vals[self.rng.choice(n, k, replace=False)] = (self.rng.standard_normal(k) * np.pi * 1e3).astype(dt)
            e, f, enc, idx, pv = E.alp_encode(vals)
            patches = A.sparse(self.index_array(idx), A.primitive(pv, validity="ALL_VALID"), n) if idx.size else None
            u, ref, shift = self.for_parts(enc)
            child = A.frame_of_reference(self.leaf(u, ["bp"], sliced=False), ref, shift, A.PTYPE_OF_NP[enc.dtype])
            return A.alp(child, e, f, patches), vals, None
        upt = A.unsigned_of(pt)
        u = self.ints(upt, n, "narrow")
        if not patched:
            u &= u.dtype.type(0x1F)
        ref = 3 if pt in UNSIGNED else -5
        varg, m = self.validity(n)
        child = self.leaf(u, ["bpp" if patched else "bp"], varg, m, sliced=self.chance(0.3))
        vals = (u + np.array([ref], dt).view(u.dtype)[0]).view(dt)
        return A.frame_of_reference(child, ref, 0, pt), vals, m

    def chunked_root(self, kind: str):
        lens = self.chunk_lens(STRING_ROW_CAP if kind == "str" else ROW_CAP)
        parts = [None] * len(lens)
        rare_first = {"prim": ["ZIGZAG", "ALP_RD", "ALP", "RUN_END", "FL_DELTA", "SPARSE", "CONSTANT", "DICT", "FL_FOR",
                               "FL_BITPACKED", "PRIMITIVE"],
                      "bool": ["ROARING_BOOL", "BYTE_BOOL", "RUN_END_BOOL", "SPARSE", "CONSTANT", "BOOL"],
                      "str": ["VARBINVIEW", "FSST", "DICT", "VARBIN"]}[kind]
        pt = self.pick(UNSIGNED + SIGNED + SIGNED + FLOATS + FLOATS)
        utf8 = self.chance(0.6)
        order = [e for e in rare_first if kind != "prim" or pt in PTYPES_OF[e]]
        if kind != "prim":
            k = int(self.rng.integers(0, len(order)))
            order = order[k:] + order[:k]
        big = sorted(range(len(lens)), key=lambda i: -lens[i])
        if kind == "prim" and len(lens) >= 2 and lens[big[1]] > 8 and self.chance(0.9):
            a, b = (big[0], big[1]) if self.chance(0.5) else (big[1], big[0])  # patched and patch-free K1 chunks
            parts[a] = self.k1_chunk(pt, lens[a], True)
            parts[b] = self.k1_chunk(pt, lens[b], False)
        at = 0
        for i, n in enumerate(lens):
            if parts[i] is not None:
                continue
            if n == 0:
                enc = self.pick([e for e in order if e in EMPTY_OK and (kind != "str" or e != "DICT")])
            else:
                enc, at = order[at % len(order)], at + 1
            if kind == "prim":
                parts[i] = self.prim_node(enc, pt, n, sliced=None if n else False)
            elif kind == "bool":
                parts[i] = self.bool_node(enc, n)
            else:
                parts[i] = self.str_node(enc, n, utf8)
        zero = np.zeros(0, NP_OF_PTYPE[pt] if kind == "prim" else bool)
        node = A.chunked([p[0] for p in parts])
        if kind == "str":
            vals = [s for p in parts for s in p[1]]
        else:
            vals = np.concatenate([zero] + [p[1] for p in parts])
        valid = None
        if any(p[2] is not None for p in parts):
            valid = np.concatenate([np.ones(p[0].len, bool) if p[2] is None else p[2] for p in parts])
        sliceable = ("PRIMITIVE", "FL_BITPACKED", "FL_FOR", "ZIGZAG", "ALP", "DICT", "FL_DELTA", "RUN_END", "VARBINVIEW",
                     "BOOL")  # oracle_tree.slice_any restates these (and a primitive Sparse)
        ok = all(ENC_NAME[p[0].encoding] in sliceable or (p[0].encoding == ENC["SPARSE"] and kind == "prim")
                 for p in parts)
        if ok and self.chance(0.4) and node.len > 2:  # a slice of the whole ChunkedArray
            a, b = sorted(int(x) for x in self.rng.integers(0, node.len + 1, 2))
            if a != b:
                node, vals, valid = slice_any(node, a, b), vals[a:b], None if valid is None else valid[a:b]
        return node, vals, valid

    def root(self, enc: str, kind: str):
        if enc == "CHUNKED":
            return self.chunked_root(kind)
        n = int(self.pick(SINGLE_LENS if enc in EMPTY_OK and kind != "str" else SINGLE_LENS[1:]))
        if kind == "prim":
            if enc in ("SPARSE", "CONSTANT") and self.chance(0.25):
                return self.bool_node(enc, n) + ("bool",)
            if enc == "DICT" and self.chance(0.3):
                return self.str_node("DICT", min(n, STRING_ROW_CAP), self.chance(0.6)) + ("str",)
            return self.prim_node(enc, self.pick(PTYPES_OF[enc]), n)
        if kind == "bool":
            return self.bool_node(enc, n)
        return self.str_node(enc, min(n, STRING_ROW_CAP), self.chance(0.6))

    # -- compute inputs
    def take_sets(self, n: int) -> list:
        r = self.rng

        def typed(ix):
            ix = np.asarray(ix, np.int64)
            hi = max(n - 1, 0)
            dts = [d for d in (np.uint8, np.int8, np.uint16, np.int16, np.uint32, np.int32, np.uint64, np.int64)
                   if hi <= np.iinfo(d).max]
            return ix.astype(self.pick(dts))

        out = [("empty", typed([]))]
        if n == 0:
            return out
        edges = [i for i in (0, n - 1, 1023, 1024, 1025) if 0 <= i < n]
        out.append(("one", typed([self.pick(edges + [int(r.integers(0, n))])])))
        few = edges + edges[:2] + [int(x) for x in r.integers(0, n, 16)]
        few = [few[i] for i in r.permutation(len(few))][:16]
        out.append(("few", typed(few)))
        many = np.concatenate([r.integers(0, n, n // 4 + 2), edges, edges])
        out.append(("many", typed(many[r.permutation(many.size)])))
        return out

    def predicates(self, n: int) -> list:
        r = self.rng
        one = np.zeros(n, bool)
        if n:
            one[int(self.pick([0, n - 1, int(r.integers(0, n))]))] = True
        half = r.random(n) < 0.5
        out = [("bool-50%", A.bool_array(half, bit_offset=int(self.pick([0, 3])))),
               ("bool-1%", A.bool_array(r.random(n) < 0.01)),
               ("bool-one-row", A.bool_array(one)),
               ("bool-all", A.bool_array(np.ones(n, bool))),
               ("constant-true", A.constant_bool(True, n)),
               ("constant-false", A.constant_bool(False, n))]
        if n:
            runs = np.repeat(np.arange(n + 1) % 2 == 0, r.integers(1, 40, n + 1))[:n]
            out += [("runend-50%", E.encode_runend_bool(runs, bitpack_ends=self.chance(0.5))),
                    ("runend-one-row", E.encode_runend_bool(one)),
                    ("runend-none", E.encode_runend_bool(np.zeros(n, bool)))]
        return out

    def scalars(self, kind: str, vals, valid) -> tuple:
        """-> (compare scalars, (lo_op, lo, hi_op, hi)): one taken from the data, the minimum, the
        maximum, one outside the range (where the type has one), NaN and +-0 for floats."""
        r = self.rng
        ops = self.pick([(">", "<"), (">", "<="), (">=", "<"), (">=", "<=")])
        if kind == "str":
            rows = sorted(s for i, s in enumerate(vals) if valid is None or valid[i])
            if not rows:
                return [b"", b"a"], (ops[0], b"a", ops[1], b"t")
            sc = [rows[int(r.integers(0, len(rows)))], rows[0], rows[-1], rows[-1] + b"\xff", b""]
            return sc, (ops[0], rows[len(rows) // 4], ops[1], rows[(3 * len(rows)) // 4])
        v = np.asarray(vals)
        live = v if valid is None else v[valid]
        if v.dtype.kind == "f":
            live = live[~np.isnan(live)]
        if live.size == 0:
            z = v.dtype.type(0)
            return [z, v.dtype.type(1)], (ops[0], z, ops[1], v.dtype.type(1))
        s = np.sort(live)
        sc = [live[int(r.integers(0, live.size))], s[0], s[-1]]
        if v.dtype.kind == "f":
            sc += [np.nextafter(s[-1], v.dtype.type(np.inf)) if np.isfinite(s[-1]) else np.nextafter(s[0], -s[-1]),
                   v.dtype.type(np.nan), v.dtype.type(0.0), v.dtype.type(-0.0)]
        else:
            info = np.iinfo(v.dtype)
            if int(s[-1]) < info.max:
                sc.append(v.dtype.type(int(s[-1]) + 1))
            elif int(s[0]) > info.min:
                sc.append(v.dtype.type(int(s[0]) - 1))
        return sc, (ops[0], s[live.size // 4], ops[1], s[(3 * live.size) // 4])

    # -- columns composed by route, for the seeded batches of tests/batch_cases.py
    @staticmethod
    def packed_epilogues(pt: str) -> list:
        """The packed shapes a chunk of ptype `pt` can have (PACKED_EPILOGUES)."""
        if pt in FLOATS:
            return ["alp-for"]
        return ["bp", "for", "for-shift"] if pt in UNSIGNED else ["for", "for-shift", "zz", "zz-for"]

    def cut_lens(self, n: int, k: int) -> list:
        """k chunk lengths that sum to n: cuts biased to the word, block and tile edges, zero-length
        and one-row chunks among them."""
        edges = [e for e in CUT_EDGES if e <= n] or [0]
        cuts = []
        for _ in range(k - 1):
            if cuts and self.chance(0.25):  # a zero-length or a one-row chunk
                c = cuts[int(self.rng.integers(0, len(cuts)))] + int(self.pick([0, 1]))
            elif self.chance(0.6):
                c = int(self.pick(edges)) + int(self.pick([0, 0, 1024, 4096]))
            else:
                c = int(self.rng.integers(0, n + 1))
            cuts.append(min(c, n))
        cuts = [0] + sorted(cuts) + [n]
        return [b - a for a, b in zip(cuts, cuts[1:])]

    def packed_leaf(self, u: np.ndarray, W: int, start: int, n: int, varg) -> Array:
        """Rows [start, start + n) of `u` (unsigned, values wider than W bits become patches) as a
        BitPacked array of width W with the validity `varg`: a slice when start > 0 or rows follow."""
        bp = E.encode_bitpacked(u, bit_width=W)
        patches = None
        if bp.meta["has_patches"]:
            idx = np.flatnonzero(u >> u.dtype.type(W)).astype(np.uint64)
            patches = A.sparse(self.index_array(idx), bp.children[0].children[1], u.size)
        node = A.bitpacked(bp.buffers[0], bp.ptype, W, u.size, 0, patches)
        if (start, n) != (0, u.size):
            node = slice_any(node, start, start + n)
        return A.bitpacked(node.buffers[0], node.ptype, W, n, node.meta["offset"],
                           node.children[0] if node.meta["has_patches"] else None, validity=varg)

    def packed_chunk(self, pt: str, n: int, epilogue: str, patched: bool, vkind: str = "NON_NULLABLE",
                     sliced: bool = False):
        """n >= 1 rows of ptype `pt` in the packed shape `epilogue`, its BitPacked leaf of a drawn bit
        width with or without patches (an ALP chunk: and / or exceptions), with the leaf's validity of
        kind `vkind`, a slice of a longer array when `sliced` -> (node, values, valid mask | None)."""
        r = self.rng
        T = 8 * A.ptype_width(pt)
        start, total = self.slice_window(n) if sliced else (0, n)
        varg, m = self.validity(n, [vkind])
        rows = start + np.unique(np.concatenate([r.choice(n, max(n // 40, 1), replace=False),
                                                 [0] if self.chance(0.5) else [], [n - 1] if self.chance(0.5) else []])
                                 ).astype(np.int64)  # patched rows: the first and the last row among them, or not
        if total > n and self.chance(0.7):  # ... and one outside the slice
            rows = np.append(rows, start - 1)
        if epilogue == "alp-for":
            dt = NP_OF_PTYPE[pt]
            digits = int(self.pick([0, 1] if pt == "f32" else [1, 2, 4]))
            vals = np.round(r.uniform(-1000, 1000, total), digits).astype(dt) + dt(0)  # (no -0.0: ALP gives +0.0)
            wide, exc = (patched and self.chance(0.7)), (patched and self.chance(0.6))
            if patched and not (wide or exc):
                wide = True
            if wide:  # decimals of more digits: values the leaf's width does not hold
                vals[rows] = np.round(r.uniform(1.5e5, 2e5, rows.size), digits).astype(dt)
            if exc:   # what ALP cannot encode
                at = rows[:: 2] if wide and rows.size > 1 else rows
                vals[at] = (r.standard_normal(at.size) * np.pi * 1e3).astype(dt)
            e, f, enc, idx, pv = E.alp_encode(vals)
            sp = None
            if idx.size:
                sp = slice_any(A.sparse(self.index_array(idx), A.primitive(pv, validity="ALL_VALID"), total),
                               start, start + n)
                sp = sp if sp.children[0].len else None
            u, ref, shift = self.for_parts(enc)
            base = np.delete(u, rows) if wide and rows.size < total else u
            W = max(int(base.max(initial=0)).bit_length(), 1)
            if W >= T:
                W = T - 1
            leaf = self.packed_leaf(u, W, start, n, varg)
            node = A.alp(A.frame_of_reference(leaf, ref, shift, A.PTYPE_OF_NP[enc.dtype]), e, f, sp)
            return node, vals[start: start + n].copy(), m
        upt = A.unsigned_of(pt)
        ut = NP_OF_PTYPE[upt]
        shift = {"for-shift": int(r.integers(1, 4)), "zz-for": int(self.pick([0, 0, 1]))}.get(epilogue, 0)
        top = T - 1 - shift  # the patched values stay below 2^top, so that the shift loses no bit
        W = int(r.integers(1, top)) if patched else int(r.integers(1, top + 1))
        u = r.integers(0, 1 << W, total, dtype=np.uint64)
        u[r.integers(0, total, 2)] = (1 << W) - 1  # the width's extremes are present
        u[r.integers(0, total, 2)] = 0
        if patched:
            u[rows] = r.integers(1 << W, 1 << top, rows.size, dtype=np.uint64)
        u = u.astype(ut)
        leaf = self.packed_leaf(u, W, start, n, varg)
        u = u[start: start + n]
        info = np.iinfo(NP_OF_PTYPE[pt])
        if epilogue == "bp":
            return leaf, u.copy(), m
        if epilogue in ("for", "for-shift"):  # a reference near either end of the type: the add wraps
            ref = int(self.pick([3, info.min + 7, info.max - 20, info.max // 3])) if info.min else \
                int(self.pick([3, info.max - 40, info.max // 3]))
            bits = np.array([ref], NP_OF_PTYPE[pt]).view(ut)[0]
            vals = ((u << ut(shift)) + bits).view(NP_OF_PTYPE[pt])
            return A.frame_of_reference(leaf, ref, shift, pt), vals, m
        if epilogue == "zz-for":  # ZigZag over FoR(BitPacked): the FoR is of the unsigned type
            ref = int(self.pick([0, 9, int(np.iinfo(ut).max) - 40]))
            u = (u << ut(shift)) + ut(ref)
            leaf = A.frame_of_reference(leaf, ref, shift, upt)
        vals = ((u >> ut(1)) ^ (ut(0) - (u & ut(1)))).view(NP_OF_PTYPE[pt])
        return A.zigzag(leaf), vals, m

    def empty_chunk(self, pt: str, packed: bool) -> Array:
        """A zero-length chunk: a Primitive array or, for integers, an empty FoR(BitPacked)."""
        if not packed or pt in FLOATS:
            return A.primitive(np.zeros(0, NP_OF_PTYPE[pt]), validity=self.pick([None, None, "ALL_VALID"]))
        leaf = E.encode_bitpacked(np.zeros(0, NP_OF_PTYPE[A.unsigned_of(pt)]), bit_width=3, allow_patches=False)
        return A.frame_of_reference(leaf, 0, 0, pt)

    def chunked_column(self, parts: list, pt: str, n: int, extra: int = 0, start: int = 0):
        """The ChunkedArray of `parts` ((node, values, valid mask | None) each) of n + extra rows, and
        rows [start, start + n) of it when extra > 0 -> (node, values, valid mask | None)."""
        node = A.chunked([p[0] for p in parts])
        vals = np.concatenate([np.zeros(0, NP_OF_PTYPE[pt])] + [p[1] for p in parts])
        valid = None
        if any(p[2] is not None for p in parts):
            valid = np.concatenate([np.ones(p[0].len, bool) if p[2] is None else p[2] for p in parts])
        assert node.len == n + extra
        if extra:
            node, vals = slice_any(node, start, start + n), vals[start: start + n].copy()
            valid = None if valid is None else valid[start: start + n].copy()
        return node, vals, valid

    def sliced_primitive(self, pt: str, n: int, vkind: str):
        """A Primitive array that is a slice of a longer one: its values do not start its buffer."""
        start, total = self.slice_window(n)
        vals = self.values_for("PRIMITIVE", pt, total)
        varg, m = self.validity(total, [vkind])
        node = slice_any(A.primitive(vals, validity=varg), start, start + n)
        return node, vals[start: start + n].copy(), None if m is None else m[start: start + n].copy()


@functools.lru_cache(maxsize=None)
def build(seed: int) -> TreeCase:
    """The tree of `seed`, its truth and its compute inputs; the same bytes on every call."""
    g = Gen(seed)
    enc, kind = ROOTS[seed % len(ROOTS)]
    got = g.root(enc, kind)
    if len(got) == 4:
        tree, vals, valid, kind = got
    else:
        tree, vals, valid = got
    case = TreeCase(seed, tree, vals, valid, describe(tree), kind)
    case.take_sets = g.take_sets(tree.len)
    case.predicates = g.predicates(tree.len)
    if kind != "bool":
        case.scalars, case.range = g.scalars(kind, vals, valid)
    return case


SEEDS = list(range(72))


# ---------------------------------------------------------------------------- digests
def tree_bytes(a: Array, out: list) -> list:
    """Everything a tree is made of, in walk order: each node's header, then its buffers' bytes."""
    def plain(v):  # (numpy scalars print differently from one numpy to the next)
        return bytes(v) if isinstance(v, (bytes, bytearray)) else v.item() if isinstance(v, np.generic) else v

    out.append((int(a.encoding), int(a.len), int(a.dtype), str(a.ptype), bool(a.nullable), int(a.validity),
                sorted((k, plain(v)) for k, v in a.meta.items())))
    out.extend(np.ascontiguousarray(b).tobytes() for b in a.buffers)
    for c in a.children:
        tree_bytes(c, out)
    return out


def digest(case: TreeCase) -> str:
    """sha256 over `describe`, every buffer of the tree and the compute inputs: what
    tests/golden/tree_digests.json records per seed, so that a change of the generator is seen."""
    import hashlib
    h = hashlib.sha256()

    def feed(x):
        h.update(x if isinstance(x, bytes) else repr(x).encode())
        h.update(b"\x00")

    def feed_tree(a):
        for x in tree_bytes(a, []):
            feed(x)

    feed(case.describe)
    feed(case.kind)
    feed_tree(case.tree)
    for name, ix in case.take_sets:
        feed((name, str(ix.dtype)))
        feed(ix.tobytes())
    for name, p in case.predicates:
        feed(name)
        feed_tree(p)
    for s in list(case.scalars) + list(case.range or ()):
        feed(s if isinstance(s, (bytes, str)) else (str(np.asarray(s).dtype), np.asarray(s).tobytes()))
    return h.hexdigest()


if __name__ == "__main__":  # PYTHONPATH=. python tests/tree_cases.py > tests/golden/tree_digests.json
    import json
    print(json.dumps({str(s): digest(build(s)) for s in SEEDS}, indent=0))
