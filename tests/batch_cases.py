"""Seeded scan batches: the columns, masks and conjunctions one scan step sees, per seed.

Plain module: numpy, the host encoders and tree_cases.Gen -- no GPU, no torch.  `build(seed)` draws
everything from np.random.default_rng([0xBA7C, seed]), so a batch follows from its seed alone.  A
batch is what vxg_row_filter and vxg_filter_batch work on together: 6 to 10 columns of one length n
composed by ROUTE (the planner's decision, as include/vortex_gpu.h states it under "Routes, per
column"), the masks a scan can hand over and a few conjunctions over the value columns.

Columns, per batch: a packed single array (every type width, every epilogue the ptype allows, with
and without BitPacked patches and ALP exceptions, sliced or not, every validity kind); one to three
packed ChunkedArrays whose chunks each draw their own epilogue, bit width, reference, shift, slice
offset, patches and validity kind -- zero-length and one-row chunks among them, cut at the word,
block and tile edges, some of them a slice of a longer column that starts off every 64-row
boundary; a sliced Primitive array and a ChunkedArray of Primitive chunks (in place); one encoding
of Gen.prim_node / bool_node / str_node each, rotating over the seeds, and a ChunkedArray that is
packed but for one Primitive or Dict chunk (fallback).  ALP directly over BitPacked is not built:
ALP's child is signed and the constructors pack unsigned integers only.

A seed that is a tuple names a group of tree_cases seeds whose trees have one length: those trees
are the batch's columns as they stand.

`expected_route(tree)` restates the header's route rule (plus compare's gate that a ZigZag is
signed); tests/test_gpu_batches.py holds vxg_filter_batch_info to it.  tests/test_batch_cases.py
holds every column, mask and conjunction against the oracle on the CPU.
"""
from __future__ import annotations

import collections
import functools
import operator
from dataclasses import dataclass, field
from typing import Optional

import numpy as np

import tree_cases as TC
import vortex_amd.arrays as A
from tree_cases import FLOATS, SIGNED, UNSIGNED, VALIDITY_KINDS, Gen
from vortex_amd._lib import DTYPE, ENC
from vortex_amd.arrays import NP_OF_PTYPE, Array

OPS = {"==": operator.eq, "!=": operator.ne, ">": operator.gt, ">=": operator.ge, "<": operator.lt, "<=": operator.le}

# the edges the kernels are built around (mask word 64, FastLanes block 1024, tile 4096, two tiles), then odd lengths
EDGE_LENS = [0, 1, 63, 64, 65, 1023, 1024, 1025, 2047, 4095, 4096, 4097, 8193]
ODD_LENS = [200, 777, 1500, 2085, 3073, 3333, 5001, 6143, 7000, 8191, 8999]
LENS = EDGE_LENS + ODD_LENS
MAX_ROWS, MAX_COLUMNS = 9000, 10

# packed Chunked column c (counted over all seeds) has ptype PT_CYCLE[c % 22]: signed types allow four epilogues
PT_CYCLE = SIGNED * 3 + UNSIGNED * 2 + FLOATS
FALLBACK_PRIM = ["DICT", "RUN_END", "FL_DELTA", "ALP_RD", "SPARSE", "CONSTANT"]
FALLBACK_BOOL = TC.BOOL_ENCS
FALLBACK_STR = TC.STR_ENCS


@dataclass
class Column:
    tree: Array
    values: object                 # ndarray (primitive), bool mask (bool), list of bytes (strings)
    valid: Optional[np.ndarray]    # bool mask, or None = every row valid
    kind: str                      # "prim" | "bool" | "str"
    describe: str
    route: tuple                   # expected_route(tree)
    made_as: str                   # what the generator meant it to be (the route it is composed for)
    scalars: list = field(default_factory=list)
    range: Optional[tuple] = None
    seed: object = None            # (assert_canonical_is_truth names it)
    whole_slice: int = 0           # > 0: rows [whole_slice, whole_slice + n) of a longer ChunkedArray


@dataclass
class BatchCase:
    seed: object
    n: int
    columns: list
    masks: list = field(default_factory=list)          # (name, bool mask, dirty_tail)
    conjunctions: list = field(default_factory=list)   # (name, [(column index, op, scalar)], row mask by numpy)
    describe: str = ""


# ---------------------------------------------------------------------------- the route predictor
def _bitpacked(a: Optional[Array], width: int) -> bool:
    return a is not None and a.encoding == ENC["FL_BITPACKED"] and A.ptype_width(a.ptype) == width


def _bp_or_for(a: Optional[Array], width: int) -> bool:
    if a is not None and a.encoding == ENC["FL_FOR"]:
        return _bitpacked(a.children[0], width)
    return _bitpacked(a, width)


def packed_shape(a: Array) -> bool:
    """"BitPacked, FoR(BitPacked), ZigZag or ALP over either" (a ZigZag of a signed type: compare's gate)."""
    if a.dtype != DTYPE["PRIMITIVE"]:
        return False
    w = A.ptype_width(a.ptype)
    if a.encoding == ENC["FL_BITPACKED"]:
        return True
    if a.encoding == ENC["FL_FOR"]:
        return _bitpacked(a.children[0], w)
    if a.encoding == ENC["ZIGZAG"]:
        return a.ptype in SIGNED and _bp_or_for(a.children[0], w)
    if a.encoding == ENC["ALP"]:
        return _bp_or_for(a.children[0], w)
    return False


def pieces(tree: Array) -> list:
    """The array itself, or the chunks of a top-level ChunkedArray."""
    return list(tree.children[1:]) if tree.encoding == ENC["CHUNKED"] else [tree]


def expected_route(tree: Array) -> tuple:
    """("packed", non-empty packed pieces) | ("inplace", non-empty Primitive pieces) | ("fallback", 1),
    from the header's "Routes, per column": packed when the array, or every non-empty chunk of a
    top-level Chunked, has a packed shape; in place when it is a Primitive array or every non-empty
    chunk is one; everything else -- mixed chunks, every other encoding, Bool and string columns --
    falls back whole."""
    if tree.dtype != DTYPE["PRIMITIVE"]:
        return ("fallback", 1)
    live = [p for p in pieces(tree) if p.len]
    if live and all(packed_shape(p) for p in live):
        return ("packed", len(live))
    if all(p.encoding == ENC["PRIMITIVE"] for p in live):
        return ("inplace", len(live))
    return ("fallback", 1)


def epilogue_of(a: Array) -> Optional[str]:
    """The PACKED_EPILOGUES name of a packed shape (None: not one)."""
    if not packed_shape(a):
        return None
    kid = a.children[0] if a.encoding != ENC["FL_BITPACKED"] else None
    if a.encoding == ENC["FL_BITPACKED"]:
        return "bp"
    if a.encoding == ENC["FL_FOR"]:
        return "for-shift" if a.meta["shift"] else "for"
    if a.encoding == ENC["ZIGZAG"]:
        return "zz-for" if kid.encoding == ENC["FL_FOR"] else "zz"
    return "alp-for" if kid.encoding == ENC["FL_FOR"] else "alp"


def packed_leaf_of(a: Array) -> Array:
    while a.encoding != ENC["FL_BITPACKED"]:
        a = a.children[0]
    return a


# ---------------------------------------------------------------------------- truth by numpy alone
def truth_mask(col: Column, op: str, scalar) -> np.ndarray:
    """Rows where `value <op> scalar` holds and the row is valid, from the plain truth."""
    n = len(col.values)
    valid = np.ones(n, bool) if col.valid is None else np.asarray(col.valid, bool)
    if col.kind == "str":
        m = np.fromiter((OPS[op](s, scalar) for s in col.values), bool, n)
    else:
        vals = np.asarray(col.values)
        with np.errstate(invalid="ignore"):
            m = np.asarray(OPS[op](vals, np.asarray(scalar).astype(vals.dtype)), bool)
    return m & valid


# ---------------------------------------------------------------------------- columns
class BatchGen(Gen):
    def __init__(self, seed_words):
        super().__init__(0)
        self.rng = np.random.default_rng([0xBA7C] + [int(w) for w in seed_words])

    def vkind(self) -> str:
        return self.pick(VALIDITY_KINDS)

    def packed_single(self, n: int):
        pt = self.pick(UNSIGNED + SIGNED + FLOATS)
        if n == 0:  # (an empty FoR(BitPacked): integers)
            pt = self.pick(UNSIGNED + SIGNED)
            return self.empty_chunk(pt, True), np.zeros(0, NP_OF_PTYPE[pt]), None
        return self.packed_chunk(pt, n, self.pick(self.packed_epilogues(pt)), self.chance(0.5), self.vkind(),
                                 sliced=self.chance(0.5))

    def packed_chunks(self, pt: str, lens: list, base: int) -> list:
        """One packed chunk per length; non-empty chunk i takes (epilogue, patched) number base + i of
        the ptype's list, so one column holds different epilogues (and widths: each chunk draws its own)."""
        cells = [(e, p) for e in self.packed_epilogues(pt) for p in (False, True)]
        parts, i = [], 0
        for m in lens:
            if m == 0:
                parts.append((self.empty_chunk(pt, self.chance(0.6)), np.zeros(0, NP_OF_PTYPE[pt]), None))
                continue
            epi, patched = cells[(base + i) % len(cells)]
            i += 1
            parts.append(self.packed_chunk(pt, m, epi, patched, self.vkind(), sliced=self.chance(0.4)))
        return parts

    def window(self, n: int):
        """(extra, start): the column is rows [start, start + n) of n + extra rows; start off a 64-row boundary."""
        if n < 2 or not self.chance(0.35):
            return 0, 0
        start = int(self.pick([1, 7, 63, 65, 1000, 1023, 1025, 1500]))
        return start + int(self.pick([0, 1, 9, 1024])), start

    def packed_chunked(self, n: int, pt: str, base: int):
        extra, start = self.window(n)
        lens = self.cut_lens(n + extra, int(self.rng.integers(2, 8)))
        parts = self.packed_chunks(pt, lens, base)
        return self.chunked_column(parts, pt, n, extra, start) + (start if extra else 0,)

    def inplace_single(self, n: int):
        pt = self.pick(UNSIGNED + SIGNED + FLOATS)
        if n == 0:
            vals = np.zeros(0, NP_OF_PTYPE[pt])
            return A.primitive(vals, validity=self.pick([None, "ALL_VALID"])), vals, None
        return self.sliced_primitive(pt, n, self.vkind())

    def inplace_chunked(self, n: int):
        pt = self.pick(UNSIGNED + SIGNED + FLOATS)
        parts = []
        for m in self.cut_lens(n, int(self.rng.integers(2, 7))):
            if m == 0:
                parts.append((self.empty_chunk(pt, False), np.zeros(0, NP_OF_PTYPE[pt]), None))
            elif self.chance(0.4):
                parts.append(self.sliced_primitive(pt, m, self.vkind()))
            else:
                vals = self.values_for("PRIMITIVE", pt, m)
                varg, vm = self.validity(m, [self.vkind()])
                parts.append((A.primitive(vals, validity=varg), vals, vm))
        return self.chunked_column(parts, pt, n)

    def fallback_chunked(self, n: int):
        """Packed chunks but for one Primitive or Dict chunk: the column falls back whole."""
        pt = self.pick(UNSIGNED + SIGNED + FLOATS)
        lens = self.cut_lens(n, int(self.rng.integers(2, 6)))
        parts = self.packed_chunks(pt, lens, int(self.rng.integers(0, 8)))
        live = [i for i, m in enumerate(lens) if m]
        i = int(self.pick(live))
        if self.chance(0.5):
            parts[i] = self.prim_node("DICT", pt, lens[i], sliced=False)
        else:
            vals = self.values_for("PRIMITIVE", pt, lens[i])
            varg, vm = self.validity(lens[i], [self.vkind()])
            parts[i] = (A.primitive(vals, validity=varg), vals, vm)
        return self.chunked_column(parts, pt, n)


def _column(got, kind: str, made_as: str, seed) -> Column:
    tree, vals, valid = got[:3]
    return Column(tree, vals, valid, kind, TC.describe(tree), expected_route(tree), made_as, seed=seed,
                  whole_slice=got[3] if len(got) > 3 else 0)


def _columns(g: BatchGen, seed: int, n: int) -> list:
    cols = [_column(g.packed_single(n), "prim", "packed", seed),
            _column(g.inplace_single(n), "prim", "inplace", seed),
            _column(g.inplace_chunked(n), "prim", "inplace-chunked", seed)]
    n_chunked = 0 if n < 2 else 1 if n < 64 else 2 if n < 1023 else 3
    for j in range(n_chunked):
        # column c = 3 * seed + j of all seeds' packed Chunked columns: its ptype by PT_CYCLE, and its first chunk's
        # (epilogue, patched) three further down the ptype's list at every visit, so that the seeds cover the list
        c = 3 * seed + j
        pt = PT_CYCLE[c % len(PT_CYCLE)]
        visit = (c // len(PT_CYCLE)) * PT_CYCLE.count(pt) + PT_CYCLE[: c % len(PT_CYCLE)].count(pt)
        cols.append(_column(g.packed_chunked(n, pt, 3 * visit), "prim", "packed-chunked", seed))
    enc = FALLBACK_PRIM[seed % len(FALLBACK_PRIM)]
    cols.append(_column(g.prim_node(enc, g.pick(TC.PTYPES_OF[enc]), n), "prim", "fallback", seed))
    if n >= 2:
        cols.append(_column(g.fallback_chunked(n), "prim", "fallback-chunked", seed))
    cols.append(_column(g.str_node(FALLBACK_STR[seed % len(FALLBACK_STR)], n, g.chance(0.6)), "str", "fallback", seed))
    cols.append(_column(g.bool_node(FALLBACK_BOOL[seed % len(FALLBACK_BOOL)], n), "bool", "fallback", seed))
    assert len(cols) <= MAX_COLUMNS
    order = g.rng.permutation(len(cols))
    return [cols[i] for i in order]


# ---------------------------------------------------------------------------- masks
def _masks(g: BatchGen, n: int) -> list:
    r = g.rng
    first, last = np.zeros(n, bool), np.zeros(n, bool)
    first[:1] = True
    last[max(n - 1, 0):] = True
    runs = np.repeat(np.arange(n + 1) % 2 == 0, r.integers(1, 41, n + 1))[:n]
    out = [("zero", np.zeros(n, bool), False), ("all", np.ones(n, bool), False), ("first", first, False),
           ("last", last, False), ("50%", r.random(n) < 0.5, False), ("2%", r.random(n) < 0.02, False),
           ("words", (np.arange(n) // 64) % 2 == 0, False), ("runs", runs, False)]
    if n >= 3072:  # one whole 1024-row block empty between full ones
        hole = np.ones(n, bool)
        b = 1024 * int(r.integers(1, n // 1024 - 1))
        hole[b: b + 1024] = False
        out.append(("hole", hole, False))
    out.append(("dirty-tail", r.random(n) < 0.4, True))  # the bits past n in the last word are all set
    return out


# ---------------------------------------------------------------------------- conjunctions
def _conjunctions(g: BatchGen, cols: list, n: int, long_one: bool) -> list:
    def some_valid(i):
        return cols[i].valid is None or bool(np.any(cols[i].valid))

    every = [i for i, c in enumerate(cols) if c.kind != "bool"]
    value = [i for i in every if some_valid(i)] or every  # (a column without a valid row empties every conjunction)
    prims = [i for i in value if cols[i].kind == "prim"] or [i for i in every if cols[i].kind == "prim"]
    strs = [i for i in value if cols[i].kind == "str"] or [i for i in every if cols[i].kind == "str"]
    nullable = [i for i in value if cols[i].valid is not None] or value
    live_prims = prims

    def candidates(i):
        c = cols[i]
        lo_op, lo, hi_op, hi = c.range
        sc = c.scalars
        return [(lo_op, lo), (hi_op, hi), (">=", sc[1]), ("<=", sc[2] if len(sc) > 2 else sc[-1]), ("!=", sc[0]),
                ("==", sc[0]), ("<", sc[-1]), (">", sc[-1])]

    def conjunct(i, running, mild=False):
        """One conjunct on column i: the first of its candidates, in a drawn order, that leaves rows."""
        cand = candidates(i)
        cand = cand[2:5] if mild else cand
        order = [cand[j] for j in g.rng.permutation(len(cand))]
        for op, s in order:
            if n == 0 or (running & truth_mask(cols[i], op, s)).any():
                return (i, op, s)
        return (i,) + order[0]

    def ranged(among):
        """A column of `among`, in a drawn order, whose two-sided range keeps some rows and drops some."""
        order = [among[j] for j in g.rng.permutation(len(among))]
        for i in order:
            lo_op, lo, hi_op, hi = cols[i].range
            k = int((truth_mask(cols[i], lo_op, lo) & truth_mask(cols[i], hi_op, hi)).sum())
            if 0 < k < n:
                return i
        return order[0]

    def finish(name, conj):
        m = np.ones(n, bool)
        for i, op, s in conj:
            m &= truth_mask(cols[i], op, s)
        return (name, conj, m)

    def extend(conj, more, mild=False):
        running = finish("", conj)[2]
        for i in more:
            c = conjunct(i, running, mild)
            conj.append(c)
            running &= truth_mask(cols[c[0]], c[1], c[2])
        return conj

    out = []
    # a two-sided range on one column beside conjuncts on other columns, a string among them
    p = ranged(live_prims)
    lo_op, lo, hi_op, hi = cols[p].range
    others = [int(g.pick(strs))] + [int(g.pick([i for i in value if i != p] or value))
                                    for _ in range(int(g.rng.integers(0, 3)))]
    out.append(finish("range+others", extend([(p, lo_op, lo), (p, hi_op, hi)], others)))
    # one column in three conjuncts: the first lower bound pairs with the first upper bound
    t = ranged(live_prims)
    lo_op, lo, hi_op, hi = cols[t].range
    sc = cols[t].scalars
    third = g.pick([(">=", sc[1]), ("!=", sc[0]), ("<=", sc[min(2, len(sc) - 1)])])
    triple = [(t, lo_op, lo), (t, hi_op, hi), (t,) + tuple(third)]
    out.append(finish("one-column-thrice", [triple[i] for i in g.rng.permutation(3)]))
    # a conjunct on a nullable column, a string conjunct
    out.append(finish("nullable+string", extend([], [int(g.pick(nullable)), int(g.pick(strs))])))
    if g.chance(0.5):
        out.append(finish("single", extend([], [int(g.pick(value))])))
    if long_one:  # 17 conjuncts: the 16-bitmap combine takes two launches
        cyc = [value[i % len(value)] for i in range(15)]
        out = out[:3] + [finish("seventeen", extend([(p, cols[p].range[0], cols[p].range[1]),
                                                       (p, cols[p].range[2], cols[p].range[3])], cyc, mild=True))]
        assert len(out[-1][1]) == 17
    return out


# ---------------------------------------------------------------------------- build
def _describe(seed, n, cols) -> str:
    return f"batch {seed}: n={n} " + " | ".join(f"{c.route[0]}:{c.describe}" for c in cols)


LONG_CONJUNCTION_SEED = 7  # n = 1025


@functools.lru_cache(maxsize=None)
def build(seed) -> BatchCase:
    """The batch of `seed` (an integer, or a tuple of tree_cases seeds of one length); the same bytes on every call."""
    if isinstance(seed, tuple):
        cases = [TC.build(s) for s in seed]
        n = cases[0].tree.len
        assert all(c.tree.len == n for c in cases)
        g = BatchGen([0x67] + list(seed))
        cols = [Column(c.tree, c.values, c.valid, c.kind, c.describe, expected_route(c.tree), "tree", list(c.scalars),
                       c.range, seed=c.seed) for c in cases]
    else:
        g = BatchGen([seed])
        n = LENS[seed % len(LENS)]
        cols = _columns(g, seed, n)
        for c in cols:
            if c.kind != "bool":
                c.scalars, c.range = g.scalars(c.kind, c.values, c.valid)
    case = BatchCase(seed, n, cols, describe=_describe(seed, n, cols))
    case.masks = _masks(g, n)
    value = [c for c in cols if c.kind != "bool"]
    if value and any(c.kind == "str" for c in cols) and any(c.kind == "prim" for c in cols):
        case.conjunctions = _conjunctions(g, cols, n, seed == LONG_CONJUNCTION_SEED)
    elif value:  # a group of existing trees without a string (or without a primitive) column: ranges only
        for i, c in enumerate(cols):
            if c.kind != "bool" and len(case.conjunctions) < 4:
                conj = [(i, c.range[0], c.range[1]), (i, c.range[2], c.range[3])]
                m = truth_mask(c, *conj[0][1:]) & truth_mask(c, *conj[1][1:])
                case.conjunctions.append((f"range-{i}", conj, m))
    case.masks += [(f"conjunction-{name}", m, False) for name, _, m in case.conjunctions]
    return case


def tree_groups() -> list:
    """Every group of two or more tree_cases seeds whose trees have one length, as a tuple of seeds."""
    by_len = collections.defaultdict(list)
    for s in TC.SEEDS:
        by_len[TC.build(s).tree.len].append(s)
    return [tuple(v) for _, v in sorted(by_len.items()) if len(v) >= 2]


GENERATED_SEEDS = list(range(24))
BATCH_SEEDS = GENERATED_SEEDS + tree_groups()


def seed_id(seed) -> str:
    return str(seed) if not isinstance(seed, tuple) else "trees-" + "-".join(str(s) for s in seed)
