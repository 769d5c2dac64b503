"""GPU: every seeded tree and scan batch through the FILE READER and then every route of the engine,
bit for bit.

tests/test_gpu_trees.py and tests/test_gpu_batches.py upload every buffer of a Python Array as its own
allocation.  A scan does not: it parses a Vortex file, copies a column's chunk range to the device
with one H2D copy and lets the reader (vortex_amd/csrc/serde.cpp) build the vxg_array tree with
pointers into that one region -- buffers 64-byte aligned and back to back, separated by zero padding
and flatbuffer bytes, the column's end covered by REGION_SLACK, the chunk offsets a separate device
buffer, every child's dtype, nullability and length derived from its parent's metadata.  Here the
inputs come through VortexFile + DeviceColumns only (tests/file_cases.py writes the files); nothing
calls Array.to on a tree under test, and the node handed to the engine is the reader's own.

Per tree seed: the direct canonicalize (file.scan) and a plan (launched, refreshed, launched again),
for the whole column and for every chunk range of file_cases.chunk_ranges; the same with every byte
of the region that is no buffer of the tree overwritten with 0xA5, then 0x00; a plan over the columns
of eight files (both plan-batch settings, both VXG_PLAN_FUSE settings); take, filter, compare and the
row filter on the reader's node with the case's own inputs.  Per batch seed: vxg_row_filter with each
conjunction over the reader's column nodes and vxg_filter_batch of all the file's columns under each
mask, the info counters held to batch_cases.expected_route.  Expectations are the oracle's, computed
from file_cases.as_file's trees (tests/test_file_cases.py holds those against the truth on the CPU);
equality is exact, and every assertion names the seed and the tree.
"""
import ctypes as C

import numpy as np
import pytest

import batch_cases as BC
import compare_bytes_expected
import compare_expected
import file_cases as FC
import row_filter_expected
import tree_cases as TC
import vortex_amd as V
import vortex_amd._lib as L
import vortex_amd.arrays as A
from file_tree_check import leaf_buffers
from filter_batch_run import run
from oracle_tree import canon, filter_canon
from plan_env import env_set, plan_mode
from rows_check import check_rows, full
from take_expected import take_canon
from test_gpu_batches import check_info
from vortex_amd.file import REGION_SLACK, DeviceColumns, VortexFile, scan

pytestmark = pytest.mark.gpu

OPS = list(compare_expected.OPS)
GROUPS = [FC.TREE_SEEDS[i: i + 8] for i in range(0, len(FC.TREE_SEEDS), 8)]
VALUE_SEEDS = [s for s in FC.TREE_SEEDS if TC.build(s).kind != "bool"]  # compare and row filter take no Bool column
BATCH_IDS = [BC.seed_id(s) for s in FC.BATCH_SEEDS]
POISONS = [0xA5, 0x00]


def _dev():
    import torch
    return torch.device("cuda", 0)


@pytest.fixture(autouse=True)
def stop_after_a_gpu_fault(ctx):
    """A tree that faults the device ends the session: nothing more is started on a faulted GPU."""
    yield
    try:
        ctx.sync()
    except V.VortexGpuError as e:
        if e.kind == "HipError":
            pytest.exit(f"the GPU reported {e}: not starting further GPU tests", returncode=3)


class Staged:
    """A tree seed's file, its column in device memory as the reader built it, and the oracle's
    canonical of the written chunks (computed once)."""

    def __init__(self, seed, ctx):
        self.tf = FC.tree_file(seed)
        self.case = self.tf.case
        self.kind = self.case.kind
        self.k = len(self.tf.chunks)
        self.tree = FC.range_tree(self.tf, 0, self.k)  # the column as the reader states it: a ChunkedArray of its chunks
        self.want, self.valid = canon(self.tree)
        self.file = VortexFile(self.tf.data)
        self.dc = DeviceColumns(self.file, ctx)
        self.node = self.dc.nodes[0]
        self.rows = compare_bytes_expected.rows_of(self.tree) if self.kind == "str" else None

    def at(self, route):
        return f"seed {self.case.seed} [file: {route}]: {self.case.describe}"


_STAGED: dict = {}


def staged(seed, ctx) -> Staged:
    if seed not in _STAGED:
        _STAGED[seed] = Staged(seed, ctx)
    return _STAGED[seed]


def direct(ctx, node):
    """vxg_canonicalize of a reader's node into outputs allocated here (what file.scan does per column)."""
    keep: list = []
    o, res = A.alloc_canonical(ctx, node, keep)
    L.check(ctx.lib.vxg_canonicalize(ctx.handle, C.byref(node), C.byref(o), ctx.stream_ptr()))
    if res.validity is not None and not o.validity:
        res.validity = None
    res._keep = keep
    ctx.sync()
    return res


def plan_twice(ctx, dc, kind, want, valid, at):
    """One plan over the reader's nodes of `dc`: launched, the bytes copied again, launched again."""
    plan = A.Plan(dc.nodes, ctx)
    try:
        for launch in (1, 2):
            res = plan.launch(sync=True)[0]
            check_rows(kind, res, want, valid, at + f", plan launch {launch}")
            dc.refresh()
            ctx.sync()
    finally:
        plan.close()


# ---------------------------------------------------------------------------- decode
@pytest.mark.parametrize("seed", FC.TREE_SEEDS)
def test_decode(ctx, seed):
    st = staged(seed, ctx)
    res = scan(st.file, ctx)[0]
    check_rows(st.kind, res, st.want, st.valid, st.at("scan"))
    plan_twice(ctx, st.dc, st.kind, st.want, st.valid, st.at("whole column"))
    check_rows(st.kind, res, st.want, st.valid, st.at("scan, after the plan"))
    for c0, c1 in FC.chunk_ranges(st.tf):
        want, valid = canon(FC.range_tree(st.tf, c0, c1))
        dc = DeviceColumns(st.file, ctx, None, c0, c1)
        at = st.at(f"chunks [{c0}, {c1}) of {st.k}")
        check_rows(st.kind, direct(ctx, dc.nodes[0]), want, valid, at + ", direct")
        plan_twice(ctx, dc, st.kind, want, valid, at)


def poison(dc, value: int) -> int:
    """Every byte of the column's device region that lies in no buffer of the reader's tree -- the
    message flatbuffers, the zero padding between buffers, the REGION_SLACK tail -- overwritten with
    `value`.  Returns how many bytes that were."""
    import torch
    region, node = dc.regions[0], dc.nodes[0]
    host = region.cpu().numpy().copy()
    keep = np.zeros(host.size, bool)
    base = region.data_ptr()
    for ptr, n in leaf_buffers(node):
        if ptr == dc.offsets[0].data_ptr():  # the chunk offsets: a buffer of their own
            continue
        assert base <= ptr and ptr + n <= base + host.size
        keep[ptr - base: ptr - base + n] = True
    host[~keep] = value
    region.copy_(torch.from_numpy(host))
    return int((~keep).sum())


@pytest.mark.parametrize("seed", FC.TREE_SEEDS)
def test_poisoned_region(ctx, seed):
    """What lies between and after the buffers is not the tree's: decode must not depend on it."""
    st = staged(seed, ctx)
    before = direct(ctx, st.node)
    check_rows(st.kind, before, st.want, st.valid, st.at("direct, before the poison"))
    dc = DeviceColumns(st.file, ctx)  # a region of its own: the staged one stays as the file is
    for value in POISONS:
        assert poison(dc, value) >= REGION_SLACK
        ctx.sync()
        at = st.at(f"region poisoned with {value:#04x}")
        check_rows(st.kind, direct(ctx, dc.nodes[0]), st.want, st.valid, at + ", direct")
        plan = A.Plan(dc.nodes, ctx)
        try:
            for launch in (1, 2):
                check_rows(st.kind, plan.launch(sync=True)[0], st.want, st.valid, at + f", plan launch {launch}")
        finally:
            plan.close()
    check_rows(st.kind, before, st.want, st.valid, st.at("direct, after the poisoned runs"))


@pytest.mark.parametrize("fuse", ["1", "0"])
@pytest.mark.parametrize("batch", ["1", "0"])
@pytest.mark.parametrize("group", range(len(GROUPS)))
def test_plan_over_eight_files(ctx, group, batch, fuse):
    """One plan over the columns of eight files -- the mix of regions a multi-column scan records:
    every output checked on two launches, and the direct outputs taken before it checked again."""
    sts = [staged(s, ctx) for s in GROUPS[group]]
    before = [direct(ctx, st.node) for st in sts]
    with env_set(VXG_PLAN_FUSE=fuse), plan_mode(batch):
        plan = A.Plan([st.node for st in sts], ctx)
    try:
        for launch in (1, 2):
            res = plan.launch(sync=True)
            for st, r in zip(sts, res):
                check_rows(st.kind, r, st.want, st.valid,
                           st.at(f"plan of seeds {GROUPS[group]} batch={batch} fuse={fuse} launch {launch}"))
    finally:
        plan.close()
    for st, d in zip(sts, before):
        check_rows(st.kind, d, st.want, st.valid, st.at(f"direct, after the plan of seeds {GROUPS[group]}"))


# ---------------------------------------------------------------------------- compute on the reader's node
@pytest.mark.parametrize("seed", FC.TREE_SEEDS)
def test_take(ctx, seed):
    st = staged(seed, ctx)
    for name, idx in st.case.take_sets:
        want, wvalid = take_canon(st.tree, idx, canonical=(st.want, st.valid) if st.kind == "str" else None)
        for force in (False, True):
            res = A.take(st.node, idx, ctx, force_canonical=force)
            check_rows(st.kind, res, want, wvalid, st.at(f"take {name}: {idx.size} x {idx.dtype} force_canonical={force}"))


@pytest.mark.parametrize("seed", FC.TREE_SEEDS)
def test_filter(ctx, seed):
    st = staged(seed, ctx)
    for name, pred in st.case.predicates:
        want, wvalid = filter_canon(st.tree, pred)
        res = A.filter(st.node, pred.to(_dev()), ctx)
        check_rows(st.kind, res, want, wvalid, st.at(f"filter {name}"))


def compare_want(st, op, scalar):
    """-> (values bitmap, validity bitmap | None) of compare(column, op, scalar)."""
    if st.kind == "str":
        return compare_bytes_expected.expected(st.tree, op, scalar, rows=st.rows)[:2]
    m = compare_expected.compare_values(np.asarray(st.want), st.valid, op, scalar)
    return compare_expected.bitmap(m), (None if st.valid is None else compare_expected.bitmap(st.valid))


@pytest.mark.parametrize("seed", VALUE_SEEDS)
def test_compare(ctx, seed):
    st = staged(seed, ctx)
    n = st.tree.len
    nb = ((n + 63) // 64) * 8
    for scalar in st.case.scalars:
        for op in OPS:
            want, _ = compare_want(st, op, scalar)
            for null_as_false in (False, True):
                at = st.at(f"compare {op} {scalar!r} null_as_false={null_as_false}")
                res = A.compare(st.node, op, scalar, ctx, null_as_false=null_as_false)
                assert res.kind == "bool" and res.len == n, at
                assert res.values.cpu().numpy()[:nb].tobytes() == want, "values differ, " + at
                if null_as_false or res.validity is None:
                    assert res.validity is None and (null_as_false or full(st.valid, n).all()), "validity differs, " + at
                else:
                    assert res.validity.cpu().numpy()[:nb].tobytes() == compare_expected.bitmap(full(st.valid, n)), \
                        "validity differs, " + at


@pytest.mark.parametrize("seed", VALUE_SEEDS)
def test_row_filter(ctx, seed):
    st = staged(seed, ctx)
    lo_op, lo, hi_op, hi = st.case.range
    want, mask, count = row_filter_expected.expected([(st.tree, lo_op, lo), (st.tree, hi_op, hi)])
    nb = ((st.tree.len + 63) // 64) * 8
    kept, kvalid = filter_canon(st.tree, A.bool_array(mask))
    for flags, name in ((L.ROWF_FUSE_RANGES, "paired"), (L.ROWF_NO_FUSE_RANGES, "unpaired")):
        at = st.at(f"row filter {lo_op} {lo!r} and {hi_op} {hi!r}, {name}")
        res = A.row_filter([(st.node, lo_op, lo), (st.node, hi_op, hi)], ctx, flags=flags)
        assert res.values.cpu().numpy()[:nb].tobytes() == want, "mask differs, " + at
        assert res.true_count == count, f"true count {res.true_count} != {count}, " + at
        # both conjuncts name the reader's one node: a primitive column's bounds pair (vortex_gpu.h, "Range pairing")
        paired = st.kind == "prim" and flags == L.ROWF_FUSE_RANGES
        assert res.info["range_pairs"] == (1 if paired else 0), (res.info, at)
        got = A.filter(st.node, A.predicate_from(res), ctx)
        check_rows(st.kind, got, kept, kvalid, at + ", then filter")


# ---------------------------------------------------------------------------- batches
class StagedBatch:
    """A batch's file, all of its columns in device memory as the reader built them, and the columns
    as the reader states them (ChunkedArrays of the written chunks) for the oracle."""

    def __init__(self, seed, ctx):
        self.bf = FC.batch_file(seed)
        self.case = self.bf.case
        self.cols = self.case.columns
        self.trees = [FC.range_tree(c, 0, len(c.chunks)) for c in self.bf.columns]
        self.file = VortexFile(self.bf.data)
        self.dc = DeviceColumns(self.file, ctx)
        self.nodes = self.dc.nodes

    def at(self, what):
        return f"[file: {what}] {self.case.describe}"


@pytest.mark.parametrize("seed", FC.BATCH_SEEDS, ids=BATCH_IDS)
def test_batch_row_filter_and_filter_batch(ctx, seed):
    st = StagedBatch(seed, ctx)
    n = st.case.n
    nb = ((n + 63) // 64) * 8
    assert st.file.row_count == n and [int(nd.len) for nd in st.nodes] == [n] * len(st.cols), st.at("staging")
    for name, conj, mask in st.case.conjunctions:
        want_bits, wmask, count = row_filter_expected.expected([(st.trees[i], op, s) for i, op, s in conj])
        assert np.array_equal(wmask, mask)
        preds = [(st.nodes[i], op, s) for i, op, s in conj]
        for flags, fname in ((0, "engine's choice"), (L.ROWF_FUSE_RANGES, "paired"), (L.ROWF_NO_FUSE_RANGES, "unpaired")):
            at = st.at(f"conjunction {name} {[(i, op, s) for i, op, s in conj]!r}, {fname}")
            res = V.row_filter(preds, ctx, flags=flags)
            assert res.values.cpu().numpy()[:nb].tobytes() == want_bits, "mask differs, " + at
            assert res.true_count == count, f"true count {res.true_count} != {count}, " + at
            info = res.info
            assert info["predicates"] == len(conj), (info, at)
            assert info["compare_passes"] == info["predicates"] - info["range_pairs"], (info, at)
            if flags == L.ROWF_NO_FUSE_RANGES:
                assert info["range_pairs"] == 0, (info, at)
    for name, mask, dirty in st.case.masks:
        k = int(mask.sum())
        pred = A.bool_array(mask)
        want = [filter_canon(t, pred) for t in st.trees]
        at = st.at(f"mask {name}, k={k}")
        info = run(ctx, st.trees, mask, 0, dirty, want=want, at=at, nodes=st.nodes)
        check_info(info, st.cols, n, k, at)
