"""GPU: every seeded tree of tests/tree_cases.py through every route of the engine, bit for bit.

One tree per seed goes through the direct canonicalize, a plan of its own (launched twice), a plan
over the trees of eight consecutive seeds (both plan-batch settings, both VXG_PLAN_FUSE settings),
take (empty / one / at most 16 / more than a quarter of the rows, with and without
force_canonical), filter (Bool, RunEndBool and constant predicates at five densities), compare (six
operators, scalars from the data and outside it, null_as_false both ways) and the row filter (a
two-sided range, paired and unpaired, then fed to filter).  Every route carries its own CPU
expectation (oracle_tree.canon / filter_canon, take_expected, compare_expected,
compare_bytes_expected, row_filter_expected); equality is exact, values as bytes, validity as
masks, strings as views and heap byte for byte.  Every assertion names the seed and the tree.
"""
import functools

import numpy as np
import pytest

import compare_bytes_expected
import compare_expected
import row_filter_expected
import tree_cases as TC
import vortex_amd as V
import vortex_amd._lib as L
import vortex_amd.arrays as A
from oracle_tree import canon, filter_canon
from plan_env import env_set, plan_mode
from rows_check import check_rows, full
from take_expected import take_canon

pytestmark = pytest.mark.gpu

OPS = list(compare_expected.OPS)
GROUPS = [TC.SEEDS[i: i + 8] for i in range(0, len(TC.SEEDS), 8)]
VALUE_SEEDS = [s for s in TC.SEEDS if TC.build(s).kind != "bool"]  # compare and row filter take no Bool column


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
    """A seed's case, its tree in device memory and the oracle's canonical of it (computed once)."""

    def __init__(self, seed):
        self.case = TC.build(seed)
        self.tree = self.case.tree
        self.dev = self.tree.to(_dev())
        self.want, self.valid = canon(self.tree)
        self.rows = None
        if self.case.kind == "str":
            self.rows = compare_bytes_expected.rows_of(self.tree)

    def at(self, route):
        return f"seed {self.case.seed} [{route}]: {self.case.describe}"


@functools.lru_cache(maxsize=None)
def staged(seed) -> Staged:
    return Staged(seed)


# ---------------------------------------------------------------------------- canonicalize
def picked(selection, name) -> bool:
    """`name` is among the inputs a route was asked to run (None: every input of the case)."""
    return selection is None or name in selection


# The routes as callables of (ctx, st): the tests below run them on the default stream with every
# input of the case; tests/test_gpu_streams.py runs them on a caller's stream with a selection.
def direct_and_plan(ctx, st):
    kind = st.case.kind
    direct = A.canonicalize(st.dev, ctx)
    check_rows(kind, direct, st.want, st.valid, st.at("direct"))
    plan = A.Plan([st.dev], ctx)
    try:
        for launch in (1, 2):  # the first launch, then a replay
            res = plan.launch(sync=True)[0]
            check_rows(kind, res, st.want, st.valid, st.at(f"plan launch {launch}"))
    finally:
        plan.close()
    check_rows(kind, direct, st.want, st.valid, st.at("direct, after the plan"))


@pytest.mark.parametrize("seed", TC.SEEDS)
def test_direct_and_plan(ctx, seed):
    direct_and_plan(ctx, staged(seed))


def plan_over_eight_trees(ctx, group, batch, fuse):
    sts = [staged(s) for s in GROUPS[group]]
    direct = [A.canonicalize(st.dev, ctx) for st in sts]
    with env_set(VXG_PLAN_FUSE=fuse), plan_mode(batch):
        plan = A.Plan([st.dev for st in sts], ctx)
    try:
        for launch in (1, 2):
            res = plan.launch(sync=True)
            for st, r in zip(sts, res):
                check_rows(st.case.kind, r, st.want, st.valid,
                           st.at(f"plan of seeds {GROUPS[group]} batch={batch} fuse={fuse} launch {launch}"))
    finally:
        plan.close()
    for st, d in zip(sts, direct):
        check_rows(st.case.kind, d, st.want, st.valid, st.at(f"direct, after the plan of seeds {GROUPS[group]}"))


@pytest.mark.parametrize("fuse", ["1", "0"])
@pytest.mark.parametrize("batch", ["1", "0"])
@pytest.mark.parametrize("group", range(len(GROUPS)))
def test_plan_over_eight_trees(ctx, group, batch, fuse):
    """One plan over eight trees: every output checked on two launches, and the direct outputs taken
    before it checked again afterwards (a plan that writes outside its own outputs is seen)."""
    plan_over_eight_trees(ctx, group, batch, fuse)


# ---------------------------------------------------------------------------- take
def take(ctx, st, sets=None):
    """`sets`: names of the take sets to run."""
    for name, idx in st.case.take_sets:
        if not picked(sets, name):
            continue
        want, wvalid = take_canon(st.tree, idx, canonical=(st.want, st.valid) if st.case.kind == "str" else None)
        for force in (False, True):
            res = A.take(st.dev, idx, ctx, force_canonical=force)
            check_rows(st.case.kind, res, want, wvalid,
                       st.at(f"take {name}: {idx.size} x {idx.dtype} force_canonical={force}"))


@pytest.mark.parametrize("seed", TC.SEEDS)
def test_take(ctx, seed):
    take(ctx, staged(seed))


# ---------------------------------------------------------------------------- filter
def filter_rows(ctx, st, predicates=None):
    """`predicates`: names of the predicates to run."""
    for name, pred in st.case.predicates:
        if not picked(predicates, name):
            continue
        want, wvalid = filter_canon(st.tree, pred)
        res = A.filter(st.dev, pred.to(_dev()), ctx)
        check_rows(st.case.kind, res, want, wvalid, st.at(f"filter {name}"))


@pytest.mark.parametrize("seed", TC.SEEDS)
def test_filter(ctx, seed):
    filter_rows(ctx, staged(seed))


# ---------------------------------------------------------------------------- compare
def compare_want(st, op, scalar):
    """-> (values bitmap, validity bitmap | None, row mask) of compare(tree, op, scalar)."""
    if st.case.kind == "str":
        return compare_bytes_expected.expected(st.tree, op, scalar, rows=st.rows)
    m = compare_expected.compare_values(np.asarray(st.want), st.valid, op, scalar)
    return compare_expected.bitmap(m), (None if st.valid is None else compare_expected.bitmap(st.valid)), m


def compare(ctx, st, scalars=None, ops=None):
    """`scalars`: positions in the case's list of scalars to run; `ops`: the operators."""
    n = st.tree.len
    nb = ((n + 63) // 64) * 8
    for i, scalar in enumerate(st.case.scalars):
        if not picked(scalars, i):
            continue
        for op in OPS:
            if not picked(ops, op):
                continue
            want, want_valid, _ = compare_want(st, op, scalar)
            for null_as_false in (False, True):
                at = st.at(f"compare {op} {scalar!r} null_as_false={null_as_false}")
                res = A.compare(st.dev, op, scalar, ctx, null_as_false=null_as_false)
                assert res.kind == "bool" and res.len == n, at
                assert res.values.cpu().numpy()[:nb].tobytes() == want, "values differ, " + at
                if null_as_false or res.validity is None:
                    assert res.validity is None and (null_as_false or full(st.valid, n).all()), "validity differs, " + at
                else:
                    assert res.validity.cpu().numpy()[:nb].tobytes() == compare_expected.bitmap(full(st.valid, n)), \
                        "validity differs, " + at


@pytest.mark.parametrize("seed", VALUE_SEEDS)
def test_compare(ctx, seed):
    compare(ctx, staged(seed))


# ---------------------------------------------------------------------------- row filter
def row_filter(ctx, st):
    lo_op, lo, hi_op, hi = st.case.range
    want, mask, count = row_filter_expected.expected([(st.tree, lo_op, lo), (st.tree, hi_op, hi)])
    nb = ((st.tree.len + 63) // 64) * 8
    kept, kvalid = filter_canon(st.tree, A.bool_array(mask))
    for flags, name in ((L.ROWF_FUSE_RANGES, "paired"), (L.ROWF_NO_FUSE_RANGES, "unpaired")):
        at = st.at(f"row filter {lo_op} {lo!r} and {hi_op} {hi!r}, {name}")
        res = A.row_filter([(st.dev, lo_op, lo), (st.dev, hi_op, hi)], ctx, flags=flags)
        assert res.values.cpu().numpy()[:nb].tobytes() == want, "mask differs, " + at
        assert res.true_count == count, f"true count {res.true_count} != {count}, " + at
        got = A.filter(st.dev, A.predicate_from(res), ctx)
        check_rows(st.case.kind, got, kept, kvalid, at + ", then filter")


@pytest.mark.parametrize("seed", VALUE_SEEDS)
def test_row_filter(ctx, seed):
    row_filter(ctx, staged(seed))
