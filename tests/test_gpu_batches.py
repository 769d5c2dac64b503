"""GPU: every seeded batch of tests/batch_cases.py through vxg_row_filter and vxg_filter_batch, bit for bit.

A batch's columns go through vxg_filter_batch under every mask of the batch (filter_batch_run.run:
exactly-sized guarded outputs, byte equality with oracle_tree.filter_canon) and the call's info
counters are held to batch_cases.expected_route, so a column that silently takes another route
fails; every conjunction goes through vxg_row_filter under the three pairing flags and its result,
as it stands, into vxg_filter_batch over all columns of the batch; and the binding's outputs are
held to vxg_filter_array's, column by column.  tests/test_batch_cases.py holds the expectations
against the plain truth on the CPU.  Every input is a valid tree; every assertion names the batch.
"""
import functools

import numpy as np
import pytest

import batch_cases as BC
import row_filter_expected
import vortex_amd as V
import vortex_amd._lib as L
import vortex_amd.arrays as A
from filter_batch_run import mask_tensor, run
from oracle_tree import filter_canon
from test_gpu_trees import check_rows, picked
from vortex_amd._lib import ENC

pytestmark = pytest.mark.gpu

CANON = L.FILTB_CANONICALIZE
SEEDS = BC.BATCH_SEEDS
IDS = [BC.seed_id(s) for s in SEEDS]


def _dev():
    import torch
    return torch.device("cuda", 0)


@pytest.fixture(autouse=True)
def stop_after_a_gpu_fault(ctx):
    """A batch that faults the device ends the session: nothing more is started on a faulted GPU."""
    yield
    try:
        ctx.sync()
    except V.VortexGpuError as e:
        if e.kind == "HipError":
            pytest.exit(f"the GPU reported {e}: not starting further GPU tests", returncode=3)


def to_device(a: A.Array) -> A.Array:
    """Array.to, but a Primitive array that is a slice of a longer host buffer keeps its place in that
    buffer: the whole buffer goes up and the node points into it, off the buffer's first byte."""
    import torch

    def mv(b):
        arr = np.ascontiguousarray(b)
        base = arr.base
        if a.encoding == ENC["PRIMITIVE"] and isinstance(base, np.ndarray) and base.flags.c_contiguous and arr.nbytes:
            off = arr.__array_interface__["data"][0] - base.__array_interface__["data"][0]
            if 0 < off and off + arr.nbytes <= base.nbytes:
                whole = torch.from_numpy(base.reshape(-1).view(np.uint8).copy()).to(_dev())
                return whole[off: off + arr.nbytes]
        return b

    moved = A.Array(a.encoding, a.len, a.dtype, a.ptype, a.nullable, a.validity, dict(a.meta),
                    [mv(b) for b in a.buffers], [])
    moved = moved.to(_dev())  # (a device tensor stays where it lies)
    moved.children = [to_device(c) for c in a.children]
    return moved


class Staged:
    """A batch, its columns in device memory and the oracle's filtered columns per mask (computed once)."""

    def __init__(self, seed):
        self.case = BC.build(seed)
        self.cols = self.case.columns
        self.trees = [c.tree for c in self.cols]
        self.dev = [to_device(c.tree) if c.made_as.startswith("inplace") else c.tree.to(_dev()) for c in self.cols]
        self._want = {}
        for c, d in zip(self.cols, self.dev):
            if c.made_as == "inplace" and self.case.n:
                assert d.encoding == ENC["PRIMITIVE"] and d.buffers[0].storage_offset() > 0, self.at("staging")

    def want(self, name, mask):
        if name not in self._want:
            pred = A.bool_array(mask)
            self._want[name] = [filter_canon(t, pred) for t in self.trees]
        return self._want[name]

    def at(self, what):
        return f"[{what}] {self.case.describe}"


@functools.lru_cache(maxsize=4)
def staged(seed) -> Staged:
    return Staged(seed)


def check_info(info, cols, n, k, at, forced=False):
    """vxg_filter_batch_info against the routes batch_cases.expected_route predicts."""
    strings = sum(c.kind == "str" for c in cols)
    assert info["columns"] == len(cols) and info["mask_scans"] == (1 if n else 0), (info, at)
    if k == 0:  # nothing is launched after the count
        assert (info["fallback_arrays"], info["inplace_arrays"], info["packed_chunks"], info["packed_launches"],
                info["patch_launches"]) == (0, 0, 0, 0, 0), (info, at)
        assert info["syncs"] == (1 if n else 0), (info, at)
        return
    assert info["syncs"] == 1 + strings, (info, at)
    if forced:
        assert (info["packed_launches"], info["inplace_arrays"], info["patch_launches"], info["packed_chunks"]) == \
            (0, 0, 0, 0), (info, at)
        assert info["fallback_arrays"] == len(cols), (info, at)
        return
    by = {r: [c.route[1] for c in cols if c.route[0] == r] for r in ("packed", "inplace", "fallback")}
    assert info["fallback_arrays"] == len(by["fallback"]), (info, by, at)
    assert info["inplace_arrays"] == sum(by["inplace"]), (info, by, at)
    assert info["packed_chunks"] == sum(by["packed"]), (info, by, at)
    assert info["packed_launches"] >= len(by["packed"]), (info, by, at)


# The routes as callables of (ctx, st): the tests below run them on the default stream with every
# input of the batch; tests/test_gpu_streams.py runs them on a caller's stream with a selection.
def filter_batch(ctx, st, masks=None):
    """`masks`: names of the masks to run."""
    n = st.case.n
    conj_masks = [name for name, _, _ in st.case.masks if name.startswith("conjunction-")]
    for name, mask, dirty in st.case.masks:
        if not picked(masks, name):
            continue
        k = int(mask.sum())
        want = st.want(name, mask)
        at = st.at(f"mask {name}, k={k}")
        info = run(ctx, st.dev, mask, 0, dirty, want=want, at=at)
        check_info(info, st.cols, n, k, at)
        if name == "50%" or name == (conj_masks or [None])[0]:
            forced = run(ctx, st.dev, mask, CANON, dirty, want=want, at=at + " canonicalize")
            check_info(forced, st.cols, n, k, at + " canonicalize", forced=True)
        if name == "50%":
            # the columns in reverse order: no out depends on its neighbours
            info = run(ctx, st.dev[::-1], mask, 0, dirty, want=want[::-1], at=at + " reversed")
            check_info(info, st.cols[::-1], n, k, at + " reversed")
            # every out pointer NULL: the engine allocates (and vxg_free releases) what it hands back
            info = run(ctx, st.dev, mask, 0, dirty, want=want, allocate=True, at=at + " engine-allocated")
            check_info(info, st.cols, n, k, at + " engine-allocated")


@pytest.mark.parametrize("seed", SEEDS, ids=IDS)
def test_filter_batch(ctx, seed):
    filter_batch(ctx, staged(seed))


def row_filter_then_filter_batch(ctx, st, conjunctions=None):
    """`conjunctions`: names of the conjunctions to run."""
    n = st.case.n
    nb = ((n + 63) // 64) * 8
    for name, conj, mask in st.case.conjunctions:
        if not picked(conjunctions, name):
            continue
        want_bits, wmask, count = row_filter_expected.expected([(st.trees[i], op, s) for i, op, s in conj])
        assert np.array_equal(wmask, mask)
        kept = st.want("conjunction-" + name, mask)
        preds = [(st.dev[i], op, s) for i, op, s in conj]
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
                if len(conj) == 17 and n:
                    assert info["combine_launches"] == 2, (info, at)
            # the result as it stands is the batch's mask: every column, predicate columns included
            outs, k, binfo = V.filter_batch(st.dev, res, ctx)
            assert k == count, (k, count, at)
            check_info(binfo, st.cols, n, k, at + ", then filter_batch")
            for c, got, (wvals, wvalid) in zip(st.cols, outs, kept):
                check_rows(c.kind, got, wvals, wvalid, at + f", then filter_batch: {c.describe}")


@pytest.mark.parametrize("seed", SEEDS, ids=IDS)
def test_row_filter_then_filter_batch(ctx, seed):
    row_filter_then_filter_batch(ctx, staged(seed))


@pytest.mark.parametrize("seed", SEEDS, ids=IDS)
def test_filter_batch_matches_filter_array(ctx, seed):
    """The binding's out of every column equals A.filter(column, predicate), field by field."""
    import torch
    st = staged(seed)
    n = st.case.n
    name, mask, _ = next(m for m in st.case.masks if m[0] == "50%")
    outs, k, info = V.filter_batch(st.dev, mask_tensor(mask), ctx, length=n)
    assert k == int(mask.sum())
    check_info(info, st.cols, n, k, st.at("binding, mask 50%"))
    dpred = A.bool_array(mask).to(_dev())
    for c, t, got in zip(st.cols, st.dev, outs):
        at = st.at(f"binding against filter_array: {c.describe}")
        ref = A.filter(t, dpred, ctx)
        assert (got.kind, got.len, got.ptype) == (ref.kind, ref.len, ref.ptype), at
        for f in ("values", "views", "data", "validity"):
            a, b = getattr(got, f), getattr(ref, f)
            assert (a is None) == (b is None), (f, at)
            assert a is None or torch.equal(a, b), (f, at)
        assert got.data_buffers == ref.data_buffers, at
