"""GPU: every route of the engine on a caller's NON-BLOCKING stream, bit for bit.

Every other GPU test runs on the legacy default stream, where the runtime serialises whatever the
engine issues.  A scan owns its streams, and a stream created with hipStreamNonBlocking does not
synchronise with the default stream: an internal launch, memset, copy or readback on the wrong
stream, a host table reused before its asynchronous upload was consumed, or a readback that waits on
the wrong stream are all invisible there.  Here every test makes tests/side_stream.py's side stream
current, and every engine call that takes a stream is issued as hold -> call -> held
(side_stream.HeldContext): a device-side delay is enqueued first, and for every asynchronous call
`held` must be true when the call returns on the host -- the whole call was enqueued behind its own
producers, so anything it issued on another stream ran too early and the bytes differ.  A
synchronous call waits the delay out; only its result is checked.  TABLE states which is which.

The routes, inputs and expectations are those of tests/test_gpu_trees.py, tests/test_gpu_batches.py,
tests/test_gpu_entry_points.py, tests/test_gpu_encode.py and tests/test_gpu_file_trees.py -- imported,
not copied -- with the same exactness: bytes, validity masks, views and heap.  Inputs are uploaded
and complete before a route starts; the file route alone has the upload itself behind the delay
(pinned file bytes, a non-blocking copy), which is what holds vxg_canonical_layout's promise that a
layout query sees every upload already enqueued.  The last test runs two side streams over one
context, alternately, both held.
"""
import contextlib
import ctypes as C

import numpy as np
import pytest

import batch_cases as BC
import entry_cases as EC
import file_cases as FC
import side_stream as SS
import test_gpu_batches as TB
import test_gpu_encode as TE
import test_gpu_entry_points as TP
import test_gpu_trees as TT
import tree_cases as TC
import vortex_amd as V
import vortex_amd._lib as L
import vortex_amd.arrays as A
import vortex_amd.encode as E
import vortex_amd.gpu_encode as G
from oracle_tree import canon, filter_canon
from rows_check import check_rows
from take_expected import take_canon
from vortex_amd.file import DeviceColumns, VortexFile, scan

pytestmark = pytest.mark.gpu

TAKE_SETS = ("few", "many")
PREDICATES = ("bool-50%", "runend-50%", "constant-true")
# compare is thinned for time (the file must not cost much more than tests/test_gpu_trees.py): equality,
# one strict and one non-strict ordering, one in each direction, instead of all six operators
COMPARE_OPS = ("==", "<", ">=")
EIGHT_TREE_MODES = [("1", "1"), ("0", "0")]  # (VXG_PLAN_BATCH, VXG_PLAN_FUSE)
BATCH_IDS = [BC.seed_id(s) for s in BC.BATCH_SEEDS]
PAIRS = [(TC.SEEDS[i], TC.SEEDS[i + 1]) for i in range(0, len(TC.SEEDS) - 1, 2)]
STALE = 0xFF  # what a column's device region holds before the held upload (see test_file_route)


def compare_scalars(case) -> tuple:
    """Positions in case.scalars: the scalar taken from the data and the one outside it (the last of
    a list too short to have one)."""
    return (0, min(3, len(case.scalars) - 1))


# ---------------------------------------------------------------------------- which calls are asynchronous
ASYNC, SYNC = True, False


def row(prim, boolean, string):
    return {"prim": prim, "bool": boolean, "str": string}


def every(kind_is_async):
    return row(kind_is_async, kind_is_async, kind_is_async)


# entry point -> kind of the array(s) -> the call returns once enqueued (ASYNC: `held` is asserted on
# every call) or waits on its stream somewhere (SYNC: only the result is checked).  Each SYNC names
# the wait that makes it so; each ASYNC the code that was read to find none.
TABLE = {
    # direct canonicalize into caller-allocated outputs
    "vxg_canonicalize": every(ASYNC),       # planner_decode.hip:771-795 launches only; strings: planner_strings.hip:315-325 skips the layout readback
    "vxg_plan_launch": every(ASYNC),        # plan.hip:473-489: hipLaunchKernel / hipGraphLaunch only
    "vxg_take_array_ex": row(ASYNC, ASYNC,  # planner_take.hip:108-139: launches only
                             SYNC),         # planner_take.hip:256, 305 (heap size: planner_strings.hip:448)
    "vxg_filter_array": every(SYNC),        # planner_filter.hip:35 (count: planner_strings.hip:448), :38; capi.hip:676
    "vxg_compare_scalar": every(ASYNC),     # planner_compare.hip:117-198: launches only (vortex_gpu.h "Asynchronous on `stream`")
    "vxg_compare_bytes": every(SYNC),       # planner_compare.hip:312 (VarBinView buffer table), :506 (scalar over 64 bytes), planner_strings.hip:91 (canonicalized FSST)
    "vxg_row_filter": row(ASYNC, ASYNC,     # planner_compare.hip:204-289: compare_impl passes + launch_and_count
                          SYNC),            # its string conjuncts go through compare_bytes (planner_compare.hip:260)
    "vxg_filter_batch": every(SYNC),        # planner_filter.hip:185 (count), :106 (a string column's heap size)
    # the per-encoding kernels (capi.hip:280-457, 718-776): argument checks and one launch each
    **{name: every(ASYNC) for name in TP.CALL},
    # the encoders
    "vxg_bitpack": every(ASYNC),            # capi.hip:584-613: fl_pack_* launch only
    "vxg_for_bitpack": every(ASYNC),        # capi.hip:615-619: the same launch
    "vxg_for_encode": every(ASYNC),         # capi.hip:621-629: launch_for_encode only
    "vxg_compute_int_stats": every(SYNC),   # encode_gpu.hip:407 (vortex_gpu.h "Synchronous")
    "vxg_gather_patches": every(SYNC),      # encode_gpu.hip:378
    "vxg_alp_encode": every(SYNC),          # encode_gpu.hip:482, 503
    "vxg_fsst_compress": every(SYNC),       # fsst_encode.hip:340, 356
}


# ---------------------------------------------------------------------------- fixtures
@pytest.fixture(autouse=True)
def stop_after_a_gpu_fault(ctx):
    """A route that faults the device ends the session: nothing more is started on a faulted GPU."""
    yield
    try:
        ctx.sync()
    except V.VortexGpuError as e:
        if e.kind == "HipError":
            pytest.exit(f"the GPU reported {e}: not starting further GPU tests", returncode=3)


@pytest.fixture(scope="module")
def delay():
    """side_stream.DELAY_MS as torch.cuda._sleep cycles on this device, calibrated once."""
    return SS.calibrate(SS.side_stream(0), SS.DELAY_MS)


@pytest.fixture
def held(ctx, delay):
    return SS.HeldContext(ctx, delay, TABLE)


@contextlib.contextmanager
def on_side(ctx, i: int = 0):
    """Side stream `i` current; what was uploaded before is complete, and the stream is drained on the
    way out (also after a failed assertion: the next test starts on an idle device)."""
    import torch
    ctx.sync()
    torch.cuda.synchronize()
    s = SS.side_stream(i)
    try:
        with torch.cuda.stream(s):
            yield s
    finally:
        s.synchronize()


def warm_then_held(route, ctx, held, *args, **kwargs):
    """The route once as it is on the side stream, then again with every call held.  A first use loads
    code objects and grows the stream's memory pools: host time of the process, not of the call, and
    nothing a delay should be sized for."""
    route(ctx, *args, **kwargs)
    route(held, *args, **kwargs)


# ---------------------------------------------------------------------------- trees
@pytest.mark.parametrize("seed", TC.SEEDS)
def test_direct_and_plan(ctx, held, seed):
    st = TT.staged(seed)
    with on_side(ctx):
        warm_then_held(TT.direct_and_plan, ctx, held, st)
        assert held.check(st.case.kind, st.at("side stream"), expect=("vxg_canonicalize", "vxg_plan_launch")) == 3


@pytest.mark.parametrize("batch,fuse", EIGHT_TREE_MODES)
@pytest.mark.parametrize("group", range(len(TT.GROUPS)))
def test_plan_over_eight_trees(ctx, held, group, batch, fuse):
    sts = [TT.staged(s) for s in TT.GROUPS[group]]
    with on_side(ctx):
        warm_then_held(TT.plan_over_eight_trees, ctx, held, group, batch, fuse)
        at = f"side stream, plan of seeds {TT.GROUPS[group]} batch={batch} fuse={fuse}"
        assert held.check("prim", at, expect=("vxg_canonicalize", "vxg_plan_launch")) == len(sts) + 2


@pytest.mark.parametrize("seed", TC.SEEDS)
def test_take(ctx, held, seed):
    st = TT.staged(seed)
    sets = [name for name, _ in st.case.take_sets if name in TAKE_SETS]
    with on_side(ctx):
        warm_then_held(TT.take, ctx, held, st, sets=TAKE_SETS)
        assert held.check(st.case.kind, st.at("side stream"), expect=("vxg_take_array_ex",) if sets else ()) == 2 * len(sets)


@pytest.mark.parametrize("seed", TC.SEEDS)
def test_filter(ctx, held, seed):
    st = TT.staged(seed)
    preds = [name for name, _ in st.case.predicates if name in PREDICATES]
    with on_side(ctx):
        warm_then_held(TT.filter_rows, ctx, held, st, predicates=PREDICATES)
        assert held.check(st.case.kind, st.at("side stream"), expect=("vxg_filter_array",)) == len(preds)


@pytest.mark.parametrize("seed", TT.VALUE_SEEDS)
def test_compare(ctx, held, seed):
    st = TT.staged(seed)
    picked = set(compare_scalars(st.case))
    entry = "vxg_compare_bytes" if st.case.kind == "str" else "vxg_compare_scalar"
    with on_side(ctx):
        warm_then_held(TT.compare, ctx, held, st, scalars=picked, ops=COMPARE_OPS)
        assert held.check(st.case.kind, st.at("side stream"), expect=(entry,)) == len(picked) * len(COMPARE_OPS) * 2


@pytest.mark.parametrize("seed", TT.VALUE_SEEDS)
def test_row_filter(ctx, held, seed):
    st = TT.staged(seed)
    with on_side(ctx):
        warm_then_held(TT.row_filter, ctx, held, st)
        assert held.check(st.case.kind, st.at("side stream"), expect=("vxg_row_filter", "vxg_filter_array")) == 4


# ---------------------------------------------------------------------------- batches
def batch_kind(st, conj=None) -> str:
    """The TABLE kind of a call over a batch's columns (`conj`: over a conjunction's columns only)."""
    cols = st.cols if conj is None else [st.cols[i] for i, _, _ in conj]
    return "str" if any(c.kind == "str" for c in cols) else "prim"


@pytest.mark.parametrize("seed", BC.BATCH_SEEDS, ids=BATCH_IDS)
def test_filter_batch(ctx, held, seed):
    st = TB.staged(seed)
    conj = [name for name, _, _ in st.case.masks if name.startswith("conjunction-")][:1]
    with on_side(ctx):
        warm_then_held(TB.filter_batch, ctx, held, st, masks=["50%"] + conj)
        held.check(batch_kind(st), st.at("side stream"), expect=("vxg_filter_batch",))


@pytest.mark.parametrize("seed", BC.BATCH_SEEDS, ids=BATCH_IDS)
def test_row_filter_then_filter_batch(ctx, held, seed):
    st = TB.staged(seed)
    first = st.case.conjunctions[:1]
    with on_side(ctx):
        warm_then_held(TB.row_filter_then_filter_batch, ctx, held, st, conjunctions=[name for name, _, _ in first])
        for _, conj, _ in first:
            held.check(batch_kind(st, conj), st.at("side stream"), expect=("vxg_row_filter", "vxg_filter_batch"))


# ---------------------------------------------------------------------------- per-encoding entry points
@pytest.mark.parametrize("entry", EC.ENTRY_POINTS)
def test_entry_points(ctx, held, entry):
    """tests/test_gpu_entry_points.py's valid cases with the side stream's pointer: the same guard bytes,
    the same byte-for-byte comparison."""
    cases = [c for c in EC.cases(entry) if c.error is None]
    assert cases
    with on_side(ctx):
        TP.run_all(cases, ctx.lib, ctx)  # (as warm_then_held: the first use of the kernels)
        TP.run_all(cases, held.lib, held)
        calls = held.check("prim", entry, expect=(entry,))
    assert calls == len(cases)


# ---------------------------------------------------------------------------- encoders
@pytest.mark.parametrize("n", [1, 1025, 5000])
def test_encoders(ctx, held, n):
    """The encoders are synchronous: their stream-ordered scratch (hipMallocAsync / hipFreeAsync on the
    caller's stream) and their readbacks are what runs here, against the host encoders."""
    rng = np.random.default_rng(7000 + n)
    with on_side(ctx):
        for T, W in ((8, 3), (16, 11), (32, 7), (64, 33)):
            v = (rng.integers(0, 2**63, n, dtype=np.uint64) & np.uint64((1 << W) - 1)).astype(TE.UT[T])
            G.bitpack(ctx, TE.dev(v), f"u{T}", W)  # (as warm_then_held, here and below)
            g = G.bitpack(held, TE.dev(v), f"u{T}", W)
            assert TE.host_bytes(g) == E.bitpack_buffer(v, W).tobytes(), (T, W, n)
        held.check("prim", f"bitpack n={n}", expect=("vxg_bitpack",))
        for dt in (np.int32, np.uint16, np.int64):
            for v in TE._for_cases(rng, dt, n):
                for allow in (True, False):
                    h = E.encode_for_bitpacked(v, allow_patches=allow)
                    for c in (ctx, held):
                        g = G.encode_for_bitpacked(c, TE.dev(v), A.PTYPE_OF_NP[np.dtype(dt)], allow_patches=allow)
                        TE.assert_same_tree(g, h)
                        if g.encoding != A.ENC["CONSTANT"]:
                            TE.roundtrip(g, c, v)
        held.check("prim", f"encode_for_bitpacked n={n}", expect=("vxg_compute_int_stats",))
        prices = np.round(rng.uniform(1, 100000, n) * 100) / 100
        if n > 10:
            prices[rng.choice(n, n // 1000 + 1, replace=False)] = rng.standard_normal(n // 1000 + 1) * 1e9
        singles = (np.round(rng.uniform(-500, 500, n) * 10) / 10).astype(np.float32)
        for c in (ctx, held):
            TE.assert_alp_same(c, prices, "f64")
            TE.assert_alp_same(c, singles, "f32")
        held.check("prim", f"encode_alp n={n}", expect=("vxg_alp_encode",))


def test_fsst_reference_sentences(ctx, held):
    with on_side(ctx):
        for op in ("i32", "i64"):
            warm_then_held(TE._fsst_gpu_vs_host, ctx, held, TE.FSST_SENTENCES, op)
        held.check("str", "fsst sentences", expect=("vxg_fsst_compress", "vxg_canonicalize"))


# ---------------------------------------------------------------------------- the file route
def pinned(data):
    """A file's bytes in page-locked host memory (what a scan reads into)."""
    import torch
    t = torch.from_numpy(np.frombuffer(bytes(data), np.uint8).copy())
    return t.pin_memory()


def direct(hctx, node):
    """vxg_canonical_layout + vxg_canonicalize of a reader's node (what file.scan does per column)."""
    keep: list = []
    o, res = A.alloc_canonical(hctx, node, keep)
    L.check(hctx.lib.vxg_canonicalize(hctx.handle, C.byref(node), C.byref(o), hctx.stream_ptr()))
    if res.validity is not None and not o.validity:
        res.validity = None
    res._keep = keep
    hctx.sync()
    return res


@pytest.mark.parametrize("seed", FC.TREE_SEEDS)
def test_file_route(ctx, held, delay, seed):
    """The only route with the upload itself behind the delay.

    First as a scan issues it: hold, DeviceColumns, scan.  (DeviceColumns uploads its chunk offsets
    with a blocking copy, which waits that delay out, so this part orders less than it looks.)  Then
    with nothing in between: the column's device region is overwritten with STALE bytes and the stream
    drained; then hold, DeviceColumns.refresh() -- non-blocking copies from pinned memory, asserted
    `held` -- and the layout query, the direct canonicalize and a plan over the reader's nodes
    (launch, refresh, launch).  vxg_canonical_layout takes no stream: what it reads on the device
    (the FSST lengths) must be the file's bytes, not the stale ones.  STALE is 0xFF: lengths read
    from it are larger than the file's, so a layout that read them would ask for too large a heap
    (caught by the heap comparison), never for one the decode overruns."""
    tf = FC.tree_file(seed)
    case = tf.case
    tree = FC.range_tree(tf, 0, len(tf.chunks))
    want, valid = canon(tree)
    at = f"seed {case.seed} [file, side stream]: {case.describe}"
    file = VortexFile(pinned(tf.data))
    with on_side(ctx) as s:
        check_rows(case.kind, scan(file, ctx)[0], want, valid, at + ", scan, not held")  # (as warm_then_held)
        warm = DeviceColumns(file, ctx)
        plan = A.Plan(warm.nodes, ctx)
        try:
            check_rows(case.kind, plan.launch(sync=True)[0], want, valid, at + ", plan, not held")
        finally:
            plan.close()

        SS.hold(s, delay)
        dc = DeviceColumns(file, held)
        res = scan(file, held)[0]
        check_rows(case.kind, res, want, valid, at + ", scan")
        held.check(case.kind, at + ", scan", expect=("vxg_canonicalize",))

        for region in dc.regions:
            region.fill_(STALE)
        s.synchronize()
        ev = SS.hold(s, delay)
        dc.refresh()
        assert SS.held(ev), f"the upload was not enqueued behind the delay of {delay.ms:.3f} ms, {at}"
        check_rows(case.kind, direct(held, dc.nodes[0]), want, valid, at + ", direct after a held upload")
        held.check(case.kind, at + ", direct", expect=("vxg_canonicalize",))

        for region in dc.regions:
            region.fill_(STALE)
        s.synchronize()
        ev = SS.hold(s, delay)
        dc.refresh()
        assert SS.held(ev), f"the upload was not enqueued behind the delay of {delay.ms:.3f} ms, {at}"
        plan = A.Plan(dc.nodes, held)
        try:
            for launch in (1, 2):
                out = plan.launch(sync=False)[0]
                dc.refresh()
                held.sync()
                check_rows(case.kind, out, want, valid, at + f", plan launch {launch}")
        finally:
            plan.close()
        assert held.check(case.kind, at + ", plan", expect=("vxg_plan_launch",)) == 2
    file.close()


# ---------------------------------------------------------------------------- two streams, one context
@pytest.mark.parametrize("pair", PAIRS, ids=[f"{a}-{b}" for a, b in PAIRS])
def test_two_streams_one_context(ctx, delay, pair):
    """Two side streams, both held, the trees of two consecutive seeds: direct canonicalize, take `many`
    and filter `bool-50%` enqueued alternately from one host thread, then both released and both
    checked exactly.  This is where stream-ordered temporaries of one stream are handed out again
    while the other stream's work is pending.  Indices and predicates are uploaded before the holds.
    The asynchronous calls (TABLE) come first, so that they are enqueued while both streams are blocked.
    That is not asserted here: on an MI355X, in 18 of the 36 pairs a call that takes stream-ordered
    temporaries returned only after the OTHER stream's delay had run out -- hipMallocAsync does not hand
    out blocks whose hipFreeAsync is still pending on another stream, and apparently waits for them on
    the host.  The results are exact either way; the single-stream tests above hold every such call."""
    import torch
    dev = torch.device("cuda", 0)
    sts = [TT.staged(s) for s in pair]
    streams = [SS.side_stream(0), SS.side_stream(1)]
    many = [next((idx for name, idx in st.case.take_sets if name == "many"), None) for st in sts]
    many_dev = [None if idx is None else torch.from_numpy(np.ascontiguousarray(idx)).to(dev) for idx in many]
    half = [next(p for name, p in st.case.predicates if name == "bool-50%") for st in sts]
    half_dev = [p.to(dev) for p in half]
    ctx.sync()
    torch.cuda.synchronize()
    got = [{}, {}]

    def on(i, fn):
        with torch.cuda.stream(streams[i]):
            return fn()

    for i in (0, 1):  # (as warm_then_held; the outputs go back to their stream's pool)
        on(i, lambda: A.canonicalize(sts[i].dev, ctx))
        if many[i] is not None:
            on(i, lambda: A.take(sts[i].dev, many_dev[i], ctx))
        on(i, lambda: A.filter(sts[i].dev, half_dev[i], ctx))
    # up to four asynchronous calls, with their output allocations, go behind one hold per stream
    wide = SS.Delay(4 * delay.cycles, 4 * delay.ms)
    for s in streams:
        SS.hold(s, wide)
    try:
        for i in (0, 1):
            got[i]["direct"] = on(i, lambda: A.canonicalize(sts[i].dev, ctx, sync=False))
        for i in (0, 1):
            if many[i] is not None and sts[i].case.kind != "str":
                got[i]["take"] = on(i, lambda: A.take(sts[i].dev, many_dev[i], ctx, sync=False))
        # the synchronous calls (TABLE) wait their own stream's delay out
        for i in (0, 1):
            if many[i] is not None and sts[i].case.kind == "str":
                got[i]["take"] = on(i, lambda: A.take(sts[i].dev, many_dev[i], ctx))
        for i in (0, 1):
            got[i]["filter"] = on(i, lambda: A.filter(sts[i].dev, half_dev[i], ctx))
    finally:
        for s in streams:
            s.synchronize()
    ctx.sync()
    for i, st in enumerate(sts):
        kind = st.case.kind
        at = st.at(f"stream {i} of two, beside seed {pair[1 - i]}")
        check_rows(kind, got[i]["direct"], st.want, st.valid, at + ", direct")
        if "take" in got[i]:
            w, wv = take_canon(st.tree, many[i], canonical=(st.want, st.valid) if kind == "str" else None)
            check_rows(kind, got[i]["take"], w, wv, at + ", take many")
        w, wv = filter_canon(st.tree, half[i])
        check_rows(kind, got[i]["filter"], w, wv, at + ", filter bool-50%")


