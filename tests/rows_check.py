"""A Canonical of rows the engine returned against the oracle's (values, validity) -- plain module,
shared by the GPU tests (tests/test_gpu_trees.py, tests/test_gpu_batches.py, tests/test_gpu_file_trees.py)."""
import numpy as np


def full(mask, n):
    return np.ones(n, bool) if mask is None else np.asarray(mask, bool)


def check_rows(kind, res, want, wvalid, at):
    """A Canonical of rows (canonicalize, a plan, take, filter) against (values, validity) as
    oracle_tree.canon states them."""
    if kind == "prim":
        want = np.ascontiguousarray(want)
        got = res.numpy()
        assert res.len == want.size and got.dtype == want.dtype, "length or dtype differs, " + at
        assert got.tobytes() == want.tobytes(), "values differ, " + at
    elif kind == "bool":
        assert res.kind == "bool" and res.len == len(want), "length differs, " + at
        assert np.array_equal(res.numpy(), np.asarray(want, bool)), "bits differ, " + at
    else:
        wviews, wheap = want
        wheap = wheap if isinstance(wheap, list) else [wheap]
        assert res.len == wviews.shape[0], "length differs, " + at
        assert res.views.cpu().numpy().tobytes() == np.ascontiguousarray(wviews).tobytes(), "views differ, " + at
        gheap = res.buffers()
        if len(wheap) == 1 and wheap[0].size == 0:  # (an empty heap is no buffer or an empty one)
            assert sum(b.size for b in gheap) == 0, "heap differs, " + at
        else:
            assert [b.tobytes() for b in gheap] == [np.ascontiguousarray(b).tobytes() for b in wheap], \
                "heap differs, " + at
    gvalid = res.validity_mask()
    assert np.array_equal(full(gvalid, res.len), full(wvalid, res.len)), "validity differs, " + at
