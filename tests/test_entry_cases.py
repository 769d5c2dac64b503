"""CPU: the expectations of the per-encoding entry-point tests are sound before anything runs on
a GPU.  For every case of tests/entry_cases.py the bytes the oracle's vxo_* function wrote equal
an independent plain-numpy statement of the operation (decode(encode(x)) == x for the codecs,
values[codes] for take, np.repeat for run-end, np.packbits for the bool ones, np.full for fill),
and where a case expects an error the oracle, where it has the same check, reports one too."""
import numpy as np
import pytest

import entry_cases as EC
from vortex_amd._lib import GPU_SIGNATURES, STATUS


@pytest.mark.parametrize("entry", EC.ENTRY_POINTS)
def test_oracle_equals_the_plain_statement(entry):
    valid = rejected = 0
    for c in EC.cases(entry):
        if c.error is None:
            valid += 1
            assert c.oracle_rc == 0, c.name
            assert c.outs and set(c.plain) == set(c.outs), c.name
            for name, o in c.outs.items():
                assert o.want is not None and len(o.want) == o.nbytes == len(c.plain[name]), (c.name, name)
                assert o.want == c.plain[name], (c.name, name)
        else:
            rejected += 1
            assert c.error in STATUS.values() and c.error != "OK" and c.at in ("call", "sync"), c.name
            assert c.oracle_rc in (None, -1), c.name  # the oracle rejects what it can check
            if c.at == "sync":  # found by a kernel: the oracle must have the same finding
                assert c.oracle_rc == -1, c.name
    assert valid >= 1, "every entry point has a parity case"
    # (vxg_bytebool_to_bits rejects nothing but null pointers: tests/test_gpu_entry_points.py)
    assert rejected >= 1 or entry == "vxg_bytebool_to_bits"


def test_every_per_encoding_entry_point_has_cases():
    assert set(EC.ENTRY_POINTS) < set(GPU_SIGNATURES)
    assert len(EC.ENTRY_POINTS) == 17


def test_case_shapes_reach_the_kernel_paths():
    """The size sets the kernels' paths depend on (vector body / tail, block and span edges)."""
    assert EC.n_set(8) == [0, 1, 2, 3, 255, 256, 257, 1023, 1024, 1025, 4097]
    assert EC.n_set(1) == [0, 1, 15, 16, 17, 255, 256, 257, 1023, 1024, 1025, 4097]
    assert EC.n_set(16) == [0, 1, 2, 255, 256, 257, 1023, 1024, 1025, 4097]
    # both sides of the thread-per-run / span kernel choice (len <= 16 * n_runs) are taken
    by_name = {c.name: c for c in EC.cases("vxg_runend_decode")}
    assert "vw4-u32-mean16-o0-n10000" in by_name and "vw4-u32-mean17-o5-n2049" in by_name
    short, long_ = by_name["vw4-u32-mean1-o0-n10000"].args, by_name["vw4-u32-mean300-o0-n10000"].args
    assert short["len"] <= 16 * short["n_runs"] and long_["len"] > 16 * long_["n_runs"]
    for c in EC.cases("vxg_runend_decode"):
        if c.error and c.at == "sync":
            assert (c.args["len"] <= 16 * c.args["n_runs"]) == c.name.endswith("mean1"), c.name


def test_bits_at_layout():
    assert EC.bits_at(np.array([1], np.uint8), 0) == b"\x01\x00\x00\x00"
    assert EC.bits_at(np.array([1, 1], np.uint8), 31) == b"\x00\x00\x00\x80\x01\x00\x00\x00"
    assert EC.bits_at(np.ones(32, np.uint8), 32) == bytes(4) + b"\xff" * 4


def test_sliced_runs_are_what_slice_leaves():
    """runend/compute.rs:104-119: the ends are not rebased, the first kept run holds row `offset`,
    the last one reaches offset + len."""
    r = np.random.default_rng(0)
    for mean, offset, n in ((1, 0, 1), (16, 5, 2049), (300, 5, 10_000), (17, 0, 2047)):
        ends = EC.sliced_runs(r, mean, offset, n)
        assert (np.diff(ends.astype(np.int64)) > 0).all() and ends[0] > offset and ends[-1] >= offset + n
        if ends.size > 1:
            assert ends[-2] <= offset + n  # only the last run may be cut (or be the lookup's extra run)
        assert EC.run_lengths(ends, offset, n).sum() == n
