"""CPU: the expected-value helper of the compare tests reproduces the reference's own literals
(tests/golden/compare_kat.json: encodings/alp/src/alp/compute.rs:159-201 and
vortex-array/src/array/primitive/compute/compare.rs:136-187), and the ctypes mirror of the new
entry point matches the header."""
import ctypes as C
import json
import subprocess
from pathlib import Path

import numpy as np
import pytest

import vortex_amd._lib as L
import vortex_amd.arrays as A
import vortex_amd.encode as E
from compare_expected import bitmap, compare_values, expected

ROOT = Path(__file__).resolve().parent.parent
KAT = json.loads((ROOT / "tests" / "golden" / "compare_kat.json").read_text())["cases"]


def _column(case):
    dt = A.NP_OF_PTYPE[case["ptype"]]
    raw = case["values"] * case["repeat"]
    valid = np.array([v is not None for v in raw])
    vals = np.array([0 if v is None else v for v in raw], dtype=dt)
    return vals, (None if valid.all() else valid)


def _rhs(case):
    r = case["rhs"]
    if isinstance(r, list):  # an array right-hand side: its nulls make the row null as well
        return np.array([0 if v is None else v for v in r]), np.array([v is not None for v in r])
    return r, None


@pytest.mark.parametrize("case", KAT, ids=[c["name"] for c in KAT])
def test_reference_literals(case):
    vals, valid = _column(case)
    if case["encoding"] == "alp":
        tree = E.encode_alp(vals)
    else:
        tree = A.primitive(vals, validity=valid)
    rhs, rhs_valid = _rhs(case)
    _, _, mask = expected(tree, case["op"], rhs)
    if rhs_valid is not None:
        mask = mask & rhs_valid
    want = case["true_rows"]
    rows = list(range(len(vals))) if want == "all" else ([] if want == "none" else want)
    assert np.flatnonzero(mask).tolist() == rows


def test_alp_literals_are_the_reference_encodings():
    """alp/compute.rs:159-166 and :188-192: 1025 x 1.234f32 encodes to 1234s without patches, the
    five-element array has patches -- so the GPU tests that reuse them exercise what the
    reference's tests exercise."""
    from oracle_tree import canon
    a = E.encode_alp(np.full(1025, 1.234, dtype=np.float32))
    assert not a.meta["has_patches"]
    assert (canon(a.children[0])[0] == 1234).all()
    b = E.encode_alp(np.array([1.234, 1.5, 19.0, np.e, 1_000_000.9], dtype=np.float32))
    assert b.meta["has_patches"]


def test_ieee_and_signedness():
    f = np.array([np.nan, -0.0, 0.0, np.inf, -np.inf, 1.5], dtype=np.float32)
    assert compare_values(f, None, "==", 0.0).tolist() == [False, True, True, False, False, False]
    assert compare_values(f, None, "!=", np.nan).all()
    for op in ("<", "<=", ">", ">=", "=="):
        assert not compare_values(f, None, op, np.nan).any()
    i = np.array([-1, 0, 1], dtype=np.int8)
    assert compare_values(i, None, "<", 0).tolist() == [True, False, False]
    assert compare_values(i.view(np.uint8), None, "<", 1).tolist() == [False, True, False]
    assert compare_values(i, np.array([False, True, True]), "<=", 0).tolist() == [False, True, False]


def test_bitmap_layout():
    assert bitmap([]) == b""
    assert bitmap([True]) == b"\x01" + bytes(7)
    assert bitmap([False] * 64 + [True]) == bytes(8) + b"\x01" + bytes(7)
    assert len(bitmap(np.ones(1025, bool))) == 17 * 8


def test_compare_info_layout_and_ops(tmp_path):
    """VxgCompareInfo and CMP_OP mirror the header (sizes, offsets, enum values)."""
    fields = [f for f, _ in L.VxgCompareInfo._fields_]
    ops = {"==": "EQ", "!=": "NOT_EQ", ">": "GT", ">=": "GTE", "<": "LT", "<=": "LTE"}
    src = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{ROOT}/include/vortex_gpu.h"', "int main(){",
           'printf("size %zu\\n", sizeof(vxg_compare_info));', 'printf("flag %d\\n", VXG_CMP_NULL_AS_FALSE);']
    src += [f'printf("{f} %zu\\n", offsetof(vxg_compare_info, {f}));' for f in fields]
    src += [f'printf("{name} %d\\n", VXG_CMP_{name});' for name in ops.values()]
    src.append("return 0;}")
    (tmp_path / "ci.c").write_text("\n".join(src))
    subprocess.run(["gcc", str(tmp_path / "ci.c"), "-o", str(tmp_path / "ci")], check=True)
    got = dict(ln.split() for ln in subprocess.run([str(tmp_path / "ci")], capture_output=True, text=True,
                                                    check=True).stdout.splitlines())
    assert int(got["size"]) == C.sizeof(L.VxgCompareInfo)
    assert int(got["flag"]) == L.CMP_NULL_AS_FALSE
    for f in fields:
        assert int(got[f]) == getattr(L.VxgCompareInfo, f).offset
    for sym, name in ops.items():
        assert int(got[name]) == L.CMP_OP[sym]
