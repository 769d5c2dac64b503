"""CPU: the expected-value helper of the string compare tests reproduces the reference's own
literals (tests/golden/compare_bytes_kat.json: varbin/compute/compare.rs basic_test,
varbinview/compute.rs basic_test, encodings/fsst/src/compute.rs test_compare_fsst), orders bytes
as arrow does, and the ctypes mirror of vxg_compare_bytes matches the header."""
import ctypes as C
import json
import subprocess
from pathlib import Path

import numpy as np
import pytest

import vortex_amd._lib as L
import vortex_amd.arrays as A
import vortex_amd.encode as E
from compare_bytes_expected import compare_rows, expected, rows_of
from compare_expected import bitmap

ROOT = Path(__file__).resolve().parent.parent
KAT = json.loads((ROOT / "tests" / "golden" / "compare_bytes_kat.json").read_text())["cases"]


def _tree(case):
    rows = [None if r is None else r.encode() for r in case["rows"]]
    if case["encoding"] == "varbinview":
        return E.encode_varbinview(rows)
    if case["encoding"] == "fsst":
        return E.encode_fsst(rows)
    heap, offs, valid = E.strings_to_heap(rows)
    return A.varbin(A.primitive(offs.astype(np.int32)), A.primitive(heap), validity=None if valid.all() else valid)


@pytest.mark.parametrize("case", KAT, ids=[c["source"] for c in KAT])
def test_reference_literals(case):
    tree = _tree(case)
    values, validity, mask = expected(tree, case["op"], case["scalar"])
    valid = np.array([r is not None for r in case["rows"]])
    want = np.array(case["buffer"])
    assert (mask[valid] == want[valid]).all()
    assert not mask[~valid].any()  # value bits of null rows are 0
    assert values == bitmap(want & valid)
    assert validity == (None if valid.all() else bitmap(valid))


def test_every_encoding_gives_the_same_rows():
    rows = [b"", b"a", b"ab", b"twelve bytes", b"thirteen byte", b"\xff\x00\x80", b"a" * 40]
    for tree in (E.encode_varbinview(rows), E.encode_fsst(rows), E.encode_dict_strings(rows),
                 A.chunked([E.encode_fsst(rows[:3]), E.encode_varbinview(rows[3:])])):
        assert rows_of(tree)[0] == rows


def test_unsigned_and_prefix_order():
    rows = [b"\xff", b"a", b"ab", b"abc", b"", b"b"]
    m = lambda op, s: compare_rows(rows, None, op, s).tolist()  # noqa: E731
    assert m(">", b"a") == [True, False, True, True, False, True]        # 0xFF is above every ASCII byte
    assert m("<", b"abc") == [False, True, True, False, True, False]     # a proper prefix is smaller
    assert m("<", b"a") == [False, False, False, False, True, False]     # b"" is below everything non-empty
    assert m(">=", b"") == [True] * 6
    assert m("==", "ab") == [False, False, True, False, False, False]    # a str scalar is its UTF-8 bytes
    assert m("<=", "é") == [False, True, True, True, True, True]    # 0xC3 0xA9: above ASCII, below 0xFF


def test_nulls_are_false_and_keep_validity():
    tree = E.encode_dict_strings_nullable([b"x", None, b"y", b"x"])
    values, validity, mask = expected(tree, "!=", b"x")
    assert mask.tolist() == [False, False, True, False]
    assert validity == bitmap([True, False, True, True])


def test_compare_bytes_info_layout(tmp_path):
    """VxgCompareBytesInfo mirrors the header (size, offsets); the ABI version is 10."""
    fields = [f for f, _ in L.VxgCompareBytesInfo._fields_]
    src = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{ROOT}/include/vortex_gpu.h"', "int main(){",
           'printf("size %zu\\n", sizeof(vxg_compare_bytes_info));', 'printf("abi %d\\n", VXG_ABI_VERSION);']
    src += [f'printf("{f} %zu\\n", offsetof(vxg_compare_bytes_info, {f}));' for f in fields]
    src.append("return 0;}")
    (tmp_path / "cbi.c").write_text("\n".join(src))
    subprocess.run(["gcc", str(tmp_path / "cbi.c"), "-o", str(tmp_path / "cbi")], check=True)
    got = dict(ln.split() for ln in subprocess.run([str(tmp_path / "cbi")], capture_output=True, text=True,
                                                    check=True).stdout.splitlines())
    assert int(got["size"]) == C.sizeof(L.VxgCompareBytesInfo)
    assert int(got["abi"]) == L.ABI_VERSION == 10
    assert fields == ["dict_launches", "dict_chunks", "table_launches", "direct_launches", "direct_chunks",
                      "fallback_arrays"]
    for f in fields:
        assert int(got[f]) == getattr(L.VxgCompareBytesInfo, f).offset
    assert "vxg_compare_bytes" in L.GPU_SIGNATURES
