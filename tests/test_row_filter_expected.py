"""CPU: the expected-value helper of the row filter tests against hand-written literals, and the
ctypes mirrors of vxg_row_filter against the header (a compiled sizeof/offsetof probe)."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np

import vortex_amd._lib as L
import vortex_amd.arrays as A
import vortex_amd.encode as E
from row_filter_expected import expected

ROOT = Path(__file__).resolve().parent.parent
SIGNATURE = L.GPU_SIGNATURES["vxg_row_filter"]  # the helper is the checker of this entry point: no symbol, no tests


def test_hand_written_literal():
    a = A.primitive(np.array([1, 5, 9, 5, 2, 7, 5, 3, 8, 5], dtype=np.int32))
    b = A.primitive(np.array([0.5, 1.5, 2.5, 3.5, 0.5, 1.5, 2.5, 3.5, 0.5, 1.5]))
    s = E.encode_varbinview([b"x", b"y", b"x", b"y", b"y", b"y", b"y", b"z", b"y", b"y"])
    bits, mask, count = expected([(a, ">=", 3), (a, "<", 8), (b, "<", 3.0), (s, "==", b"y")])
    #  a in [3, 8):  . 5 . 5 . 7 5 3 . 5      b < 3.0: rows 0 1 2 4 5 6 8 9      s == y: rows 1 3 4 5 6 8 9
    assert mask.tolist() == [False, True, False, False, False, True, True, False, False, True]
    assert count == 4
    assert bits == bytes([0b01100010, 0b00000010, 0, 0, 0, 0, 0, 0])  # LSB first, one zero-padded 64-bit word


def test_a_null_in_any_column_clears_the_row():
    n = 6
    a = A.primitive(np.arange(n, dtype=np.uint32), validity=np.array([1, 1, 0, 1, 1, 1], bool))
    s = E.encode_dict_strings_nullable([b"k", None, b"k", b"k", b"k", b"j"])
    _, mask, count = expected([(a, "!=", 100), (s, "==", b"k")])
    assert mask.tolist() == [True, False, False, True, True, False]  # row 1: null string, row 2: null number
    assert count == 3
    # != is true against every value, yet not at a null: null_as_false, not Kleene
    assert expected([(a, "!=", 100)])[1].tolist() == [True, True, False, True, True, True]


def test_lower_bound_above_upper_bound_is_empty():
    a = A.primitive(np.arange(100, dtype=np.int16))
    bits, mask, count = expected([(a, ">", 60), (a, "<", 40)])
    assert not mask.any() and count == 0 and bits == bytes(16)


def test_nan_bound_is_empty():
    a = A.primitive(np.array([1.0, np.nan, -0.0, 0.0]))
    assert expected([(a, ">=", float("nan")), (a, "<", 5.0)])[2] == 0
    assert expected([(a, ">=", -0.0), (a, "<=", 0.0)])[1].tolist() == [False, False, True, True]


def _probe(tmp_path, name, ctype, fields, extra=()):
    src = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{ROOT}/include/vortex_gpu.h"', "int main(){",
           f'printf("size %zu\\n", sizeof({ctype}));']
    src += [f'printf("{f} %zu\\n", offsetof({ctype}, {f}));' for f in fields]
    src += list(extra)
    src.append("return 0;}")
    (tmp_path / f"{name}.c").write_text("\n".join(src))
    subprocess.run(["gcc", str(tmp_path / f"{name}.c"), "-o", str(tmp_path / name)], check=True)
    out = subprocess.run([str(tmp_path / name)], capture_output=True, text=True, check=True).stdout
    return dict(ln.split() for ln in out.splitlines())


def test_row_filter_struct_layouts(tmp_path):
    """VxgPredicate and VxgRowFilterInfo mirror the header (size, offsets), the flags have the
    header's values and the ABI version is still 10."""
    pf = [f for f, _ in L.VxgPredicate._fields_]
    assert pf == ["column", "op", "reserved", "scalar_host", "scalar_len"]
    got = _probe(tmp_path, "pred", "vxg_predicate", pf,
                 ['printf("abi %d\\n", VXG_ABI_VERSION);', 'printf("fuse %d\\n", VXG_ROWF_FUSE_RANGES);',
                  'printf("nofuse %d\\n", VXG_ROWF_NO_FUSE_RANGES);'])
    assert int(got["size"]) == C.sizeof(L.VxgPredicate) == 32
    for f in pf:
        assert int(got[f]) == getattr(L.VxgPredicate, f).offset
    assert int(got["abi"]) == L.ABI_VERSION == 10
    assert int(got["fuse"]) == L.ROWF_FUSE_RANGES == 1
    assert int(got["nofuse"]) == L.ROWF_NO_FUSE_RANGES == 2

    inf = [f for f, _ in L.VxgRowFilterInfo._fields_]
    assert inf == ["predicates", "range_pairs", "compare_passes", "range_launches", "fused_launches",
                   "fallback_arrays", "combine_launches", "reserved"]
    got = _probe(tmp_path, "info", "vxg_row_filter_info", inf)
    assert int(got["size"]) == C.sizeof(L.VxgRowFilterInfo) == 32
    for f in inf:
        assert int(got[f]) == getattr(L.VxgRowFilterInfo, f).offset


def test_signature_is_bound():
    res, args = SIGNATURE
    assert res is L.ST and len(args) == 8
    assert args[1] == C.POINTER(L.VxgPredicate) and args[6] == C.POINTER(L.VxgRowFilterInfo)
