"""take_canon (the CPU expectation of vxg_take_array_ex) on hand-written literals, and the Python
mirror of the new C ABI pieces.  Runs without a GPU."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

import vortex_amd._lib as L
import vortex_amd.arrays as A
import vortex_amd.encode as E
from take_expected import take_canon

ROOT = Path(__file__).resolve().parent.parent

ROWS = [b"hello", None, b"world", b"a string longer than twelve"]
INDICES = [3, 1, 0, 0]


def varbin_literal():
    heap = np.frombuffer(b"helloworlda string longer than twelve", np.uint8).copy()
    offs = np.array([0, 5, 5, 10, 37], np.int32)
    return A.varbin(A.primitive(offs), A.primitive(heap), validity=[True, False, True, True])


def test_take_canon_varbin_literal():
    (views, heap), valid = take_canon(varbin_literal(), INDICES)
    assert heap.tobytes() == b"a string longer than twelvehellohello"
    assert valid.tolist() == [True, False, True, True]
    assert views.shape == (4, 16)
    # view 0: not inline -- length 27, prefix, buffer 0, offset 0
    assert views[0].tobytes() == np.uint32(27).tobytes() + b"a st" + np.uint32(0).tobytes() + np.uint32(0).tobytes()
    assert views[1].tobytes() == bytes(16)
    inline = np.uint32(5).tobytes() + b"hello" + bytes(7)
    assert views[2].tobytes() == inline and views[3].tobytes() == inline


@pytest.mark.parametrize("make", [E.encode_fsst, E.encode_dict_strings_nullable, E.encode_varbinview],
                         ids=["fsst", "dict", "varbinview"])
def test_take_canon_is_the_same_for_every_encoding(make):
    (wv, wh), wvalid = take_canon(varbin_literal(), INDICES)
    (views, heap), valid = take_canon(make(ROWS), INDICES)
    assert heap.tobytes() == wh.tobytes()
    assert views.tobytes() == wv.tobytes()
    assert valid.tolist() == wvalid.tolist()


def test_take_canon_primitive_bool_and_bounds():
    v = np.arange(10, dtype=np.int32) * 3
    vals, valid = take_canon(A.primitive(v, validity=v % 2 == 0), [9, 0, 9])
    assert vals.tolist() == [27, 0, 27] and valid.tolist() == [False, True, False]
    m = np.array([True, False, True, True])
    vals, valid = take_canon(A.bool_array(m), np.array([1, 1, 3], np.uint8))
    assert vals.tolist() == [False, False, True] and valid is None
    (views, heap), valid = take_canon(E.encode_varbinview([b"x"]), np.zeros(0, np.int64))
    assert views.shape == (0, 16) and heap.size == 0
    for bad in ([4], [-1]):
        with pytest.raises(IndexError):
            take_canon(varbin_literal(), bad)


def test_take_info_layout(tmp_path):
    """VxgTakeInfo mirrors the header (size, offsets); the flag and the ABI version as well."""
    fields = [f for f, _ in L.VxgTakeInfo._fields_]
    src = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{ROOT}/include/vortex_gpu.h"', "int main(){",
           'printf("size %zu\\n", sizeof(vxg_take_info));', 'printf("abi %d\\n", VXG_ABI_VERSION);',
           'printf("flag %d\\n", VXG_TAKE_CANONICALIZE);']
    src += [f'printf("{f} %zu\\n", offsetof(vxg_take_info, {f}));' for f in fields]
    src.append("return 0;}")
    (tmp_path / "ti.c").write_text("\n".join(src))
    subprocess.run(["gcc", str(tmp_path / "ti.c"), "-o", str(tmp_path / "ti")], check=True)
    got = dict(ln.split() for ln in subprocess.run([str(tmp_path / "ti")], capture_output=True, text=True,
                                                    check=True).stdout.splitlines())
    assert int(got["size"]) == C.sizeof(L.VxgTakeInfo)
    assert int(got["abi"]) == L.ABI_VERSION == 10
    assert int(got["flag"]) == L.TAKE_CANONICALIZE
    assert fields == ["packed_launches", "dict_arrays", "direct_arrays", "fallback_arrays"]
    for f in fields:
        assert int(got[f]) == getattr(L.VxgTakeInfo, f).offset


def test_take_signature():
    assert "vxg_take_array_ex" in L.GPU_SIGNATURES
    assert len(L.GPU_SIGNATURES["vxg_take_array_ex"][1]) == len(L.GPU_SIGNATURES["vxg_take_array"][1]) + 2
    assert L.ABI_VERSION == 10
