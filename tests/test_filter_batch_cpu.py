"""CPU: the binding of vxg_filter_batch against the header (a compiled sizeof/offsetof probe), the
package export and the generated Rust FFI."""
import ctypes as C
import subprocess
import sys
from pathlib import Path

import vortex_amd as V
import vortex_amd._lib as L

ROOT = Path(__file__).resolve().parent.parent
SIGNATURE = L.GPU_SIGNATURES["vxg_filter_batch"]  # no symbol in the binding, no tests


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


def test_info_struct_mirrors_the_header(tmp_path):
    fields = [f for f, _ in L.VxgFilterBatchInfo._fields_]
    assert fields == ["columns", "mask_scans", "syncs", "packed_launches", "packed_chunks", "patch_launches",
                      "inplace_arrays", "fallback_arrays"]
    got = _probe(tmp_path, "fbinfo", "vxg_filter_batch_info", fields,
                 ['printf("abi %d\\n", VXG_ABI_VERSION);', 'printf("canon %d\\n", VXG_FILTB_CANONICALIZE);'])
    assert int(got["size"]) == C.sizeof(L.VxgFilterBatchInfo) == 32
    for f in fields:
        assert int(got[f]) == getattr(L.VxgFilterBatchInfo, f).offset
    assert int(got["abi"]) == L.ABI_VERSION == 10  # detected by the symbol: the version stays
    assert int(got["canon"]) == L.FILTB_CANONICALIZE == 1


def test_signature_is_bound():
    res, args = SIGNATURE
    assert res is L.ST and len(args) == 10
    assert args[1] == C.POINTER(C.POINTER(L.VxgArray)) and args[6] == C.POINTER(L.VxgCanonical)
    assert args[7] == C.POINTER(C.c_uint64) and args[8] == C.POINTER(L.VxgFilterBatchInfo)
    assert args[2] is C.c_uint32 and args[4] is C.c_uint64 and args[5] is C.c_uint32


def test_header_declares_the_entry_point():
    text = (ROOT / "include" / "vortex_gpu.h").read_text()
    assert "vxg_status vxg_filter_batch(vxg_ctx* ctx, const vxg_array* const* columns, uint32_t n_columns," in text
    assert "#define VXG_ABI_VERSION 10" in text


def test_package_exports_filter_batch():
    assert callable(V.filter_batch) and "filter_batch" in V.__all__
    assert V.filter_batch is V.arrays.filter_batch


def test_rust_ffi_is_current():
    r = subprocess.run([sys.executable, str(ROOT / "tools" / "gen_ffi_rs.py"), "--check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    ffi = (ROOT / "rust" / "vortex-gpu" / "src" / "ffi.rs").read_text()
    assert "pub fn vxg_filter_batch(" in ffi and "pub struct vxg_filter_batch_info" in ffi
