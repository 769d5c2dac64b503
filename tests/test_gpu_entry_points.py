"""GPU: every per-encoding C entry point (include/vortex_gpu.h, "per-encoding kernels") called
directly, against the oracle, byte for byte -- float outputs as raw bits, no tolerance anywhere.

The cases are tests/entry_cases.py's (their expectations are checked on the CPU by
tests/test_entry_cases.py).  Every valid case: upload the inputs, call the entry point with a
caller-allocated output between two 64-byte guards, sync, compare the output with the oracle's
bytes and the guards with their pattern.  Every rejected case: the status the case names, from the
call or from the next vxg_stream_sync, nothing written outside the output, and a clean sync after.
"""
import ctypes as C

import numpy as np
import pytest

import entry_cases as EC
import vortex_amd as V
from vortex_amd._lib import STATUS, VxgDictChunk

pytestmark = pytest.mark.gpu

GUARD = 64        # bytes of GUARD_BYTE before and after every output
GUARD_BYTE = 0xA5
CODE = {name: code for code, name in STATUS.items()}


def _vp(addr):
    return C.c_void_p(addr) if addr else None


class Guarded:
    """A caller-allocated device output of o.nbytes (+ o.slack) bytes between two guards."""

    def __init__(self, o: EC.Out, init=None):
        import torch
        self.o = o
        self.lo = GUARD + o.shift
        self.n = o.nbytes + o.slack
        self.t = torch.full((self.lo + self.n + GUARD + 16,), GUARD_BYTE, dtype=torch.uint8, device="cuda")
        assert self.t.data_ptr() % 16 == 0
        init = o.init if init is None else init
        start = np.full(self.n, EC.FILL, dtype=np.uint8)
        if init is not None:
            start[: len(init)] = np.frombuffer(init, np.uint8)
        self.start = start
        if self.n:
            self.t[self.lo: self.lo + self.n].copy_(torch.from_numpy(start))
        self.ptr = self.t.data_ptr() + self.lo

    def read(self):
        """-> (output bytes [0, nbytes), guards intact?) after a sync."""
        h = self.t.cpu().numpy()
        intact = bool((h[: self.lo] == GUARD_BYTE).all() and (h[self.lo + self.n:] == GUARD_BYTE).all())
        return h[self.lo: self.lo + self.o.nbytes], intact


def upload(a: np.ndarray, shift: int = 0):
    """-> (tensor, address) of a's bytes, `shift` bytes after a 16-byte boundary; 0 for no bytes."""
    import torch
    b = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    if b.size == 0:
        return None, 0
    t = torch.zeros(((b.size + shift + 15) // 16) * 16 + 16, dtype=torch.uint8, device="cuda")
    t[shift: shift + b.size].copy_(torch.from_numpy(b))
    return t, t.data_ptr() + shift


# ---- one caller per entry point: (lib, ctx handle, stream, case args, pointers) -> status ----
def _pt(name):
    return V.PTYPE[name]


def call_bitunpack(lib, h, s, a, p):
    return lib.vxg_bitunpack(h, _pt(a["ptype"]), a["W"], a["offset"], a["len"], _vp(p["packed"]), a["packed_bytes"],
                             _vp(p["out"]), s)


def call_bitunpack_for(lib, h, s, a, p):
    return lib.vxg_bitunpack_for(h, _pt(a["ptype"]), a["W"], a["offset"], a["len"], _vp(p["packed"]), a["packed_bytes"],
                                 a["reference"], a["shift"], a["zigzag"], _vp(p["out"]), s)


def call_bitunpack_alp(lib, h, s, a, p):
    return lib.vxg_bitunpack_alp(h, _pt(a["ptype"]), a["W"], a["offset"], a["len"], _vp(p["packed"]), a["packed_bytes"],
                                 a["reference"], a["shift"], a["e"], a["f"], _vp(p["out"]), s)


def call_bitunpack_dict(lib, h, s, a, p):
    return lib.vxg_bitunpack_dict(h, _pt(a["ptype"]), a["W"], a["offset"], a["len"], _vp(p["packed"]), a["packed_bytes"],
                                  _vp(p["dict"]), a["dict_len"], a["vw"], _vp(p["out"]), s)


def call_bitunpack_dict_chunks(lib, h, s, a, p):
    tab = (VxgDictChunk * max(len(a["chunks"]), 1))()
    for i, ch in enumerate(a["chunks"]):
        tab[i].packed = p[f"packed{i}"] or None
        tab[i].dict_values = p[f"dict{i}"] or None
        tab[i].out = (p["out"] + ch["out_offset"]) if p["out"] else None
        tab[i].n_blocks, tab[i].len, tab[i].dict_len = ch["n_blocks"], ch["len"], ch["dict_len"]
    return lib.vxg_bitunpack_dict_chunks(h, _pt(a["ptype"]), a["W"], a["vw"], tab if p.get("chunk_table", 1) else None,
                                         len(a["chunks"]), s)


def call_patch(lib, h, s, a, p):
    return lib.vxg_patch(h, _pt(a["ptype"]), _vp(p["out"]), a["out_len"], _pt(a["indices_ptype"]), _vp(p["indices"]),
                         a["indices_offset"], _vp(p["values"]), a["n_patches"], s)


def call_for_decode(lib, h, s, a, p):
    return lib.vxg_for_decode(h, _pt(a["ptype"]), _vp(p["in"]), a["n"], a["reference"], a["shift"], _vp(p["out"]), s)


def call_zigzag_decode(lib, h, s, a, p):
    return lib.vxg_zigzag_decode(h, _pt(a["ptype"]), _vp(p["in"]), a["n"], _vp(p["out"]), s)


def call_alp_decode(lib, h, s, a, p):
    return lib.vxg_alp_decode(h, _pt(a["ptype"]), _vp(p["encoded"]), a["n"], a["e"], a["f"], _vp(p["out"]), s)


def call_alprd_decode(lib, h, s, a, p):
    d = np.ascontiguousarray(a["dict"], dtype=np.uint16)
    return lib.vxg_alprd_decode(h, _pt(a["ptype"]), _vp(p["left"]), d.ctypes.data if p.get("dict_host", 1) else None,
                                d.size, a["right_bw"], _vp(p["right"]), a["n"], _vp(p["exc_pos"]), _vp(p["exc_vals"]),
                                a["n_exc"], _vp(p["out"]), s)


def call_take(lib, h, s, a, p):
    return lib.vxg_take(h, a["vw"], _vp(p["values"]), a["n_values"], _pt(a["codes_ptype"]), _vp(p["codes"]), a["n"],
                        _vp(p["out"]), s)


def call_delta_decode(lib, h, s, a, p):
    return lib.vxg_delta_decode(h, _pt(a["ptype"]), _vp(p["bases"]), a["n_bases"], _vp(p["deltas"]), a["n_deltas"],
                                a["offset"], a["len"], _vp(p["out"]), s)


def call_runend_decode(lib, h, s, a, p):
    return lib.vxg_runend_decode(h, a["vw"], _vp(p["values"]), _pt(a["ends_ptype"]), _vp(p["ends"]), a["n_runs"],
                                 a["offset"], a["len"], _vp(p["out"]), s)


def call_runend_bool_decode(lib, h, s, a, p):
    return lib.vxg_runend_bool_decode(h, _pt(a["ends_ptype"]), _vp(p["ends"]), a["n_runs"], a["offset"], a["start"],
                                      a["len"], _vp(p["out"]), a["out_bit_offset"], s)


def call_bytebool_to_bits(lib, h, s, a, p):
    return lib.vxg_bytebool_to_bits(h, _vp(p["bytes"]), a["n"], _vp(p["out"]), a["out_bit_offset"], s)


def call_fill(lib, h, s, a, p):
    sc = C.create_string_buffer(a["scalar"], len(a["scalar"]))
    return lib.vxg_fill(h, a["vw"], C.cast(sc, C.c_void_p) if p.get("scalar", 1) else None, a["n"], _vp(p["out"]), s)


def call_fsst_decode(lib, h, s, a, p):
    return lib.vxg_fsst_decode(h, _vp(p["symbols"]), _vp(p["sym_lens"]), a["n_symbols"], _vp(p["codes"]),
                               _pt(a["offs_ptype"]), _vp(p["offsets"]), _pt(a["lens_ptype"]), _vp(p["lens"]), a["n"],
                               _vp(p.get("validity", 0)), _vp(p["scratch"]), _vp(p["heap"]), _vp(p["views"]), s)


CALL = {
    "vxg_bitunpack": call_bitunpack,
    "vxg_bitunpack_for": call_bitunpack_for,
    "vxg_bitunpack_alp": call_bitunpack_alp,
    "vxg_bitunpack_dict": call_bitunpack_dict,
    "vxg_bitunpack_dict_chunks": call_bitunpack_dict_chunks,
    "vxg_patch": call_patch,
    "vxg_for_decode": call_for_decode,
    "vxg_zigzag_decode": call_zigzag_decode,
    "vxg_alp_decode": call_alp_decode,
    "vxg_alprd_decode": call_alprd_decode,
    "vxg_take": call_take,
    "vxg_delta_decode": call_delta_decode,
    "vxg_runend_decode": call_runend_decode,
    "vxg_fsst_decode": call_fsst_decode,
    "vxg_runend_bool_decode": call_runend_bool_decode,
    "vxg_bytebool_to_bits": call_bytebool_to_bits,
    "vxg_fill": call_fill,
}


class Staged:
    """A case's inputs on the device and its guarded outputs."""

    def __init__(self, c: EC.Case, lib):
        self.keep, self.p, self.outs = [], {}, {}
        for name, o in c.outs.items():
            init = np.ascontiguousarray(c.bufs[c.inplace]).tobytes() if c.inplace and name == "out" else None
            self.outs[name] = Guarded(o, init)
            self.p[name] = self.outs[name].ptr
        if c.entry == "vxg_fsst_decode":  # scratch of exactly vxg_fsst_scratch_bytes(n) bytes
            self.outs["scratch"] = Guarded(EC.Out(int(lib.vxg_fsst_scratch_bytes(c.args["n"]))))
            self.p["scratch"] = self.outs["scratch"].ptr
        for name, a in c.bufs.items():
            if name == c.inplace:
                self.p[name] = self.p["out"]
                continue
            t, addr = upload(a, c.shift_in.get(name, 0))
            self.keep.append(t)
            self.p[name] = addr


def run_case(c: EC.Case, lib, ctx):
    """-> None, or what went wrong (one line)."""
    st = Staged(c, lib)
    status = CALL[c.entry](lib, ctx.handle, ctx.stream_ptr(), c.args, st.p)
    sync = "OK"
    try:
        ctx.sync()
    except V.VortexGpuError as e:
        sync = e.kind
        ctx.sync()  # the error word was cleared: the next sync is clean (raises if it is not)
    want_call = c.error if c.error and c.at == "call" else "OK"
    want_sync = c.error if c.error and c.at == "sync" else "OK"
    if STATUS.get(status, status) != want_call:
        return f"call returned {STATUS.get(status, status)} ({lib.vxg_last_error().decode(errors='replace')}), want {want_call}"
    if sync != want_sync:
        return f"sync returned {sync}, want {want_sync}"
    for name, g in st.outs.items():
        got, intact = g.read()
        if not intact:
            return f"guard bytes around {name} were written"
        want = g.o.want
        if c.error and c.at == "call":
            want = g.start[: g.o.nbytes].tobytes()  # a rejected call writes nothing
        if want is not None and got.tobytes() != want:
            w = np.frombuffer(want, np.uint8)
            bad = np.flatnonzero(got != w)
            return f"{name}: {bad.size} of {w.size} bytes differ from the oracle, first at byte {int(bad[0])}"
    return None


def run_all(cases, lib, ctx):
    failed = [(c.name, why) for c in cases if (why := run_case(c, lib, ctx)) is not None]
    assert not failed, f"{len(failed)} of {len(cases)} cases failed: " + "; ".join(f"{n}: {w}" for n, w in failed[:8])


@pytest.mark.parametrize("entry", EC.ENTRY_POINTS)
def test_parity_with_the_oracle(ctx, entry):
    cases = [c for c in EC.cases(entry) if c.error is None]
    assert cases
    run_all(cases, V.gpu_lib(), ctx)


@pytest.mark.parametrize("entry", [e for e in EC.ENTRY_POINTS if e != "vxg_bytebool_to_bits"])
def test_rejected_arguments(ctx, entry):
    """Bad arguments get the status the reference's error has -- from the call where the host can
    see it, from the next sync where only a kernel can (an index, a code, an end) -- nothing is
    written outside the output, and the error word does not leak into the next sync."""
    cases = [c for c in EC.cases(entry) if c.error is not None]
    assert cases
    run_all(cases, V.gpu_lib(), ctx)
    ctx.sync()


# Pointers each entry point must check for null before it launches (host status only: the guard
# returns before any launch, include/vortex_gpu.h "per-encoding kernels").  Not listed: pointers
# that may be null for valid input (FSST code bytes / heap / validity, the packed buffer at W = 0).
NULL_CHECKED = {
    "vxg_bitunpack": ["packed", "out"],
    "vxg_bitunpack_for": ["packed", "out"],
    "vxg_bitunpack_alp": ["packed", "out"],
    "vxg_bitunpack_dict": ["packed", "dict", "out"],
    "vxg_bitunpack_dict_chunks": ["packed0", "dict0", "out", "chunk_table"],
    "vxg_patch": ["indices", "values", "out"],
    "vxg_for_decode": ["in", "out"],
    "vxg_zigzag_decode": ["in", "out"],
    "vxg_alp_decode": ["encoded", "out"],
    "vxg_alprd_decode": ["left", "right", "exc_pos", "exc_vals", "dict_host", "out"],
    "vxg_take": ["values", "codes", "out"],
    "vxg_delta_decode": ["bases", "deltas", "out"],
    "vxg_runend_decode": ["values", "ends", "out"],
    "vxg_fsst_decode": ["symbols", "sym_lens", "offsets", "lens", "scratch", "views"],
    "vxg_runend_bool_decode": ["ends", "out"],
    "vxg_bytebool_to_bits": ["bytes", "out"],
    "vxg_fill": ["scalar", "out"],
}


@pytest.mark.parametrize("entry", EC.ENTRY_POINTS)
def test_null_pointers_are_invalid_arguments(ctx, entry):
    lib = V.gpu_lib()
    names = NULL_CHECKED[entry]

    def usable(c):  # a valid case that touches every pointer
        return (c.error is None and not c.inplace and all(o.nbytes for o in c.outs.values())
                and all(c.bufs[n].size for n in names if n in c.bufs) and c.args.get("n_exc", 1) and c.args.get("W", 1))

    c = next(c for c in EC.cases(entry) if usable(c))
    st = Staged(c, lib)
    for name in names:
        assert st.p.get(name, 1), name
        p = dict(st.p)
        p[name] = 0
        status = CALL[entry](lib, ctx.handle, ctx.stream_ptr(), c.args, p)
        assert STATUS.get(status) == "InvalidArgument", (name, STATUS.get(status, status))
        assert b"null" in lib.vxg_last_error()
    assert CALL[entry](lib, None, ctx.stream_ptr(), c.args, st.p) == CODE["InvalidArgument"]  # null context
    ctx.sync()
    for name, g in st.outs.items():  # nothing was launched
        got, intact = g.read()
        assert intact and got.tobytes() == g.start[: g.o.nbytes].tobytes(), name


def test_value_width_zero_does_not_divide_by_zero(ctx):
    """vxg_bitunpack_dict(value_width = 0) used to reach `uintptr_t(out) % 0` in make_k1_job."""
    lib = V.gpu_lib()
    c = next(c for c in EC.cases("vxg_bitunpack_dict") if c.name == "value-width-0")
    assert run_case(c, lib, ctx) is None
    assert b"value width" in lib.vxg_last_error()


@pytest.mark.parametrize("entry", ["vxg_take", "vxg_fill", "vxg_for_decode"])
def test_grid_stride_second_trip(ctx, entry):
    """More elements than the launch cap's threads (32768 workgroups of 256): some thread's
    grid-stride loop makes a second trip."""
    c = EC.grid_stride_case(entry)
    assert c.args["n"] > EC.GRID_CAP_THREADS * (2 if entry == "vxg_for_decode" else 1)
    assert run_case(c, V.gpu_lib(), ctx) is None
