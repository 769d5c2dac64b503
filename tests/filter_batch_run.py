"""One vxg_filter_batch call and its comparison with oracle_tree.filter_canon (plain module).

`run` goes through the C ABI with caller-provided outputs sized exactly for the k selected rows plus
GUARD bytes of 0xFF: the guards must come back untouched, k must be the mask's popcount and each out
must equal what filter(column, mask) gives, byte for byte.  It has two halves: `call` issues the
call and copies every buffer to the host; `check_outputs` asserts, and needs no GPU (so
tests/test_batch_cases.py can show that it fails when a byte is wrong).  With allocate=True every
out pointer is NULL: the engine allocates, the buffers are copied out and released with vxg_free.
"""
import ctypes as C
from dataclasses import dataclass, field
from typing import Optional

import numpy as np

import vortex_amd as V
import vortex_amd._lib as L
import vortex_amd.arrays as A
from oracle_tree import filter_canon

GUARD = 64


def _dev():
    import torch
    return torch.device("cuda", 0)


def mask_bytes(mask: np.ndarray, dirty_tail: bool = False) -> np.ndarray:
    """The bitmap of a bool mask: whole u64 words, the bits past len zero (or all set)."""
    n = mask.size
    nb = ((n + 63) // 64) * 8
    bits = np.zeros(nb * 8, dtype=bool)
    bits[:n] = mask
    if dirty_tail:
        bits[n:] = True
    return np.packbits(bits, bitorder="little") if nb else np.zeros(0, np.uint8)


def mask_tensor(mask: np.ndarray, dirty_tail: bool = False):
    """The device bitmap of a bool mask: whole u64 words, the bits past len zero (or all set)."""
    import torch
    host = mask_bytes(mask, dirty_tail)
    return torch.from_numpy(np.concatenate([host, np.zeros(8, np.uint8)])).to(_dev())  # (never an empty tensor)


def _kind(tree):
    return {A.DTYPE["PRIMITIVE"]: "primitive", A.DTYPE["BOOL"]: "bool"}.get(tree.dtype, "varbinview")


def _guarded(nbytes: int):
    import torch
    return torch.full((nbytes + GUARD,), 0xFF, dtype=torch.uint8, device=_dev())


@dataclass
class HostBuffer:
    """One output buffer as it came back: its bytes (guard included), the size the caller gave it
    and the device pointer it was passed as (None: the engine allocated it)."""
    bytes: np.ndarray
    nbytes: int
    ptr: Optional[int] = None


@dataclass
class HostOut:
    """The fields of one vxg_canonical after the call, in host memory."""
    len: int
    dtype: int
    kind: int
    values_bytes: int = 0
    data_bytes: int = 0
    n_data_buffers: int = 0
    data_buffers: list = field(default_factory=list)   # (offset, len) of the table's first entry
    validity: int = 0                                   # the pointer as the engine left it (0 = NULL)


def buffer_sizes(trees, want, k: int):
    """name -> bytes of every buffer column i needs for k selected rows."""
    vbytes = ((k + 31) // 32) * 4
    out = []
    for t, (wvals, _) in zip(trees, want):
        kind = _kind(t)
        if kind == "primitive":
            b = {"values": k * A.ptype_width(t.ptype)}
        elif kind == "bool":
            b = {"values": vbytes}
        else:
            b = {"views": 16 * k, "data": len(wvals[1])}
        if t.nullable:
            b["validity"] = vbytes
        out.append(b)
    return out


def call(ctx, trees, mask: np.ndarray, flags: int = 0, dirty_tail: bool = False, want=None, allocate: bool = False,
         nodes=None):
    """vxg_filter_batch of `trees` under `mask` -> (k, host buffers, outs, info) with everything in
    host memory.  `nodes`: prepared vxg_array nodes of `trees` (e.g. the file reader's, over a file's
    bytes in device memory) that go to the engine as they stand; by default every tree is uploaded
    and flattened here."""
    import torch
    n, k = mask.size, int(mask.sum())
    keep: list = []
    if nodes is None:
        nodes = [A.flatten(t.to(_dev()), keep) for t in trees]
    cols = (C.POINTER(L.VxgArray) * len(trees))(*[C.pointer(nd) for nd in nodes])
    outs = (L.VxgCanonical * len(trees))()
    mt = mask_tensor(mask, dirty_tail)
    sizes = buffer_sizes(trees, want, k)
    bufs = []
    for i, t in enumerate(trees):
        b = {}
        if not allocate:
            b = {name: _guarded(nbytes) for name, nbytes in sizes[i].items()}
            for name, buf in b.items():
                setattr(outs[i], name, buf.data_ptr())
            if "data" in b:
                outs[i].data_bytes = sizes[i]["data"]
        if _kind(t) == "varbinview":
            table = (L.VxgDataBuffer * 1)()
            keep.append(table)
            outs[i].data_buffers, outs[i].data_buffers_cap = table, 1
        bufs.append(b)
    kk = C.c_uint64(1 << 60)
    info = L.VxgFilterBatchInfo()
    L.check(ctx.lib.vxg_filter_batch(ctx.handle, cols, len(trees), C.c_void_p(mt.data_ptr()) if n else None, n, flags,
                                     outs, C.byref(kk), C.byref(info), ctx.stream_ptr()))
    ctx.sync()
    host, houts = [], []
    for i, t in enumerate(trees):
        o = outs[i]
        if allocate:  # what the engine allocated: copied out (D2D into a torch buffer), then released
            h = {}
            for name, nbytes in sizes[i].items():
                ptr = getattr(o, name)
                if not ptr:
                    continue
                got = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=_dev())
                if nbytes:
                    L.check(ctx.lib.vxg_memcpy_d2d(ctx.handle, C.c_void_p(got.data_ptr()), C.c_void_p(ptr), nbytes,
                                                   ctx.stream_ptr()))
                    ctx.sync()
                L.check(ctx.lib.vxg_free(ctx.handle, C.c_void_p(ptr)))
                h[name] = HostBuffer(got.cpu().numpy()[:nbytes], nbytes, None)
            host.append(h)
        else:
            host.append({name: HostBuffer(buf.cpu().numpy(), sizes[i][name], buf.data_ptr())
                         for name, buf in bufs[i].items()})
        table = [(int(o.data_buffers[0].offset), int(o.data_buffers[0].len))] if _kind(t) == "varbinview" else []
        houts.append(HostOut(int(o.len), int(o.dtype), int(o.kind), int(o.values_bytes), int(o.data_bytes),
                             int(o.n_data_buffers), table, int(o.validity or 0)))
    return int(kk.value), host, houts, {f: int(getattr(info, f)) for f, _ in info._fields_}


def check_outputs(host, outs, want, trees, n: int, k: int, flags: int = 0, at: str = ""):
    """Every out of one call against (values, validity) as filter_canon states them: untouched guard
    bytes, the header, the values / views + heap and the validity bitmap, byte for byte."""
    vbytes = ((k + 31) // 32) * 4
    for i, t in enumerate(trees):
        (wvals, wvalid), o, b = want[i], outs[i], host[i]
        what = (i, t.encoding, n, k, flags, at)
        for name, hb in b.items():
            assert (hb.bytes[hb.nbytes:] == 0xFF).all(), ("guard bytes written", name) + what
        assert o.len == k and o.dtype == t.dtype, what
        kind = _kind(t)
        if kind == "primitive":
            assert o.kind == V.ENC["PRIMITIVE"] and o.values_bytes == k * A.ptype_width(t.ptype), what
            if k:  # (k == 0 with engine-allocated outs: nothing is allocated)
                assert b["values"].bytes[: o.values_bytes].tobytes() == wvals.tobytes(), ("values differ",) + what
        elif kind == "bool":
            assert o.kind == V.ENC["BOOL"], what
            if k:  # (k == 0: nothing is launched, so nothing zeroes the buffers)
                wbits = np.zeros(vbytes * 8, bool)
                wbits[:k] = wvals
                assert b["values"].bytes[:vbytes].tobytes() == np.packbits(wbits, bitorder="little").tobytes(), \
                    ("bits differ",) + what
        else:
            wv, wh = wvals
            assert o.kind == V.ENC["VARBINVIEW"] and o.data_bytes == len(wh) and o.n_data_buffers == 1, what
            if k:
                assert b["views"].bytes[: 16 * k].tobytes() == wv.tobytes(), ("views differ",) + what
                assert b["data"].bytes[: len(wh)].tobytes() == wh.tobytes(), ("heap differs",) + what
            assert o.data_buffers[0] == (0, len(wh)), what
        if wvalid is None:
            assert not o.validity, what
        elif k:
            assert o.validity and "validity" in b, what
            assert b["validity"].ptr is None or o.validity == b["validity"].ptr, what
            wbits = np.zeros(vbytes * 8, bool)
            wbits[:k] = wvalid
            assert b["validity"].bytes[:vbytes].tobytes() == np.packbits(wbits, bitorder="little").tobytes(), \
                ("validity differs",) + what


def run(ctx, trees, mask: np.ndarray, flags: int = 0, dirty_tail: bool = False, want=None, allocate: bool = False,
        at: str = "", nodes=None):
    """vxg_filter_batch of `trees` under `mask` into exactly-sized guarded buffers; every out is
    compared with filter_canon.  Returns the info counters."""
    n, k = mask.size, int(mask.sum())
    want = want if want is not None else [filter_canon(t, A.bool_array(mask)) for t in trees]
    kk, host, outs, res = call(ctx, trees, mask, flags, dirty_tail, want, allocate, nodes)
    assert kk == k, (kk, k, at)
    check_outputs(host, outs, want, trees, n, k, flags, at)
    assert res["columns"] == len(trees) and res["mask_scans"] == (1 if n else 0), (res, at)
    return res
