"""String compare-with-a-scalar against canonicalize, the least a caller paid for a string
predicate before (canonicalize, copy to the host, compare there).

Times `vxg_compare_bytes` and `vxg_canonicalize` (into caller-allocated views + data) of the same
arrays with device events, after a warm-up, alternating the two in one process (round r: K
compares, then K canonicalizes), and reports the median, minimum and maximum ms per call over the
rounds:
  c5_shipmode     l_shipmode of BASELINE C5: 92 chunks of 64 Ki rows, Dict(VarBin, BitPacked u64 codes); == "AIR"
  dict_64mi       one unchunked Dict(VarBin) of 64 Mi rows over the same 7 values; == "AIR"
  c5_comment_eq   l_comment of C5: 92 FSST chunks; == <a comment present in the data>
  c5_comment_lt   the same column; < "m"
(tools/lineitem.py's value domains and cascades; only these columns are generated).  Algorithmic
bytes over 8 TB/s: compare reads the array's buffers (packed codes + dictionary, or code bytes +
offsets + lengths + symbols) and writes the bitmap; canonicalize reads the same and writes views +
heap.  A case passes when compare's median is not above canonicalize's by more than the spread
(max - min) the rounds themselves show.  Usage:
  python tools/bench_compare_bytes.py [--rounds 20] [--calls 5] [--rows N] [--values N] [--out FILE]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import statistics
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))

HBM_BPS = 8e12


def shipmode_chunk(codes):
    import vortex_amd.arrays as A
    import vortex_amd.encode as E
    from lineitem import SHIPMODE
    heap, offs, _ = E.strings_to_heap(SHIPMODE)
    values = A.varbin(A.primitive(offs.astype(np.int32)), A.primitive(heap))
    return A.dict_array(values, E.encode_bitpacked(codes.astype(np.uint64), allow_patches=False))


def comment_chunk(rng, n):
    """One l_comment chunk as tools/lineitem.py draws it -> (FSST array, heap, offsets)."""
    import vortex_amd.encode as E
    from lineitem import WORDS
    lens = rng.integers(10, 44, n)
    wl = np.array([len(w) + 1 for w in WORDS])
    ids = rng.integers(0, len(WORDS), int(int(lens.sum()) / wl.mean() * 1.2) + 16)
    stream = b" ".join(WORDS[i] for i in ids)
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    heap = np.frombuffer(stream[: int(offs[-1])], dtype=np.uint8).copy()
    return E.encode_fsst_from_heap(heap, offs), heap, offs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--calls", type=int, default=5, help="back-to-back calls between two events")
    ap.add_argument("--values", type=int, default=64 << 20, help="rows of the unchunked Dict")
    ap.add_argument("--rows", type=int, default=6_001_215, help="rows of the C5 columns")
    ap.add_argument("--out", type=str, default="")
    args = ap.parse_args()
    import torch
    import vortex_amd as V
    import vortex_amd.arrays as A
    from lineitem import CHUNK_ROWS, SHIPMODE
    from vortex_amd import _lib

    assert torch.cuda.is_available(), "bench_compare_bytes needs a GPU"
    dev = torch.device("cuda", 0)
    ctx = V.Context(0)
    air = SHIPMODE.index(b"AIR")
    n_chunks = (args.rows + CHUNK_ROWS - 1) // CHUNK_ROWS
    sizes = [min(CHUNK_ROWS, args.rows - c * CHUNK_ROWS) for c in range(n_chunks)]

    codes = [np.random.default_rng([7, c]).integers(0, 7, n) for c, n in enumerate(sizes)]
    shipmode = A.chunked([shipmode_chunk(c) for c in codes])
    big_codes = np.random.default_rng(42).integers(0, 7, args.values)
    comments = [comment_chunk(np.random.default_rng([8, c]), n) for c, n in enumerate(sizes)]
    comment = A.chunked([t for t, _, _ in comments])
    _, h0, o0 = comments[n_chunks // 2]
    present = h0[o0[1000 % sizes[n_chunks // 2]]: o0[1000 % sizes[n_chunks // 2] + 1]].tobytes()

    def comment_mask(op, s):
        out = []
        for _, heap, offs in comments:
            if op == "<":  # every comment has at least 10 bytes: its first byte decides against a 1-byte scalar
                out.append(heap[offs[:-1]] < s[0])
            else:
                m = np.diff(offs) == len(s)
                for i in np.flatnonzero(m):
                    m[i] = heap[offs[i]: offs[i + 1]].tobytes() == s
                out.append(m)
        return np.concatenate(out)

    cases = [("c5_shipmode", "chunked dict(varbin, bitpacked u64) (l_shipmode)", shipmode, "==", b"AIR",
              lambda: np.concatenate(codes) == air),
             ("dict_64mi", "dict(varbin, bitpacked u64), 7 values", shipmode_chunk(big_codes), "==", b"AIR",
              lambda: big_codes == air),
             ("c5_comment_eq", "chunked fsst (l_comment)", comment, "==", present, lambda: comment_mask("==", present)),
             ("c5_comment_lt", "chunked fsst (l_comment)", comment, "<", b"m", lambda: comment_mask("<", b"m"))]
    results = []
    for name, enc, tree, op, scalar, want_mask in cases:
        keep: list = []
        dtree = tree.to(dev)
        node = A.flatten(dtree, keep)
        n = tree.len
        nb = ((n + 63) // 64) * 8
        bits = torch.empty(max(nb, 8), dtype=torch.uint8, device=dev)
        cmp_out = _lib.VxgCanonical()
        cmp_out.values = bits.data_ptr()
        can_out, can = A.alloc_canonical(ctx, node, keep)
        sc = (C.c_uint8 * len(scalar)).from_buffer_copy(scalar)
        info = _lib.VxgCompareBytesInfo()

        def compare():
            _lib.check(ctx.lib.vxg_compare_bytes(ctx.handle, C.byref(node), _lib.CMP_OP[op], sc, len(scalar), 0,
                                                 C.byref(cmp_out), C.byref(info), ctx.stream_ptr()))

        def canonicalize():
            _lib.check(ctx.lib.vxg_canonicalize(ctx.handle, C.byref(node), C.byref(can_out), ctx.stream_ptr()))

        for _ in range(3):  # warm-up: code objects, the stream-ordered pool
            compare()
            canonicalize()
        ctx.sync()
        want = np.packbits(want_mask(), bitorder="little")  # the result must be right before its time means anything
        got = bits.cpu().numpy()[: want.size]
        assert (got == want).all(), f"{name}: compare disagrees with the generated data"
        times = {"compare": [], "canonicalize": []}
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(args.rounds):
            for key, fn in (("compare", compare), ("canonicalize", canonicalize)):
                e0.record()
                for _k in range(args.calls):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                times[key].append(e0.elapsed_time(e1) / args.calls)
        read = tree.nbytes()
        canon_out = int(can.views.numel()) + int(can.data.numel())
        row = {"case": name, "encoding": enc, "rows": n, "op": op, "scalar_len": len(scalar),
               "true_rows": int(np.unpackbits(want, bitorder="little").sum()), "rounds": args.rounds,
               "calls_per_round": args.calls, "info": {f: int(getattr(info, f)) for f, _ in info._fields_}}
        for key, out_bytes in (("compare", nb), ("canonicalize", canon_out)):
            med = statistics.median(times[key])
            row[key] = {"ms_median": round(med, 5), "ms_min": round(min(times[key]), 5), "ms_max": round(max(times[key]), 5),
                        "bytes": read + out_bytes, "hbm_frac": round((read + out_bytes) / (med * 1e-3) / HBM_BPS, 4)}
        spread = max(row[k]["ms_max"] - row[k]["ms_min"] for k in ("compare", "canonicalize"))
        row["speedup"] = round(row["canonicalize"]["ms_median"] / row["compare"]["ms_median"], 3)
        row["spread_ms"] = round(spread, 5)
        row["not_slower"] = bool(row["compare"]["ms_median"] <= row["canonicalize"]["ms_median"] + spread)
        results.append(row)
        print(json.dumps(row), flush=True)
        del dtree, bits, keep, can
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps({"device": torch.cuda.get_device_name(0), "results": results}, indent=1) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
