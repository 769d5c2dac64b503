"""String take on the compressed forms against canonicalize-then-gather, over index density.

Times `vxg_take_array_ex` (views and data caller-allocated, so no allocation is timed) with flags 0
(the in-place path of the encoding) and with VXG_TAKE_CANONICALIZE (the whole array canonicalized
into temporaries, then gathered) with device events, after a warm-up, alternating the two in one
process (round r: K in-place calls, then K forced ones), and reports the median, minimum and maximum
ms per call over the rounds.  The call is synchronous (the heap size is read back), so a call's time
includes that round trip.  Columns (tools/bench_compare_bytes.py's generators and sizes):
  varbin_comment  l_comment of BASELINE C5 as one VarBin (i32 offsets), --rows rows
  fsst_comment    the same rows as one FSST array (offsets and lengths FoR + BitPacked)
  dict_shipmode   Dict(VarBin, BitPacked u64 codes) over the 7 l_shipmode values, --values rows
each with n_indices = len/1024, len/64, len/8, len/4, len/2 and len, random (with repeats) and sorted.  The first
result of every case is checked against the generated rows before its time means anything.  Usage:
  python tools/bench_take_strings.py [--rounds 10] [--calls 3] [--rows N] [--values N] [--out FILE]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--calls", type=int, default=3, help="back-to-back calls between two events")
    ap.add_argument("--values", type=int, default=64 << 20, help="rows of the Dict column")
    ap.add_argument("--rows", type=int, default=6_001_215, help="rows of the l_comment columns")
    ap.add_argument("--out", type=str, default="")
    args = ap.parse_args()
    import torch
    import vortex_amd as V
    import vortex_amd.arrays as A
    from bench_compare_bytes import comment_chunk, shipmode_chunk
    from lineitem import SHIPMODE
    from vortex_amd import _lib

    assert torch.cuda.is_available(), "bench_take_strings needs a GPU"
    dev = torch.device("cuda", 0)
    ctx = V.Context(0)

    fsst, heap, offs = comment_chunk(np.random.default_rng([8, 0]), args.rows)
    varbin = A.varbin(A.primitive(offs.astype(np.int32)), A.primitive(heap))
    big_codes = np.random.default_rng(42).integers(0, 7, args.values)
    ship_heap = np.frombuffer(b"".join(SHIPMODE), np.uint8)
    ship_offs = np.concatenate([[0], np.cumsum([len(s) for s in SHIPMODE])]).astype(np.int64)

    def rows_of_comment(idx):
        return offs[idx], offs[idx + 1]

    def rows_of_shipmode(idx):
        c = big_codes[idx]
        return ship_offs[c], ship_offs[c + 1]

    columns = [("varbin_comment", "varbin(i32 offsets) (l_comment)", varbin, heap, rows_of_comment),
               ("fsst_comment", "fsst (l_comment)", fsst, heap, rows_of_comment),
               ("dict_shipmode", "dict(varbin, bitpacked u64), 7 values", shipmode_chunk(big_codes), ship_heap, rows_of_shipmode)]
    results = []
    for name, enc, tree, src_heap, rows_of in columns:
        keep: list = []
        dtree = tree.to(dev)
        node = A.flatten(dtree, keep)
        n = tree.len
        for div in (1024, 64, 8, 4, 2, 1):
            k = n // div
            for order in ("random", "sorted"):
                idx = np.random.default_rng([9, div]).integers(0, n, k).astype(np.uint32)
                if order == "sorted":
                    idx.sort()
                b0, b1 = rows_of(idx.astype(np.int64))
                heap_bytes = int((b1 - b0).sum())
                it = torch.from_numpy(idx.view(np.uint8)).to(dev)
                views = torch.empty(max(16 * k, 16), dtype=torch.uint8, device=dev)
                data = torch.empty(heap_bytes + 16, dtype=torch.uint8, device=dev)
                table = (_lib.VxgDataBuffer * 1)()
                infos = {}

                def call(flags):
                    out = _lib.VxgCanonical()
                    out.views, out.data, out.data_bytes = views.data_ptr(), data.data_ptr(), heap_bytes
                    out.data_buffers, out.data_buffers_cap = table, 1
                    info = _lib.VxgTakeInfo()
                    _lib.check(ctx.lib.vxg_take_array_ex(ctx.handle, C.byref(node), A.PTYPE["u32"], C.c_void_p(it.data_ptr()),
                                                         k, flags, C.byref(out), C.byref(info), ctx.stream_ptr()))
                    infos[flags] = {f: int(getattr(info, f)) for f, _ in info._fields_}
                    return out

                variants = (("in_place", 0), ("canonical", _lib.TAKE_CANONICALIZE))
                for key, flags in variants:  # warm-up, and the result checked against the generated rows
                    data.zero_()
                    out = call(flags)
                    ctx.sync()
                    assert int(out.data_bytes) == heap_bytes, f"{name}/{key}: heap size {out.data_bytes} != {heap_bytes}"
                    m = min(k, 2000)
                    want = b"".join(src_heap[int(a): int(b)].tobytes() for a, b in zip(b0[:m], b1[:m]))
                    assert data[: len(want)].cpu().numpy().tobytes() == want, f"{name}/{key}: taken bytes differ"
                    call(flags)
                ctx.sync()
                times = {key: [] for key, _ in variants}
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                for _ in range(args.rounds):
                    for key, flags in variants:
                        e0.record()
                        for _k in range(args.calls):
                            call(flags)
                        e1.record()
                        torch.cuda.synchronize()
                        times[key].append(e0.elapsed_time(e1) / args.calls)
                row = {"case": name, "encoding": enc, "rows": n, "n_indices": k, "len_over_n": div, "order": order,
                       "heap_bytes": heap_bytes, "rounds": args.rounds, "calls_per_round": args.calls,
                       "info": infos[0], "info_canonical": infos[_lib.TAKE_CANONICALIZE]}
                for key, _ in variants:
                    t = times[key]
                    row[key] = {"ms_median": round(statistics.median(t), 5), "ms_min": round(min(t), 5),
                                "ms_max": round(max(t), 5)}
                row["speedup"] = round(row["canonical"]["ms_median"] / row["in_place"]["ms_median"], 3)
                row["spread_ms"] = round(max(row[key]["ms_max"] - row[key]["ms_min"] for key, _ in variants), 5)
                row["not_slower"] = bool(row["in_place"]["ms_median"] <= row["canonical"]["ms_median"] + row["spread_ms"])
                results.append(row)
                print(json.dumps(row), flush=True)
                del it, views, data
        del dtree, keep
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps({"device": torch.cuda.get_device_name(0), "results": results}, indent=1) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
