"""Compare-with-a-scalar against canonicalize, the least a caller paid for a predicate before.

Times `vxg_compare_scalar(<)` and `vxg_canonicalize` of the same arrays with device events, after
a warm-up, alternating the two in one process (round r: K compares, then K canonicalizes), and
reports the median, minimum and maximum ms per call over the rounds:
  c1        BASELINE C1: BitPacked u32, W = 7, 64 Mi values
  c5_i64    l_partkey of BASELINE C5: 92 chunks of 64 Ki rows, FoR(BitPacked) i64
  c5_f64    l_extendedprice of C5: 92 chunks, ALP(FoR(BitPacked)) f64 with patches
(the C5 columns use tools/lineitem.py's value domains and cascades, only these two columns are
generated).  Achieved bytes/s counts packed + patches + bitmap (+ validity) for compare and
packed + patches + values for canonicalize, over 8 TB/s.  Usage:
  python tools/bench_compare.py [--rounds 20] [--calls 5] [--values N] [--out FILE]
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


def c5_column(name: str, rows: int, chunk_rows: int):
    """One lineitem column as bench-vortex writes it: 64 Ki-row chunks, each compressed alone."""
    import vortex_amd.arrays as A
    import vortex_amd.encode as E
    chunks = []
    for c in range((rows + chunk_rows - 1) // chunk_rows):
        rng = np.random.default_rng([7, c])
        n = min(chunk_rows, rows - c * chunk_rows)
        partkey = rng.integers(1, 200_001, n)
        if name == "l_partkey":
            chunks.append(E.encode_for_bitpacked(partkey.astype(np.int64)))
        else:  # l_extendedprice = quantity * retail price, two decimals
            qty = rng.integers(1, 51, n)
            retail = (90_000 + (partkey // 10) % 20_001 + 100 * (partkey % 1_000)) / 100.0
            chunks.append(E.encode_alp(np.round(qty * retail, 2)))
    return A.chunked(chunks)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--calls", type=int, default=5, help="back-to-back calls between two events")
    ap.add_argument("--values", type=int, default=64 << 20, help="values of the C1 array")
    ap.add_argument("--rows", type=int, default=6_001_215, help="rows of the C5 columns")
    ap.add_argument("--out", type=str, default="")
    args = ap.parse_args()
    import torch
    import vortex_amd as V
    import vortex_amd.arrays as A
    import vortex_amd.encode as E
    from vortex_amd import _lib

    assert torch.cuda.is_available(), "bench_compare needs a GPU"
    dev = torch.device("cuda", 0)
    ctx = V.Context(0)
    rng = np.random.default_rng(42)
    cases = [("c1", "fastlanes.bitpacked u32 W=7",
              E.encode_bitpacked(rng.integers(0, 128, args.values, dtype=np.uint32), bit_width=7, allow_patches=False), 24),
             ("c5_i64", "chunked fastlanes.for(bitpacked) i64 (l_partkey)", c5_column("l_partkey", args.rows, 64 * 1024),
              100_000),
             ("c5_f64", "chunked alp(for(bitpacked)) f64 (l_extendedprice)",
              c5_column("l_extendedprice", args.rows, 64 * 1024), 50_000.0)]
    results = []
    for name, enc, tree, scalar in cases:
        keep: list = []
        dtree = tree.to(dev)
        node = A.flatten(dtree, keep)
        n, w = tree.len, A.ptype_width(tree.ptype)
        nb = ((n + 63) // 64) * 8
        bits = torch.empty(max(nb, 8), dtype=torch.uint8, device=dev)
        vals = torch.empty(max(n * w, 16), dtype=torch.uint8, device=dev)
        cmp_out, can_out = _lib.VxgCanonical(), _lib.VxgCanonical()
        cmp_out.values, can_out.values = bits.data_ptr(), vals.data_ptr()
        sc = (C.c_uint8 * 8)(*np.array([scalar]).astype(A.NP_OF_PTYPE[tree.ptype]).tobytes().ljust(8, b"\0"))
        info = _lib.VxgCompareInfo()

        def compare():
            _lib.check(ctx.lib.vxg_compare_scalar(ctx.handle, C.byref(node), _lib.CMP_OP["<"], sc, 0, C.byref(cmp_out),
                                                  C.byref(info), ctx.stream_ptr()))

        def canonicalize():
            _lib.check(ctx.lib.vxg_canonicalize(ctx.handle, C.byref(node), C.byref(can_out), ctx.stream_ptr()))

        for _ in range(3):  # warm-up: code objects, the stream-ordered pool
            compare()
            canonicalize()
        ctx.sync()
        # the two must agree before their times mean anything
        host = vals.cpu().numpy()[: n * w].view(A.NP_OF_PTYPE[tree.ptype])
        with np.errstate(invalid="ignore"):
            want = np.packbits(host < np.array([scalar]).astype(host.dtype)[0], bitorder="little")
        got = bits.cpu().numpy()[: want.size]
        assert (got == want).all(), f"{name}: compare disagrees with canonicalize"
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
        row = {"case": name, "encoding": enc, "values": n, "true_rows": int(np.unpackbits(want, bitorder="little").sum()),
               "rounds": args.rounds, "calls_per_round": args.calls, "info": {f: int(getattr(info, f)) for f, _ in info._fields_}}
        for key, out_bytes in (("compare", nb), ("canonicalize", n * w)):
            med = statistics.median(times[key])
            row[key] = {"ms_median": round(med, 5), "ms_min": round(min(times[key]), 5), "ms_max": round(max(times[key]), 5),
                        "bytes": read + out_bytes, "hbm_frac": round((read + out_bytes) / (med * 1e-3) / HBM_BPS, 4)}
        row["speedup"] = round(row["canonicalize"]["ms_median"] / row["compare"]["ms_median"], 3)
        results.append(row)
        print(json.dumps(row), flush=True)
        del dtree, bits, vals, keep
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps({"device": torch.cuda.get_device_name(0), "results": results}, indent=1) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
