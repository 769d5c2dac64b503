"""filter(batch, mask) of a scan: one vxg_filter_batch against one vxg_filter_array per column.

Times three ways of filtering the ten numeric packed columns of a BASELINE C5-shaped lineitem batch
(92 chunks of 64 Ki rows; tools/lineitem.py's value domains and cascades: six FoR(BitPacked) i64 /
i32 columns and four ALP(FoR(BitPacked)) f64 columns) by one device mask:
  batch        vxg_filter_batch, flags 0: the mask counted once, the columns in the packed domain
  batch_canon  vxg_filter_batch with VXG_FILTB_CANONICALIZE: the mask counted once, every column
               canonicalized into a temporary and compacted
  per_column   one vxg_filter_array per column over a Bool array wrapped around the mask: what a
               caller did before vxg_filter_batch (a count, a scan and a wait per column)
under three masks: TPC-H Q6's filter evaluated by vxg_row_filter, a random mask at one half, and
an all-true mask.  Device events, a warm-up, the variants alternating in one process (round r: K
calls of each); median, minimum and maximum ms per call over the rounds.  The outputs of the three
variants must be identical before their times mean anything.  `not_slower`: batch's median is at
most per_column's plus the spread (the largest max - min of the variants).  bytes_moved is the
HBM traffic each variant needs by construction (packed bytes read once; a canonicalizing variant
also writes and re-reads width bytes per row; every variant reads the mask per column and writes
the selected rows).  Usage:
  python tools/bench_filter_batch.py [--rounds 10] [--calls 3] [--rows N] [--out FILE]
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

STARTDATE = 8035  # 1992-01-01, tools/lineitem.py
NUMERIC = ["l_partkey", "l_suppkey", "l_linenumber", "l_quantity", "l_extendedprice", "l_discount", "l_tax",
           "l_shipdate", "l_commitdate", "l_receiptdate"]


def numeric_chunk(c: int, rows: int, chunk_rows: int) -> dict:
    """The ten columns of chunk c in tools/lineitem.py's value domains (its string columns and the
    RunEnd l_orderkey are not generated)."""
    rng = np.random.default_rng([7, c])
    n = min(chunk_rows, rows - c * chunk_rows)
    runs = rng.integers(1, 8, n)
    starts = np.cumsum(runs) - runs
    runs = runs[starts < n]
    order_of_row = np.repeat(np.arange(runs.size), runs)[:n]
    linenumber = (np.arange(n) - np.repeat(np.cumsum(runs) - runs, runs)[:n]) + 1
    od = (STARTDATE + rng.integers(0, 2406, runs.size))[order_of_row]
    ship = od + rng.integers(1, 122, n)
    qty = rng.integers(1, 51, n)
    partkey = rng.integers(1, 200_001, n)
    retail = (90_000 + (partkey // 10) % 20_001 + 100 * (partkey % 1_000)) / 100.0
    return {"l_partkey": partkey.astype(np.int64), "l_suppkey": rng.integers(1, 10_001, n).astype(np.int64),
            "l_linenumber": linenumber.astype(np.int64), "l_quantity": qty.astype(np.float64),
            "l_extendedprice": np.round(qty * retail, 2), "l_discount": rng.integers(0, 11, n) / 100.0,
            "l_tax": rng.integers(0, 9, n) / 100.0, "l_shipdate": ship.astype(np.int32),
            "l_commitdate": (od + rng.integers(30, 91, n)).astype(np.int32),
            "l_receiptdate": (ship + rng.integers(1, 31, n)).astype(np.int32)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--calls", type=int, default=3, help="back-to-back calls between two events")
    ap.add_argument("--rows", type=int, default=6_001_215, help="rows of the C5 batch")
    ap.add_argument("--out", type=str, default="")
    args = ap.parse_args()
    import torch
    import vortex_amd as V
    import vortex_amd.arrays as A
    from lineitem import encode_column
    from vortex_amd import _lib

    assert torch.cuda.is_available(), "bench_filter_batch needs a GPU"
    dev = torch.device("cuda", 0)
    ctx = V.Context(0)
    n, chunk_rows = args.rows, 64 * 1024
    enc = {name: [] for name in NUMERIC}
    for c in range((n + chunk_rows - 1) // chunk_rows):
        for name, v in numeric_chunk(c, n, chunk_rows).items():
            enc[name].append(encode_column(name, v))
    trees = {name: A.chunked(chunks) for name, chunks in enc.items()}
    keep: list = []
    dtrees = {k: t.to(dev) for k, t in trees.items()}
    nodes = [A.flatten(dtrees[k], keep) for k in NUMERIC]
    widths = [A.ptype_width(trees[k].ptype) for k in NUMERIC]
    cols = (C.POINTER(_lib.VxgArray) * len(nodes))(*[C.pointer(nd) for nd in nodes])
    nb = ((n + 63) // 64) * 8

    # the masks
    d0, d1 = 8766, 9131  # 1994-01-01, 1995-01-01
    q6 = V.row_filter([(dtrees["l_shipdate"], ">=", d0), (dtrees["l_shipdate"], "<", d1), (dtrees["l_discount"], ">=", 0.05),
                       (dtrees["l_discount"], "<=", 0.07), (dtrees["l_quantity"], "<", 24.0)], ctx)
    rng = np.random.default_rng(11)
    half = np.zeros(nb * 8, bool)
    half[:n] = rng.random(n) < 0.5
    ones = np.zeros(nb * 8, bool)
    ones[:n] = True
    masks = [("q6", q6.values), ("half", torch.from_numpy(np.packbits(half, bitorder="little")).to(dev)),
             ("all_true", torch.from_numpy(np.packbits(ones, bitorder="little")).to(dev))]

    variants = ("batch", "batch_canon", "per_column")
    outs = {v: [torch.empty(max(n * w, 16), dtype=torch.uint8, device=dev) for w in widths] for v in variants}
    packed_bytes = sum(trees[k].nbytes() for k in NUMERIC)
    results = []
    for mname, mt in masks:
        pred = A.Array(A.ENC["BOOL"], n, A.DTYPE["BOOL"], "u8", False, A.VALIDITY["NON_NULLABLE"],
                       {"first_byte_bit_offset": 0}, [mt])
        pnode = A.flatten(pred, keep)
        infos = {v: _lib.VxgFilterBatchInfo() for v in variants[:2]}
        ks = {}

        def batch(key, flags):
            o = (_lib.VxgCanonical * len(nodes))()
            for i, buf in enumerate(outs[key]):
                o[i].values = buf.data_ptr()
            k = C.c_uint64()
            _lib.check(ctx.lib.vxg_filter_batch(ctx.handle, cols, len(nodes), C.c_void_p(mt.data_ptr()), n, flags, o,
                                                C.byref(k), C.byref(infos[key]), ctx.stream_ptr()))
            ks[key] = int(k.value)

        def per_column():
            for i, buf in enumerate(outs["per_column"]):
                o = _lib.VxgCanonical()
                o.values = buf.data_ptr()
                _lib.check(ctx.lib.vxg_filter_array(ctx.handle, C.byref(nodes[i]), C.byref(pnode), C.byref(o),
                                                    ctx.stream_ptr()))
                ks["per_column"] = int(o.len)

        fns = (("batch", lambda: batch("batch", 0)), ("batch_canon", lambda: batch("batch_canon", _lib.FILTB_CANONICALIZE)),
               ("per_column", per_column))
        for _ in range(2):  # warm-up: code objects, the stream-ordered pool
            for _, fn in fns:
                fn()
        ctx.sync()
        k = ks["batch"]
        assert ks["batch_canon"] == k and ks["per_column"] == k, f"{mname}: the variants count differently"
        for i, w in enumerate(widths):  # identical outputs before the times count
            ref = outs["per_column"][i][: k * w]
            for v in variants[:2]:
                assert torch.equal(outs[v][i][: k * w], ref), f"{mname}: {v} differs from per_column in {NUMERIC[i]}"
        times = {key: [] for key, _ in fns}
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(args.rounds):
            for key, fn in fns:
                e0.record()
                for _k in range(args.calls):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                times[key].append(e0.elapsed_time(e1) / args.calls)
        selected = sum(k * w for w in widths)
        canon = sum(n * w for w in widths)
        moved = {"batch": packed_bytes + len(widths) * nb + selected,
                 "batch_canon": packed_bytes + 2 * canon + len(widths) * nb + selected,
                 "per_column": packed_bytes + 2 * canon + 4 * len(widths) * nb + selected}
        row = {"mask": mname, "rows": n, "true_rows": k, "columns": len(widths), "rounds": args.rounds,
               "calls_per_round": args.calls, "packed_bytes": packed_bytes, "bytes_moved": moved,
               "info": {v: {f: int(getattr(infos[v], f)) for f, _ in infos[v]._fields_} for v in infos}}
        for key, _ in fns:
            t = times[key]
            row[key] = {"ms_median": round(statistics.median(t), 5), "ms_min": round(min(t), 5), "ms_max": round(max(t), 5)}
        row["batch_over_per_column"] = round(row["batch"]["ms_median"] / row["per_column"]["ms_median"], 4)
        row["batch_over_batch_canon"] = round(row["batch"]["ms_median"] / row["batch_canon"]["ms_median"], 4)
        row["spread_ms"] = round(max(row[key]["ms_max"] - row[key]["ms_min"] for key, _ in fns), 5)
        row["not_slower"] = bool(row["batch"]["ms_median"] <= row["per_column"]["ms_median"] + row["spread_ms"])
        results.append(row)
        print(json.dumps(row), flush=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps({"device": torch.cuda.get_device_name(0), "results": results}, indent=1) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
