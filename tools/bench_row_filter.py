"""A scan's row filter: a range as one two-sided compare against two one-sided compares.

Times `vxg_row_filter` with VXG_ROWF_FUSE_RANGES and with VXG_ROWF_NO_FUSE_RANGES (mask + true
count), and the same conjuncts issued as separate `vxg_compare_scalar` calls with null_as_false
(what a caller could do before vxg_row_filter; their masks are NOT combined), with device events,
after a warm-up, the three variants alternating in one process (round r: K calls of each), and
reports the median, minimum and maximum ms per call over the rounds:
  range     l_shipdate >= 1994-01-01 AND l_shipdate < 1995-01-01 on a BASELINE C5-shaped column:
            92 chunks of 64 Ki rows, FoR(BitPacked) i32
  q6        TPC-H Q6's filter: that range AND l_discount >= 0.05 AND l_discount <= 0.07
            (ALP(FoR(BitPacked)) f64) AND l_quantity < 24 (ALP(FoR(BitPacked)) f64)
(tools/lineitem.py's value domains and cascades; only these columns are generated).  bytes/s is the
packed bytes of the columns, read once, over the median time.  The masks of the two flags must be
identical and the count must be numpy's before their times mean anything.  Usage:
  python tools/bench_row_filter.py [--rounds 20] [--calls 5] [--rows N] [--out FILE]
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
STARTDATE = 8035  # 1992-01-01, tools/lineitem.py


def c5_columns(rows: int, chunk_rows: int):
    """l_shipdate, l_discount and l_quantity as bench-vortex writes them: 64 Ki-row chunks, each
    compressed alone -> ({name: ChunkedArray}, {name: plain values})."""
    import vortex_amd.arrays as A
    import vortex_amd.encode as E
    enc = {"l_shipdate": [], "l_discount": [], "l_quantity": []}
    plain = {k: [] for k in enc}
    for c in range((rows + chunk_rows - 1) // chunk_rows):
        rng = np.random.default_rng([7, c])
        n = min(chunk_rows, rows - c * chunk_rows)
        ship = (STARTDATE + rng.integers(0, 2406, n) + rng.integers(1, 122, n)).astype(np.int32)
        disc = rng.integers(0, 11, n) / 100.0
        qty = rng.integers(1, 51, n).astype(np.float64)
        for name, v, tree in (("l_shipdate", ship, E.encode_for_bitpacked(ship)), ("l_discount", disc, E.encode_alp(disc)),
                              ("l_quantity", qty, E.encode_alp(qty))):
            enc[name].append(tree)
            plain[name].append(v)
    return {k: A.chunked(v) for k, v in enc.items()}, {k: np.concatenate(v) for k, v in plain.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--calls", type=int, default=5, help="back-to-back calls between two events")
    ap.add_argument("--rows", type=int, default=6_001_215, help="rows of the C5 columns")
    ap.add_argument("--out", type=str, default="")
    args = ap.parse_args()
    import torch
    import vortex_amd as V
    import vortex_amd.arrays as A
    from vortex_amd import _lib

    assert torch.cuda.is_available(), "bench_row_filter needs a GPU"
    dev = torch.device("cuda", 0)
    ctx = V.Context(0)
    trees, plain = c5_columns(args.rows, 64 * 1024)
    keep: list = []
    dtrees = {k: t.to(dev) for k, t in trees.items()}
    nodes = {k: A.flatten(t, keep) for k, t in dtrees.items()}
    n = args.rows
    nb = ((n + 63) // 64) * 8
    d0, d1 = 8766, 9131  # 1994-01-01, 1995-01-01
    rng_preds = [("l_shipdate", ">=", d0), ("l_shipdate", "<", d1)]
    shapes = [("range", rng_preds),
              ("q6", rng_preds + [("l_discount", ">=", 0.05), ("l_discount", "<=", 0.07), ("l_quantity", "<", 24.0)])]
    results = []
    for name, preds in shapes:
        arr = (_lib.VxgPredicate * len(preds))()
        scalars = []
        for i, (col, op, s) in enumerate(preds):
            sc = (C.c_uint8 * 8)(*np.array([s]).astype(A.NP_OF_PTYPE[trees[col].ptype]).tobytes().ljust(8, b"\0"))
            scalars.append(sc)
            arr[i].column = C.pointer(nodes[col])
            arr[i].op = _lib.CMP_OP[op]
            arr[i].scalar_host = C.cast(sc, C.c_void_p)
        masks = {f: torch.empty(max(nb, 8), dtype=torch.uint8, device=dev) for f in ("fuse", "no_fuse")}
        counts = {f: torch.zeros(1, dtype=torch.int64, device=dev) for f in masks}
        singles = [torch.empty(max(nb, 8), dtype=torch.uint8, device=dev) for _ in preds]
        infos = {f: _lib.VxgRowFilterInfo() for f in masks}

        def row_filter(key):
            out = _lib.VxgCanonical()
            out.values = masks[key].data_ptr()
            flag = _lib.ROWF_FUSE_RANGES if key == "fuse" else _lib.ROWF_NO_FUSE_RANGES
            _lib.check(ctx.lib.vxg_row_filter(ctx.handle, arr, len(preds), flag, C.byref(out),
                                              C.c_void_p(counts[key].data_ptr()), C.byref(infos[key]), ctx.stream_ptr()))

        def separate():
            for i, (col, op, _) in enumerate(preds):
                out = _lib.VxgCanonical()
                out.values = singles[i].data_ptr()
                _lib.check(ctx.lib.vxg_compare_scalar(ctx.handle, C.byref(nodes[col]), _lib.CMP_OP[op], scalars[i],
                                                      _lib.CMP_NULL_AS_FALSE, C.byref(out), None, ctx.stream_ptr()))

        variants = (("fuse", lambda: row_filter("fuse")), ("no_fuse", lambda: row_filter("no_fuse")),
                    ("separate_compares", separate))
        for _ in range(3):  # warm-up: code objects, the stream-ordered pool
            for _, fn in variants:
                fn()
        ctx.sync()
        ops = {">=": np.greater_equal, "<=": np.less_equal, "<": np.less, ">": np.greater}
        want = np.ones(n, bool)
        for col, op, s in preds:
            want &= ops[op](plain[col], s)
        got = {f: masks[f].cpu().numpy()[:nb] for f in masks}
        assert (got["fuse"] == got["no_fuse"]).all(), f"{name}: the two flags disagree"
        assert (np.unpackbits(got["fuse"], bitorder="little")[:n].astype(bool) == want).all(), f"{name}: wrong mask"
        assert int(counts["fuse"].item()) == int(counts["no_fuse"].item()) == int(want.sum()), f"{name}: wrong count"
        times = {k: [] for k, _ in variants}
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(args.rounds):
            for key, fn in variants:
                e0.record()
                for _k in range(args.calls):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                times[key].append(e0.elapsed_time(e1) / args.calls)
        read = sum(trees[c].nbytes() for c in {c for c, _, _ in preds})
        row = {"case": name, "conjuncts": [f"{c} {op} {s}" for c, op, s in preds], "rows": n, "true_rows": int(want.sum()),
               "rounds": args.rounds, "calls_per_round": args.calls, "packed_bytes_read_once": read,
               "info": {f: {k: int(getattr(infos[f], k)) for k, _ in infos[f]._fields_ if k != "reserved"} for f in infos}}
        for key, _ in variants:
            med = statistics.median(times[key])
            row[key] = {"ms_median": round(med, 5), "ms_min": round(min(times[key]), 5), "ms_max": round(max(times[key]), 5),
                        "bytes_per_s": round(read / (med * 1e-3)), "hbm_frac": round(read / (med * 1e-3) / HBM_BPS, 4)}
        row["fuse_over_no_fuse"] = round(row["fuse"]["ms_median"] / row["no_fuse"]["ms_median"], 4)
        results.append(row)
        print(json.dumps(row), flush=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps({"device": torch.cuda.get_device_name(0), "results": results}, indent=1) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
