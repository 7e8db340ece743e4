#!/usr/bin/env python3
"""Device MergeRecords of K ordered resident records against the device Sort of the same rows (MI355X).

For each key shape and each K in --ks (default 2, 8, 32), --rows rows in total (default 100 M) are made resident as K ordered records
of rows / K rows each, and once more as ONE record holding the same rows (the concatenation). fdb_merge_bench times, with HIP events on
the call's stream, medians of 7 calls after 2 warm-up calls,
  merge_ms    keys + order check (its host round trip included) + the ceil(log2 K) rounds
  round_ms    every round alone; round_gbs = rows x (8 W + 4) bytes read and written / that time
  gather_ms   the gather of the result's columns out of the K inputs
and fdb_sort_bench, in the same process, sort_ms of the one record (tools/sort_bench.py's figure). Both are taken twice (two medians of
7): the second figures are merge_ms_again / sort_ms_again, their distance is the run-to-run spread the comparison has to clear. Shapes:
  int64       one int64 key                          (W = 1)
  dict1000    one dictionary key of 1 000 values     (W = 1, 10 bits)
  two_words   two int64 keys                         (W = 2)
One JSON line per (shape, K) on stdout, appended to --out (profiles/merge_bench.jsonl) when given.

    python tools/merge_bench.py [--rows N] [--ks 2,8,32] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import pyarrow as pa  # noqa: E402

from frostdb_amd import physicalplan as pp  # noqa: E402

ENTRIES = [b"value-%04d" % ((k * 389) % 1000) for k in range(1000)]
ENTRY_OF_RANK = np.argsort(np.array([(k * 389) % 1000 for k in range(1000)])).astype(np.uint32)  # the entry that holds the r-th smallest value


def ordered_piece(shape, rng, m):
    """The columns of one ordered record of m rows (built ordered: nothing is sorted on the host)."""
    if shape == "int64":
        return {"k": pa.array(np.cumsum(rng.integers(0, 2000, m, dtype=np.int64)))}
    if shape == "dict1000":
        ranks = (np.arange(m, dtype=np.int64) * 1000 // max(m, 1)).astype(np.int64)
        return {"k": pa.DictionaryArray.from_arrays(pa.array(ENTRY_OF_RANK[ranks]), pa.array(ENTRIES, type=pa.binary()))}
    assert shape == "two_words"
    return {"a": pa.array(np.arange(m, dtype=np.int64) * 16 // max(m, 1)), "b": pa.array(np.cumsum(rng.integers(0, 2000, m, dtype=np.int64)))}


COLUMNS = {"int64": [("k",)], "dict1000": [("k",)], "two_words": [("a",), ("b",)]}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--ks", default="2,8,32")
    ap.add_argument("--shapes", default="int64,dict1000,two_words")
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    rng = np.random.default_rng(1)
    for shape in args.shapes.split(","):
        columns = COLUMNS[shape]
        for k in [int(x) for x in args.ks.split(",")]:
            m = args.rows // k
            pieces = [ordered_piece(shape, rng, m) for _ in range(k)]
            names = list(pieces[0].keys())
            rbs = [pp.ResidentBatch(pa.RecordBatch.from_arrays(list(p.values()), names=names)) for p in pieces]
            whole = pp.ResidentBatch(pa.RecordBatch.from_arrays([pa.concat_arrays([p[n] for p in pieces]) for n in names], names=names))
            del pieces
            try:
                r = pp.ResidentBatch.merge_bench(rbs, columns, reps=args.reps, warmup=args.warmup)
                s = whole.sort_bench(columns, reps=args.reps, warmup=args.warmup)
                r2 = pp.ResidentBatch.merge_bench(rbs, columns, reps=args.reps, warmup=args.warmup)
                s2 = whole.sort_bench(columns, reps=args.reps, warmup=args.warmup)
            finally:
                for rb in rbs + [whole]:
                    rb.close()
            rows = m * k
            moved = rows * (8 * r["words"] + 4) * 2  # every round reads and writes every (key, position) pair once
            line = {"tool": "merge_bench", "shape": shape, "k": k, "rows": rows, "words": r["words"], "rounds": len(r["round_ms"]),
                    "merge_ms": round(r["merge_ms"], 3), "merge_ms_again": round(r2["merge_ms"], 3), "gather_ms": round(r["gather_ms"], 3),
                    "round_ms": [round(x, 3) for x in r["round_ms"]], "round_gbs": [round(moved / (x * 1e-3) / 1e9) for x in r["round_ms"]],
                    "sort_ms": round(s["sort_ms"], 3), "sort_ms_again": round(s2["sort_ms"], 3), "sort_passes": s["passes"],
                    "merge_over_sort": round(r["merge_ms"] / s["sort_ms"], 3), "reps": args.reps, "warmup": args.warmup, "date": time.strftime("%Y-%m-%d")}
            text = json.dumps(line)
            print(text, flush=True)
            if args.out:
                with open(args.out, "a") as f:
                    f.write(text + "\n")
    assert pp.live_allocations()["device_blocks"] == 0


if __name__ == "__main__":
    main()
