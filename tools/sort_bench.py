#!/usr/bin/env python3
"""Device Sort of a resident record against its yardstick (MI355X).

For each shape a record of --rows rows (default 100 M) is made resident and fdb_sort_bench times, with HIP events on the call's stream,
  sort_ms        what fdb_batch_sort_indices runs on the device before its copy-out: one key kernel + one radix pass per key word
  bare_sort_ms   bare fdb_sort_pairs_u64 calls with the same pass count and bit widths, in the same process: the yardstick
each the median of 7 calls after 2 warm-up calls. The key kernels' share is the difference. Shapes:
  int64          one int64 key                                           (1 pass of 64 bits)
  dict1000       one dictionary key of 1 000 values                      (1 pass of 10 bits)
  three_columns  a nullable int64, a float64, a nullable dictionary      (4 passes: 1, 64, 64 and 4 bits)
One JSON line per shape on stdout, appended to --out (profiles/sort_bench.jsonl) when given.

    python tools/sort_bench.py [--rows N] [--out FILE]
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


def dictionary(rng, n, entries, mask=None):
    idx = pa.array(rng.integers(0, len(entries), n, dtype=np.uint32), mask=mask)
    return pa.DictionaryArray.from_arrays(idx, pa.array(entries, type=pa.binary()))


def shapes(rng, n):
    yield "int64", {"k": pa.array(rng.integers(np.iinfo(np.int64).min, np.iinfo(np.int64).max, n, dtype=np.int64))}, [("k",)]
    yield "dict1000", {"k": dictionary(rng, n, [b"value-%04d" % ((k * 389) % 1000) for k in range(1000)])}, [("k",)]
    mask = rng.random(n) < 0.2
    yield "three_columns", {"i": pa.array(rng.integers(-1000, 1000, n, dtype=np.int64), mask=mask), "f": pa.array(rng.standard_normal(n)),
                            "d": dictionary(rng, n, [b"w%d" % k for k in range(7)], mask=rng.random(n) < 0.2)}, [("i",), ("f", True), ("d", False, True)]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    rng = np.random.default_rng(1)
    for name, cols, columns in shapes(rng, args.rows):
        rec = pa.RecordBatch.from_arrays(list(cols.values()), names=list(cols.keys()))
        rb = pp.ResidentBatch(rec)
        del rec, cols
        try:
            r = rb.sort_bench(columns, reps=args.reps, warmup=args.warmup)
        finally:
            rb.close()
        line = {"tool": "sort_bench", "shape": name, "rows": args.rows, "passes": r["passes"], "sort_ms": round(r["sort_ms"], 3),
                "bare_sort_ms": round(r["bare_sort_ms"], 3), "key_kernels_ms": round(r["sort_ms"] - r["bare_sort_ms"], 3),
                "rows_per_s": round(args.rows / (r["sort_ms"] * 1e-3)), "reps": args.reps, "warmup": args.warmup, "date": time.strftime("%Y-%m-%d")}
        text = json.dumps(line)
        print(text, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(text + "\n")
    assert pp.live_allocations()["device_blocks"] == 0


if __name__ == "__main__":
    main()
