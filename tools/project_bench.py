"""Measurement aid: the Projection operator's generated kernel (fdb_project_kernel) over resident records, against the plain copy rate of
the same box in the same run.

  python tools/project_bench.py [--rows 100000000] [--records 4] [--avg-rows 10000000] [--copy-probe tools/copy_probe]

* `value * timestamp` alone over --rows resident rows in --records records (one launch): 16 B read + 8 B written per row.
* the AVG projection `sum(value) / convert(count(value), float64) as avg(value)` over a record shaped like cfg 5's resident Finish
  (--avg-rows groups: a float64 sum and an int64 count column): 16 B read + 8 B written per row, one division per row.
Kernel time is the plan's own hipEvent pair around the launch (set_timing), median of 7 after two warm-up calls. The ceiling is
tools/copy_probe's best `2 read : 1 written` line (build it with hipcc first); without the probe only the rates are printed.
One JSON line per measurement on stdout."""
import argparse
import json
import os
import re
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import pyarrow as pa  # noqa: E402
import torch  # noqa: E402,F401  (one ROCm stack per process: before the library)

from frostdb_amd import physicalplan as pp  # noqa: E402
from frostdb_amd.logicalplan import Col, Convert  # noqa: E402


def measure(plan, records, passes=7, warmup=2):
    plan.set_timing(True)
    ms = []
    for k in range(warmup + passes):
        before = plan.stats()["kernel_ms"]
        outs = plan.ProjectResidentMany(records)
        after = plan.stats()["kernel_ms"]
        for o in outs:
            o.close()
        if k >= warmup:
            ms.append(after - before)
    ms.sort()
    return ms[len(ms) // 2], ms[0], ms[-1]


def copy_ceiling(path):
    """Best and worst GB/s among copy_probe's non-temporal `2 read : 1 written` lines (the spread across its grid sizes), or None."""
    if not path or not os.path.exists(path):
        return None
    out = subprocess.run([path], check=True, capture_output=True, text=True, timeout=120).stdout
    rates = [float(m.group(1)) for ln in out.splitlines() if "(2 read : 1 written)" in ln and "nt=1" in ln for m in [re.search(r"([0-9.]+) GB/s", ln)] if m]
    return (max(rates), min(rates)) if rates else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--records", type=int, default=4)
    ap.add_argument("--avg-rows", type=int, default=10_000_000)
    ap.add_argument("--copy-probe", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "copy_probe"))
    args = ap.parse_args()
    ceiling = copy_ceiling(args.copy_probe)
    rng = np.random.default_rng(1)

    def report(name, rows, med, lo, hi):
        gbs = rows * 24 / med / 1e6
        line = {"what": name, "rows": rows, "kernel_ms_median": round(med, 4), "kernel_ms_min": round(lo, 4), "kernel_ms_max": round(hi, 4), "gb_per_s": round(gbs, 1),
                "bytes_per_row": 24}
        if ceiling:
            line.update({"copy_probe_gb_per_s": ceiling[0], "copy_probe_worst_grid_gb_per_s": ceiling[1], "fraction_of_copy": round(gbs / ceiling[0], 3)})
        print(json.dumps(line), flush=True)

    per = args.rows // args.records
    recs = [pp.ResidentBatch(pa.RecordBatch.from_arrays([pa.array(rng.integers(-10**6, 10**6, per, dtype=np.int64)), pa.array(rng.integers(0, 10**9, per, dtype=np.int64))],
                                                        names=["value", "timestamp"])) for _ in range(args.records)]
    plan = pp.Projection([Col("value") * Col("timestamp")])
    report("value * timestamp", per * args.records, *measure(plan, recs))
    plan.Close()
    for r in recs:
        r.close()

    n = args.avg_rows
    fin = pp.ResidentBatch(pa.RecordBatch.from_arrays([pa.array(rng.standard_normal(n) * 1e4), pa.array(rng.integers(1, 40, n, dtype=np.int64))], names=["sum(value)", "count(value)"]))
    plan = pp.Projection([(Col("sum(value)") / Convert(Col("count(value)"), "float64")).Alias("avg(value)")])
    report("avg(value) over a cfg 5-shaped Finish", n, *measure(plan, [fin]))
    plan.Close()
    fin.close()


if __name__ == "__main__":
    main()
