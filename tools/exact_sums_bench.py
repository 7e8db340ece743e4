"""Cost of exact float64 sums (fdb_plan_set_exact_sums) against the ordinary plan on the same resident records.

One JSON line: per configuration and mode (plain / exact), ms per step (push of every resident record + Finish, host clock around
work that ends in a device synchronise), scan-kernel ms (hipEvent pairs of fdb_plan_set_timing) and Finish ms (from the end of the
scan to the finished record). Both modes run alternately, step by step, in the same process, so they see the same machine state.

  python tools/exact_sums_bench.py --config 5 --rows 100000000          # cfg 5: 32 label columns, 10 M groups
  python tools/exact_sums_bench.py --config 2 --rows 100000000          # cfg 2: code=='200' + SUM(value) BY labels.path
  FDB_NO_JIT=1 python tools/exact_sums_bench.py --config 5 ...          # the ahead-of-time scan_hash_kernel

Needs a GPU; there is no fallback."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=int, choices=(2, 5), default=5)
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--chunk-rows", type=int, default=25_000_000)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--modes", default="plain,exact")
    args = ap.parse_args()

    from frostdb_amd import physicalplan as pp
    from frostdb_amd import synth
    from frostdb_amd.logicalplan import Col, DynCol, Sum

    if pp.device_count() < 1:
        raise SystemExit("no HIP device visible")
    if args.config == 5:
        filt, aggs, groups = None, [Sum(Col("value"))], [DynCol("labels")]
    else:
        filt, aggs, groups = Col("labels.code") == "200", [Sum(Col("value"))], [Col("labels.path")]
    rbs = []
    for i, off in enumerate(range(0, args.rows, args.chunk_rows)):
        n = min(args.chunk_rows, args.rows - off)
        rec = synth.cfg5_chunk(0, i, n) if args.config == 5 else synth.prometheus_chunk(0, i, n, row_base=off)
        rbs.append(pp.ResidentBatch(rec))
        del rec
    modes = args.modes.split(",")
    res = {m: {"step_ms": [], "scan_kernel_ms": [], "finish_ms": [], "groups": 0, "kernel": ""} for m in modes}
    for step in range(args.warmup + args.steps):
        for m in modes:
            plan = pp.HashAggregatePlan(filt, aggs, groups)
            if m == "exact":
                plan.set_exact_sums(True)
            plan.set_timing(True)
            t0 = time.perf_counter()
            plan.CallbackResident(rbs)
            n_groups = plan.num_groups()  # waits for the scan
            t1 = time.perf_counter()
            out = plan.Finish()
            t2 = time.perf_counter()
            st = plan.stats()
            res[m]["kernel"] = plan.last_kernel()
            plan.Close()
            if step >= args.warmup:
                res[m]["step_ms"].append((t2 - t0) * 1e3)
                res[m]["scan_kernel_ms"].append(st["kernel_ms"])
                res[m]["finish_ms"].append((t2 - t1) * 1e3)
                res[m]["groups"] = int(n_groups)
                res[m]["rows_out"] = out.num_rows
            del out
    for b in rbs:
        b.close()
    line = {"tool": "exact_sums_bench", "config": args.config, "rows": args.rows, "steps": args.steps, "no_jit": bool(os.environ.get("FDB_NO_JIT"))}
    for m in modes:
        r = res[m]
        line[m] = {"ms_per_step": statistics.median(r["step_ms"]), "scan_kernel_ms": statistics.median(r["scan_kernel_ms"]),
                   "finish_ms": statistics.median(r["finish_ms"]), "step_ms_all": [round(x, 2) for x in r["step_ms"]],
                   "groups": r["groups"], "kernel": r["kernel"]}
    if "plain" in line and "exact" in line:
        line["exact_over_plain_scan"] = line["exact"]["scan_kernel_ms"] / max(line["plain"]["scan_kernel_ms"], 1e-9)
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
