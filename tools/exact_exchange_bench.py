"""Cost of exact float64 sums (fdb_plan_set_exact_sums) in the cross-GPU exchange (fdb_plan_exchange) against the ordinary plan.

N in-process ranks on ONE GPU (fdb_comm_init_local: the peer-to-peer transport, every rank a thread), a cfg 5-shaped query (32 label
columns, ~10 M groups, SUM(value)); the rows are cut into 8 chunks once and rank r of N scans chunks r, r + N, …. Per N and mode
(plain / exact), alternating step by step: bytes per packed row and the host milliseconds of the exchange's phases — export (re-key +
partition, limb payloads included), all-to-all, import (the owner's rank-by-rank merges) — from the library's FDB_PROFILE marks, the
slowest rank per phase, median over steps. `merge_ms` is the wall clock of merge_alltoall from a barrier that all ranks pass together.

  python tools/exact_exchange_bench.py --rows 100000000 --ranks 2,4,8
  python tools/exact_exchange_bench.py --rows 40000000 --groups 4000000   # N ranks' tables share ONE GPU's memory: a smaller cfg 5

Needs a GPU; there is no fallback."""
import argparse
import json
import os
import re
import statistics
import sys
import tempfile
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PHASES = {"exchange: export": "export_ms", "exchange: all-to-all": "alltoall_ms", "exchange: import": "import_ms"}
MARK = re.compile(r"\[fdb\] (exchange: [a-z-]+)\s+([0-9.]+) us")
ROWS = re.compile(r"\[fdb\] exchange rows (\d+) x (\d+) bytes")


def run_threads(n, fn):
    out, errs = [None] * n, []

    def work(r):
        try:
            out[r] = fn(r)
        except BaseException as e:  # noqa: BLE001
            errs.append(e)

    ts = [threading.Thread(target=work, args=(r,)) for r in range(n)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(timeout=600)
    if any(t.is_alive() for t in ts):
        raise SystemExit("a rank is stuck in a collective")
    if errs:
        raise errs[0]
    return out


class StderrCapture:
    """The library's FDB_PROFILE lines (C stderr, fd 2) of one exchange, into a temporary file."""

    def __enter__(self):
        sys.stderr.flush()
        self.f = tempfile.TemporaryFile(mode="w+b")
        self.saved = os.dup(2)
        os.dup2(self.f.fileno(), 2)
        return self

    def __exit__(self, *exc):
        os.dup2(self.saved, 2)
        os.close(self.saved)
        self.f.seek(0)
        self.text = self.f.read().decode(errors="replace")
        self.f.close()


def free_gib() -> float:
    try:
        import torch
        return torch.cuda.mem_get_info(0)[0] / 2**30
    except Exception:  # noqa: BLE001  (a progress note only)
        return float("nan")


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--groups", type=int, default=10_000_000, help="distinct groups over all rows (cfg 5: 10 M)")
    ap.add_argument("--ranks", default="2,4,8")
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--modes", default="plain,exact")
    args = ap.parse_args()

    from frostdb_amd import comm as fcomm
    from frostdb_amd import physicalplan as pp
    from frostdb_amd import synth
    from frostdb_amd.logicalplan import Col, DynCol, Sum

    if pp.device_count() < 1:
        raise SystemExit("no HIP device visible")
    aggs, groups = [Sum(Col("value"))], [DynCol("labels")]
    n_chunks = 8
    rbs = []
    for i in range(n_chunks):
        rec = synth.cfg5_chunk(0, i, args.rows // n_chunks, n_groups=args.groups)
        rbs.append(pp.ResidentBatch(rec))
        del rec
    modes = args.modes.split(",")
    line = {"tool": "exact_exchange_bench", "config": 5, "rows": args.rows, "groups": args.groups, "steps": args.steps, "no_jit": bool(os.environ.get("FDB_NO_JIT"))}
    for world in [int(x) for x in args.ranks.split(",")]:
        comms = fcomm.Comm.init_local([0] * world)
        res = {m: {k: [] for k in list(PHASES.values()) + ["merge_ms"]} for m in modes}
        info = {m: {} for m in modes}
        for step in range(args.warmup + args.steps):
            for m in modes:
                barrier = threading.Barrier(world)

                def rank_fn(r):
                    plan = pp.HashAggregatePlan(None, aggs, groups)
                    if m == "exact":
                        plan.set_exact_sums(True)
                    try:
                        try:
                            plan.CallbackResident([rbs[c] for c in range(r, n_chunks, world)])
                            plan.num_groups()  # waits for the scan
                        except BaseException:
                            barrier.abort()  # (the other ranks leave instead of waiting for this one)
                            raise
                        barrier.wait(timeout=300)
                        t0 = time.perf_counter()
                        shard = comms[r].merge_alltoall(plan)
                        t1 = time.perf_counter()
                        groups_here = shard.num_groups()
                        shard.Close()
                        return (t1 - t0) * 1e3, groups_here
                    finally:
                        plan.Close()

                os.environ["FDB_PROFILE"] = "1"
                try:
                    with StderrCapture() as cap:
                        out = run_threads(world, rank_fn)
                finally:
                    del os.environ["FDB_PROFILE"]
                per = {k: [] for k in PHASES.values()}
                for name, us in MARK.findall(cap.text):
                    if name in PHASES:
                        per[PHASES[name]].append(float(us) / 1e3)
                rows = [(int(a), int(b)) for a, b in ROWS.findall(cap.text)]
                info[m] = {"row_bytes": rows[0][1] if rows else None, "rows_exported": sum(a for a, _ in rows),
                           "groups": sum(g for _, g in out)}
                print("ranks %d step %d %s: merge %.1f ms, %s, device free %.1f GiB" % (world, step, m, max(t for t, _ in out), info[m], free_gib()),
                      file=sys.stderr, flush=True)
                if step >= args.warmup:
                    for k, v in per.items():
                        res[m][k].append(max(v) if v else float("nan"))
                    res[m]["merge_ms"].append(max(t for t, _ in out))
        for c in comms:
            c.close()
        entry = {}
        for m in modes:
            entry[m] = dict(info[m])
            for k, v in res[m].items():
                entry[m][k] = round(statistics.median(v), 3)
            entry[m]["merge_ms_all"] = [round(x, 2) for x in res[m]["merge_ms"]]
        if "plain" in entry and "exact" in entry:
            entry["exact_over_plain"] = {k: round(entry["exact"][k] / max(entry["plain"][k], 1e-9), 2) for k in list(PHASES.values()) + ["merge_ms"]}
        line["ranks_%d" % world] = entry
    for b in rbs:
        b.close()
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
