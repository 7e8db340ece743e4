#!/usr/bin/env python
"""End-to-end number for SURVEY §8(f).3: Parquet row groups (bytes in host memory) → resident batches decoded on the device →
the cfg 2 query, against the same data imported as Arrow records decoded by pyarrow on the host (what the reference's
ParquetConverter does with parquet-go). Prints one JSON line. Run on the GPU box."""
import io, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, pyarrow as pa, pyarrow.parquet as pq
from frostdb_amd import build as fb
fb.build()
from frostdb_amd import physicalplan as pp, synth
from frostdb_amd.logicalplan import Col, Sum
from tests.parquet_util import row_group_chunks, write_parquet

rows, rg_rows = int(sys.argv[1]) if len(sys.argv) > 1 else 20_000_000, 5_000_000
rec = synth.prometheus_chunk(0, 0, rows)
t = pa.Table.from_batches([rec])
t = t.set_column(0, "labels.code", t.column(0).cast(pa.binary())).set_column(1, "labels.path", t.column(1).cast(pa.binary()))
variant = os.environ.get("PQ_VARIANT", "plain")  # "plain": UNCOMPRESSED, PLAIN int64; "delta_snappy": timestamp DELTA_BINARY_PACKED, pages SNAPPY; "numeric_dict", "lz4_raw": below
kw = {}
if variant == "delta_snappy":
    kw = dict(compression="SNAPPY", column_encoding={"timestamp": "DELTA_BINARY_PACKED"}, use_dictionary=["labels.code", "labels.path"])
import torch
def pinned_groups(data):
    """the file's bytes in PINNED host memory (what a host that reads parts for the GPU would read into); chunks are (address, length)"""
    groups = [row_group_chunks(data, g) for g in range(pq.ParquetFile(io.BytesIO(data)).metadata.num_row_groups)]
    pinned = torch.empty(len(data), dtype=torch.uint8, pin_memory=True)
    pinned.numpy()[:] = np.frombuffer(data, dtype=np.uint8)
    def _pin(ch):
        out = []
        for nm, ty, opt, u8, b, cd in ch:
            off = data.find(b[:64]) if len(b) >= 64 else data.find(b)
            if data[off:off + len(b)] != b:  # (a prefix that also occurs earlier, e.g. equal dictionary pages: search for the whole chunk)
                off = data.find(b)
            assert data[off:off + len(b)] == b
            out.append((nm, ty, opt, u8, (pinned.data_ptr() + off, len(b)), cd))
        return out
    return [(_pin(ch), n) for ch, n in groups], pinned

if variant == "numeric_dict":
    # Dictionary-encoded numeric columns against their PLAIN twins: `value` rounded to one decimal (a few thousand distinct values) and
    # an int64 `status` of ≈ 50 values, the same table written twice. One process, the two files decoded alternately (boxes differ by
    # several per cent, so the A/B is inside one call), median of $PQ_PASSES (default 31) passes each; a pass = file bytes → resident
    # batches (one fdb_batches_from_parquet call) → released. One JSON line per file and one with the ratio.
    rng = np.random.default_rng(1)
    status = pa.array((100 + rng.integers(0, 50, rows) * 10).astype(np.int64))
    t = t.set_column(t.schema.get_field_index("value"), "value", pa.array(np.round(t.column("value").to_numpy(), 1))).append_column("status", status)
    passes = int(os.environ.get("PQ_PASSES", "31"))
    files = {"numeric_dict": write_parquet(t, row_group_size=rg_rows, data_page_size=1 << 20, use_dictionary=True),
             "numeric_plain": write_parquet(t, row_group_size=rg_rows, data_page_size=1 << 20)}
    md = pq.ParquetFile(io.BytesIO(files["numeric_dict"])).metadata.row_group(0)
    assert all(md.column(j).has_dictionary_page for j in range(md.num_columns) if md.column(j).path_in_schema in ("value", "status"))
    loaded = {k: pinned_groups(v) for k, v in files.items()}
    def decode(k):
        keep = pp.ResidentBatch.from_parquet_many(loaded[k][0])
        for b in keep: b.close()
    # the two files decode to the same columns
    for g in range(len(loaded["numeric_dict"][0])):
        a, b = (pp.ResidentBatch.from_parquet(*loaded[k][0][g]) for k in ("numeric_dict", "numeric_plain"))
        ta, tb = a.to_arrow(), b.to_arrow()
        for nm in ("value", "status", "timestamp"):
            assert ta.column(nm).equals(tb.column(nm)), nm
        a.close(); b.close()
    times = {k: [] for k in files}
    stats = {k: {"host_ms": 0.0, "device_ms": 0.0} for k in files}
    for k in files: decode(k); decode(k)  # warm-up
    for _ in range(passes):
        for k in files:
            s0 = pp.parquet_stats(); t0 = time.perf_counter(); decode(k); dt = time.perf_counter() - t0; s1 = pp.parquet_stats()
            times[k].append(dt)
            for f in stats[k]: stats[k][f] += s1[f] - s0[f]
    out = {}
    for k in files:
        ts = sorted(times[k]); med = ts[len(ts) // 2]
        out[k] = {"variant": k, "rows": rows, "row_groups": len(loaded[k][0]), "parquet_bytes": len(files[k]), "passes": passes, "median_s_per_pass": med, "min_s": ts[0],
                  "p90_s": ts[int(len(ts) * 0.9)], "rows_per_s": rows / med, "parquet_GB_per_s": len(files[k]) / med / 1e9,
                  "host_ms_per_pass": stats[k]["host_ms"] / passes, "device_ms_per_pass": stats[k]["device_ms"] / passes}
        print(json.dumps(out[k]))
    print(json.dumps({"metric": "decode time, dictionary-encoded numeric file / PLAIN numeric file (medians, alternating passes in one process)",
                      "ratio": out["numeric_dict"]["median_s_per_pass"] / out["numeric_plain"]["median_s_per_pass"],
                      "bytes_ratio": len(files["numeric_dict"]) / len(files["numeric_plain"])}))
    sys.exit(0)

if variant == "lz4_raw":
    # The file with LZ4_RAW pages (codec 7 in the footer: pyarrow's metadata API says "LZ4" for 5 and 7 alike): the PLAIN float64 `value`
    # pages are literals and are inflated on the device, the rest on the host. One process, the default and the all-host path
    # ($FDB_PARQUET_HOST_INFLATE, read per call) decoded alternately, median and 10th / 90th percentile of $PQ_PASSES (default 15) passes
    # each; a pass = file bytes → resident batches (one fdb_batches_from_parquet call) → released. One JSON line per path and one with the ratio.
    from tests.lz4_cases import footer_codecs
    passes = int(os.environ.get("PQ_PASSES", "15"))
    data = write_parquet(t, row_group_size=rg_rows, data_page_size=1 << 20, compression="LZ4_RAW", use_dictionary=["labels.code", "labels.path"])
    assert set(footer_codecs(data)) == {7}
    groups, pinned = pinned_groups(data)
    groups = [([c[:5] + ("LZ4_RAW",) for c in ch], n) for ch, n in groups]
    def decode(host):
        if host: os.environ["FDB_PARQUET_HOST_INFLATE"] = "1"
        else: os.environ.pop("FDB_PARQUET_HOST_INFLATE", None)
        keep = pp.ResidentBatch.from_parquet_many(groups)
        for b in keep: b.close()
    # the two paths decode to the same columns
    tabs = []
    for host in (False, True):
        if host: os.environ["FDB_PARQUET_HOST_INFLATE"] = "1"
        else: os.environ.pop("FDB_PARQUET_HOST_INFLATE", None)
        keep = pp.ResidentBatch.from_parquet_many(groups); tabs.append([b.to_arrow() for b in keep])
        for b in keep: b.close()
    assert all(x.equals(y) for x, y in zip(*tabs)); del tabs
    names = {False: "lz4_raw_device_inflate", True: "lz4_raw_host_inflate"}
    times = {h: [] for h in names}; stats = {h: {"host_ms": 0.0, "device_ms": 0.0} for h in names}; dev_pages = {}
    for h in names: decode(h); decode(h)  # warm-up
    for _ in range(passes):
        for h in names:
            d0 = pp.parquet_device_pages(7); s0 = pp.parquet_stats(); t0 = time.perf_counter(); decode(h); dt = time.perf_counter() - t0; s1 = pp.parquet_stats()
            times[h].append(dt); dev_pages[h] = pp.parquet_device_pages(7)["pages"] - d0["pages"]
            for f in stats[h]: stats[h][f] += s1[f] - s0[f]
    out = {}
    for h, k in names.items():
        ts = sorted(times[h]); med = ts[len(ts) // 2]
        out[h] = {"variant": k, "rows": rows, "row_groups": len(groups), "parquet_bytes": len(data), "passes": passes, "median_s_per_pass": med, "min_s": ts[0],
                  "p10_s": ts[int(len(ts) * 0.1)], "p90_s": ts[int(len(ts) * 0.9)], "rows_per_s": rows / med, "parquet_GB_per_s": len(data) / med / 1e9,
                  "host_ms_per_pass": stats[h]["host_ms"] / passes, "device_ms_per_pass": stats[h]["device_ms"] / passes, "device_inflated_pages_per_pass": dev_pages[h]}
        print(json.dumps(out[h]))
    print(json.dumps({"metric": "decode time, LZ4_RAW pages of literals inflated on the device / every page on the host (medians, alternating passes in one process)",
                      "ratio": out[False]["median_s_per_pass"] / out[True]["median_s_per_pass"]}))
    sys.exit(0)

data = write_parquet(t, row_group_size=rg_rows, data_page_size=1 << 20, **kw)
groups, pinned = pinned_groups(data)
n_rg = len(groups)
q = (Col("labels.code") == "200", [Sum(Col("value"))], [Col("labels.path")])

def run_device():
    plan = pp.HashAggregatePlan(*q)
    # every row group in one call (fdb_batches_from_parquet); $PQ_ONE_BY_ONE: one call per row group, one after the other
    keep = [pp.ResidentBatch.from_parquet(ch, n) for ch, n in groups] if os.environ.get("PQ_ONE_BY_ONE") else pp.ResidentBatch.from_parquet_many(groups)
    plan.CallbackResident(keep)
    out = plan.Finish(); plan.Close()
    for k in keep: k.close()
    return out

def run_host_decode():
    plan = pp.HashAggregatePlan(*q)
    pf = pq.ParquetFile(io.BytesIO(data), read_dictionary=["labels.code", "labels.path"])
    for g in range(n_rg):
        for b in pf.read_row_group(g).to_batches():
            plan.Callback(b)
    out = plan.Finish(); plan.Close()
    return out

a, b = run_device(), run_host_decode()
da = dict(zip(a.column(0).to_pylist(), a.column(1).to_pylist())); db = dict(zip(b.column(0).to_pylist(), b.column(1).to_pylist()))
assert da.keys() == db.keys() and all(abs(da[k] - db[k]) <= 1e-9 * abs(db[k]) for k in da)
res = {}
for name, fn in ((("device_decode", run_device),) if os.environ.get("PQ_DEVICE_ONLY") else (("device_decode", run_device), ("host_decode_pyarrow", run_host_decode))):
    fn(); t0 = time.perf_counter(); n = 3
    for _ in range(n): fn()
    dt = (time.perf_counter() - t0) / n
    res[name] = {"s_per_pass": dt, "rows_per_s": rows / dt, "parquet_GB_per_s": len(data) / dt / 1e9}
print(json.dumps({"metric": "rows/sec parquet bytes (host memory) → filter + aggregate result", "variant": variant, "rows": rows, "row_groups": n_rg, "parquet_bytes": len(data), **res}))
