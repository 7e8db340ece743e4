#!/usr/bin/env python3
"""A resident record written as a Parquet row group on the device (ResidentBatch.to_parquet) against what a caller has to do without it (MI355X).

The record has the shape of bench.py's config 2 at --rows rows (default 20 M): an int64 timestamp, a float64 value with 5 % NULLs and five
label columns — dictionaries of 10, 50, 100, 500 and 1 000 entries, 10 % NULLs each, the first one ordered as the leading sorting column
of a compacted part is. In ONE process, medians of --reps passes after --warmup:
  to_parquet_ms     fdb_batch_to_parquet + fdb_bytes_free: the C call, the file in the library's (pinned) buffer
  python_ms         ResidentBatch.to_parquet(): the same + the copy into a Python bytes object
  survey_ms … host_tail_ms   its passes timed apart: FDB_PROFILE=1 passes of their own (the encode pass is then waited for by itself),
                    read from the library's stderr lines; copy_ms is the one device→host copy of the file image
  floor_ms          a bare device→host copy of as many bytes as the file has, into pinned memory: what the link allows
  arrow_write_ms    to_arrow() followed by pyarrow.parquet.write_table with matching options (one row group, UNCOMPRESSED, data pages
                    V1, dictionary encoding for the label columns only, no statistics): what a caller does at the parent commit;
                    export_ms is its to_arrow() part (--baseline-reps passes, default 3)
With --delta the `timestamp` column is written DELTA_BINARY_PACKED (fdb_batch_to_parquet_encoded): the line's own figures — file_bytes,
to_parquet_ms, the phases, among them delta_compact_ms / delta_survey_ms (block survey + page walk, with the wait for the tables) /
delta_encode_ms — are then the DELTA call's, and the PLAIN call on the same record in the same process goes into the same line as
plain_file_bytes, plain_to_parquet_ms, plain_to_parquet_min_ms / _max_ms (its spread over the repetitions: the yardstick) and plain_*_ms phases.
With --snappy every column is written SNAPPY and `timestamp` DELTA_BINARY_PACKED + SNAPPY (fdb_batch_to_parquet_compressed): the line's
own figures are the SNAPPY call's — among the phases place_compress_ms (the host's body bytes placed + the compress kernel), scan_ms (the
size scan with the wait for the page sizes), final_layout_ms and gather_ms — and the uncompressed PLAIN call on the same record in the
same process goes into the line as with --delta, with plain_floor_ms, the bare copy of ITS file's bytes, beside floor_ms, that of the
compressed file's.
With --lz4 every column is written LZ4_RAW and `timestamp` DELTA_BINARY_PACKED + LZ4_RAW (codec 7 at fdb_batch_to_parquet_compressed): the
line's own figures are the LZ4 call's — among the phases place_ms (the host's body bytes placed; the SNAPPY compress launch has nothing to
do), lz_compress_ms (the compress kernel of fdb_pqlz4.hip), scan_ms (the walk with the carry and the wait for the page sizes),
final_layout_ms, gather_ms (the launch that moves uncompressed chunks: none here) and lz_gather_ms — and both the --snappy call
(snappy_file_bytes, snappy_to_parquet_ms with its spread, snappy_place_compress_ms / _scan_ms / _final_layout_ms / _gather_ms) and the
uncompressed PLAIN call on the same record in the same process go into the same line.
With --stats the record is written uncompressed and PLAIN with statistics="page" (fdb_batch_to_parquet_indexed): chunk bounds, ColumnIndex
and OffsetIndex of every column. The line's own figures are that call's — among the phases stats_ms, the min / max pass of
fdb_pqstats.hip timed apart (rank upload, table reset, kernel, its wait), and wait_ms, what is then left of the survey's wait — and the
call without statistics on the same record in the same process, in front of it, goes into the line as with --delta.
With --bloom the record is written uncompressed and PLAIN with bloom filters on `timestamp` and on the label column `labels.l4`
(fdb_batch_to_parquet_filtered): 20 M distinct values at 10 bits each — a filter of 25 MB, up to four 64-bit atomic ORs a row — beside
1 000 entries, whose filter is found set after the first rows and costs its loads. The line's own figures are that call's — among the
phases bloom_insert_ms, the insert pass of fdb_pqbloom.hip timed apart (entry hashes uploaded, bitsets zeroed, kernel, its wait), and
bloom_copy_ms, the bitsets' device→host copies — with bloom_bytes, what the filters add to the file, and the call without filters on the
same record in the same process, in front of it, goes into the line as with --delta.
With --runs the record is first SORTED by its label columns and the timestamp with the project's own sort (ResidentBatch.sort) — what a
compacted part is — and written uncompressed with runs=True (fdb_batch_to_parquet_runs): the dictionary indices and definition levels of
every column cut into RLE and bit-packed runs. The line's own figures are that call's — among the phases run_survey_ms (the compaction
of the indices by rank, the run survey and the wait for its table) and run_encode_ms — and the call without runs on the same sorted
record in the same process goes into the line as with --delta, with plain_floor_ms, the bare copy of ITS file's bytes, beside floor_ms.
The UNSORTED record, whose columns have no stretches and for which the run survey is pure cost, is written both ways as well:
unsorted_file_bytes / unsorted_to_parquet_ms / unsorted_run_survey_ms / unsorted_run_encode_ms against unsorted_plain_file_bytes /
unsorted_plain_to_parquet_ms and its _min_ms / _max_ms.
With --used the record is written uncompressed with dictionaries="used" (fdb_batch_to_parquet_grouped): every label column's dictionary
page holds the used entries only and its indices are re-keyed and packed at that width. The line's own figures are that call's — among
the phases dict_present_ms (bitmaps zeroed, the present pass of fdb_pqdict.hip, with the wait for the survey's tables and the bitmaps) and
dict_remap_ms (counts up, the remap pass), each also as a rate over the label columns' index bytes (4 B a row and column read; the remap
pass writes as many) against read_ceiling_gbs, the plain read kernel of the same run — and the call with the whole dictionaries on the
same record in the same process goes into the line as with --delta, with plain_floor_ms. --fraction F (default 1: the record as it is,
every entry used, the two passes pure cost) makes the label columns name only every ⌈1/F⌉-th entry of their dictionaries, what a filter
on another column leaves.
With --groups R the record is written in row groups of R rows (fdb_batch_to_parquet_grouped, row_group_rows = R; uncompressed, alone or
with --used): ⌈rows / R⌉ row groups, every pass launched once for the full groups and once more for a shorter last one. The line's own
figures are the grouped call's — its phases are the SUM of a call's marks, both launches — with row_groups, and the ungrouped call of the
parent path on the same record in the same process goes into the line as with --delta, with its spread and plain_floor_ms.
With --strings the record gets one more column, `id`: an all-distinct 16-byte binary value per row — what an id column is — and is written
three times (fdb_batch_to_parquet_strings): `id` in the dictionary form (the call without the option: a dictionary page of every value
plus indices), as "plain" and as "delta_length". Per form file_bytes, to_parquet_ms with its spread, the phases — among them
bytes_survey_ms (the byte survey of fdb_pqbytes.hip with the wait for the survey's tables) and bytes_encode_ms — copy_ms and floor_ms, the
bare device→host copy of that file's bytes; bytes_encode_gbs is the byte encode pass's rate over what it reads and writes (the value
bytes twice, 4 B of index a row, with "plain" 4 B of length a value), beside copy_probe_gbs, the best `1 read : 1 written` line of
--copy-probe (tools/copy_probe, built with hipcc first) run by the same command. The record WITHOUT `id`, written by this build without
the option, goes into the same line as base_to_parquet_ms with its spread: what the parent commit's call is compared with.
One JSON line on stdout, appended to --out (profiles/parquet_write_bench.jsonl) when given.

    python tools/parquet_write_bench.py [--rows N] [--page-rows N] [--delta | --snappy | --lz4 | --stats | --bloom | --runs | [--used [--fraction F]] [--groups R] | --strings [--copy-probe FILE]] [--out FILE]
"""
import argparse
import io
import json
import os
import re
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402,F401  (first: one ROCm stack per process, see tests/conftest.py)
import numpy as np  # noqa: E402
import pyarrow as pa  # noqa: E402
import pyarrow.parquet as pq  # noqa: E402

from frostdb_amd import physicalplan as pp  # noqa: E402

LABELS = [10, 50, 100, 500, 1000]
PHASES = ["survey", "layout", "encode", "copy", "host tail"]
DELTA_PHASES = ["delta compact", "delta survey", "delta encode"]
SNAPPY_PHASES = ["compress", "scan", "final layout", "gather"]
LZ4_PHASES = ["lz compress", "lz gather"]
STATS_PHASES = ["stats", "wait"]
BLOOM_PHASES = ["bloom insert", "bloom copy"]
BLOOM_COLUMNS = ["timestamp", "labels.l4"]
RUN_PHASES = ["run survey", "run encode"]
DICT_PHASES = ["dict present", "dict remap"]
BYTES_PHASES = ["bytes survey", "bytes encode"]
ID_BYTES = 16


def make_record(rows: int, seed: int = 1, fraction: float = 1.0) -> pa.RecordBatch:
    rng = np.random.default_rng(seed)
    cols = [pa.array(np.cumsum(rng.integers(0, 2000, rows, dtype=np.int64))), pa.array(rng.standard_normal(rows), mask=rng.random(rows) < 0.05)]
    names = ["timestamp", "value"]
    for k, entries in enumerate(LABELS):
        idx = rng.integers(0, entries, rows).astype(np.uint32)
        if fraction < 1.0:
            step = int(np.ceil(1.0 / fraction))
            idx = idx // step * step
        if k == 0:
            idx = np.sort(idx)
        values = pa.array(["label-%d-value-%04d" % (k, e) for e in range(entries)], type=pa.string())
        cols.append(pa.DictionaryArray.from_arrays(pa.array(idx, mask=rng.random(rows) < 0.10), values))
        names.append("labels.l%d" % k)
    return pa.RecordBatch.from_arrays(cols, names=names)


def median_ms(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        times.append((time.perf_counter() - t) * 1e3)
    return statistics.median(times), times


def profiled_phases(rb, page_rows, reps, encodings=None, compression=None, stats=None, bloom=None, runs=None, dictionaries=None, groups=0, strings=None):
    """The library's FDB_PROFILE lines of `reps` to_parquet() calls: {phase: median ms} — with `groups`, where a call marks a pass once
    per launch, the marks' sum per call."""
    os.environ["FDB_PROFILE"] = "1"
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile(mode="w+b") as tmp:
        os.dup2(tmp.fileno(), 2)
        try:
            for _ in range(reps):
                rb.to_parquet(page_rows=page_rows, encodings=encodings, compression=compression, statistics=stats, bloom_filters=bloom, runs=runs, dictionaries=dictionaries, row_group_rows=groups, strings=strings)
        finally:
            os.dup2(saved, 2)
            os.close(saved)
            del os.environ["FDB_PROFILE"]
        tmp.seek(0)
        text = tmp.read().decode("utf-8", "replace")
    out = {}
    for phase in PHASES + DELTA_PHASES + SNAPPY_PHASES + LZ4_PHASES + STATS_PHASES + BLOOM_PHASES + RUN_PHASES + DICT_PHASES + BYTES_PHASES:
        us = [float(m) for m in re.findall(r"\[fdb\] pqwrite %s\s+([0-9.]+) us" % re.escape(phase), text)]
        out[phase] = (sum(us) / reps if groups else statistics.median(us)) / 1e3 if us else None
    return out


def id_column(rows: int) -> pa.Array:
    """`rows` distinct binary values of ID_BYTES bytes: the hex digits of a bijection of the row number."""
    v = np.arange(rows, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)
    digits = np.empty((rows, ID_BYTES), dtype=np.uint8)
    for k in range(ID_BYTES):
        nib = ((v >> np.uint64(4 * k)) & np.uint64(15)).astype(np.uint8)
        digits[:, ID_BYTES - 1 - k] = np.where(nib < 10, nib + 48, nib + 87)
    offsets = (np.arange(rows + 1, dtype=np.int64) * ID_BYTES).astype(np.int32 if rows * ID_BYTES < 2**31 else np.int64)
    typ = pa.binary() if offsets.dtype == np.int32 else pa.large_binary()
    return pa.Array.from_buffers(typ, rows, [None, pa.py_buffer(offsets.tobytes()), pa.py_buffer(digits.tobytes())])


def copy_probe_gbs(path):
    """The best GB/s among copy_probe's `1 read : 1 written` lines, or None without the probe."""
    import subprocess
    if not path or not os.path.exists(path):
        return None
    out = subprocess.run([path], check=True, capture_output=True, text=True, timeout=120).stdout
    rates = [float(m.group(1)) for ln in out.splitlines() if "(1 read : 1 written)" in ln for m in [re.search(r"([0-9.]+) GB/s", ln)] if m]
    return max(rates) if rates else None


def strings_main(args):
    import ctypes
    base = make_record(args.rows)
    record = base.append_column("id", id_column(args.rows))
    r3 = lambda v: None if v is None else round(v, 3)  # noqa: E731
    line = {"tool": "parquet_write_bench", "strings": "id", "rows": args.rows, "page_rows": args.page_rows or 65536, "columns": record.num_columns, "id_bytes": ID_BYTES,
            "reps": args.reps, "warmup": args.warmup, "date": time.strftime("%Y-%m-%d")}

    def bare_copy_ms(n_bytes):
        dev = torch.empty(n_bytes, dtype=torch.uint8, device="cuda")
        host = torch.empty(n_bytes, dtype=torch.uint8).pin_memory()

        def bare_copy():
            host.copy_(dev, non_blocking=True)
            torch.cuda.synchronize()
        return median_ms(bare_copy, args.reps, args.warmup)[0]

    def measure(rb, form, prefix):
        names = rb.column_names
        data = rb.to_parquet(page_rows=args.page_rows, strings={"id": form} if form else None)
        want = len(data)
        md = pq.ParquetFile(io.BytesIO(data)).metadata
        assert md.num_rows == args.rows
        if form:
            col = md.row_group(0).column(names.index("id"))
            assert not col.has_dictionary_page and col.encodings[0] == ("PLAIN" if form == "plain" else "DELTA_LENGTH_BYTE_ARRAY"), col.encodings
        del data
        opts = pp.ParquetWriteOptions(args.page_rows, 0, None)
        forms = (ctypes.c_int8 * len(names))(*[pp.PARQUET_STRING_FORMS[form] if n == "id" else 0 for n in names])
        sopt = pp.ParquetStringOptions(ctypes.cast(forms, ctypes.c_void_p), len(names), 0)

        def c_call():
            out, n = ctypes.c_void_p(), ctypes.c_int64()
            if form:
                rc = pp.lib().fdb_batch_to_parquet_strings(rb.handle, ctypes.byref(opts), None, 0, None, 0, None, None, None, None, ctypes.byref(sopt), ctypes.byref(out), ctypes.byref(n))
            else:
                rc = pp.lib().fdb_batch_to_parquet(rb.handle, ctypes.byref(opts), ctypes.byref(out), ctypes.byref(n))
            assert rc == 0 and n.value == want, pp.lib().fdb_last_error()
            pp.lib().fdb_bytes_free(out.value)
        ms, every = median_ms(c_call, args.reps, args.warmup)
        ph = profiled_phases(rb, args.page_rows, args.reps, strings={"id": form} if form else None)
        line.update({prefix + "file_bytes": want, prefix + "to_parquet_ms": r3(ms), prefix + "to_parquet_min_ms": r3(min(every)), prefix + "to_parquet_max_ms": r3(max(every)),
                     prefix + "floor_ms": r3(bare_copy_ms(want))})
        line.update({prefix + k.replace(" ", "_") + "_ms": r3(ph[k]) for k in PHASES + (BYTES_PHASES if form else [])})
        if form and ph["bytes encode"]:
            moved = args.rows * (2 * ID_BYTES + 4 + (4 if form == "plain" else 0))
            line[prefix + "bytes_encode_gbs"] = round(moved / (ph["bytes encode"] * 1e-3) / 1e9, 1)

    rb = pp.ResidentBatch(base)
    try:
        measure(rb, None, "base_")
    finally:
        rb.close()
    del base
    rb = pp.ResidentBatch(record)
    del record
    try:
        for form, prefix in ((None, "dictionary_"), ("plain", "plain_"), ("delta_length", "delta_length_")):
            measure(rb, form, prefix)
    finally:
        rb.close()
    probe = copy_probe_gbs(args.copy_probe)
    line["copy_probe_gbs"] = None if probe is None else round(probe, 1)
    text = json.dumps(line)
    print(text, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(text + "\n")
    assert pp.live_allocations()["device_blocks"] == 0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, default=20_000_000)
    ap.add_argument("--page-rows", type=int, default=0)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--baseline-reps", type=int, default=3)
    ap.add_argument("--delta", action="store_true", help="write `timestamp` DELTA_BINARY_PACKED; the PLAIN call goes into the same line")
    ap.add_argument("--snappy", action="store_true", help="write every column SNAPPY and `timestamp` DELTA + SNAPPY; the uncompressed PLAIN call goes into the same line")
    ap.add_argument("--lz4", action="store_true", help="write every column LZ4_RAW and `timestamp` DELTA + LZ4_RAW; the --snappy call and the uncompressed PLAIN call go into the same line")
    ap.add_argument("--stats", action="store_true", help="write statistics and the page index (uncompressed, PLAIN); the call without them goes into the same line")
    ap.add_argument("--bloom", action="store_true", help="write bloom filters on `timestamp` and `labels.l4` (uncompressed, PLAIN); the call without them goes into the same line")
    ap.add_argument("--runs", action="store_true", help="sort the record by its label columns and write it with runs=True (uncompressed); the call without runs, and both calls on the unsorted record, go into the same line")
    ap.add_argument("--used", action="store_true", help="write dictionaries of used entries only (uncompressed); the call with the whole dictionaries goes into the same line")
    ap.add_argument("--fraction", type=float, default=1.0, help="with --used: the label columns name only every ceil(1/F)-th entry of their dictionaries")
    ap.add_argument("--groups", type=int, default=0, help="write row groups of this many rows (a multiple of 64; alone or with --used); the ungrouped call goes into the same line")
    ap.add_argument("--strings", action="store_true", help="add an all-distinct 16-byte `id` column and write it as a dictionary, PLAIN and DELTA_LENGTH_BYTE_ARRAY; the record without it goes into the same line")
    ap.add_argument("--copy-probe", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "copy_probe"), help="with --strings: tools/copy_probe, built with hipcc (its best copy line goes into the line)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.strings:
        assert args.delta + args.snappy + args.lz4 + args.stats + args.bloom + args.runs + args.used == 0 and args.groups == 0, "--strings stands alone"
        return strings_main(args)
    assert args.delta + args.snappy + args.lz4 + args.stats + args.bloom + args.runs + args.used <= 1, "--delta, --snappy, --lz4, --stats, --bloom, --runs or --used"
    assert 0.0 < args.fraction <= 1.0 and (args.used or args.fraction == 1.0), "--fraction goes with --used"
    assert args.groups == 0 or (args.groups > 0 and args.groups % 64 == 0 and args.delta + args.snappy + args.lz4 + args.stats + args.bloom + args.runs == 0), "--groups R: a multiple of 64, alone or with --used"
    record = make_record(args.rows, fraction=args.fraction)
    rb = pp.ResidentBatch(record)
    del record
    unsorted = None
    if args.runs:
        unsorted, rb = rb, rb.sort([("labels.l%d" % k,) for k in range(len(LABELS))] + [("timestamp",)])
    try:
        encodings = {"timestamp": "delta"} if args.delta or args.snappy or args.lz4 else None
        compression = "snappy" if args.snappy else "lz4" if args.lz4 else None
        stats = "page" if args.stats else None
        bloom = BLOOM_COLUMNS if args.bloom else None
        runs = True if args.runs else None
        dictionaries = "used" if args.used else None
        data = rb.to_parquet(page_rows=args.page_rows, encodings=encodings, compression=compression, statistics=stats, bloom_filters=bloom, runs=runs, dictionaries=dictionaries, row_group_rows=args.groups)
        file_bytes = len(data)
        md = pq.ParquetFile(io.BytesIO(data)).metadata
        row_groups = -(-args.rows // args.groups) if args.groups else 1
        assert md.num_rows == args.rows and md.num_row_groups == row_groups
        if args.delta or args.snappy or args.lz4:
            assert set(md.row_group(0).column(0).encodings) == {"DELTA_BINARY_PACKED"}
        if args.snappy or args.lz4:  # (pyarrow's metadata says "LZ4" for codec 7)
            assert all(md.row_group(0).column(j).compression == ("SNAPPY" if args.snappy else "LZ4") for j in range(md.num_columns))
            column_bytes = {md.row_group(0).column(j).path_in_schema: [md.row_group(0).column(j).total_compressed_size, md.row_group(0).column(j).total_uncompressed_size] for j in range(md.num_columns)}
        if args.stats:
            assert all(md.row_group(0).column(j).has_column_index and md.row_group(0).column(j).has_offset_index and md.row_group(0).column(j).statistics.has_min_max for j in range(md.num_columns))
        if args.runs or args.used or args.groups:
            column_bytes = {md.row_group(0).column(j).path_in_schema: sum(md.row_group(g).column(j).total_compressed_size for g in range(row_groups)) for j in range(md.num_columns)}
        if args.bloom:
            filters = {md.row_group(0).column(j).path_in_schema: md.row_group(0).column(j).to_dict().get("bloom_filter_length") for j in range(md.num_columns)}
            assert all((filters[n] is not None) == (n in BLOOM_COLUMNS) for n in filters), filters
        del data
        import ctypes
        opts = pp.ParquetWriteOptions(args.page_rows, 0, None)
        n_columns = len(rb.column_names)
        enc = (ctypes.c_int8 * n_columns)(*([1] + [0] * (n_columns - 1)))

        codecs = (ctypes.c_int8 * n_columns)(*([7 if args.lz4 else 1] * n_columns))
        snappy_codecs = (ctypes.c_int8 * n_columns)(*([1] * n_columns))

        index = pp.ParquetIndexOptions(2, 0, None, 0)
        names = rb.column_names
        bloom_on = (ctypes.c_int8 * n_columns)(*[1 if n in BLOOM_COLUMNS else 0 for n in names])
        bloom_opts = pp.ParquetBloomOptions(ctypes.cast(bloom_on, ctypes.c_void_p), n_columns, 0)

        run_opts, _keep_runs = pp._parquet_run_options(True, names, [n.startswith("labels.") for n in names])

        group_opts = pp.ParquetGroupOptions(args.groups, 1 if args.used else 0, 0)

        def c_call(delta=args.delta, want=file_bytes, snappy=args.snappy or args.lz4, indexed=args.stats, filtered=args.bloom, run_encoded=args.runs, handle=None, used=args.used or args.groups > 0):
            out, n = ctypes.c_void_p(), ctypes.c_int64()
            if used:
                rc = pp.lib().fdb_batch_to_parquet_grouped(rb.handle, ctypes.byref(opts), None, 0, None, 0, None, None, None, ctypes.byref(group_opts), ctypes.byref(out), ctypes.byref(n))
            elif run_encoded:
                rc = pp.lib().fdb_batch_to_parquet_runs(handle or rb.handle, ctypes.byref(opts), None, 0, None, 0, None, None, ctypes.byref(run_opts), ctypes.byref(out), ctypes.byref(n))
            elif handle is not None:
                rc = pp.lib().fdb_batch_to_parquet(handle, ctypes.byref(opts), ctypes.byref(out), ctypes.byref(n))
            elif filtered:
                rc = pp.lib().fdb_batch_to_parquet_filtered(rb.handle, ctypes.byref(opts), None, 0, None, 0, None, ctypes.byref(bloom_opts), ctypes.byref(out), ctypes.byref(n))
            elif indexed:
                rc = pp.lib().fdb_batch_to_parquet_indexed(rb.handle, ctypes.byref(opts), None, 0, None, 0, ctypes.byref(index), ctypes.byref(out), ctypes.byref(n))
            elif snappy:
                rc = pp.lib().fdb_batch_to_parquet_compressed(rb.handle, ctypes.byref(opts), ctypes.cast(enc, ctypes.c_void_p), n_columns, ctypes.cast(codecs, ctypes.c_void_p), n_columns,
                                                              ctypes.byref(out), ctypes.byref(n))
            elif delta:
                rc = pp.lib().fdb_batch_to_parquet_encoded(rb.handle, ctypes.byref(opts), ctypes.cast(enc, ctypes.c_void_p), n_columns, ctypes.byref(out), ctypes.byref(n))
            else:
                rc = pp.lib().fdb_batch_to_parquet(rb.handle, ctypes.byref(opts), ctypes.byref(out), ctypes.byref(n))
            assert rc == 0 and n.value == want, pp.lib().fdb_last_error()
            pp.lib().fdb_bytes_free(out.value)
        plain = {}
        if args.lz4:  # the SNAPPY call on the same record, in this process, measured the same way
            snappy_bytes = len(rb.to_parquet(page_rows=args.page_rows, encodings=encodings, compression="snappy"))

            def snappy_call():
                out, n = ctypes.c_void_p(), ctypes.c_int64()
                rc = pp.lib().fdb_batch_to_parquet_compressed(rb.handle, ctypes.byref(opts), ctypes.cast(enc, ctypes.c_void_p), n_columns, ctypes.cast(snappy_codecs, ctypes.c_void_p), n_columns,
                                                              ctypes.byref(out), ctypes.byref(n))
                assert rc == 0 and n.value == snappy_bytes, pp.lib().fdb_last_error()
                pp.lib().fdb_bytes_free(out.value)
            ms, every = median_ms(snappy_call, args.reps, args.warmup)
            ph = profiled_phases(rb, args.page_rows, args.reps, encodings, "snappy")
            plain.update({"snappy_file_bytes": snappy_bytes, "snappy_to_parquet_ms": ms, "snappy_to_parquet_min_ms": min(every), "snappy_to_parquet_max_ms": max(every),
                          "snappy_place_compress_ms": ph["compress"], "snappy_scan_ms": ph["scan"], "snappy_final_layout_ms": ph["final layout"], "snappy_gather_ms": ph["gather"]})
        if args.delta or args.snappy or args.lz4 or args.stats or args.bloom or args.runs or args.used or args.groups:  # the yardstick: the PLAIN call on the same record, in this process, measured the same way
            plain_bytes = len(rb.to_parquet(page_rows=args.page_rows))
            ms, every = median_ms(lambda: c_call(False, plain_bytes, False, False, False, False, None, False), args.reps, args.warmup)
            ph = profiled_phases(rb, args.page_rows, args.reps)
            plain.update({"plain_file_bytes": plain_bytes, "plain_to_parquet_ms": ms, "plain_to_parquet_min_ms": min(every), "plain_to_parquet_max_ms": max(every)})
            plain.update({"plain_%s_ms" % k.replace(" ", "_"): ph[k] for k in PHASES})
        to_parquet_ms, to_parquet_all = median_ms(c_call, args.reps, args.warmup)
        python_ms, _ = median_ms(lambda: rb.to_parquet(page_rows=args.page_rows, encodings=encodings, compression=compression, statistics=stats, bloom_filters=bloom, runs=runs, dictionaries=dictionaries, row_group_rows=args.groups), args.reps, 1)
        phases = profiled_phases(rb, args.page_rows, args.reps, encodings, compression, stats, bloom, runs, dictionaries, args.groups)
        if args.runs:  # the record as it was before the sort: no stretches, the run passes are pure cost
            u_bytes, u_plain_bytes = len(unsorted.to_parquet(page_rows=args.page_rows, runs=True)), len(unsorted.to_parquet(page_rows=args.page_rows))
            u_plain_ms, u_plain_all = median_ms(lambda: c_call(False, u_plain_bytes, False, False, False, False, unsorted.handle, False), args.reps, args.warmup)
            u_ms, u_all = median_ms(lambda: c_call(False, u_bytes, False, False, False, True, unsorted.handle, False), args.reps, args.warmup)
            u_phases = profiled_phases(unsorted, args.page_rows, args.reps, runs=True)
            plain.update({"unsorted_file_bytes": u_bytes, "unsorted_plain_file_bytes": u_plain_bytes, "unsorted_to_parquet_ms": u_ms, "unsorted_to_parquet_min_ms": min(u_all),
                          "unsorted_to_parquet_max_ms": max(u_all), "unsorted_plain_to_parquet_ms": u_plain_ms, "unsorted_plain_to_parquet_min_ms": min(u_plain_all),
                          "unsorted_plain_to_parquet_max_ms": max(u_plain_all), "unsorted_run_survey_ms": u_phases["run survey"], "unsorted_run_encode_ms": u_phases["run encode"],
                          "unsorted_survey_ms": u_phases["survey"], "unsorted_encode_ms": u_phases["encode"], "unsorted_copy_ms": u_phases["copy"]})

        def bare_copy_ms(n_bytes):
            dev = torch.empty(n_bytes, dtype=torch.uint8, device="cuda")
            host = torch.empty(n_bytes, dtype=torch.uint8).pin_memory()

            def bare_copy():
                host.copy_(dev, non_blocking=True)
                torch.cuda.synchronize()
            return median_ms(bare_copy, args.reps, args.warmup)[0]
        floor_ms = bare_copy_ms(file_bytes)
        read_ceiling = pp.read_ceiling(0, 2 << 30, 5) if args.used else None
        if args.snappy or args.lz4 or args.runs or args.used or args.groups:
            plain["plain_floor_ms"] = bare_copy_ms(plain["plain_file_bytes"])

        label_names = ["labels.l%d" % k for k in range(len(LABELS))]
        export_times, baseline_bytes = [], [0]

        def arrow_write():
            t = time.perf_counter()
            rec = rb.to_arrow()
            export_times.append((time.perf_counter() - t) * 1e3)
            sink = pa.BufferOutputStream()
            pq.write_table(pa.Table.from_batches([rec]), sink, row_group_size=max(1, rec.num_rows), compression="NONE", use_dictionary=label_names,
                           data_page_version="1.0", write_statistics=False, data_page_size=1 << 20)
            baseline_bytes[0] = sink.getvalue().size
        arrow_write_ms, _ = median_ms(arrow_write, args.baseline_reps, 1)
    finally:
        rb.close()
        if unsorted is not None:
            unsorted.close()
    r3 = lambda v: None if v is None else round(v, 3)  # noqa: E731
    line = {"tool": "parquet_write_bench", "rows": args.rows, "page_rows": args.page_rows or 65536, "columns": 2 + len(LABELS), "file_bytes": file_bytes,
            "to_parquet_ms": r3(to_parquet_ms), "to_parquet_min_ms": r3(min(to_parquet_all)), "python_ms": r3(python_ms), "to_parquet_gbs": round(file_bytes / (to_parquet_ms * 1e-3) / 1e9, 2),
            "survey_ms": r3(phases["survey"]), "layout_ms": r3(phases["layout"]), "encode_ms": r3(phases["encode"]), "copy_ms": r3(phases["copy"]),
            "host_tail_ms": r3(phases["host tail"]), "floor_ms": r3(floor_ms), "floor_gbs": round(file_bytes / (floor_ms * 1e-3) / 1e9, 2),
            "arrow_write_ms": r3(arrow_write_ms), "export_ms": r3(statistics.median(export_times[1:])), "arrow_file_bytes": baseline_bytes[0],
            "arrow_over_device": round(arrow_write_ms / to_parquet_ms, 2), "reps": args.reps, "warmup": args.warmup, "baseline_reps": args.baseline_reps,
            "date": time.strftime("%Y-%m-%d")}
    if args.delta:
        line.update({"delta": ["timestamp"], "to_parquet_max_ms": r3(max(to_parquet_all)), "delta_compact_ms": r3(phases["delta compact"]), "delta_survey_ms": r3(phases["delta survey"]),
                     "delta_encode_ms": r3(phases["delta encode"])})
    if args.snappy:
        line.update({"delta": ["timestamp"], "snappy": "all", "to_parquet_max_ms": r3(max(to_parquet_all)), "delta_compact_ms": r3(phases["delta compact"]),
                     "delta_survey_ms": r3(phases["delta survey"]), "delta_encode_ms": r3(phases["delta encode"]), "place_compress_ms": r3(phases["compress"]), "scan_ms": r3(phases["scan"]),
                     "final_layout_ms": r3(phases["final layout"]), "gather_ms": r3(phases["gather"]), "column_bytes": column_bytes})
    if args.lz4:
        line.update({"delta": ["timestamp"], "lz4": "all", "to_parquet_max_ms": r3(max(to_parquet_all)), "delta_compact_ms": r3(phases["delta compact"]),
                     "delta_survey_ms": r3(phases["delta survey"]), "delta_encode_ms": r3(phases["delta encode"]), "place_ms": r3(phases["compress"]), "lz_compress_ms": r3(phases["lz compress"]),
                     "scan_ms": r3(phases["scan"]), "final_layout_ms": r3(phases["final layout"]), "gather_ms": r3(phases["gather"]), "lz_gather_ms": r3(phases["lz gather"]),
                     "column_bytes": column_bytes})
    if args.stats:
        line.update({"statistics": "page", "to_parquet_max_ms": r3(max(to_parquet_all)), "stats_ms": r3(phases["stats"]), "wait_ms": r3(phases["wait"])})
    if args.bloom:
        line.update({"bloom": BLOOM_COLUMNS, "bloom_bytes": file_bytes - plain["plain_file_bytes"], "to_parquet_max_ms": r3(max(to_parquet_all)), "bloom_insert_ms": r3(phases["bloom insert"]),
                     "bloom_copy_ms": r3(phases["bloom copy"])})
    if args.runs:
        line.update({"runs": "all", "sorted_by": ["labels.l%d" % k for k in range(len(LABELS))] + ["timestamp"], "to_parquet_max_ms": r3(max(to_parquet_all)),
                     "run_survey_ms": r3(phases["run survey"]), "run_encode_ms": r3(phases["run encode"]), "column_bytes": column_bytes})
    if args.used:
        index_bytes = 4 * args.rows * len(LABELS)
        rate = lambda ms: None if not ms else round(index_bytes / (ms * 1e-3) / 1e9, 1)  # noqa: E731
        line.update({"dictionaries": "used", "fraction": args.fraction, "to_parquet_max_ms": r3(max(to_parquet_all)), "dict_present_ms": r3(phases["dict present"]), "dict_remap_ms": r3(phases["dict remap"]),
                     "index_bytes": index_bytes, "dict_present_read_gbs": rate(phases["dict present"]), "dict_remap_read_gbs": rate(phases["dict remap"]), "read_ceiling_gbs": round(read_ceiling, 1),
                     "column_bytes": column_bytes})
    if args.groups:
        line.update({"row_group_rows": args.groups, "row_groups": row_groups, "to_parquet_max_ms": r3(max(to_parquet_all)), "column_bytes": column_bytes})
    if args.delta or args.snappy or args.lz4 or args.stats or args.bloom or args.runs or args.used or args.groups:
        line.update({k: (r3(v) if isinstance(v, float) else v) for k, v in plain.items()})
    text = json.dumps(line)
    print(text, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(text + "\n")
    assert pp.live_allocations()["device_blocks"] == 0


if __name__ == "__main__":
    main()
