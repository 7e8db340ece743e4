"""RLE runs inside index and level pages, the host side (fdb_selftest_parquet_write_runs, selftest_parquet_write(runs=...)): no GPU.

1. The rule is restated in Python (tests/parquet_runs_cases.py) and the restatement pinned: a hybrid decoder written from the format's
   description decodes what it lays out, the runs are the ones the rule names on hand-checked streams, and pyarrow reads pages built
   from it.
2. The host walk's files: every run-encoded stream equals the restatement byte for byte, pyarrow and the project's chunk parser read the
   file, no page is longer than without `runs`, footer sizes and PageLocations agree with a walk of the chunk — on stretches of T − 1,
   T, T + 1 groups at a page's start, middle and end, back-to-back RLE runs, tails of 1 … 7 symbols that join, follow an RLE run or
   follow a bit-packed run, widths 1 … 17, RLE counts and bit-packed runs where the header's varint grows, n < 8, pages that stay as
   they were, levels under the NULL patterns and clustered NULLs, and mixed with SNAPPY, DELTA, the page index and bloom filters.
3. Without `runs` the older calls' bytes are unchanged; every refusal has its code and names what it refuses; header, exports,
   binding and build list the entry points; fdb_pqruns.hip compiles for gfx950 without scratch or spills."""
import ctypes
import io
import os
import re
import subprocess

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq
import pytest

from tests import parquet_pages as P
from tests import parquet_runs_cases as R
from tests import parquet_write_cases as cases
from tests.parquet_util import row_group_chunks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
ENTRY_POINTS = ["fdb_batch_to_parquet_runs", "fdb_selftest_parquet_write_runs"]
PAGE = R.PAGE


@pytest.fixture(scope="module")
def pp():
    from frostdb_amd import physicalplan
    return physicalplan


def write_and_check(pp, record, runs=True, page_rows=PAGE, expect_cut=True, parse=True, **kw) -> bytes:
    """The host walk's file with `runs`, held to the restatement; pyarrow reads it back to the record."""
    data = pp.selftest_parquet_write(record, page_rows=page_rows, runs=runs, **kw)
    plain = pp.selftest_parquet_write(record, page_rows=page_rows, **kw)
    cut = R.assert_runs_file(record, data, plain, page_rows, R.flags_of(record, runs))
    assert (cut > 0) == expect_cut, cut
    assert len(data) <= len(plain) and (len(data) < len(plain)) == expect_cut
    cases.assert_same_record(R.read_back(data), record)
    if parse and record.num_rows:
        row_group_chunks(data, 0)
    return data


# ---- 1. the restatement, pinned -----------------------------------------------------------------------------------------------------------------------
def test_thresholds():
    assert [R.threshold(w) for w in R.WIDTHS] == R.THRESHOLDS
    assert [(w + 7) // 8 for w in R.WIDTHS] == [1, 1, 1, 1, 1, 2, 2, 2, 3]


def test_the_restatement_names_the_runs_of_hand_checked_streams():
    mixed = [0, 1, 0, 1, 0, 1, 0, 1]
    ones, twos = [1] * 8, [2] * 8
    # w = 8: T = 2
    assert R.plan_of(mixed + ones + mixed, 8) == [("bp", 3)]                                  # T − 1 groups: not worth a run
    assert R.plan_of(mixed + ones * 2 + mixed, 8) == [("bp", 1), ("rle", 16), ("bp", 1)]      # T
    assert R.plan_of(ones * 2 + twos * 2, 8) == [("rle", 16), ("rle", 16)]                    # back to back
    assert R.plan_of(ones * 2 + [1, 1, 1], 8) == [("rle", 19)]                                # the tail joins
    assert R.plan_of(ones * 2 + [1, 1, 2], 8) == [("rle", 16), ("bp", 1)]                     # … does not: a run of its own
    assert R.plan_of(ones * 2 + mixed + [1, 1, 1], 8) == [("rle", 16), ("bp", 2)]             # … after a bit-packed run: one more group of it
    assert R.plan_of(mixed + ones + [1] * 7, 8) == [("bp", 3)]                                # a stretch of T − 1 and an equal tail: no run to join
    assert R.plan_of([5, 5, 5], 8) == [("bp", 1)] and R.plan_of([], 8) == []
    assert R.plan_of(ones + twos + ones, 8) == [("bp", 3)]                                    # uniform groups of different values are no stretch
    # w = 1: T = 16; w = 17: T = 1
    assert R.plan_of([1] * 120 + [0] * 8, 1) == [("bp", 16)] and R.plan_of([1] * 128 + [0] * 8, 1) == [("rle", 128), ("bp", 1)]
    assert R.plan_of(ones + mixed + twos, 17) == [("rle", 8), ("bp", 1), ("rle", 8)]
    # the bytes of one: 8-bit indices, an RLE run of 16 ones between two packed groups
    assert R.restate(mixed + ones * 2 + mixed, 8) == bytes([3]) + bytes(mixed) + bytes([32, 1]) + bytes([3]) + bytes(mixed)
    assert R.restate([1] * 128 + [0, 1, 1], 1) == bytes([0x80, 0x02, 1, 3, 0b110])


@pytest.mark.parametrize("w", R.WIDTHS)
def test_the_decoder_reads_what_the_restatement_lays_out_and_it_is_never_longer(w):
    rng = np.random.default_rng(w)
    pg = R.page_for(w)
    streams = [s for s in np.split(R.stretch_symbols(rng, w), len(R.stretch_symbols(np.random.default_rng(w), w)) // pg)] + [s for s, _ in R.tail_pieces(w)]
    streams += [rng.integers(0, 2, n) * (R.entries_for(w) - 1) for n in (1, 7, 8, 9, 500)] + [np.repeat(rng.integers(0, R.entries_for(w), 40), rng.integers(1, 60, 40))]
    kinds = set()
    for sym in streams:
        data = R.restate(sym, w)
        got, runs = R.decode_hybrid(data, w, len(sym))
        assert got == [int(s) for s in sym]
        assert runs == R.plan_of(sym, w)
        assert len(data) <= len(P.hybrid(np.asarray(sym, dtype=np.uint64), w, P.bp_plan(len(sym)), pad=0)), "longer than the one bit-packed run"
        kinds |= {k for k, _ in runs}
        for (k, c), nxt in zip(runs, runs[1:]):   # the rule's runs are maximal: two bit-packed runs never touch
            assert not (k == "bp" and nxt[0] == "bp")
    assert kinds == {"rle", "bp"}


def test_the_tail_pieces_are_what_they_say():
    for w in R.WIDTHS:
        T = R.threshold(w)
        for sym, what in R.tail_pieces(w):
            plan, t = R.plan_of(sym, w), len(sym) % 8
            if what == "joins":
                assert plan[-1] == ("rle", 8 * T + t)
            elif what == "after_rle":
                assert plan[-2:] == [("rle", 8 * T), ("bp", 1)]
            elif what == "after_bp":
                assert plan == [("rle", 8 * T), ("bp", 2)]
            else:
                assert plan == [("bp", 1)] and len(sym) < 8


def test_pyarrow_reads_pages_built_from_the_restatement():
    """One INT64 dictionary column, its entries 0 … entries − 1: pyarrow's reader gives back the indices and the NULLs the pages hold."""
    rng = np.random.default_rng(5)
    for w in (1, 3, 9, 17):
        entries = R.entries_for(w)
        idx = np.concatenate([R.stretch_symbols(rng, w)] + [s for s, _ in R.tail_pieces(w)])
        valid = R.clustered_valid(len(idx) + len(idx) // 3, 129)
        valid[np.flatnonzero(valid)[len(idx):]] = False
        valid[np.flatnonzero(~valid)[:len(idx) - int(valid.sum())]] = True
        assert int(valid.sum()) == len(idx)
        levels = valid.astype(np.uint64)
        body = bytes([w]) + R.restate(idx, w)
        lv = R.restate(levels, 1)
        body = len(lv).to_bytes(4, "little") + lv + body
        page = P.page_header(P.DATA_PAGE, len(body), len(body), len(valid), P.RLE_DICTIONARY) + body
        dictionary = P.dictionary_page(P.INT64, np.arange(entries, dtype=np.int64))
        data = P.file_of(P.chunk_of("x", P.INT64, True, False, [dictionary, page]), len(valid), len(dictionary))
        got = pq.read_table(io.BytesIO(data)).column(0).combine_chunks()
        assert got.null_count == len(valid) - len(idx)
        np.testing.assert_array_equal(np.asarray(got.is_valid()), valid)
        np.testing.assert_array_equal(got.drop_null().to_numpy(), idx.astype(np.int64))


# ---- 2. the host walk's files -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", R.WIDTHS)
def test_stretches_of_every_length_at_every_place(pp, w):
    for pattern in (None, "first_of_page", "last_of_page"):
        write_and_check(pp, R.width_record(w, pattern), page_rows=R.page_for(w))
    # values and levels chosen apart
    record = R.width_record(w, "first_of_page")
    name = record.schema.names[0]
    both = pp.selftest_parquet_write(record, page_rows=R.page_for(w), runs=True)
    assert pp.selftest_parquet_write(record, page_rows=R.page_for(w), runs=[name]) == both
    assert pp.selftest_parquet_write(record, page_rows=R.page_for(w), runs={name: True, "timestamp": None}) == both
    only_values = write_and_check(pp, record, runs={name: "values"}, page_rows=R.page_for(w))
    write_and_check(pp, record, runs={name: "levels"}, page_rows=R.page_for(w), expect_cut=False)   # (one NULL a page: no stretch of 16 level groups … but for w = 1's pages)
    assert len(only_values) >= len(both)


@pytest.mark.parametrize("w", [1, 3, 8, 9, 17])
def test_tails_of_one_to_seven_symbols(pp, w):
    for sym, what in R.tail_pieces(w):
        record = pa.RecordBatch.from_arrays([R._dict(sym, R.entries_for(w), utf8=True)], names=["labels.t"])
        write_and_check(pp, record, page_rows=512, expect_cut=what != "short" and len(set(sym.tolist())) > 1)
        # … and with NULLs between the values: the same index stream by rank
        valid = np.ones(2 * len(sym), bool)
        valid[1::2] = False
        spread = np.zeros(2 * len(sym), np.uint32)
        spread[0::2] = sym
        with_nulls = pa.RecordBatch.from_arrays([R._dict(spread, R.entries_for(w), valid)], names=["labels.t"])
        data = write_and_check(pp, with_nulls, runs={"labels.t": "values"}, page_rows=1024, expect_cut=what != "short" and len(set(sym.tolist())) > 1)
        assert len(data) > 0


def test_where_the_run_headers_grow(pp):
    """RLE counts of 63 / 64 and 8 191 / 8 192 symbols (the varint of count << 1 takes a second, a third byte), bit-packed runs of 63 /
    64 groups."""
    for w in (8, 17):
        hi = R.entries_for(w)
        rng = np.random.default_rng(w)
        for count in (63, 64, 8191, 8192):
            head = R.noise(rng, 8, hi)
            sym = np.concatenate([head, np.full(count, hi - 1), (np.arange(8 - count % 8) % (hi - 1)) if count % 8 else np.zeros(0, int), R.noise(rng, 8, hi)])
            plan = R.plan_of(sym, w)
            assert ("rle", count - count % 8) in plan
            assert len(P.varint((count - count % 8) << 1)) == (1 if count < 64 else 2 if count < 8192 else 3)
            write_and_check(pp, pa.RecordBatch.from_arrays([R._dict(sym, hi)], names=["labels.h"]), page_rows=16384)
        for groups in (63, 64):
            sym = np.concatenate([np.full(64, hi - 1), R.noise(rng, 8 * groups, hi), np.full(64, 0)])
            assert R.plan_of(sym, w) == [("rle", 64), ("bp", groups), ("rle", 64)]
            write_and_check(pp, pa.RecordBatch.from_arrays([R._dict(sym, hi)], names=["labels.h"]), page_rows=1024)


def test_pages_that_stay_as_they_are(pp):
    """n = 0, n < 8, a page of one index, a page of NULLs, a dictionary of one entry, an empty dictionary, V64 / BOOL / DELTA payloads:
    the bytes of the call without `runs`."""
    for record in (cases.rle_record(), cases.empty_dictionary_record(), cases.dict_record(200, 1), cases.duplicates_record(), cases.large_strings_record(), cases.extremes_record()):
        data = pp.selftest_parquet_write(record, page_rows=PAGE, runs=True)
        plain = pp.selftest_parquet_write(record, page_rows=PAGE)
        R.assert_runs_file(record, data, plain, PAGE, R.flags_of(record, True))
        cases.assert_same_record(R.read_back(data), record)
    for rows in (0, 1, 7):
        record = cases.mixed_record(rows, "alternate")
        assert pp.selftest_parquet_write(record, page_rows=PAGE, runs=True) == pp.selftest_parquet_write(record, page_rows=PAGE)
    record = cases.rle_record()   # pages of one index, with and without NULLs: RLE runs before, the same bytes now
    both = pp.selftest_parquet_write(record, page_rows=PAGE, runs={"labels.ordered": True})
    assert both == pp.selftest_parquet_write(record, page_rows=PAGE)
    # 8-byte and boolean columns: only their levels can change
    record = cases.mixed_record(1000, "whole_page")
    data = pp.selftest_parquet_write(record, page_rows=PAGE, runs=True, encodings={"timestamp": "delta"})
    plain = pp.selftest_parquet_write(record, page_rows=PAGE, encodings={"timestamp": "delta"})
    R.assert_runs_file(record, data, plain, PAGE, R.flags_of(record, True))


@pytest.mark.parametrize("pattern", cases.NULL_PATTERNS)
def test_levels_under_the_null_patterns(pp, pattern):
    for rows in cases.ROWS:
        record = R.levels_record(cases.valid_mask(rows, pattern))
        data = pp.selftest_parquet_write(record, page_rows=PAGE, runs=True)
        plain = pp.selftest_parquet_write(record, page_rows=PAGE)
        R.assert_runs_file(record, data, plain, PAGE, R.flags_of(record, True))
        cases.assert_same_record(R.read_back(data), record)
        if rows:
            row_group_chunks(data, 0)
    write_and_check(pp, R.levels_record(cases.valid_mask(5000, pattern, 1024)), page_rows=1024, expect_cut=pattern in ("first_of_page", "last_of_page"))


@pytest.mark.parametrize("stretch", [127, 128, 129])
def test_clustered_nulls(pp, stretch):
    record = R.levels_record(R.clustered_valid(4000, stretch))
    data = write_and_check(pp, record, page_rows=1024)
    assert data == pp.selftest_parquet_write(record, page_rows=1024, runs={n: "levels" for n in record.schema.names} | {"labels.d": True})
    write_and_check(pp, record, runs={"i": "levels", "b": "levels"}, page_rows=4096)


MIXES = [dict(compression="snappy"), dict(compression=["snappy", None, "snappy", None, "snappy"]), dict(encodings={"timestamp": "delta"}),
         dict(statistics="page", sorting_columns=[("labels.a",), ("labels.b",)]), dict(statistics="chunk"), dict(bloom_filters=["labels.a", "timestamp"]),
         dict(encodings={"timestamp": "delta"}, compression=["snappy", None, "snappy", None, "snappy"], statistics="page", sorting_columns=[("labels.a",)], bloom_filters=["labels.b", "value"])]


@pytest.mark.parametrize("k", range(len(MIXES)))
def test_runs_mixed_with_the_other_options(pp, k):
    record = R.sorted_record(3000)
    data = write_and_check(pp, record, page_rows=512, **MIXES[k])
    if "bloom_filters" in MIXES[k]:
        from tests import parquet_bloom_cases as B
        B.assert_filters(record, data, 512, MIXES[k]["bloom_filters"], 0, MIXES[k].get("statistics"), MIXES[k].get("sorting_columns"))
    elif MIXES[k].get("statistics"):   # (with filters, assert_filters has looked at the index behind them)
        from tests import parquet_index_cases as X
        X.assert_index(record, data, 512, MIXES[k]["statistics"])


def test_a_sorted_record_shrinks(pp):
    """What the feature is for: label columns of a sorted record nearly vanish."""
    record = R.sorted_record(20000, labels=2)
    data = pp.selftest_parquet_write(record, page_rows=4096, runs=True)
    plain = pp.selftest_parquet_write(record, page_rows=4096)
    sizes = lambda d: [pq.ParquetFile(io.BytesIO(d)).metadata.row_group(0).column(j).total_compressed_size for j in range(2)]
    assert sizes(data)[0] * 20 < sizes(plain)[0] and sizes(data)[1] * 2 < sizes(plain)[1], (sizes(data), sizes(plain))
    cases.assert_same_record(R.read_back(data), record)


def test_the_projects_own_parser_accepts_the_chunks(pp):
    """The project's own reader parses row group 0 of files written with runs — their pages hold many run headers now: on a machine
    without a GPU it gets as far as the device call (FDB_ERR_DEVICE, the convention of tests/test_capi_cpu.py), never FDB_ERR_INVALID;
    with one it simply succeeds."""
    for record, kw in ((R.sorted_record(3000), dict(page_rows=512)), (R.sorted_record(3000), dict(page_rows=512, compression="snappy", encodings={"timestamp": "delta"})),
                       (R.width_record(17, "first_of_page"), dict(page_rows=R.page_for(17))), (R.levels_record(R.clustered_valid(3000, 129)), dict(page_rows=1024))):
        data = pp.selftest_parquet_write(record, runs=True, **kw)
        assert data != pp.selftest_parquet_write(record, **kw)
        chunks, rows = row_group_chunks(data, 0)
        assert rows == record.num_rows
        try:
            pp.ResidentBatch.from_parquet(chunks, rows).close()
        except pp.FdbError as e:
            assert e.code == pp.FDB_ERR_DEVICE, (e.code, str(e))


# ---- 3. the unchanged path, refusals, the interface ------------------------------------------------------------------------------------------------------
def call_runs(pp, record, runs, page_rows=PAGE, codecs=None, index=None, bloom=None, encodings=None):
    opts = pp.ParquetWriteOptions(page_rows, 0, None)
    out, nb = ctypes.c_void_p(), ctypes.c_int64()
    arr = (ctypes.c_int8 * len(codecs))(*codecs) if codecs else None
    enc = (ctypes.c_int8 * len(encodings))(*encodings) if encodings else None
    with pp.ExportedBatch(record) as ex:
        rc = pp.lib().fdb_selftest_parquet_write_runs(ctypes.addressof(ex.array), ctypes.addressof(ex.schema), ctypes.byref(opts), ctypes.cast(enc, ctypes.c_void_p) if encodings else None,
                                                      len(encodings) if encodings else 0, ctypes.cast(arr, ctypes.c_void_p) if codecs else None, len(codecs) if codecs else 0,
                                                      ctypes.byref(index) if index is not None else None, ctypes.byref(bloom) if bloom is not None else None,
                                                      ctypes.byref(runs) if runs is not None else None, ctypes.byref(out), ctypes.byref(nb))
    if rc != 0:
        assert not out.value
        return rc, pp.lib().fdb_last_error().decode()
    try:
        return 0, ctypes.string_at(out.value, nb.value)
    finally:
        pp.lib().fdb_bytes_free(out.value)


def run_options(pp, entries, n=None):
    arr = (ctypes.c_int8 * max(1, len(entries)))(*entries)
    return pp.ParquetRunOptions(ctypes.cast(arr, ctypes.c_void_p), len(entries) if n is None else n, 0), arr


def test_without_runs_the_bytes_are_the_older_calls(pp):
    record = cases.mixed_record(1000, "alternate")
    n = record.num_columns
    none, _keep = run_options(pp, [0] * n)
    for codecs, compression in ((None, None), ([1] * n, "snappy")):
        for statistics, index in ((None, None), ("page", pp.ParquetIndexOptions(2, 0, None, 0))):
            old = pp.selftest_parquet_write(record, page_rows=PAGE, compression=compression if compression else [None] * n, statistics=statistics)
            assert call_runs(pp, record, None, codecs=codecs, index=index) == (0, old)
            assert call_runs(pp, record, pp.ParquetRunOptions(None, 0, 0), codecs=codecs, index=index) == (0, old)
            assert call_runs(pp, record, none, codecs=codecs, index=index) == (0, old)
    for kw in (dict(), dict(encodings={"timestamp": "delta"}), dict(compression="snappy"), dict(statistics="page", sorting_columns=[("timestamp",)]), dict(bloom_filters=["timestamp"])):
        old = pp.selftest_parquet_write(record, page_rows=PAGE, **kw)
        assert pp.selftest_parquet_write(record, page_rows=PAGE, runs=None, **kw) == old
        assert pp.selftest_parquet_write(record, page_rows=PAGE, runs=[], **kw) == old
        assert pp.selftest_parquet_write(record, page_rows=PAGE, runs={"timestamp": None, "labels.utf8": None}, **kw) == old
    stretched = R.sorted_record(1000)
    assert pp.selftest_parquet_write(stretched, page_rows=PAGE, runs=True) != pp.selftest_parquet_write(stretched, page_rows=PAGE)
    # bit 1 on a required column is ignored; True skips the indices of columns that have none
    required = pa.RecordBatch.from_arrays([pa.array(np.arange(100, dtype=np.int64))], names=["dense"])
    opt, _keep = run_options(pp, [2])
    assert call_runs(pp, required, opt) == (0, pp.selftest_parquet_write(required, page_rows=PAGE))
    assert pp.selftest_parquet_write(required, page_rows=PAGE, runs=True) == pp.selftest_parquet_write(required, page_rows=PAGE)


def test_refusals(pp):
    record = cases.mixed_record(100, "alternate")
    n = record.num_columns
    names = record.schema.names
    one = [0] * n
    one[names.index("labels.utf8")] = 3
    for count in (1, n - 1, n + 1, -1):
        opt, _keep = run_options(pp, one, n=count)
        rc, text = call_runs(pp, record, opt)
        assert rc == pp.FDB_ERR_INVALID and "has %d entries" % count in text, (count, text)
    rc, text = call_runs(pp, record, pp.ParquetRunOptions(None, n, 0))
    assert rc == pp.FDB_ERR_INVALID and "entries" in text
    for entry in (-1, 4, 127):
        opt, _keep = run_options(pp, [0, entry] + [0] * (n - 2))
        rc, text = call_runs(pp, record, opt)
        assert rc == pp.FDB_ERR_INVALID and "columns[1] is %d" % entry in text, text
    for name in ("timestamp", "count", "value", "flag", "dense"):
        for bits in (1, 3):
            opt, _keep = run_options(pp, [bits if k == names.index(name) else 0 for k in range(n)])
            rc, text = call_runs(pp, record, opt)
            assert rc == pp.FDB_ERR_UNSUPPORTED and "column %s is not one" % name in text, text
        opt, _keep = run_options(pp, [2 if k == names.index(name) else 0 for k in range(n)])
        assert call_runs(pp, record, opt)[0] == 0
    # everything the older calls refuse stays refused
    opt, _keep = run_options(pp, one)
    rc, text = call_runs(pp, record, opt, page_rows=100)
    assert rc == pp.FDB_ERR_INVALID and "page_rows" in text
    rc, text = call_runs(pp, record, opt, codecs=[2] + [0] * (n - 1))
    assert rc == pp.FDB_ERR_INVALID and "codecs[0] is 2" in text
    rc, text = call_runs(pp, record, opt, index=pp.ParquetIndexOptions(3, 0, None, 0))
    assert rc == pp.FDB_ERR_INVALID and "statistics is 3" in text
    rc, text = call_runs(pp, record, opt, bloom=pp.ParquetBloomOptions(None, 0, 65))
    assert rc == pp.FDB_ERR_INVALID and "bits_per_value is 65" in text
    rc, text = call_runs(pp, record, opt, encodings=[0, 0, 1] + [0] * (n - 3))
    assert rc == pp.FDB_ERR_UNSUPPORTED and "DELTA" in text
    # the binding's own
    for kw, code, text in (({"runs": ["nobody"]}, pp.FDB_ERR_INVALID, "nobody"), ({"runs": {"nobody": None}}, pp.FDB_ERR_INVALID, "nobody"), ({"runs": "labels.utf8"}, pp.FDB_ERR_INVALID, "`runs` is"),
                           ({"runs": [3]}, pp.FDB_ERR_INVALID, "names no column"), ({"runs": {"labels.utf8": "both"}}, pp.FDB_ERR_INVALID, "'both'"), ({"runs": {"labels.utf8": 1}}, pp.FDB_ERR_INVALID, "unknown run streams"),
                           ({"runs": ["timestamp"]}, pp.FDB_ERR_UNSUPPORTED, "timestamp"), ({"runs": {"flag": "values"}}, pp.FDB_ERR_UNSUPPORTED, "flag")):
        with pytest.raises(pp.FdbError) as e:
            pp.selftest_parquet_write(record, **kw)
        assert e.value.code == code and text in str(e.value), (kw, str(e.value))
    # a row that points past its dictionary is still the survey's to refuse
    bad = pa.DictionaryArray.from_arrays(pa.array([0, 1, 0], type=pa.uint32()), pa.array([b"a", b"b"], type=pa.binary()))
    idx = np.frombuffer(bad.indices.buffers()[1], dtype=np.uint32).copy()
    idx[1] = 7
    wrong = pa.DictionaryArray.from_arrays(pa.Array.from_buffers(pa.uint32(), 3, [None, pa.py_buffer(idx.tobytes())]), bad.dictionary, safe=False)
    with pytest.raises(pp.FdbError) as e:
        pp.selftest_parquet_write(pa.RecordBatch.from_arrays([wrong], names=["d"]), runs=True)
    assert e.value.code == pp.FDB_ERR_INVALID and "out of range" in str(e.value)


def test_entry_points_are_in_library_header_exports_and_binding(pp):
    L = pp.lib()
    header = open(os.path.join(ROOT, "include", "frostdb_amd.h")).read()
    exports = open(os.path.join(ROOT, "frostdb_amd", "csrc", "exports.map")).read()
    for name in ENTRY_POINTS:
        assert re.search(r"^FDB_API int %s\(.*const fdb_parquet_bloom_options\* bloom /\* NULL: none \*/, const fdb_parquet_run_options\* runs /\* NULL: none \*/, uint8_t\*\* bytes, int64_t\* n_bytes\);" % name,
                         header, flags=re.M), name
        assert name in exports and re.search(r"global:\s*fdb_\*;", exports)
        assert getattr(L, name).argtypes is not None and len(getattr(L, name).argtypes) == len(getattr(L, name.replace("_runs", "_filtered")).argtypes) + 1
    assert re.search(r"typedef struct fdb_parquet_run_options \{\s*const int8_t\* columns;[^}]*int32_t n_columns;[^}]*int32_t pad;[^}]*\} fdb_parquet_run_options;", header)
    assert [f[0] for f in pp.ParquetRunOptions._fields_] == ["columns", "n_columns", "pad"] and ctypes.sizeof(pp.ParquetRunOptions) == 16
    assert (pp.ParquetRunOptions.columns.offset, pp.ParquetRunOptions.n_columns.offset, pp.ParquetRunOptions.pad.offset) == (0, 8, 12)
    assert ctypes.sizeof(pp.ParquetBloomOptions) == 16 and ctypes.sizeof(pp.ParquetIndexOptions) == 24 and ctypes.sizeof(pp.ParquetWriteOptions) == 16   # pinned: the older structs keep their layouts
    build = open(os.path.join(ROOT, "frostdb_amd", "build.py")).read()
    assert "fdb_pqruns.hip" in build and "fdb_pqruns.h" in build


def test_run_kernels_compile_for_gfx950_without_scratch(tmp_path):
    """fdb_pqruns.hip compiled offline for gfx950 with the flags of the writer's compile test: the resource report shows the three kernels,
    no scratch and no spills."""
    src = os.path.join(ROOT, "frostdb_amd", "csrc", "fdb_pqruns.hip")
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-munsafe-fp-atomics", "-I", os.path.join(ROOT, "frostdb_amd", "csrc"),
                        "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", str(tmp_path / "fdb_pqruns.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    remarks = [ln.split("remark:", 1)[1].split("[-Rpass")[0].strip() for ln in r.stderr.splitlines() if "remark:" in ln]
    names = [u for u in remarks if u.startswith("Function Name:")]
    print(" | ".join(remarks))
    assert len(names) == 3 and all(any(k in u for u in names) for k in ("pqr_compact_kernel", "pqr_survey_kernel", "pqr_encode_kernel")), names
    scratch = [u for u in remarks if "ScratchSize" in u]
    assert len(scratch) == 3 and all("ScratchSize [bytes/lane]: 0" in u for u in scratch), remarks
    spills = [u for u in remarks if "Spill" in u]
    assert spills and all(re.search(r"Spill: 0\b", u) for u in spills), remarks
