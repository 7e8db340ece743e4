"""Statistics and the page index in the Parquet writer on the device (fdb_batch_to_parquet_indexed, ResidentBatch.to_parquet(statistics=...)):
the file is byte for byte the one the host walk writes (fdb_selftest_parquet_write_indexed — which tests/test_parquet_index_cpu.py holds
against pyarrow and a restatement of the rules) on the record families of the CPU tests and on the shapes where the min / max kernel can
go wrong — rows around a validity word and around a tile, a page of two tiles (two workgroups meet in one slot), a short last tile, a
tile of NULLs in front of one with values, more (column, page, tile) items than the launch has workgroups, 32 columns in one call, a
rank table of more than 65 536 entries — with and without DELTA and SNAPPY columns. pyarrow and the project's own reader read the files
back, and a sorted record's page bounds are the oracle's first and last rows."""
import gc
import io
import os
import re
import struct

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq
import pytest

from frostdb_amd import physicalplan as pp
from tests import parquet_index_cases as X, parquet_write_cases as cases, sort_oracle
from tests.parquet_util import row_group_chunks

pytestmark = pytest.mark.gpu
PAGE = X.PAGE
MAX_GRID = int(re.search(r"^#define FDB_PQW_MAX_GRID (\d+)", open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "frostdb_amd", "csrc", "fdb_pqwrite.h")).read(), flags=re.M).group(1))


def read_back(data: bytes) -> pa.RecordBatch:
    t = pq.read_table(io.BytesIO(data)).combine_chunks()
    return pa.RecordBatch.from_arrays([c.chunk(0) if c.num_chunks else pa.array([], type=c.type) for c in t.columns], names=t.schema.names)


def check(record: pa.RecordBatch, statistics="page", page_rows: int = PAGE, reread: bool = True, rules: bool = True, **kw) -> bytes:
    """to_parquet(statistics) of the resident record == the host walk's file; the rules hold; from_parquet and pyarrow read it back."""
    rb = pp.ResidentBatch(record)
    try:
        data = rb.to_parquet(page_rows=page_rows, statistics=statistics, **kw)
        want = pp.selftest_parquet_write(record, page_rows=page_rows, statistics=statistics, **kw)
        assert len(data) == len(want), (len(data), len(want))
        if data != want:
            a, b = np.frombuffer(data, dtype=np.uint8), np.frombuffer(want, dtype=np.uint8)
            diff = np.flatnonzero(a != b)
            raise AssertionError("the device's file differs from the host walk's at %d bytes, first at %s" % (len(diff), diff[:8]))
        if rules:
            X.assert_index(record, data, page_rows, statistics, kw.get("index_size_limit", 0))
        if reread:
            cases.assert_same_record(read_back(data), record)
            if record.num_rows > 0:
                chunks, rows = row_group_chunks(data, 0)
                back = pp.ResidentBatch.from_parquet(chunks, rows)
                try:
                    cases.assert_same_record(back.to_arrow(), rb.to_arrow())
                finally:
                    back.close()
        return data
    finally:
        rb.close()


ENC = {"timestamp": "delta", "dense": "delta"}
MIXES = [dict(), dict(encodings=ENC), dict(compression="snappy"), dict(encodings=ENC, compression=["snappy", None] * 4 + ["snappy"])]


# ---- 1. identity with the host walk ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("statistics", ["chunk", "page"])
@pytest.mark.parametrize("family", sorted(X.FAMILIES))
def test_the_families_of_the_cpu_tests(family, statistics):
    check(X.FAMILIES[family](), statistics)


@pytest.mark.parametrize("pattern", cases.NULL_PATTERNS)
def test_every_kind_around_a_word_and_a_tile(pattern):
    for rows in (0, 1, 63, 64, 65, 1000, 4095, 4096, 4097):
        record = cases.mixed_record(rows, pattern)
        for k, mix in enumerate(MIXES):
            if rows in (64, 4097) or k == 0:
                check(record, "page", reread=k == 0, **mix)
        check(record, "chunk", reread=False)
        check(record, "page", page_rows=4096, reread=False)


def test_a_page_of_two_tiles_and_a_short_last_tile():
    """Pages of 8 192 rows: two workgroups fold into one slot; the record's last page is one full tile and a tile of 100 rows."""
    rows = 2 * 8192 + 4096 + 100
    for pattern in ("none", "alternate"):
        record = cases.mixed_record(rows, pattern, dict_size=300)
        for mix in MIXES:
            check(record, "page", page_rows=8192, reread=not mix, **mix)
        check(record, "chunk", page_rows=8192, reread=False)
    # the bounds of a page sit in one tile each: the minimum in the second, the maximum in the first
    v = np.tile(np.arange(8192, dtype=np.int64), 2)
    v[100], v[8192 + 4096 + 7] = 10**12, -10**12
    f = v.astype(np.float64)
    f[5000] = np.nan
    data = check(pa.RecordBatch.from_arrays([pa.array(v), pa.array(f), pa.array(v.view(np.uint64))], names=["i", "f", "u"]), "page", page_rows=8192)
    ci = X.column_index(data, X.chunk_fields(data)[0]["column_index"])
    assert ci["min_values"] == [struct.pack("<q", 0), struct.pack("<q", -10**12)] and ci["max_values"] == [struct.pack("<q", 10**12), struct.pack("<q", 8191)]


def test_a_tile_of_nulls_in_front_of_one_with_values():
    rows = 8192 + 4096 + 33
    r = np.arange(rows)
    valid = (r % 8192) >= 4096                      # every page: a tile of NULLs, then values
    behind = (r % 8192) < 4096                      # … and the other way round
    rng = np.random.default_rng(9)
    idx = rng.integers(0, 40, rows).astype(np.uint32)
    entries = pa.array(["e%02d" % (39 - i) for i in range(40)], type=pa.string())
    cols = [pa.array(rng.integers(-10**9, 10**9, rows), mask=~valid), pa.array(rng.standard_normal(rows), mask=~behind),
            pa.DictionaryArray.from_arrays(pa.array(idx, mask=~valid), entries), pa.DictionaryArray.from_arrays(pa.array(idx, mask=~behind), entries),
            pa.array(rng.random(rows) < 0.5, mask=~valid), pa.array(rng.integers(0, 2**64, rows, dtype=np.uint64), mask=~behind)]
    record = pa.RecordBatch.from_arrays(cols, names=["i", "f", "d", "d2", "b", "u"])
    check(record, "page", page_rows=8192)
    check(record, "page", page_rows=8192, compression="snappy", encodings={"i": "delta"}, reread=False)
    check(record, "chunk", page_rows=8192, reread=False)


def test_more_items_than_workgroups():
    """17 columns × 70 pages of 64 rows: more (column, page, tile) items than the capped launch has workgroups, so the strided loop goes
    round; the last page is short."""
    rows = 70 * 64 - 9
    rng = np.random.default_rng(17)
    cols, names = [], []
    for k in range(17):
        valid = rng.random(rows) < (0.6 if k % 3 else 1.0)
        if k % 4 == 3:
            cols.append(pa.DictionaryArray.from_arrays(pa.array(rng.integers(0, 50, rows).astype(np.uint32), mask=~valid), pa.array([b"v%02d" % ((i * 7) % 50) for i in range(50)], type=pa.binary())))
        elif k % 4 == 2:
            cols.append(pa.array(rng.standard_normal(rows), mask=~valid))
        else:
            v = rng.integers(-2**40, 2**40, rows)
            cols.append(pa.array(v if k % 4 == 0 else v.astype(np.uint64), mask=~valid))
        names.append("c%02d" % k)
    assert 17 * -(-rows // 64) > MAX_GRID
    record = pa.RecordBatch.from_arrays(cols, names=names)
    check(record, "page", page_rows=64)
    check(record, "chunk", page_rows=64, reread=False)
    check(record, "page", page_rows=64, compression="snappy", encodings={"c00": "delta", "c01": "delta"}, reread=False)


def test_32_columns_in_one_call():
    rows = 20011
    rng = np.random.default_rng(32)
    cols, names, encodings = [], [], []
    for k in range(32):
        valid = rng.random(rows) < (0.5 + 0.5 * (k % 3 == 0))
        if k % 8 == 7:
            cols.append(pa.DictionaryArray.from_arrays(pa.array(rng.integers(0, 1000, rows).astype(np.uint32), mask=~valid), pa.array(["label-%04d" % ((i * 37) % 1000) for i in range(1000)], type=pa.string())))
        elif k % 8 == 5:
            cols.append(pa.array(rng.standard_normal(rows) * 10.0**(k - 16), mask=~valid))
        else:
            v = np.cumsum(rng.integers(0, [1, 3, 2000, 2**20, 2**40, 2**62][k % 6] + 1, rows, dtype=np.int64))
            cols.append(pa.array(v if k % 2 == 0 else v.view(np.uint64), mask=~valid))
        names.append("c%02d" % k)
        encodings.append("delta" if k % 8 == 1 else None)
    record = pa.RecordBatch.from_arrays(cols, names=names)
    check(record, "page", page_rows=4096, encodings=encodings)
    check(record, "page", page_rows=4096, encodings=encodings, compression=["snappy", None] * 16, reread=False)


def test_a_dictionary_of_more_than_65536_entries():
    record = cases.dict_record(3000, 65537)
    check(record, "page", page_rows=1024)
    check(record, "chunk", page_rows=1024, compression="snappy", reread=False)
    check(record, "page", page_rows=1024, index_size_limit=3, reread=False)


def test_limits_and_sorting_columns():
    record = X.strings_record()
    for limit in (1, 15, 17, 65536):
        check(record, "page", index_size_limit=limit, reread=False)
    record = cases.mixed_record(1000, "alternate")
    want = [("timestamp",), ("labels.utf8", True), (2, False, True)]
    for statistics in (None, "chunk", "page"):
        data = check(record, statistics, sorting_columns=want, rules=statistics is not None)
        got = pq.ParquetFile(io.BytesIO(data)).metadata.row_group(0).sorting_columns
        assert [(s.column_index, s.descending, s.nulls_first) for s in got] == [(0, False, False), (4, True, False), (2, False, True)]


# ---- 2. a pipeline --------------------------------------------------------------------------------------------------------------------------------
def test_from_parquet_sort_to_parquet_indexed():
    rng = np.random.default_rng(71)
    n = 3000
    rec = pa.RecordBatch.from_arrays([pa.array(rng.integers(0, 10**12, n), type=pa.int64()),
                                      pa.DictionaryArray.from_arrays(pa.array(rng.integers(0, 4, n).astype(np.uint32)), pa.array([b"c", b"a", b"d", b"b"], type=pa.binary())),
                                      pa.array(rng.standard_normal(n), mask=rng.random(n) < 0.1)], names=["timestamp", "labels.a", "x"])
    made = []
    try:
        src = pp.ResidentBatch(rec)
        made.append(src)
        chunks, rows = row_group_chunks(src.to_parquet(encodings={"timestamp": "delta"}, compression="snappy", statistics="page"), 0)
        loaded = pp.ResidentBatch.from_parquet(chunks, rows)
        made.append(loaded)
        ordered = loaded.sort([("timestamp",)])
        made.append(ordered)
        kw = dict(page_rows=256, encodings={"timestamp": "delta"}, compression="snappy", statistics="page", sorting_columns=[("timestamp",)])
        data = ordered.to_parquet(**kw)
        assert data == pp.selftest_parquet_write(ordered.to_arrow(), **kw)
        order = np.asarray(sort_oracle.sort_indices(rec, [(0,)]), dtype=np.int64)
        ts = np.asarray(rec.column(0))[order]
        first = X.chunk_fields(data)[0]
        ci = X.column_index(data, first["column_index"])
        assert ci["boundary_order"] == X.ASCENDING and not any(ci["null_pages"])
        assert ci["min_values"] == [struct.pack("<q", int(ts[p])) for p in range(0, n, 256)]
        assert ci["max_values"] == [struct.pack("<q", int(ts[min(p + 256, n) - 1])) for p in range(0, n, 256)]
        assert (first["min_value"], first["max_value"]) == (struct.pack("<q", int(ts[0])), struct.pack("<q", int(ts[-1])))
        assert [(s.column_index, s.descending, s.nulls_first) for s in pq.ParquetFile(io.BytesIO(data)).metadata.row_group(0).sorting_columns] == [(0, False, False)]
        X.assert_index(ordered.to_arrow(), data, 256, "page")
        chunks, rows = row_group_chunks(data, 0)
        again = pp.ResidentBatch.from_parquet(chunks, rows)
        made.append(again)
        cases.assert_same_record(again.to_arrow(), ordered.to_arrow())
    finally:
        for rb in made:
            rb.close()


# ---- 3. the unchanged path, refusals, allocations ----------------------------------------------------------------------------------------------------
def test_without_the_new_arguments_the_bytes_are_the_older_ones():
    gc.collect()
    record = cases.mixed_record(1000, "alternate")
    rb = pp.ResidentBatch(record)
    try:
        enc = {"timestamp": "delta"}
        for kw in (dict(), dict(encodings=enc), dict(compression="snappy"), dict(encodings=enc, compression="snappy")):
            old = rb.to_parquet(page_rows=64, **kw)
            assert old == pp.selftest_parquet_write(record, page_rows=64, **kw)
            assert rb.to_parquet(page_rows=64, statistics=None, index_size_limit=0, sorting_columns=None, **kw) == old
            assert rb.to_parquet(page_rows=64, sorting_columns=[], **kw) == old
        before = pp.live_allocations()
        for kw in (dict(statistics="pages"), dict(statistics="page", index_size_limit=65537), dict(index_size_limit=-1), dict(sorting_columns=[(99,)]),
                   dict(sorting_columns=[("timestamp",), (0, True)]), dict(statistics="chunk", sorting_columns=["nobody"])):
            with pytest.raises(pp.FdbError) as e:
                rb.to_parquet(**kw)
            assert e.value.code == pp.FDB_ERR_INVALID, kw
            assert pp.live_allocations() == before, kw
        with pytest.raises(pp.FdbError) as e:
            rb.to_parquet(statistics="page", encodings={"value": "delta"})
        assert e.value.code == pp.FDB_ERR_UNSUPPORTED and pp.live_allocations() == before
    finally:
        rb.close()


def test_everything_is_released():
    """Last in the module: whatever the tests above made — the min / max table, rank tables, images, returned bytes — is gone."""
    gc.collect()
    record = cases.mixed_record(1000, "alternate")
    rb = pp.ResidentBatch(record)
    for page_rows in (64, 0):
        rb.to_parquet(page_rows=page_rows, encodings={"timestamp": "delta"}, compression="snappy", statistics="page", sorting_columns=[("timestamp",)])
        rb.to_parquet(page_rows=page_rows, statistics="chunk")
    rb.close()
    gc.collect()
    assert all(v == 0 for v in pp.live_allocations().values()), pp.live_allocations()
