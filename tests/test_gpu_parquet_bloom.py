"""Bloom filters in the Parquet writer on the device (fdb_batch_to_parquet_filtered, ResidentBatch.to_parquet(bloom_filters=...)): the file
is byte for byte the one the host walk writes (fdb_selftest_parquet_write_filtered — which tests/test_parquet_bloom_cpu.py holds against
pyarrow's own filters and a restatement of the rule) on the record families of the CPU tests and on the shapes where the insert kernel
can go wrong — rows around a validity word and around a tile, a page of two tiles, a tile of NULLs between tiles of values, more
(column, page, tile) items than the launch has workgroups, 32 filtered columns in one call, every row the same value (all lanes meet in
one block), every row distinct, a table of more than 65 536 entry hashes — with and without DELTA, SNAPPY and the page index. pyarrow
and the project's own reader read the files back, and of a sorted record every row's value is in its filter."""
import gc
import io
import os
import re

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq
import pytest

from frostdb_amd import physicalplan as pp
from tests import parquet_bloom_cases as B, parquet_index_cases as X, parquet_write_cases as cases
from tests.parquet_util import row_group_chunks

pytestmark = pytest.mark.gpu
PAGE = B.PAGE
MAX_GRID = int(re.search(r"^#define FDB_PQW_MAX_GRID (\d+)", open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "frostdb_amd", "csrc", "fdb_pqwrite.h")).read(), flags=re.M).group(1))


def read_back(data: bytes) -> pa.RecordBatch:
    t = pq.read_table(io.BytesIO(data)).combine_chunks()
    return pa.RecordBatch.from_arrays([c.chunk(0) if c.num_chunks else pa.array([], type=c.type) for c in t.columns], names=t.schema.names)


def filterable(record: pa.RecordBatch):
    return [n for n in record.schema.names if record.column(n).type != pa.bool_()]


def check(record: pa.RecordBatch, bloom_filters=None, bits: int = 0, page_rows: int = PAGE, reread: bool = True, rules: bool = True, **kw) -> bytes:
    """to_parquet(bloom_filters) of the resident record == the host walk's file; the rule holds; from_parquet and pyarrow read it back."""
    chosen = filterable(record) if bloom_filters is None else bloom_filters
    rb = pp.ResidentBatch(record)
    try:
        data = rb.to_parquet(page_rows=page_rows, bloom_filters=chosen, bloom_bits_per_value=bits, **kw)
        want = pp.selftest_parquet_write(record, page_rows=page_rows, bloom_filters=chosen, bloom_bits_per_value=bits, **kw)
        assert len(data) == len(want), (len(data), len(want))
        if data != want:
            a, b = np.frombuffer(data, dtype=np.uint8), np.frombuffer(want, dtype=np.uint8)
            diff = np.flatnonzero(a != b)
            raise AssertionError("the device's file differs from the host walk's at %d bytes, first at %s" % (len(diff), diff[:8]))
        if rules:
            B.assert_filters(record, data, page_rows, chosen, bits, kw.get("statistics"), kw.get("sorting_columns"), kw.get("index_size_limit", 0))
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
MIXES = [dict(), dict(encodings=ENC), dict(compression="snappy"), dict(statistics="page"),
         dict(encodings=ENC, compression=["snappy", None] * 4 + ["snappy"], statistics="page", sorting_columns=[("timestamp",)])]


# ---- 1. identity with the host walk ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", sorted(B.FAMILIES))
def test_the_families_of_the_cpu_tests(family):
    record = B.FAMILIES[family]()
    check(record)
    check(record, statistics="page", reread=False)
    check(record, filterable(record)[::2], bits=1, compression="snappy", reread=False)


@pytest.mark.parametrize("pattern", cases.NULL_PATTERNS)
def test_every_kind_around_a_word_and_a_tile(pattern):
    for rows in (0, 1, 63, 64, 65, 1000, 4095, 4096, 4097):
        record = cases.mixed_record(rows, pattern)
        for k, mix in enumerate(MIXES):
            if rows in (64, 4097) or k == 0:
                check(record, reread=k == 0, **mix)
        check(record, page_rows=4096, reread=False)   # one short and one full tile


def test_a_page_of_two_tiles_and_a_short_last_tile():
    """Pages of 8 192 rows: two workgroups set bits of one filter; the record's last page is one full tile and a tile of 100 rows."""
    rows = 2 * 8192 + 4096 + 100
    for pattern in ("none", "alternate"):
        record = cases.mixed_record(rows, pattern, dict_size=300)
        for mix in MIXES:
            check(record, page_rows=8192, reread=not mix, rules=not mix, **mix)


def test_a_tile_of_nulls_between_tiles_of_values():
    rows = 3 * 4096 + 33
    r = np.arange(rows)
    middle = (r // 4096) != 1                      # the second tile is NULLs, tiles of values around it
    edges = (r // 4096) == 1                       # … and the other way round
    rng = np.random.default_rng(9)
    idx = rng.integers(0, 40, rows).astype(np.uint32)
    entries = pa.array(["e%02d" % (39 - i) for i in range(40)], type=pa.string())
    cols = [pa.array(rng.integers(-10**9, 10**9, rows), mask=~middle), pa.array(rng.standard_normal(rows), mask=~edges),
            pa.DictionaryArray.from_arrays(pa.array(idx, mask=~middle), entries), pa.DictionaryArray.from_arrays(pa.array(idx, mask=~edges), entries),
            pa.array(rng.integers(0, 2**64, rows, dtype=np.uint64), mask=~edges)]
    record = pa.RecordBatch.from_arrays(cols, names=["i", "f", "d", "d2", "u"])
    check(record, page_rows=3 * 4096)
    check(record, page_rows=8192, compression="snappy", encodings={"i": "delta"}, statistics="page", reread=False)


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
    check(record, page_rows=64)
    check(record, page_rows=64, compression="snappy", encodings={"c00": "delta", "c01": "delta"}, statistics="page", reread=False)


def test_32_filtered_columns_in_one_call():
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
    check(record, page_rows=4096, encodings=encodings)
    check(record, page_rows=4096, encodings=encodings, compression=["snappy", None] * 16, statistics="page", reread=False)


def test_every_row_the_same_value_and_every_row_distinct():
    rows = 8193
    same = pa.RecordBatch.from_arrays([pa.array(np.full(rows, 1234567, dtype=np.int64)), pa.array(np.full(rows, -0.0)), X._dict(np.full(rows, 2), [b"a", b"b", b"the one", b"d"]),
                                       pa.array(np.full(rows, 7, dtype=np.uint64), mask=np.arange(rows) % 3 == 1)], names=["i", "f", "d", "u_null"])
    data = check(same, page_rows=4096)   # all lanes meet in one block: the run rule and the loads keep the atomics few, the bits are the same
    for (off, length), col in zip(B.filter_fields(data), range(4)):
        num_bytes, header_len = B.read_header(data, off)
        assert sum(bin(b).count("1") for b in data[off + header_len:off + length]) == 8, col   # one value: eight bits
    check(same, page_rows=64, bits=1, reread=False)
    rng = np.random.default_rng(8193)
    distinct = pa.RecordBatch.from_arrays([pa.array(rng.permutation(rows).astype(np.int64) * 104729), pa.array(np.arange(rows, dtype=np.float64)),
                                           X._dict(rng.permutation(rows), [b"entry-%05d" % i for i in range(rows)]), pa.array(np.arange(rows, dtype=np.uint64) << np.uint64(40))],
                                          names=["i", "f", "d", "u"])
    check(distinct, page_rows=4096)
    check(distinct, page_rows=1024, bits=64, statistics="page", reread=False)


def test_a_dictionary_of_more_than_65536_entries():
    check(B.wide_dictionary_record(), ["labels.wide"])
    check(B.wide_dictionary_record(3 * PAGE))
    record = cases.dict_record(3000, 65537)
    check(record, page_rows=1024)
    check(record, page_rows=1024, compression="snappy", statistics="page", reread=False)


# ---- 2. a pipeline --------------------------------------------------------------------------------------------------------------------------------
def test_from_parquet_sort_to_parquet_filtered():
    rng = np.random.default_rng(71)
    n = 3000
    rec = pa.RecordBatch.from_arrays([pa.DictionaryArray.from_arrays(pa.array(rng.integers(0, 4, n).astype(np.uint32)), pa.array([b"c", b"a", b"d", b"b", b"unused"], type=pa.binary())),
                                      pa.array(rng.integers(0, 10**12, n), type=pa.int64()), pa.array(rng.random(n) < 0.5),
                                      pa.array(rng.standard_normal(n), mask=rng.random(n) < 0.1)], names=["labels.a", "timestamp", "flag", "x"])
    made = []
    try:
        src = pp.ResidentBatch(rec)
        made.append(src)
        chunks, rows = row_group_chunks(src.to_parquet(encodings={"timestamp": "delta"}, compression="snappy", bloom_filters=["timestamp"]), 0)
        loaded = pp.ResidentBatch.from_parquet(chunks, rows)
        made.append(loaded)
        ordered = loaded.sort([("labels.a",), ("timestamp",)])
        made.append(ordered)
        kw = dict(page_rows=256, encodings={"timestamp": "delta"}, compression="snappy", statistics="page", sorting_columns=[("labels.a",), ("timestamp",)], bloom_filters="sorting")
        data = ordered.to_parquet(**kw)
        back = ordered.to_arrow()
        assert data == pp.selftest_parquet_write(back, **kw)
        B.assert_filters(back, data, 256, "sorting", 0, "page", kw["sorting_columns"])
        fields = B.filter_fields(data)
        assert [f is not None for f in fields] == [True, True, False, False]
        for j in (0, 1):   # every row's value of the sorted record is present in its column's filter
            off, length = fields[j]
            num_bytes, header_len = B.read_header(data, off)
            bitset = data[off + header_len:off + length]
            col = back.column(j)
            values = col.dictionary_decode().to_pylist() if j == 0 else [int(v).to_bytes(8, "little", signed=True) for v in col.to_pylist()]
            assert all(B.maybe(bitset, B.xxh64(v)) for v in values)
        chunks, rows = row_group_chunks(data, 0)
        again = pp.ResidentBatch.from_parquet(chunks, rows)
        made.append(again)
        cases.assert_same_record(again.to_arrow(), back)
        cases.assert_same_record(read_back(data), back)
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
        for kw in (dict(), dict(encodings=enc), dict(compression="snappy"), dict(encodings=enc, compression="snappy"), dict(statistics="page", sorting_columns=[("timestamp",)])):
            old = rb.to_parquet(page_rows=64, **kw)
            assert old == pp.selftest_parquet_write(record, page_rows=64, **kw)
            assert rb.to_parquet(page_rows=64, bloom_filters=None, bloom_bits_per_value=0, **kw) == old
            assert rb.to_parquet(page_rows=64, bloom_filters=[], bloom_bits_per_value=3, **kw) == old
            assert rb.to_parquet(page_rows=64, bloom_filters={"timestamp": False}, **kw) == old
        assert rb.to_parquet(page_rows=64, bloom_filters="sorting") == rb.to_parquet(page_rows=64)
        assert rb.to_parquet(page_rows=64, bloom_filters="sorting", sorting_columns=[("flag",)]) == rb.to_parquet(page_rows=64, sorting_columns=[("flag",)])
        before = pp.live_allocations()
        for kw in (dict(bloom_filters=["nobody"]), dict(bloom_filters="sorted"), dict(bloom_filters=["timestamp"], bloom_bits_per_value=65), dict(bloom_bits_per_value=-1),
                   dict(bloom_filters=["timestamp"], page_rows=100), dict(bloom_filters=["timestamp"], statistics="page", index_size_limit=65537)):
            with pytest.raises(pp.FdbError) as e:
                rb.to_parquet(**kw)
            assert e.value.code == pp.FDB_ERR_INVALID, kw
            assert pp.live_allocations() == before, kw
        for kw in (dict(bloom_filters=["flag"]), dict(bloom_filters=["timestamp"], encodings={"value": "delta"})):
            with pytest.raises(pp.FdbError) as e:
                rb.to_parquet(**kw)
            assert e.value.code == pp.FDB_ERR_UNSUPPORTED and pp.live_allocations() == before, kw
    finally:
        rb.close()


def test_everything_is_released():
    """Last in the module: whatever the tests above made — the table of bitsets, entry hashes, images, returned bytes — is gone."""
    gc.collect()
    record = cases.mixed_record(1000, "alternate")
    rb = pp.ResidentBatch(record)
    for page_rows in (64, 0):
        rb.to_parquet(page_rows=page_rows, encodings={"timestamp": "delta"}, compression="snappy", statistics="page", sorting_columns=[("timestamp",)], bloom_filters="sorting")
        rb.to_parquet(page_rows=page_rows, bloom_filters=B.EIGHT_BYTE_AND_STRINGS, bloom_bits_per_value=64)
    rb.close()
    gc.collect()
    assert all(v == 0 for v in pp.live_allocations().values()), pp.live_allocations()
