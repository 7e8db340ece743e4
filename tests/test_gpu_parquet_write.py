"""The Parquet writer on the device (fdb_batch_to_parquet, ResidentBatch.to_parquet): for every shape of tests/test_parquet_write_cpu.py
the file is byte for byte the one the host walk writes (fdb_selftest_parquet_write — which the CPU tests hold against pyarrow), pyarrow and
the project's own reader read it back to the record, and the shapes only a device run reaches — a tile of the packer and a page of the
default size ∓ one row, tiles that contribute no value in front of tiles that start in the middle of a word, more work items than a
launch has workgroups, 32 dictionary columns in one call — come out the same way. Pipelines end in to_parquet as they end in the
reference: from_parquet → sort, three ordered records → merge, filter() output."""
import gc
import io

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq
import pytest

from frostdb_amd import physicalplan as pp
from frostdb_amd.logicalplan import Col, Sum
from tests import merge_oracle, parquet_write_cases as cases, sort_oracle
from tests.parquet_util import row_group_chunks

pytestmark = pytest.mark.gpu


def check(record: pa.RecordBatch, page_rows: int = 0, optional=None, reread: bool = True) -> bytes:
    """to_parquet of the resident record == the host walk's file; pyarrow reads it back; so does from_parquet."""
    rb = pp.ResidentBatch(record)
    try:
        data = rb.to_parquet(page_rows=page_rows, optional=optional)
        want = pp.selftest_parquet_write(record, page_rows=page_rows, optional=optional)
        assert len(data) == len(want), (len(data), len(want))
        if data != want:
            a, b = np.frombuffer(data, dtype=np.uint8), np.frombuffer(want, dtype=np.uint8)
            diff = np.flatnonzero(a != b)
            raise AssertionError("the device's file differs from the host walk's at %d bytes, first at %s" % (len(diff), diff[:8]))
        cases.assert_reads_back(record, data, optional if isinstance(optional, dict) else None)
        if reread and record.num_rows > 0:
            chunks, rows = row_group_chunks(data, 0)
            back = pp.ResidentBatch.from_parquet(chunks, rows)
            try:
                cases.assert_same_record(back.to_arrow(), rb.to_arrow())
            finally:
                back.close()
        return data
    finally:
        rb.close()


# ---- 1. identity with the host walk, every shape of the CPU tests ------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", cases.NULL_PATTERNS)
def test_every_column_kind_rows_and_null_pattern(pattern):
    for rows in cases.ROWS:
        check(cases.mixed_record(rows, pattern), page_rows=cases.PAGE)


def test_dictionary_sizes():
    for entries in cases.DICT_SIZES:
        check(cases.dict_record(1000, entries), page_rows=cases.PAGE)


def test_rle_pages_extremes_duplicates_and_empty_dictionaries():
    check(cases.rle_record(), page_rows=cases.PAGE)
    check(cases.extremes_record(), page_rows=cases.PAGE)
    check(cases.duplicates_record(), page_rows=cases.PAGE)
    check(cases.empty_dictionary_record(), page_rows=cases.PAGE)
    check(cases.large_strings_record(), page_rows=cases.PAGE)


def test_options():
    record = cases.mixed_record(1000, "none")
    names = record.schema.names
    check(record, page_rows=cases.PAGE, optional={n: False for n in names})
    check(record, page_rows=128, optional={"timestamp": True, "labels.utf8": False})
    check(record)
    check(cases.mixed_record(1000, "alternate"), page_rows=1 << 24)


def test_a_zero_row_batch():
    record = cases.mixed_record(0, "none")
    check(record)
    rb = pp.ResidentBatch(cases.mixed_record(100, "alternate"))
    empty = rb.take([])
    try:
        cases.assert_reads_back(record, empty.to_parquet())
    finally:
        rb.close()
        empty.close()


# ---- 2. what only a device run reaches ---------------------------------------------------------------------------------------------------------
def wide_record(rows: int, entries: int, valid: np.ndarray, seed: int = 0) -> pa.RecordBatch:
    rng = np.random.default_rng(seed + rows)
    idx = rng.integers(0, entries, rows).astype(np.uint32)
    idx[np.flatnonzero(valid)[-1]] = entries - 1
    ents = pa.array([b"%x" % i for i in range(entries)], type=pa.binary())
    cols = [pa.DictionaryArray.from_arrays(pa.array(idx, mask=~valid), ents), pa.array(rng.integers(-2**62, 2**62, rows), type=pa.int64(), mask=~valid),
            pa.array(rng.random(rows) < 0.5, mask=~valid), pa.array(rng.standard_normal(rows))]
    return pa.RecordBatch.from_arrays(cols, names=["labels.w", "timestamp", "flag", "value"])


@pytest.mark.parametrize("rows", [63, 64, 65, 4095, 4096, 4097, 65535, 65536, 65537, 100003])
def test_rows_around_a_wave_a_tile_and_a_default_page(rows):
    valid = np.random.default_rng(rows).random(rows) < 0.8
    valid[-1] = True
    check(wide_record(rows, 1000, valid))   # width 10


def test_width_17_with_one_null_in_the_first_tile():
    rows = 3 * 4096 + 77
    valid = np.ones(rows, dtype=bool)
    valid[5] = False   # 4095 values × 17 bits: the second tile starts in the middle of a word
    check(wide_record(rows, 65537, valid))


def test_tiles_without_values_in_front_of_tiles_that_start_mid_word():
    rows = 5 * 4096 + 3
    for entries in (3, 65537):
        valid = np.ones(rows, dtype=bool)
        valid[7] = False
        valid[4096:3 * 4096] = False       # two tiles contribute nothing
        valid[3 * 4096 + 1::2] = False
        check(wide_record(rows, entries, valid))
    valid = np.zeros(rows, dtype=bool)
    valid[2 * 4096 + 100] = True           # one value in the whole record
    check(wide_record(rows, 300, valid))


def test_more_work_items_than_workgroups():
    """100 003 rows in pages of 64: 1 563 pages × 4 columns, more (column, page) and (column, page, tile) items than a launch has workgroups
    (FDB_PQW_MAX_GRID = 1 024) — the loops of both kernels go round."""
    rows = 100003
    valid = np.random.default_rng(3).random(rows) < 0.7
    check(wide_record(rows, 257, valid), page_rows=64)


def test_32_dictionary_columns_in_one_call():
    """… at the default page size: 32 columns × 3 pages × 16 tiles, the encode loop goes round."""
    rows = 140003
    rng = np.random.default_rng(32)
    cols, names = [], []
    for k in range(32):
        entries = [1, 2, 5, 17, 300, 1000, 70000, 3][k % 8]
        valid = rng.random(rows) < (0.5 + 0.5 * (k % 3 == 0))
        idx = rng.integers(0, entries, rows).astype(np.uint32)
        if k % 5 == 4:
            idx = np.sort(idx)   # an ordered column: pages of one index
        cols.append(pa.DictionaryArray.from_arrays(pa.array(idx, mask=~valid), pa.array(["l%d-%d" % (k, e) for e in range(entries)], type=pa.string())))
        names.append("labels.l%02d" % k)
    check(pa.RecordBatch.from_arrays(cols, names=names), reread=False)


# ---- 3. pipelines ------------------------------------------------------------------------------------------------------------------------------
def read_back(data: bytes) -> pa.RecordBatch:
    t = pq.read_table(io.BytesIO(data)).combine_chunks()
    return pa.RecordBatch.from_arrays([c.chunk(0) if c.num_chunks else pa.array([], type=c.type) for c in t.columns], names=t.schema.names)


def shard(rng, n):
    valid = rng.random(n) < 0.85
    a = pa.DictionaryArray.from_arrays(pa.array(rng.integers(0, 4, n).astype(np.uint32), mask=~valid), pa.array([b"c", b"a", b"d", b"b"], type=pa.binary()))
    b = pa.DictionaryArray.from_arrays(pa.array(rng.integers(0, 23, n).astype(np.uint32)), pa.array([b"l%02d" % ((k * 7) % 23) for k in range(23)], type=pa.binary()))
    return pa.RecordBatch.from_arrays([a, b, pa.array(rng.integers(0, 1000, n), type=pa.int64()), pa.array(rng.standard_normal(n), mask=rng.random(n) < 0.1)],
                                      names=["labels.a", "labels.b", "v", "x"])


def test_from_parquet_sort_to_parquet():
    rec = shard(np.random.default_rng(61), 3000)
    made = []
    try:
        src = pp.ResidentBatch(rec)
        made.append(src)
        chunks, rows = row_group_chunks(src.to_parquet(), 0)
        loaded = pp.ResidentBatch.from_parquet(chunks, rows)
        made.append(loaded)
        ordered = loaded.sort([("labels.a",), ("labels.b",), ("v",)])
        made.append(ordered)
        data = ordered.to_parquet(page_rows=256)
        want = rec.take(pa.array(sort_oracle.sort_indices(rec, [(0,), (1,), (2,)]), type=pa.int64()))
        cases.assert_same_record(read_back(data), merge_oracle.decoded_record(want))
        # the leading sorting column of the ordered record is run after run: its pages are RLE runs, the file is smaller than the unordered one
        assert len(data) < len(loaded.to_parquet(page_rows=256))
    finally:
        for rb in made:
            rb.close()


def test_merge_of_three_ordered_records_to_parquet():
    rng = np.random.default_rng(62)
    columns = [(0,), (1,)]
    records = []
    for n in (2500, 70, 4100):
        rec = shard(rng, n)
        records.append(rec.take(pa.array(sort_oracle.sort_indices(rec, columns), type=pa.int64())))
    rbs = [pp.ResidentBatch(r) for r in records]
    try:
        merged = pp.ResidentBatch.merge(rbs, columns)
        rbs.append(merged)
        data = merged.to_parquet(page_rows=512)
        cases.assert_same_record(read_back(data), merge_oracle.merge(records, columns))
    finally:
        for rb in rbs:
            rb.close()


def test_filter_output_to_parquet():
    rec = shard(np.random.default_rng(63), 9000)
    plan = pp.HashAggregatePlan(Col("v") > 300, [Sum(Col("v"))], [Col("labels.a")])
    made = []
    try:
        rb = pp.ResidentBatch(rec)
        made.append(rb)
        filtered = plan.FilterResident(rb)
        made.append(filtered)
        data = filtered.to_parquet(page_rows=1024)
        keep = np.flatnonzero(np.asarray(rec.column("v")) > 300)
        want = rec.take(pa.array(keep))
        assert 0 < len(keep) < rec.num_rows
        cases.assert_same_record(read_back(data), merge_oracle.decoded_record(want))
        assert data == pp.selftest_parquet_write(filtered.to_arrow(), page_rows=1024)
    finally:
        for rb in made:
            rb.close()
        plan.Close()


# ---- 4. refusals, allocations ------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_nothing_behind_and_the_device_usable():
    gc.collect()
    record = cases.mixed_record(1000, "alternate")
    rb = pp.ResidentBatch(record)
    try:
        before = pp.live_allocations()
        n = record.num_columns
        for kw in ({"page_rows": 63}, {"page_rows": 100}, {"page_rows": -64}, {"page_rows": (1 << 24) + 64}, {"optional": [False] * (n - 1)}, {"optional": [2] * n},
                   {"optional": {"value": False}}, {"optional": {"labels.utf8": False}}):
            with pytest.raises(pp.FdbError) as e:
                rb.to_parquet(**kw)
            assert e.value.code == pp.FDB_ERR_INVALID, kw
            assert pp.live_allocations() == before, kw   # refused before anything was allocated or launched
        assert rb.to_parquet(page_rows=64) == pp.selftest_parquet_write(record, page_rows=64)
        assert pp.live_allocations() == before           # the image and the returned bytes are gone
    finally:
        rb.close()


@pytest.mark.parametrize("kw,code,text", cases.DOUBLY_WRONG)
def test_a_doubly_wrong_call_is_refused_as_the_host_walk_refuses_it(kw, code, text):
    record = cases.mixed_record(64, "alternate")
    with pytest.raises(pp.FdbError) as host:
        pp.selftest_parquet_write(record, page_rows=cases.PAGE, **kw)
    rb = pp.ResidentBatch(record)
    try:
        before = pp.live_allocations()
        with pytest.raises(pp.FdbError) as device:
            rb.to_parquet(page_rows=cases.PAGE, **kw)
        assert pp.live_allocations() == before   # refused before anything was allocated or launched
    finally:
        rb.close()
    assert device.value.code == host.value.code == getattr(pp, code)
    assert str(device.value) == str(host.value) and text in str(device.value)


def test_everything_is_released():
    gc.collect()
    before = pp.live_allocations()
    rb = pp.ResidentBatch(cases.mixed_record(1000, "alternate"))
    for page_rows in (64, 0):
        rb.to_parquet(page_rows=page_rows)
    rb.close()
    assert pp.live_allocations() == before
