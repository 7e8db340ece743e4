"""DELTA_BINARY_PACKED in the Parquet writer on the device (fdb_batch_to_parquet_encoded, ResidentBatch.to_parquet(encodings=...)): the file
is byte for byte the one the host walk writes (fdb_selftest_parquet_write_encoded — which tests/test_parquet_delta_cpu.py holds against
pyarrow's reader and the byte oracle of tests/parquet_pages.py) on the shapes where the kernels can go wrong — rows around a miniblock, a
block and two blocks, a page that spans two tiles of the compaction pass, a default page ∓, more pages and more blocks than a launch has
workgroups and waves, 32 DELTA columns in one call, a whole page of NULLs between pages of values. The project's own reader reads the
files back, and a pipeline ends in a DELTA column as a compacted part does."""
import gc
import io

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq
import pytest

from frostdb_amd import physicalplan as pp
from tests import merge_oracle, parquet_write_cases as cases, sort_oracle
from tests.parquet_util import row_group_chunks
from tests.test_parquet_delta_cpu import families

pytestmark = pytest.mark.gpu


def check(record: pa.RecordBatch, encodings, page_rows: int = 0, reread: bool = True) -> bytes:
    """to_parquet(encodings) of the resident record == the host walk's file; from_parquet reads it back to the record."""
    rb = pp.ResidentBatch(record)
    try:
        data = rb.to_parquet(page_rows=page_rows, encodings=encodings)
        want = pp.selftest_parquet_write(record, page_rows=page_rows, encodings=encodings)
        assert len(data) == len(want), (len(data), len(want))
        if data != want:
            a, b = np.frombuffer(data, dtype=np.uint8), np.frombuffer(want, dtype=np.uint8)
            diff = np.flatnonzero(a != b)
            raise AssertionError("the device's file differs from the host walk's at %d bytes, first at %s" % (len(diff), diff[:8]))
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


def read_back(data: bytes) -> pa.RecordBatch:
    t = pq.read_table(io.BytesIO(data)).combine_chunks()
    return pa.RecordBatch.from_arrays([c.chunk(0) if c.num_chunks else pa.array([], type=c.type) for c in t.columns], names=t.schema.names)


def shapes_record(rows: int, pattern: str, page: int, widths=(0, 1, 7, 31, 32, 33, 63, 64)) -> pa.RecordBatch:
    """The value families of the CPU tests (every named one, a spread of the exact-width ones), int64 and uint64 by turns, each once
    with the NULL pattern and — the first four — once without NULLs, beside a float64 and a dictionary column that stay as they are."""
    valid = cases.valid_mask(rows, pattern, page)
    keep = {"w%02d" % w for w in widths}
    cols, names = [], []
    for k, (name, bits) in enumerate((n, b) for n, b in families(rows) if not n.startswith("w") or n in keep):
        typ = pa.int64() if k % 2 == 0 else pa.uint64()
        cols.append(pa.array(bits.view(np.int64) if k % 2 == 0 else bits, type=typ, mask=~valid))
        names.append("d." + name)
        if k < 4:
            cols.append(pa.array(bits.view(np.int64) if k % 2 == 0 else bits, type=typ))
            names.append("dense." + name)
    rng = np.random.default_rng(rows)
    cols.append(pa.array(rng.standard_normal(rows), mask=~valid))
    names.append("value")
    cols.append(pa.DictionaryArray.from_arrays(pa.array(rng.integers(0, 5, rows).astype(np.uint32), mask=~valid), pa.array(cases.dict_entries(5, True), type=pa.string())))
    names.append("labels.l")
    return pa.RecordBatch.from_arrays(cols, names=names)


def delta_of(record: pa.RecordBatch):
    return {n: "delta" for n in record.schema.names if n.startswith("d")}


# ---- 1. identity with the host walk ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", cases.NULL_PATTERNS)
def test_rows_around_a_miniblock_a_block_and_two_blocks(pattern):
    for rows in (1, 2, 33, 34, 129, 130, 258):
        for page_rows in (64, 192):
            record = shapes_record(rows, pattern, page_rows)
            check(record, delta_of(record), page_rows=page_rows)


@pytest.mark.parametrize("pattern", ["none", "alternate", "first_of_page"])
def test_a_page_that_spans_two_tiles(pattern):
    record = shapes_record(4097, pattern, 4160)
    check(record, delta_of(record), page_rows=4160)


@pytest.mark.parametrize("pattern", ["none", "alternate", "whole_page"])
def test_a_default_page_and_a_short_one(pattern):
    record = shapes_record(70001, pattern, 65536, widths=(0, 11, 64))
    check(record, delta_of(record))


def test_more_pages_than_workgroups():
    """70 000 rows in pages of 64: 1 094 pages per column — with 17 DELTA columns more (column, page) and (column, page, block) items than
    any of the capped launches has workgroups × waves, so every strided loop goes round."""
    record = shapes_record(70000, "alternate", 64, widths=(0, 11, 64))
    assert sum(n.startswith("d") for n in record.schema.names) * -(-70000 // 64) > 4 * 1024
    check(record, delta_of(record), page_rows=64)


def test_32_delta_columns_in_one_call():
    rows = 20011
    rng = np.random.default_rng(32)
    cols, names = [], []
    for k in range(32):
        step = [1, 3, 2000, 2**20, 2**40, 2**62][k % 6]
        v = np.cumsum(rng.integers(-step if k % 4 == 3 else 0, step, rows, dtype=np.int64))
        valid = rng.random(rows) < (0.5 + 0.5 * (k % 3 == 0))
        cols.append(pa.array(v if k % 2 == 0 else v.view(np.uint64), mask=~valid))
        names.append("d%02d" % k)
    record = pa.RecordBatch.from_arrays(cols, names=names)
    check(record, ["delta"] * 32, page_rows=4096)


def test_a_whole_page_of_nulls_between_pages_of_values():
    rows = 3 * 256 + 17
    valid = np.ones(rows, dtype=bool)
    valid[256:512] = False
    ts = np.cumsum(np.random.default_rng(5).integers(0, 2000, rows, dtype=np.int64))
    record = pa.RecordBatch.from_arrays([pa.array(ts, mask=~valid), pa.array(ts.view(np.uint64) + np.uint64(2**63), mask=~valid)], names=["timestamp", "count"])
    data = check(record, ["delta", "delta"], page_rows=256)
    cases.assert_same_record(read_back(data), record)   # pyarrow's reader too


# ---- 2. a pipeline ------------------------------------------------------------------------------------------------------------------------------
def test_from_parquet_sort_to_parquet_with_the_sorting_column_delta():
    rng = np.random.default_rng(71)
    n = 3000
    rec = pa.RecordBatch.from_arrays([pa.array(rng.integers(0, 10**12, n), type=pa.int64(), mask=rng.random(n) < 0.1),
                                      pa.DictionaryArray.from_arrays(pa.array(rng.integers(0, 4, n).astype(np.uint32)), pa.array([b"c", b"a", b"d", b"b"], type=pa.binary())),
                                      pa.array(rng.standard_normal(n))], names=["timestamp", "labels.a", "x"])
    made = []
    try:
        src = pp.ResidentBatch(rec)
        made.append(src)
        chunks, rows = row_group_chunks(src.to_parquet(encodings={"timestamp": "delta"}), 0)   # the part as it was written: DELTA already
        loaded = pp.ResidentBatch.from_parquet(chunks, rows)
        made.append(loaded)
        ordered = loaded.sort([("timestamp",)])
        made.append(ordered)
        data = ordered.to_parquet(page_rows=256, encodings={"timestamp": "delta"})
        want = rec.take(pa.array(sort_oracle.sort_indices(rec, [(0,)]), type=pa.int64()))
        cases.assert_same_record(read_back(data), merge_oracle.decoded_record(want))
        assert data == pp.selftest_parquet_write(ordered.to_arrow(), page_rows=256, encodings={"timestamp": "delta"})
        assert len(data) < len(ordered.to_parquet(page_rows=256))   # sorted: the deltas are narrower than the values
    finally:
        for rb in made:
            rb.close()


# ---- 3. refusals, allocations ---------------------------------------------------------------------------------------------------------------------
def test_refusals_come_before_any_launch_and_leave_nothing_behind():
    gc.collect()
    record = cases.mixed_record(1000, "alternate")
    rb = pp.ResidentBatch(record)
    try:
        before = pp.live_allocations()
        n = record.num_columns
        for encodings, code in (({"value": "delta"}, pp.FDB_ERR_UNSUPPORTED), ({"flag": "delta"}, pp.FDB_ERR_UNSUPPORTED), ({"labels.utf8": "delta"}, pp.FDB_ERR_UNSUPPORTED),
                                ({"plain_str": "delta"}, pp.FDB_ERR_UNSUPPORTED), (["delta"] * (n - 1), pp.FDB_ERR_INVALID), ({"nobody": "delta"}, pp.FDB_ERR_INVALID),
                                (["zstd"] + [None] * (n - 1), pp.FDB_ERR_INVALID)):
            with pytest.raises(pp.FdbError) as e:
                rb.to_parquet(encodings=encodings)
            assert e.value.code == code, encodings
            assert pp.live_allocations() == before, encodings
        assert rb.to_parquet(page_rows=64, encodings=[None] * n) == rb.to_parquet(page_rows=64)
        assert pp.live_allocations() == before
    finally:
        rb.close()


def test_everything_is_released():
    """Last in the module: whatever the tests above made — scratch, tables, images, returned bytes — is gone."""
    gc.collect()
    record = cases.mixed_record(1000, "alternate")
    rb = pp.ResidentBatch(record)
    for page_rows in (64, 0):
        rb.to_parquet(page_rows=page_rows, encodings={"timestamp": "delta", "count": "delta", "dense": "delta"})
    rb.close()
    gc.collect()
    assert all(v == 0 for v in pp.live_allocations().values()), pp.live_allocations()
