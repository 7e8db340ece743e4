"""SNAPPY in the Parquet writer on the device (fdb_batch_to_parquet_compressed, ResidentBatch.to_parquet(compression=...)): the file is byte
for byte the one the host walk writes (fdb_selftest_parquet_write_compressed — which tests/test_parquet_snappy_cpu.py holds against
pyarrow, both Snappy decoders and a walker of the elements) on the shapes where the kernels can go wrong — page bodies around one and two
fragments, a page of many fragments, more fragments than a launch has waves, 32 compressed columns in one call, compressed beside
uncompressed columns, DELTA + SNAPPY on one column, an empty dictionary, a whole page of NULLs, no rows. The project's own reader and
pyarrow read the files back, the device decoder inflates every data page, and a pipeline ends in a compressed part."""
import gc
import io

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq
import pytest

from frostdb_amd import physicalplan as pp
from tests import merge_oracle, parquet_snappy_cases as S, parquet_write_cases as cases, sort_oracle
from tests.parquet_util import row_group_chunks
from tests.test_parquet_snappy_cpu import corpus, CORPORA

pytestmark = pytest.mark.gpu
F = S.FRAGMENT


def check(record: pa.RecordBatch, compression, page_rows: int = 0, encodings=None, reread: bool = True, optional=None) -> bytes:
    """to_parquet(compression) of the resident record == the host walk's file; from_parquet and pyarrow read it back to the record."""
    rb = pp.ResidentBatch(record)
    try:
        data = rb.to_parquet(page_rows=page_rows, optional=optional, encodings=encodings, compression=compression)
        want = pp.selftest_parquet_write(record, page_rows=page_rows, optional=optional, encodings=encodings, compression=compression)
        assert len(data) == len(want), (len(data), len(want))
        if data != want:
            a, b = np.frombuffer(data, dtype=np.uint8), np.frombuffer(want, dtype=np.uint8)
            diff = np.flatnonzero(a != b)
            raise AssertionError("the device's file differs from the host walk's at %d bytes, first at %s" % (len(diff), diff[:8]))
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


def read_back(data: bytes) -> pa.RecordBatch:
    t = pq.read_table(io.BytesIO(data)).combine_chunks()
    return pa.RecordBatch.from_arrays([c.chunk(0) if c.num_chunks else pa.array([], type=c.type) for c in t.columns], names=t.schema.names)


# ---- 1. identity with the host walk ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", cases.NULL_PATTERNS)
def test_every_kind_under_every_null_pattern(pattern):
    for rows in (1, 9, 64, 65, 129, 1000):
        record = cases.mixed_record(rows, pattern)
        check(record, "snappy", page_rows=cases.PAGE)
        check(record, "snappy", page_rows=cases.PAGE, encodings={"timestamp": "delta", "count": "delta", "dense": "delta"})


@pytest.mark.parametrize("n_bytes", [1, 3, 4, 5, F - 1, F, F + 1, 2 * F - 1, 2 * F, 2 * F + 1])
def test_bodies_around_one_and_two_fragments(n_bytes):
    record, page_rows = S.bits_record(n_bytes)
    check(record, "snappy", page_rows=page_rows, reread=n_bytes < 8)
    rows = n_bytes // 8 + 1
    numbers = pa.RecordBatch.from_arrays([pa.array(np.random.default_rng(n_bytes).integers(0, 1000, rows).astype(np.int64), mask=np.arange(rows) % 9 == 4)], names=["c"])
    check(numbers, "snappy", page_rows=-(-rows // 64) * 64)


def test_the_shapes_of_the_rule():
    """The byte strings of the CPU tests' rule shapes, each as a page body: match and literal lengths, offsets at the one-byte form's edge,
    runs of every period starting mid-window, a match at and over the fragment's end, incompressible fragments."""
    payloads = []
    for literal in (60, 61, 256, 257):
        a = S.noise(literal, literal)
        for length in (4, 11, 12, 64, 65, 68, 129):
            again = bytes(a[literal - 8 + i % 8] for i in range(length))
            payloads.append(a + again + S.noise(literal + 1000, 8 + (-(literal + length)) % 8))
    for offset in (2047, 2048):
        a = S.noise(offset, offset)
        payloads.append(a + a[:8] + S.noise(offset + 1, 8 + (-(offset + 8)) % 8))
    for period in (1, 2, 3, 4, 5, 7, 8, 13, 15, 16, 17, 63, 64, 65):
        unit = S.noise(period, period)
        payloads.append(S.noise(12, 100) + (unit * 300)[:300] + S.noise(13, 8))
    a = S.noise(6, F - 40)
    payloads.append(a + a[-200:-160] + S.noise(7, 64))
    a = S.noise(8, F - 24)
    payloads.append(a + a[-200:-120] + S.noise(9, 8))
    payloads.append(S.noise(5, 2 * F))
    payloads.append(bytes(8 * F))  # one run over eight fragments
    cols = [pa.array(np.frombuffer(p, dtype=np.int64)) for p in payloads]
    for c in cols:  # each alone in a page of its own size
        check(pa.RecordBatch.from_arrays([c], names=["bytes"]), "snappy", page_rows=-(-len(c) // 64) * 64, reread=False)


@pytest.mark.parametrize("name", CORPORA)
def test_the_ratio_corpora(name):
    check(pa.RecordBatch.from_arrays([corpus(name)], names=["c"]), "snappy", page_rows=32768, optional=[False])


def test_a_page_of_many_fragments():
    rows = 65536 + 70
    rng = np.random.default_rng(3)
    record = pa.RecordBatch.from_arrays([pa.array(rng.integers(0, 100, rows).astype(np.int64)), pa.array(rng.standard_normal(rows), mask=rng.random(rows) < 0.3),
                                         pa.array(np.cumsum(rng.integers(0, 2000, rows)).astype(np.int64))], names=["few", "value", "timestamp"])
    check(record, "snappy", page_rows=65536, encodings={"timestamp": "delta"})


def test_more_fragments_than_waves():
    """9 columns in 1 563 pages each: more (page, fragment) items than the capped compress launch has waves (2 048 workgroups of two), and
    more pages than the scan's, so every strided loop goes round; the gather's too."""
    record = cases.mixed_record(100_000, "alternate")
    assert record.num_columns * -(-100_000 // 64) > 2 * 2048
    check(record, "snappy", page_rows=64)
    check(record, ["snappy", None] * 4 + ["snappy"], page_rows=64)


def test_32_compressed_columns_in_one_call():
    rows = 20011
    rng = np.random.default_rng(32)
    cols, names, encodings = [], [], []
    for k in range(32):
        step = [1, 3, 2000, 2**20, 2**40, 2**62][k % 6]
        v = np.cumsum(rng.integers(0, step, rows, dtype=np.int64))
        valid = rng.random(rows) < (0.5 + 0.5 * (k % 3 == 0))
        cols.append(pa.array(v if k % 2 == 0 else v.view(np.uint64), mask=~valid))
        names.append("c%02d" % k)
        encodings.append("delta" if k % 4 == 1 else None)
    check(pa.RecordBatch.from_arrays(cols, names=names), ["snappy"] * 32, page_rows=4096, encodings=encodings)


# ---- 2. mixes -------------------------------------------------------------------------------------------------------------------------------------
def test_mixes():
    record = cases.mixed_record(1000, "whole_page")
    n = record.num_columns
    for compression in ({"timestamp": "snappy", "labels.utf8": "snappy"}, [None] * (n - 1) + ["snappy"], ["snappy"] + [None] * (n - 1), ["snappy", None] * 4 + ["snappy"]):
        check(record, compression, page_rows=cases.PAGE, encodings={"timestamp": "delta", "dense": "delta"})
    check(cases.empty_dictionary_record(), "snappy", page_rows=cases.PAGE)
    check(cases.rle_record(), "snappy", page_rows=cases.PAGE)
    check(cases.dict_record(3000, 65537), "snappy", page_rows=1024)
    check(cases.mixed_record(0, "none"), "snappy")
    check(cases.mixed_record(0, "none"), {"labels.utf8": "snappy"})


def test_the_device_decoder_inflates_every_data_page():
    record = cases.mixed_record(5000, "alternate")
    rb = pp.ResidentBatch(record)
    try:
        data, plain = rb.to_parquet(page_rows=1024, compression="snappy"), rb.to_parquet(page_rows=1024)
    finally:
        rb.close()
    S.assert_compressed_file(pp, record, data, plain, "snappy", device=0)
    big = pa.RecordBatch.from_arrays([corpus("integers_0_100"), corpus("cumsum")], names=["a", "b"])   # pages of eight fragments
    rb = pp.ResidentBatch(big)
    try:
        data, plain = rb.to_parquet(page_rows=32768, compression="snappy"), rb.to_parquet(page_rows=32768)
    finally:
        rb.close()
    S.assert_compressed_file(pp, big, data, plain, "snappy", device=0)


# ---- 3. a pipeline --------------------------------------------------------------------------------------------------------------------------------
def test_from_parquet_sort_to_parquet_compressed():
    rng = np.random.default_rng(71)
    n = 3000
    rec = pa.RecordBatch.from_arrays([pa.array(rng.integers(0, 10**12, n), type=pa.int64(), mask=rng.random(n) < 0.1),
                                      pa.DictionaryArray.from_arrays(pa.array(rng.integers(0, 4, n).astype(np.uint32)), pa.array([b"c", b"a", b"d", b"b"], type=pa.binary())),
                                      pa.array(rng.standard_normal(n))], names=["timestamp", "labels.a", "x"])
    made = []
    try:
        src = pp.ResidentBatch(rec)
        made.append(src)
        chunks, rows = row_group_chunks(src.to_parquet(encodings={"timestamp": "delta"}, compression="snappy"), 0)   # the part as it was written
        loaded = pp.ResidentBatch.from_parquet(chunks, rows)
        made.append(loaded)
        ordered = loaded.sort([("timestamp",)])
        made.append(ordered)
        data = ordered.to_parquet(page_rows=256, encodings={"timestamp": "delta"}, compression="snappy")
        want = rec.take(pa.array(sort_oracle.sort_indices(rec, [(0,)]), type=pa.int64()))
        cases.assert_same_record(read_back(data), merge_oracle.decoded_record(want))
        assert data == pp.selftest_parquet_write(ordered.to_arrow(), page_rows=256, encodings={"timestamp": "delta"}, compression="snappy")
        chunks, rows = row_group_chunks(data, 0)
        again = pp.ResidentBatch.from_parquet(chunks, rows)
        made.append(again)
        cases.assert_same_record(again.to_arrow(), ordered.to_arrow())
    finally:
        for rb in made:
            rb.close()


# ---- 4. the unchanged path, refusals, allocations ----------------------------------------------------------------------------------------------------
def test_without_codecs_the_path_and_the_bytes_are_the_older_ones():
    gc.collect()
    record = cases.mixed_record(1000, "alternate")
    rb = pp.ResidentBatch(record)
    try:
        n = record.num_columns
        enc = {"timestamp": "delta"}
        old, old_delta = rb.to_parquet(page_rows=64), rb.to_parquet(page_rows=64, encodings=enc)
        assert old == pp.selftest_parquet_write(record, page_rows=64) and old_delta == pp.selftest_parquet_write(record, page_rows=64, encodings=enc)
        for compression in (None, [None] * n, ["uncompressed"] * n, {}, {"value": "uncompressed"}):
            assert rb.to_parquet(page_rows=64, compression=compression) == old
            assert rb.to_parquet(page_rows=64, encodings=enc, compression=compression) == old_delta
        before = pp.live_allocations()
        for compression, code in ((["snappy"] * (n - 1), pp.FDB_ERR_INVALID), ({"nobody": "snappy"}, pp.FDB_ERR_INVALID), (["zstd"] + [None] * (n - 1), pp.FDB_ERR_INVALID)):
            with pytest.raises(pp.FdbError) as e:
                rb.to_parquet(compression=compression)
            assert e.value.code == code, compression
            assert pp.live_allocations() == before, compression
        with pytest.raises(pp.FdbError) as e:
            rb.to_parquet(encodings={"value": "delta"}, compression="snappy")
        assert e.value.code == pp.FDB_ERR_UNSUPPORTED and pp.live_allocations() == before
    finally:
        rb.close()


def test_everything_is_released():
    """Last in the module: whatever the tests above made — staging and final images, scratch, tables, returned bytes — is gone."""
    gc.collect()
    record = cases.mixed_record(1000, "alternate")
    rb = pp.ResidentBatch(record)
    for page_rows in (64, 0):
        rb.to_parquet(page_rows=page_rows, encodings={"timestamp": "delta"}, compression="snappy")
    rb.close()
    gc.collect()
    assert all(v == 0 for v in pp.live_allocations().values()), pp.live_allocations()
