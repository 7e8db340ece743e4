"""LZ4_RAW in the Parquet writer on the device (ResidentBatch.to_parquet(compression="lz4"), codec 7 at fdb_batch_to_parquet_*): the file is
byte for byte the one the host walk writes (fdb_selftest_parquet_write_* — which tests/test_parquet_lz4_cpu.py holds against liblz4, the
project's decoder and a walker of the sequences) on the shapes where the three kernels of fdb_pqlz4.hip can go wrong — page bodies around
the block's end conditions and one and two fragments, literal runs that cross fragments and whole fragments, a page of more than 64
fragments, more fragments than the compress launch has waves, 32 LZ4 columns in one call, SNAPPY beside LZ4_RAW beside uncompressed
columns, an empty dictionary, a whole page of NULLs, no rows. The device decoder inflates every data page, a pipeline ends in an LZ4 part,
and a call without an LZ4 column marks no LZ4 pass and writes the older bytes."""
import gc
import io
import os
import re
import subprocess
import sys

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq
import pytest

from frostdb_amd import physicalplan as pp
from tests import merge_oracle, parquet_lz4_cases as Z, parquet_write_cases as cases, sort_oracle
from tests.parquet_util import row_group_chunks

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = Z.F


def check(record: pa.RecordBatch, compression, page_rows: int = 0, reread: bool = True, **kw) -> bytes:
    """to_parquet(compression) of the resident record == the host walk's file; from_parquet and pyarrow read it back to the record."""
    rb = pp.ResidentBatch(record)
    try:
        data = rb.to_parquet(page_rows=page_rows, compression=compression, **kw)
        want = pp.selftest_parquet_write(record, page_rows=page_rows, compression=compression, **kw)
        assert len(data) == len(want), (len(data), len(want))
        if data != want:
            a, b = np.frombuffer(data, dtype=np.uint8), np.frombuffer(want, dtype=np.uint8)
            diff = np.flatnonzero(a != b)
            raise AssertionError("the device's file differs from the host walk's at %d bytes, first at %s" % (len(diff), diff[:8]))
        if reread:
            cases.assert_same_record(read_back(data), record)
            if record.num_rows > 0 and "row_group_rows" not in kw:
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
    for rows in (1, 9, 64, 65, 129, 1000):  # below, at and over a wave; pages of cases.PAGE rows, a packer tile's share of them
        record = cases.mixed_record(rows, pattern)
        check(record, "lz4", page_rows=cases.PAGE)
        check(record, "lz4", page_rows=cases.PAGE, encodings={"timestamp": "delta", "count": "delta", "dense": "delta"})


def test_the_writer_s_own_shapes():
    for record in (cases.rle_record(), cases.extremes_record(), cases.duplicates_record(), cases.large_strings_record(), cases.dict_record(1000, 257)):
        check(record, "lz4", page_rows=cases.PAGE)
    check(cases.dict_record(3000, 65537), "lz4", page_rows=1024)


@pytest.mark.parametrize("kind", Z.BODY_KINDS)
def test_body_lengths(kind):
    for n_bytes in Z.BODY_LENGTHS:
        record, page_rows = Z.body_bits(n_bytes, kind)
        check(record, "lz4", page_rows=page_rows, reread=n_bytes < 8)


def test_the_shapes_of_the_rule():
    """The byte strings of the CPU tests' rule shapes, each as a page body of its own."""
    for name, payload in Z.rule_shapes().items():
        record, page_rows = Z.bytes_record(payload)
        try:
            check(record, "lz4", page_rows=page_rows, reread=False)
        except AssertionError as e:
            raise AssertionError("%s: %s" % (name, e))


@pytest.mark.parametrize("name", Z.CORPORA)
def test_the_ratio_corpora(name):
    check(pa.RecordBatch.from_arrays([Z.corpus(name)], names=["c"]), "lz4", page_rows=32768, optional=[False])


def test_a_page_of_more_than_64_fragments():
    """One page of 65 × 4 096 + 70 rows of 8 bytes: 66 fragments, noise fragments between compressible ones, so the carry is reset and
    added to across the scan's 64th fragment."""
    rows = 65 * 4096 + 70
    rng = np.random.default_rng(3)
    few = rng.integers(0, 100, rows).astype(np.int64)
    for k in (2, 3, 40, 63, 64):  # whole fragments without a match
        few[k * 4096:(k + 1) * 4096] = rng.integers(-2**62, 2**62, 4096)
    record = pa.RecordBatch.from_arrays([pa.array(few), pa.array(np.cumsum(rng.integers(0, 2000, rows)).astype(np.int64))], names=["few", "timestamp"])
    page_rows = -(-rows // 64) * 64
    assert rows * 8 > 64 * F
    check(record, "lz4", page_rows=page_rows, optional=[False, False])
    check(record, "lz4", page_rows=page_rows, encodings={"timestamp": "delta"})


def test_more_fragments_than_waves():
    """9 columns in 1 563 pages each: more (page, fragment) items than the capped compress launch has waves (2 048 workgroups of two), and
    more pages than the scan's and the gather's grids, so every strided loop goes round."""
    record = cases.mixed_record(100_000, "alternate")
    assert record.num_columns * -(-100_000 // 64) > 2 * 2048
    check(record, "lz4", page_rows=64)
    check(record, ["lz4", "snappy", None] * 3, page_rows=64)


def test_32_lz4_columns_in_one_call():
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
    check(pa.RecordBatch.from_arrays(cols, names=names), ["lz4"] * 32, page_rows=4096, encodings=encodings)


# ---- 2. mixes -------------------------------------------------------------------------------------------------------------------------------------
def test_mixes():
    record = cases.mixed_record(1000, "whole_page", dict_size=300)   # (a whole page of NULLs among its pages)
    n = record.num_columns
    mix = ["snappy", "lz4", None, "lz4", "snappy", "lz4", None, "snappy", "lz4"]
    for compression in (mix, {"timestamp": "lz4", "labels.utf8": "lz4", "flag": "snappy"}, [None] * (n - 1) + ["lz4"], ["lz4"] + [None] * (n - 1)):
        check(record, compression, page_rows=cases.PAGE, encodings={"timestamp": "delta", "dense": "delta"})
    check(record, mix, page_rows=cases.PAGE, encodings={"timestamp": "delta"}, statistics="page", bloom_filters=["labels.bin", "timestamp"], runs=True, dictionaries="used")
    check(record, mix, page_rows=64, encodings={"timestamp": "delta"}, statistics="page", bloom_filters=["labels.bin"], runs=True, dictionaries="used", row_group_rows=64)
    check(cases.empty_dictionary_record(), "lz4", page_rows=cases.PAGE)
    check(cases.rle_record(), "lz4", page_rows=cases.PAGE)
    check(cases.mixed_record(0, "none"), "lz4")
    check(cases.mixed_record(0, "none"), {"labels.utf8": "lz4"})


def test_the_device_decoder_inflates_every_data_page():
    record = cases.mixed_record(5000, "alternate")
    rb = pp.ResidentBatch(record)
    try:
        data, plain = rb.to_parquet(page_rows=1024, compression="lz4"), rb.to_parquet(page_rows=1024)
    finally:
        rb.close()
    Z.assert_compressed_file(pp, record, data, plain, "lz4", device=0)
    big = pa.RecordBatch.from_arrays([Z.corpus("integers_0_100"), Z.corpus("cumsum")], names=["a", "b"])   # pages of eight fragments
    rb = pp.ResidentBatch(big)
    try:
        data, plain = rb.to_parquet(page_rows=32768, compression="lz4"), rb.to_parquet(page_rows=32768)
    finally:
        rb.close()
    Z.assert_compressed_file(pp, big, data, plain, "lz4", device=0)


# ---- 3. a pipeline --------------------------------------------------------------------------------------------------------------------------------
def test_from_parquet_sort_to_parquet_lz4():
    rng = np.random.default_rng(71)
    n = 3000
    rec = pa.RecordBatch.from_arrays([pa.array(rng.integers(0, 10**12, n), type=pa.int64(), mask=rng.random(n) < 0.1),
                                      pa.DictionaryArray.from_arrays(pa.array(rng.integers(0, 4, n).astype(np.uint32)), pa.array([b"c", b"a", b"d", b"b"], type=pa.binary())),
                                      pa.array(rng.standard_normal(n))], names=["timestamp", "labels.a", "x"])
    made = []
    try:
        src = pp.ResidentBatch(rec)
        made.append(src)
        chunks, rows = row_group_chunks(src.to_parquet(encodings={"timestamp": "delta"}, compression="lz4"), 0)   # the part as it was written
        loaded = pp.ResidentBatch.from_parquet(chunks, rows)
        made.append(loaded)
        ordered = loaded.sort([("timestamp",)])
        made.append(ordered)
        data = ordered.to_parquet(page_rows=256, encodings={"timestamp": "delta"}, compression="lz4")
        want = rec.take(pa.array(sort_oracle.sort_indices(rec, [(0,)]), type=pa.int64()))
        cases.assert_same_record(read_back(data), merge_oracle.decoded_record(want))
        assert data == pp.selftest_parquet_write(ordered.to_arrow(), page_rows=256, encodings={"timestamp": "delta"}, compression="lz4")
        chunks, rows = row_group_chunks(data, 0)
        again = pp.ResidentBatch.from_parquet(chunks, rows)
        made.append(again)
        cases.assert_same_record(again.to_arrow(), ordered.to_arrow())
    finally:
        for rb in made:
            rb.close()


# ---- 4. the unchanged path, refusals, allocations ----------------------------------------------------------------------------------------------------
PROFILE_SCRIPT = """
import sys
from frostdb_amd import physicalplan as pp
from tests import parquet_write_cases as cases
rb = pp.ResidentBatch(cases.mixed_record(1000, "alternate"))
rb.to_parquet(page_rows=64, encodings={"timestamp": "delta"}, compression=eval(sys.argv[1]))
rb.close()
"""


def test_without_an_lz4_column_no_lz4_pass_is_launched():
    """FDB_PROFILE=1 marks every pass it waits for: `pqwrite lz compress` and `pqwrite lz gather` once each in a call with an LZ4 column,
    and in no call without — which marks what it marked before, and writes the older bytes."""
    marks = {}
    for compression in ("None", "'snappy'", "{'timestamp': 'lz4', 'value': 'snappy'}", "'lz4'"):
        r = subprocess.run([sys.executable, "-c", PROFILE_SCRIPT, compression], cwd=ROOT, env=dict(os.environ, FDB_PROFILE="1"), capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-2000:]
        marks[compression] = re.findall(r"^\[fdb\] (pqwrite [a-z ]+?)\s+[\d.]+ us$", r.stderr, flags=re.M)
    for compression in ("None", "'snappy'"):
        assert not [m for m in marks[compression] if m.startswith("pqwrite lz")], marks[compression]
    assert "pqwrite compress" not in marks["None"] and marks["'snappy'"].count("pqwrite compress") == 1 and marks["'snappy'"].count("pqwrite gather") == 1
    for compression in ("{'timestamp': 'lz4', 'value': 'snappy'}", "'lz4'"):
        assert marks[compression].count("pqwrite lz compress") == 1 and marks[compression].count("pqwrite lz gather") == 1, marks[compression]
    record = cases.mixed_record(1000, "alternate")
    rb = pp.ResidentBatch(record)
    try:
        n = record.num_columns
        assert rb.to_parquet(page_rows=64, compression=[None] * n) == rb.to_parquet(page_rows=64) == pp.selftest_parquet_write(record, page_rows=64)
        assert rb.to_parquet(page_rows=64, compression="snappy") == pp.selftest_parquet_write(record, page_rows=64, compression="snappy")
        before = pp.live_allocations()
        for compression in (["lz4"] * (n - 1), {"nobody": "lz4"}, ["lz4_raw"] + [None] * (n - 1)):
            with pytest.raises(pp.FdbError) as e:
                rb.to_parquet(compression=compression)
            assert e.value.code == pp.FDB_ERR_INVALID, compression
            assert pp.live_allocations() == before, compression
        with pytest.raises(pp.FdbError) as e:
            rb.to_parquet(encodings={"value": "delta"}, compression="lz4")
        assert e.value.code == pp.FDB_ERR_UNSUPPORTED and pp.live_allocations() == before
    finally:
        rb.close()


def test_everything_is_released():
    """Last in the module: whatever the tests above made — staging and final images, scratch, tables, returned bytes — is gone."""
    gc.collect()
    record = cases.mixed_record(1000, "alternate")
    rb = pp.ResidentBatch(record)
    for page_rows in (64, 0):
        rb.to_parquet(page_rows=page_rows, encodings={"timestamp": "delta"}, compression="lz4")
        rb.to_parquet(page_rows=page_rows, compression=["lz4", "snappy", None] * 3)
    rb.close()
    gc.collect()
    assert all(v == 0 for v in pp.live_allocations().values()), pp.live_allocations()
