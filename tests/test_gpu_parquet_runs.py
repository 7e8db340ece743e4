"""RLE runs inside index and level pages, written on the device (fdb_batch_to_parquet_runs, ResidentBatch.to_parquet(runs=...)): the file
is byte for byte the one the host walk writes (fdb_selftest_parquet_write_runs — which tests/test_parquet_runs_cpu.py holds against a
restatement of the rule, a hybrid decoder and pyarrow) at the edges of the kernels: a stretch across a tile boundary (row 4 096) and one
that ends on it, a page of two tiles with a short last tile, NULLs that put a tile's first rank 1 … 7 past a group boundary, a tile of
NULLs between tiles of values, more (stream, page) items than a launch has workgroups, 32 run-encoded columns in one call, a dictionary
of 65 537 entries (T = 1), runs across the chunks the walk takes a page in, and runs mixed with SNAPPY, DELTA, the page index and bloom
filters. pyarrow and the project's own reader read every file back."""
import gc
import os
import re

import numpy as np
import pyarrow as pa
import pytest

from frostdb_amd import physicalplan as pp
from tests import parquet_runs_cases as R, parquet_write_cases as cases, sort_oracle
from tests.parquet_util import row_group_chunks

pytestmark = pytest.mark.gpu
MAX_GRID = int(re.search(r"^#define FDB_PQW_MAX_GRID (\d+)", open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "frostdb_amd", "csrc", "fdb_pqwrite.h")).read(), flags=re.M).group(1))
TILE = 4096
CHUNK = 8 * int(re.search(r"^#define FDB_PQR_CHUNK (\d+)", open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "frostdb_amd", "csrc", "fdb_pqruns.h")).read(), flags=re.M).group(1))  # symbols a workgroup takes at a step


def check(record: pa.RecordBatch, runs=True, page_rows: int = R.PAGE, reread: bool = True, rules: bool = False, **kw) -> bytes:
    """to_parquet(runs) of the resident record == the host walk's file; pyarrow and from_parquet read it back. `rules`: the file is
    also held to the restatement (the CPU tests do that for the host walk; here for the shapes only this module has)."""
    rb = pp.ResidentBatch(record)
    try:
        data = rb.to_parquet(page_rows=page_rows, runs=runs, **kw)
        want = pp.selftest_parquet_write(record, page_rows=page_rows, runs=runs, **kw)
        assert len(data) == len(want), (len(data), len(want))
        if data != want:
            a, b = np.frombuffer(data, dtype=np.uint8), np.frombuffer(want, dtype=np.uint8)
            diff = np.flatnonzero(a != b)
            raise AssertionError("the device's file differs from the host walk's at %d bytes, first at %s" % (len(diff), diff[:8]))
        if rules:
            plain = pp.selftest_parquet_write(record, page_rows=page_rows, **kw)
            assert R.assert_runs_file(record, data, plain, page_rows, R.flags_of(record, runs)) > 0
        if reread:
            cases.assert_same_record(R.read_back(data), record)
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


def stretches(rows: int, spans, hi: int, seed: int = 0) -> np.ndarray:
    """Indices below hi without a uniform group, but for [first, end) spans of hi − 1."""
    idx = R.noise(np.random.default_rng(seed), rows, hi)
    for a, b in spans:
        idx[a:b] = hi - 1
    return idx


# ---- 1. identity with the host walk at the kernels' edges ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", R.WIDTHS)
def test_every_width_and_stretch_length(w):
    for pattern in (None, "first_of_page", "alternate"):
        check(R.width_record(w, pattern), page_rows=R.page_for(w), rules=pattern is None, reread=pattern != "alternate")


def test_tails_of_every_length():
    for w in (1, 3, 9, 17):
        for sym, _what in R.tail_pieces(w):
            check(pa.RecordBatch.from_arrays([R._dict(sym, R.entries_for(w))], names=["d"]), page_rows=256, reread=False)


@pytest.mark.parametrize("pattern", cases.NULL_PATTERNS)
def test_levels_under_the_null_patterns(pattern):
    for rows in (65, 1000, TILE + 1):
        check(R.levels_record(cases.valid_mask(rows, pattern)), page_rows=R.PAGE if rows < TILE else 2 * TILE)
    for stretch in (127, 128, 129):
        check(R.levels_record(R.clustered_valid(3000, stretch)), page_rows=1024, rules=True)


def test_a_stretch_across_a_tile_boundary_and_one_that_ends_on_it():
    rows = 2 * TILE + 200
    for w in (1, 5, 17):
        hi, T = R.entries_for(w), R.threshold(w)
        for spans in ([(TILE - 800, TILE + 640)], [(TILE - 800, TILE)], [(TILE, TILE + 640)], [(TILE - 8 * T, TILE + 8 * T)], [(TILE - 8 * T, TILE)], [(100, 2 * TILE + 100)]):
            record = pa.RecordBatch.from_arrays([R._dict(stretches(rows, spans, hi, w), hi), pa.array(np.arange(rows, dtype=np.int64))], names=["labels.s", "timestamp"])
            check(record, page_rows=4 * TILE, rules=True, reread=w == 5)


def test_a_page_of_two_tiles_and_a_short_last_tile():
    rows = 2 * 8192 + TILE + 100
    for pattern in ("none", "first_of_page", "alternate"):
        valid = cases.valid_mask(rows, pattern, 8192)
        hi = 300
        idx = stretches(rows, [(1000, 5000), (8192 + 4000, 8192 + 4200), (2 * 8192 + TILE - 64, rows)], hi, 3)
        record = pa.RecordBatch.from_arrays([R._dict(idx, hi, valid, utf8=True), pa.array(np.arange(rows, dtype=np.int64), mask=~valid)], names=["labels.t", "timestamp"])
        check(record, page_rows=8192, rules=pattern != "alternate")


@pytest.mark.parametrize("shift", range(1, 8))
def test_a_tile_whose_first_rank_is_past_a_group_boundary(shift):
    """`shift` NULLs in the first tile: the second tile's first value has rank 4 096 − shift, which is `8 − shift` past a group
    boundary, and a stretch runs across it."""
    rows = 3 * TILE
    valid = np.ones(rows, bool)
    valid[np.arange(shift) * 37 + 5] = False
    hi = 9
    idx = stretches(rows, [(TILE - 1000, TILE + 1000), (2 * TILE - 16, 2 * TILE + 16)], hi, shift)
    record = pa.RecordBatch.from_arrays([R._dict(idx, hi, valid)], names=["labels.r"])
    check(record, page_rows=3 * TILE, rules=True)


def test_a_tile_of_nulls_between_tiles_of_values():
    rows = 3 * TILE + 33
    r = np.arange(rows)
    middle, edges = (r // TILE) != 1, (r // TILE) == 1
    hi = 40
    idx = stretches(rows, [(TILE - 500, 2 * TILE + 500), (3 * TILE - 8, rows)], hi, 9)
    record = pa.RecordBatch.from_arrays([R._dict(idx, hi, middle, utf8=True), R._dict(idx, hi, edges, utf8=True), pa.array(r, mask=~middle)], names=["d", "d2", "i"])
    check(record, page_rows=3 * TILE, rules=True)
    check(record, page_rows=8192, compression="snappy", encodings={"i": "delta"}, statistics="page", reread=False)


def test_more_items_than_workgroups():
    """Pages of 64 rows × 17 columns: more (stream, page) items than the launch has workgroups, every workgroup strides."""
    rows = 64 * (MAX_GRID // 17 + 3)
    rng = np.random.default_rng(4)
    valid = R.clustered_valid(rows, 40)
    cols = [R._dict(stretches(rows, [(k * 50, k * 50 + 300), (rows - 200 - k, rows - k)], 300, k), 300, valid if k % 2 else None) for k in range(16)]
    cols.append(pa.array(rng.integers(0, 9, rows), mask=~valid))
    record = pa.RecordBatch.from_arrays(cols, names=["labels.c%02d" % k for k in range(16)] + ["i"])
    assert 25 * (rows // 64) > MAX_GRID   # 16 index streams, 9 level streams
    check(record, rules=True)


def test_32_run_encoded_columns_in_one_call():
    rows = 2 * TILE + 77
    valid = R.clustered_valid(rows, 129)
    cols = [R._dict(stretches(rows, [(k * 97, k * 97 + 64 * (k + 1))], 2 + k, k), 2 + k, valid if k % 3 == 0 else None, utf8=k % 2 == 0) for k in range(32)]
    record = pa.RecordBatch.from_arrays(cols, names=["labels.c%02d" % k for k in range(32)])
    check(record, page_rows=TILE)
    check(record, runs={"labels.c%02d" % k: ("values", "levels", True)[k % 3] for k in range(32)}, page_rows=2048, compression="snappy", reread=False)


def test_a_dictionary_of_65537_entries():
    rows = 70000
    idx = np.arange(rows) % 65537
    idx[100:108], idx[5000:5007], idx[60000:66000] = 65536, 65536, 7   # one group (T = 1: an RLE run), seven symbols (none), a long stretch
    record = pa.RecordBatch.from_arrays([R._dict(idx, 65537, cases.valid_mask(rows, "first_of_page", 65536))], names=["labels.big"])
    check(record, page_rows=65536, rules=True)


def test_runs_across_the_chunks_of_the_walk():
    """Runs that start, end and lie across the walk's chunks (FDB_PQR_CHUNK groups, counted from the page's END) and their halos; RLE
    counts and bit-packed runs where the header's varint grows."""
    rows = 5 * CHUNK
    C = CHUNK
    for w, spans in ((1, [(C - 128, C), (2 * C, 2 * C + 128), (2 * C + 300, 2 * C + 500), (3 * C - 64, 3 * C + 64), (3 * C + 200, 3 * C + 200 + 8 * 8191 if C > 8 * 8191 else 4 * C - 8), (4 * C + 8, rows - 16)]),
                     (8, [(0, 8 * 63), (8 * 64, 8 * 64 + 63), (8 * 128, 8 * 128 + 64), (C - 16, C + 16), (2 * C - 8, 2 * C + 8), (3 * C - 8 * 15, 3 * C), (3 * C + 8, 3 * C + 8 + 8192), (4 * C, 4 * C + 16)]),
                     (17, [(C - 8, C), (C, C + 8), (2 * C - 8, 2 * C), (3 * C - 24, 3 * C + 8191), (rows - 2770, rows)])):
        hi = R.entries_for(w)
        record = pa.RecordBatch.from_arrays([R._dict(stretches(rows, spans, hi, w), hi)], names=["labels.x"])
        check(record, page_rows=rows, rules=True, reread=False)                 # page ends on a chunk boundary
        check(record.slice(0, rows - 8 * 37 - 3), page_rows=rows, reread=False)  # … and 37 groups and 3 symbols before one
        check(record, page_rows=rows // 2 // 64 * 64, reread=False)


MIXES = [dict(compression="snappy"), dict(encodings={"timestamp": "delta"}), dict(statistics="page", sorting_columns=[("labels.a",), ("labels.b",)]),
         dict(bloom_filters=["labels.a", "timestamp"]),
         dict(encodings={"timestamp": "delta"}, compression=["snappy", None, "snappy", None, "snappy"], statistics="page", sorting_columns=[("labels.a",)], bloom_filters=["labels.b"])]


@pytest.mark.parametrize("k", range(len(MIXES)))
def test_runs_mixed_with_the_other_options(k):
    record = R.sorted_record(10000)
    check(record, page_rows=1024, **MIXES[k])
    check(R.sorted_record(TILE + 100, seed=k), page_rows=8192, reread=False, **MIXES[k])


def test_from_parquet_sort_to_parquet_runs():
    """from_parquet → sort → to_parquet(runs=True, sorting_columns=…) → from_parquet equals the Sort's restatement
    (tests/sort_oracle.py)."""
    rng = np.random.default_rng(71)
    n = 9000
    rec = pa.RecordBatch.from_arrays([pa.DictionaryArray.from_arrays(pa.array(rng.integers(0, 4, n).astype(np.uint32)), pa.array([b"c", b"a", b"d", b"b", b"unused"], type=pa.binary())),
                                      pa.DictionaryArray.from_arrays(pa.array(rng.integers(0, 50, n).astype(np.uint32), mask=rng.random(n) < 0.3), pa.array(["v%02d" % i for i in range(50)], type=pa.string())),
                                      pa.array(rng.permutation(n).astype(np.int64)), pa.array(rng.standard_normal(n), mask=rng.random(n) < 0.1)], names=["labels.a", "labels.b", "timestamp", "x"])
    made = []
    try:
        src = pp.ResidentBatch(rec)
        made.append(src)
        chunks, rows = row_group_chunks(src.to_parquet(runs=True), 0)
        loaded = pp.ResidentBatch.from_parquet(chunks, rows)
        made.append(loaded)
        ordered = loaded.sort([("labels.a",), ("labels.b",), ("timestamp",)])
        made.append(ordered)
        kw = dict(page_rows=4096, runs=True, statistics="page", sorting_columns=[("labels.a",), ("labels.b",), ("timestamp",)])
        data = ordered.to_parquet(**kw)
        back = ordered.to_arrow()
        assert data == pp.selftest_parquet_write(back, **kw)
        plain = ordered.to_parquet(**{k: v for k, v in kw.items() if k != "runs"})
        assert len(data) < len(plain)
        chunks, rows = row_group_chunks(data, 0)
        again = pp.ResidentBatch.from_parquet(chunks, rows)
        made.append(again)
        order = sort_oracle.sort_indices(rec, [0, 1, 2])
        want = rec.take(pa.array(order))
        cases.assert_same_record(again.to_arrow(), want)
        cases.assert_same_record(R.read_back(data), want)
    finally:
        for rb in made:
            rb.close()


# ---- 2. the unchanged path, refusals, allocations ---------------------------------------------------------------------------------------------------
def test_without_runs_the_bytes_are_the_older_ones():
    gc.collect()
    record = cases.mixed_record(1000, "alternate")
    rb = pp.ResidentBatch(record)
    try:
        for kw in (dict(), dict(encodings={"timestamp": "delta"}, compression="snappy"), dict(statistics="page", bloom_filters=["timestamp"])):
            old = rb.to_parquet(page_rows=64, **kw)
            assert rb.to_parquet(page_rows=64, runs=None, **kw) == old
            assert rb.to_parquet(page_rows=64, runs=[], **kw) == old
            assert rb.to_parquet(page_rows=64, runs={"timestamp": None, "labels.utf8": None}, **kw) == old
        before = pp.live_allocations()
        for kw, code in ((dict(runs=["nobody"]), pp.FDB_ERR_INVALID), (dict(runs={"timestamp": "both"}), pp.FDB_ERR_INVALID), (dict(runs="labels.utf8"), pp.FDB_ERR_INVALID),
                         (dict(runs=True, page_rows=100), pp.FDB_ERR_INVALID), (dict(runs=["timestamp"]), pp.FDB_ERR_UNSUPPORTED), (dict(runs={"flag": "values"}), pp.FDB_ERR_UNSUPPORTED)):
            with pytest.raises(pp.FdbError) as e:
                rb.to_parquet(**kw)
            assert e.value.code == code and pp.live_allocations() == before, kw
    finally:
        rb.close()


def test_everything_is_released():
    """Last in the module: whatever the tests above made — dense indices, tables of sizes and offsets, images, returned bytes — is gone."""
    gc.collect()
    record = R.sorted_record(5000)
    rb = pp.ResidentBatch(record)
    for page_rows in (64, 0):
        rb.to_parquet(page_rows=page_rows, runs=True, encodings={"timestamp": "delta"}, compression="snappy", statistics="page", bloom_filters=["labels.a"])
        rb.to_parquet(page_rows=page_rows, runs={"labels.b": "levels", "labels.a": "values"})
    rb.close()
    gc.collect()
    assert all(v == 0 for v in pp.live_allocations().values()), pp.live_allocations()
