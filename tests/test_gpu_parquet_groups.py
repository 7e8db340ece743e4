"""Several row groups and dictionaries of used entries only, written on the device (fdb_batch_to_parquet_grouped,
ResidentBatch.to_parquet(row_group_rows=…, dictionaries="used")): the file is byte for byte the one the host walk writes
(fdb_selftest_parquet_write_grouped — which tests/test_parquet_groups_cpu.py holds against a restatement of the rule, the files of the
row slices alone and pyarrow) at the edges of the present and remap kernels (fdb_pqdict.hip): rows 1, 63, 64, 65 and around a tile
(4 096), short last units of 1 … 3 rows, a page of two tiles with a short last tile, a tile of NULLs between tiles of values, more
(column, page, tile) items than a launch has workgroups, 32 pruned columns in one call, a dictionary of 65 537 entries with three
entries and with all entries used, one value in every row, and every option mixed in — and at the edges of the groups: rows R − 1, R,
R + 1 and 2 R + 1 at R of 64 and 4 096, groups of one page and of three, pages of two tiles, a last group of one row, 17 columns × 70
groups. pyarrow and the project's own reader read every file back, all groups in one call; the chain from_parquet → sort →
to_parquet(row_group_rows=…, dictionaries="used") → from_parquet_many holds the Sort's restatement, group by group; a pass is launched
at most twice whatever the number of groups."""
import gc
import os
import re
import subprocess
import sys

import numpy as np
import pyarrow as pa
import pytest

from frostdb_amd import physicalplan as pp
from tests import parquet_bloom_cases as B, parquet_group_cases as G, parquet_runs_cases as R, parquet_write_cases as cases, sort_oracle
from tests.parquet_util import row_group_chunks

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_GRID = int(re.search(r"^#define FDB_PQW_MAX_GRID (\d+)", open(os.path.join(ROOT, "frostdb_amd", "csrc", "fdb_pqwrite.h")).read(), flags=re.M).group(1))
TILE = 4096


def check(record: pa.RecordBatch, page_rows: int = G.PAGE, reread: bool = True, rules: bool = False, **kw) -> bytes:
    """to_parquet(dictionaries="used") of the resident record == the host walk's file; pyarrow and from_parquet read it back. `rules`:
    the file is also held to the restatement (the CPU tests do that for the host walk; here for the shapes only this module has)."""
    rb = pp.ResidentBatch(record)
    try:
        data = rb.to_parquet(page_rows=page_rows, dictionaries="used", **kw)
        want = pp.selftest_parquet_write(record, page_rows=page_rows, dictionaries="used", **kw)
        assert len(data) == len(want), (len(data), len(want))
        if data != want:
            a, b = np.frombuffer(data, dtype=np.uint8), np.frombuffer(want, dtype=np.uint8)
            diff = np.flatnonzero(a != b)
            raise AssertionError("the device's file differs from the host walk's at %d bytes, first at %s" % (len(diff), diff[:8]))
        if rules:
            whole = pp.selftest_parquet_write(record, page_rows=page_rows, **kw)
            flags = R.flags_of(record, kw["runs"]) if kw.get("runs") else None
            G.assert_used_file(record, data, whole, page_rows, flags, kw.get("bloom_filters"), kw.get("bloom_bits_per_value", 0), kw.get("sorting_columns"))
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


def check_groups(record: pa.RecordBatch, rg_rows: int, page_rows: int = G.PAGE, dictionaries=None, reread: bool = True, **kw) -> bytes:
    """to_parquet(row_group_rows=…) of the resident record == the host walk's file; pyarrow reads it back, and from_parquet_many all its
    groups in one call, each the row slice of the record."""
    rb = pp.ResidentBatch(record)
    made = []
    try:
        data = rb.to_parquet(page_rows=page_rows, row_group_rows=rg_rows, dictionaries=dictionaries, **kw)
        want = pp.selftest_parquet_write(record, page_rows=page_rows, row_group_rows=rg_rows, dictionaries=dictionaries, **kw)
        assert len(data) == len(want), (len(data), len(want))
        if data != want:
            diff = np.flatnonzero(np.frombuffer(data, dtype=np.uint8) != np.frombuffer(want, dtype=np.uint8))
            raise AssertionError("the device's file differs from the host walk's at %d bytes, first at %s" % (len(diff), diff[:8]))
        gs = G.groups(data)
        assert [g["rows"] for g in gs] == [min(rg_rows, record.num_rows - i * rg_rows) for i in range(-(-record.num_rows // rg_rows))] and [g["ordinal"] for g in gs] == list(range(len(gs)))
        if reread:
            cases.assert_same_record(R.read_back(data), record)
            made = pp.ResidentBatch.from_parquet_many([row_group_chunks(data, i) for i in range(len(gs))])
            whole = rb.to_arrow()
            for i, back in enumerate(made):
                cases.assert_same_record(back.to_arrow(), whole.slice(i * rg_rows, gs[i]["rows"]))
        return data
    finally:
        for back in made:
            back.close()
        rb.close()


def spread(rows: int, entries: int, keep: int, seed: int = 0, stretch: int = 1) -> np.ndarray:
    """Indices that name `keep` of `entries` entries — the last among them — in stretches of `stretch` rows."""
    rng = np.random.default_rng(seed)
    pick = np.sort(np.concatenate([[entries - 1], rng.choice(entries - 1, keep - 1, replace=False)]))
    return pick[rng.integers(0, keep, -(-rows // stretch)).repeat(stretch)[:rows]]


# ---- 1. identity with the host walk at the kernels' edges ------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", cases.NULL_PATTERNS)
def test_the_mixed_record_under_every_null_pattern(pattern):
    for rows in (1, 63, 64, 65, 1000, TILE - 1, TILE, TILE + 1, 2 * TILE + 3):
        check(cases.mixed_record(rows, pattern, dict_size=300), page_rows=G.PAGE if rows <= 1000 else 2 * TILE, rules=rows in (65, TILE + 1), reread=rows in (1, 1000, 2 * TILE + 3))


@pytest.mark.parametrize("entries", G.DICT_SIZES)
def test_dictionary_sizes_and_how_much_of_them_is_used(entries):
    for used in G.USED:
        check(G.sized_record(entries, used), page_rows=4096 if used == "all" and entries > 4096 else G.PAGE, rules=True, reread=used in (3, "all"), statistics="chunk", bloom_filters=["labels.d"])


def test_edges_of_the_presence_words_duplicates_and_pages_of_one_index():
    check(G.word_edges_record(), rules=True)
    check(G.duplicates_record(), rules=True, statistics="page")
    for kw in (dict(), dict(runs=True), dict(compression="snappy")):
        check(G.equal_pages_record(), rules=True, **kw)


def test_short_last_units_and_a_page_of_two_tiles_with_a_short_last_tile():
    for tail in (1, 2, 3, 5):
        rows = 2 * 8192 + TILE + 96 + tail
        for pattern in ("none", "first_of_page", "alternate"):
            valid = cases.valid_mask(rows, pattern, 8192)
            record = pa.RecordBatch.from_arrays([G._dict(spread(rows, 300, 40, tail, 3), cases.dict_entries(300, True), valid, typ=pa.string()), pa.array(np.arange(rows, dtype=np.int64), mask=~valid)],
                                                names=["labels.t", "timestamp"])
            check(record, page_rows=8192, rules=pattern == "first_of_page", reread=tail == 1)


def test_a_tile_of_nulls_between_tiles_of_values():
    rows = 3 * TILE + 33
    r = np.arange(rows)
    middle, edges = (r // TILE) != 1, (r // TILE) == 1
    idx = spread(rows, 1000, 17, 9, 5)
    idx[TILE:2 * TILE] = 3   # an entry only NULL rows name: not used in `d`, the only one used in `d2`
    entries = cases.dict_entries(1000, True)
    record = pa.RecordBatch.from_arrays([G._dict(idx, entries, middle, typ=pa.string()), G._dict(idx, entries, edges, typ=pa.string()), pa.array(r, mask=~middle)], names=["d", "d2", "i"])
    data = check(record, page_rows=3 * TILE, rules=True)
    assert [d[0] for d in G.dictionary_pages(data)[:2]] == [17, 1]
    check(record, page_rows=8192, compression="snappy", encodings={"i": "delta"}, statistics="page", runs=True, reread=False)


def test_more_items_than_workgroups():
    """Pages of 64 rows × 17 pruned columns: more (column, page, tile) items than the launch has workgroups, every workgroup strides."""
    rows = 64 * (MAX_GRID // 17 + 3)
    valid = R.clustered_valid(rows, 40)
    cols = [G._dict(spread(rows, 300 + k, 5 + k, k, 1 + k % 4), cases.dict_entries(300 + k, False), valid if k % 2 else None) for k in range(17)]
    record = pa.RecordBatch.from_arrays(cols, names=["labels.c%02d" % k for k in range(17)])
    assert 17 * (rows // 64) > MAX_GRID
    check(record, rules=True)


def test_32_pruned_columns_in_one_call():
    rows = 2 * TILE + 77
    valid = R.clustered_valid(rows, 129)
    cols = [G._dict(spread(rows, 70 * (k + 1), 1 + k, k, 1 + k % 5), cases.dict_entries(70 * (k + 1), k % 2 == 0), valid if k % 3 == 0 else None, typ=pa.string() if k % 2 == 0 else pa.binary()) for k in range(32)]
    record = pa.RecordBatch.from_arrays(cols, names=["labels.c%02d" % k for k in range(32)])
    check(record, page_rows=TILE, rules=True)
    check(record, page_rows=2048, runs=True, compression="snappy", statistics="page", reread=False)


LDS_ENTRIES = 64 * int(re.search(r"^#define FDB_PQG_LDS_WORDS (\d+)", open(os.path.join(ROOT, "frostdb_amd", "csrc", "fdb_pqdict.h")).read(), flags=re.M).group(1))


def test_dictionaries_on_either_side_of_the_lds_stage():
    """The present kernel collects a tile's bits in LDS for a dictionary of at most LDS_ENTRIES (8 192) entries and sets them in global
    memory above: one entry below the bound, at it and past it, a few entries used and all of them, and both paths in one launch."""
    for entries in (LDS_ENTRIES - 1, LDS_ENTRIES, LDS_ENTRIES + 1):
        check(G.sized_record(entries, 3, rows=2 * TILE + 9), page_rows=TILE, rules=True, reread=False)
        check(G.sized_record(entries, "all"), page_rows=8192, rules=True, reread=entries == LDS_ENTRIES)
    rows = 3 * TILE + 5
    cols = [G._dict(spread(rows, e, 50, e, 2), cases.dict_entries(e, False), cases.valid_mask(rows, "alternate") if k % 2 else None) for k, e in enumerate((LDS_ENTRIES, LDS_ENTRIES + 1, 64, 70000))]
    check(pa.RecordBatch.from_arrays(cols, names=["labels.c%d" % k for k in range(4)]), page_rows=8192, rules=True)


def test_a_dictionary_of_65537_entries_with_three_and_with_all_entries_used():
    """The bitmap is 1 025 words (8 KiB), the counts 4 KiB: past the LDS stage, set and read in global memory by both kernels."""
    check(G.filtered_record(70000), page_rows=65536, rules=True, runs=True, bloom_filters=["labels.wide"])
    check(G.sized_record(65537, "all"), page_rows=8192, rules=True, statistics="page")


def test_one_value_in_every_row():
    rows = 2 * TILE + 5
    for valid in (None, cases.valid_mask(rows, "alternate")):
        record = pa.RecordBatch.from_arrays([G._dict(np.full(rows, 777), cases.dict_entries(1000, True), valid, typ=pa.string())], names=["labels.one"])
        data = check(record, page_rows=TILE, rules=True, runs=True)
        assert G.dictionary_pages(data)[0][0] == 1
    for kw in (dict(runs=True), dict(runs=True, compression="snappy", statistics="page", bloom_filters=["labels.d"])):   # … and none: the form of an empty dictionary, its run streams never active
        data = check(G.sized_record(65, 0, rows=rows), page_rows=TILE, rules=True, **kw)
        assert G.dictionary_pages(data)[0] is None


MIXES = [dict(compression="snappy"), dict(encodings={"timestamp": "delta"}), dict(statistics="page", sorting_columns=[("labels.a",), ("labels.b",)]), dict(bloom_filters=["labels.a", "timestamp"]), dict(runs=True),
         dict(encodings={"timestamp": "delta"}, compression=["snappy", None, "snappy", None, "snappy"], statistics="page", sorting_columns=[("labels.a",)], bloom_filters=["labels.b"], runs=True)]


@pytest.mark.parametrize("k", range(len(MIXES)))
def test_mixed_with_the_other_options(k):
    record = R.sorted_record(10000)
    keep = np.flatnonzero(np.arange(10000) % 7 < 2)   # what a filter leaves: a fraction of the dictionaries
    check(record.take(pa.array(keep)), page_rows=1024, rules=k in (3, 5), **MIXES[k])
    check(R.sorted_record(TILE + 100, seed=k), page_rows=8192, reread=False, **MIXES[k])


def test_from_parquet_sort_to_parquet_used():
    """from_parquet → filter-like take → sort → to_parquet(dictionaries="used", …) → from_parquet equals the Sort's restatement
    (tests/sort_oracle.py); every row's value is found in its column's filter (assert_used_file rebuilds the bitsets)."""
    rng = np.random.default_rng(71)
    n = 9000
    rec = pa.RecordBatch.from_arrays([pa.DictionaryArray.from_arrays(pa.array(rng.integers(0, 4, n).astype(np.uint32)), pa.array([b"c", b"a", b"d", b"b", b"unused"], type=pa.binary())),
                                      pa.DictionaryArray.from_arrays(pa.array((rng.integers(0, 25, n) * 2).astype(np.uint32), mask=rng.random(n) < 0.3), pa.array(["v%02d" % i for i in range(50)], type=pa.string())),
                                      pa.array(rng.permutation(n).astype(np.int64)), pa.array(rng.standard_normal(n), mask=rng.random(n) < 0.1)], names=["labels.a", "labels.b", "timestamp", "x"])
    made = []
    try:
        src = pp.ResidentBatch(rec)
        made.append(src)
        chunks, rows = row_group_chunks(src.to_parquet(dictionaries="used"), 0)
        loaded = pp.ResidentBatch.from_parquet(chunks, rows)
        made.append(loaded)
        ordered = loaded.sort([("labels.a",), ("labels.b",), ("timestamp",)])
        made.append(ordered)
        kw = dict(page_rows=4096, runs=True, statistics="page", sorting_columns=[("labels.a",), ("labels.b",), ("timestamp",)], bloom_filters="sorting")
        data = ordered.to_parquet(dictionaries="used", **kw)
        back = ordered.to_arrow()
        assert data == pp.selftest_parquet_write(back, dictionaries="used", **kw)
        whole = ordered.to_parquet(**kw)
        assert len(data) <= len(whole) + 2
        G.assert_used_file(back, data, whole, 4096, R.flags_of(back, True), "sorting", 0, kw["sorting_columns"])
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


# ---- 2. several row groups --------------------------------------------------------------------------------------------------------------------
ALL = dict(encodings={"timestamp": "delta"}, compression={"labels.utf8": "snappy", "timestamp": "snappy", "plain_bin": "snappy"}, statistics="page", sorting_columns=[("labels.bin",)],
           bloom_filters="sorting", bloom_bits_per_value=7, runs=True)


@pytest.mark.parametrize("rg_rows", [64, TILE])
@pytest.mark.parametrize("dictionaries", [None, "used"])
def test_rows_around_the_group_size(rg_rows, dictionaries):
    """A last group of R − 1 rows, of R, of one row; pages of 64 rows (R = 64: a group of one page), and at R = 4 096 pages of 2 048
    (two pages, half a tile each) and 4 096 (one)."""
    for rows in (rg_rows - 1, rg_rows, rg_rows + 1, 2 * rg_rows + 1):
        for pattern in ("none", "alternate", "whole_page"):
            record = cases.mixed_record(rows, pattern, dict_size=300)
            check_groups(record, rg_rows, 64 if rg_rows == 64 else 2048, dictionaries, reread=pattern == "alternate")
            check_groups(record, rg_rows, 64 if rg_rows == 64 else TILE, dictionaries, reread=False, **ALL)


def test_groups_of_one_page_of_three_pages_and_pages_of_two_tiles():
    for rg_rows, page_rows, rows in ((192, 64, 5 * 192 + 65), (TILE, TILE, 3 * TILE + 7), (3 * TILE, TILE, 7 * TILE + 100), (8192, 8192, 2 * 8192 + 1), (16384, 8192, 2 * 16384 + 1), (16384, 8192, 16384 + 8192 + TILE + 3)):
        record = cases.mixed_record(rows, "first_of_page", dict_size=300)
        for dictionaries in (None, "used"):
            check_groups(record, rg_rows, page_rows, dictionaries, reread=dictionaries == "used")
        check_groups(record, rg_rows, page_rows, "used", reread=False, **ALL)


def test_a_tile_of_nulls_between_tiles_of_values_in_groups():
    rows = 6 * TILE + 33
    r = np.arange(rows)
    middle = (r // TILE) % 3 != 1
    idx = spread(rows, 1000, 17, 9, 5)
    record = pa.RecordBatch.from_arrays([G._dict(idx, cases.dict_entries(1000, True), middle, typ=pa.string()), G._dict(idx, cases.dict_entries(1000, True), ~middle, typ=pa.string()), pa.array(r, mask=~middle)], names=["d", "d2", "i"])
    for dictionaries in (None, "used"):
        check_groups(record, 3 * TILE, 3 * TILE, dictionaries)
        check_groups(record, TILE, TILE, dictionaries, compression="snappy", encodings={"i": "delta"}, statistics="page", runs=True, bloom_filters=["d", "d2", "i"])   # groups that are all NULL between others


def test_17_columns_in_70_groups():
    """1 190 virtual columns of one page: every strided loop and every table per virtual column goes round; the last group is short."""
    rows = 64 * 70 - 13
    valid = R.clustered_valid(rows, 40)
    cols = [G._dict(spread(rows, 300 + k, 5 + k, k, 1 + k % 4), cases.dict_entries(300 + k, False), valid if k % 2 else None) for k in range(12)]
    cols += [pa.array(np.arange(rows, dtype=np.int64) * (k + 1), mask=~valid if k % 2 else None) for k in range(3)] + [pa.array(np.arange(rows) % 3 == 0, mask=~valid), pa.array(np.arange(rows) * 0.5)]
    names = ["labels.c%02d" % k for k in range(12)] + ["t0", "t1", "t2", "flag", "x"]
    record = pa.RecordBatch.from_arrays(cols, names=names)
    assert 17 * 70 > MAX_GRID
    for dictionaries in (None, "used"):
        data = check_groups(record, 64, 64, dictionaries)
        assert len(G.groups(data)) == 70
    check_groups(record, 64, 64, "used", reread=False, encodings={"t0": "delta", "t1": "delta"}, compression="snappy", statistics="page", sorting_columns=[("labels.c00",)], bloom_filters=names[:3] + ["t0", "x"], runs=True)


def test_32_dictionary_columns_and_wide_dictionaries_in_groups():
    rows = 2 * TILE + 77
    valid = R.clustered_valid(rows, 129)
    cols = [G._dict(spread(rows, 70 * (k + 1), 1 + k, k, 1 + k % 5), cases.dict_entries(70 * (k + 1), k % 2 == 0), valid if k % 3 == 0 else None, typ=pa.string() if k % 2 == 0 else pa.binary()) for k in range(32)]
    record = pa.RecordBatch.from_arrays(cols, names=["labels.c%02d" % k for k in range(32)])
    check_groups(record, TILE, 2048, "used")
    check_groups(record, 2048, 1024, None, reread=False, runs=True, compression="snappy", statistics="page")
    # 65 537 entries: three used — every group's bitmap past the LDS stage of LDS_ENTRIES entries — and all used
    check_groups(G.filtered_record(70000), 16384, 8192, "used", runs=True, bloom_filters=["labels.wide"])
    data = check_groups(G.sized_record(65537, "all"), 32768, 8192, "used", statistics="page")
    assert all(0 < G.group_dictionary_pages(data, rg)[0][0] <= 32768 for rg in G.groups(data))
    one = pa.RecordBatch.from_arrays([G._dict(np.full(rows, 777), cases.dict_entries(1000, True), cases.valid_mask(rows, "alternate"), typ=pa.string())], names=["labels.one"])
    data = check_groups(one, 1024, 512, "used", runs=True)
    assert all(G.group_dictionary_pages(data, rg)[0][0] == 1 for rg in G.groups(data))


@pytest.mark.parametrize("k", range(len(MIXES)))
def test_groups_mixed_with_the_other_options(k):
    record = R.sorted_record(10000)
    for dictionaries in (None, "used"):
        check_groups(record, 4096, 1024, dictionaries, reread=dictionaries == "used", **MIXES[k])


def test_from_parquet_sort_to_parquet_in_groups():
    """from_parquet → sort → to_parquet(row_group_rows=R, dictionaries="used", statistics="page", sorting_columns=…, bloom_filters="sorting")
    → from_parquet_many equals the Sort's restatement group by group; the bounds of the leading sorting column are the restatement's rows
    g·R and the group's last, ascending from group to group; every row's values are found in its own group's filters."""
    rng = np.random.default_rng(72)
    n, rg_rows = 9000, 2048
    rec = pa.RecordBatch.from_arrays([pa.DictionaryArray.from_arrays(pa.array(rng.integers(0, 40, n).astype(np.uint32)), pa.array([b"k%02d" % ((i * 7) % 41) for i in range(41)], type=pa.binary())),
                                      pa.DictionaryArray.from_arrays(pa.array((rng.integers(0, 25, n) * 2).astype(np.uint32), mask=rng.random(n) < 0.3), pa.array(["v%02d" % i for i in range(50)], type=pa.string())),
                                      pa.array(rng.permutation(n).astype(np.int64)), pa.array(rng.standard_normal(n), mask=rng.random(n) < 0.1)], names=["labels.a", "labels.b", "timestamp", "x"])
    made = []
    try:
        src = pp.ResidentBatch(rec)
        made.append(src)
        chunks, rows = row_group_chunks(src.to_parquet(), 0)
        loaded = pp.ResidentBatch.from_parquet(chunks, rows)
        made.append(loaded)
        ordered = loaded.sort([("labels.a",), ("labels.b",), ("timestamp",)])
        made.append(ordered)
        kw = dict(page_rows=512, row_group_rows=rg_rows, dictionaries="used", statistics="page", sorting_columns=[("labels.a",), ("labels.b",), ("timestamp",)], bloom_filters="sorting")
        data = ordered.to_parquet(**kw)
        assert data == pp.selftest_parquet_write(ordered.to_arrow(), **kw)
        want = rec.take(pa.array(sort_oracle.sort_indices(rec, [0, 1, 2])))
        gs = G.groups(data)
        assert len(gs) == 5
        groups = pp.ResidentBatch.from_parquet_many([row_group_chunks(data, g) for g in range(len(gs))])
        made += groups
        cases.assert_same_record(R.read_back(data), want)
        last = None
        for g, (rg, back) in enumerate(zip(gs, groups)):
            part = want.slice(g * rg_rows, rg["rows"])
            cases.assert_same_record(back.to_arrow(), part)
            assert rg["sorting_columns"] == [(0, False, False), (1, False, False), (2, False, False)]
            lead = rg["chunks"][0]
            assert (lead["min_value"], lead["max_value"]) == (part.column(0)[0].as_py(), part.column(0)[rg["rows"] - 1].as_py()), g
            assert last is None or last <= lead["min_value"]
            last = lead["max_value"]
            for j in range(3):
                off, length = rg["chunks"][j]["bloom"]
                num_bytes, header_len = B.read_header(data, off)
                hashes, _n = B.column_hashes(part.column(j))
                bitset = data[off + header_len:off + length]
                assert len(bitset) == num_bytes and all(B.maybe(bitset, h) for h in hashes), (g, j)
            assert rg["chunks"][3]["bloom"] is None
    finally:
        for rb in made:
            rb.close()


# ---- 3. the unchanged path, refusals, launches, allocations ---------------------------------------------------------------------------------
def test_without_group_options_the_bytes_are_the_older_ones_and_refusals_launch_nothing():
    gc.collect()
    record = cases.mixed_record(1000, "alternate", dict_size=300)
    rb = pp.ResidentBatch(record)
    try:
        for kw in (dict(), dict(encodings={"timestamp": "delta"}, compression="snappy"), dict(statistics="page", bloom_filters=["timestamp"]), dict(runs=True)):
            old = rb.to_parquet(page_rows=64, **kw)
            assert rb.to_parquet(page_rows=64, row_group_rows=0, dictionaries=None, **kw) == old
            assert rb.to_parquet(page_rows=64, dictionaries="whole", **kw) == old
            assert rb.to_parquet(page_rows=64, dictionaries="used", **kw) != old
        one = rb.to_parquet(page_rows=64, row_group_rows=1024)
        assert one == pp.selftest_parquet_write(record, page_rows=64, row_group_rows=1024) and G.ordinal(one) == 0
        before = pp.live_allocations()
        for kw, code in ((dict(row_group_rows=65), pp.FDB_ERR_INVALID), (dict(row_group_rows=-64), pp.FDB_ERR_INVALID), (dict(dictionaries="some"), pp.FDB_ERR_INVALID),
                         (dict(dictionaries="used", page_rows=100), pp.FDB_ERR_INVALID), (dict(row_group_rows=64, dictionaries="some"), pp.FDB_ERR_INVALID)):
            with pytest.raises(pp.FdbError) as e:
                rb.to_parquet(**kw)
            assert e.value.code == code and pp.live_allocations() == before, kw
    finally:
        rb.close()


PROFILE_SCRIPT = """
import numpy as np, pyarrow as pa
from frostdb_amd import physicalplan as pp
from tests import parquet_group_cases as G
rb = pp.ResidentBatch(G.filtered_record(20000))
rb.to_parquet(page_rows=1024, dictionaries="used", runs=True)
rb.to_parquet(page_rows=1024, runs=True)
rb.close()
"""

GROUP_PROFILE_SCRIPT = """
import sys
from frostdb_amd import physicalplan as pp
from tests import parquet_write_cases as cases
rb = pp.ResidentBatch(cases.mixed_record(64 * int(sys.argv[1]) + 9, "alternate", dict_size=300))
rb.to_parquet(page_rows=64, row_group_rows=64, dictionaries="used", encodings={"timestamp": "delta"}, compression={"labels.utf8": "snappy"}, statistics="page", bloom_filters=["labels.bin"], runs=True)
rb.close()
"""


def test_each_pass_is_launched_once():
    """FDB_PROFILE=1 marks every pass it waits for: a call with dictionaries="used" marks `pqwrite dict present` and `pqwrite dict remap`
    once each, whatever the pages and columns; a call without marks neither."""
    r = subprocess.run([sys.executable, "-c", PROFILE_SCRIPT], cwd=ROOT, env=dict(os.environ, FDB_PROFILE="1"), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    marks = re.findall(r"^\[fdb\] (pqwrite [a-z ]+?)\s+[\d.]+ us$", r.stderr, flags=re.M)
    assert marks.count("pqwrite dict present") == 1 and marks.count("pqwrite dict remap") == 1, marks
    assert marks.count("pqwrite survey") == 2 and marks.count("pqwrite encode") == 2 and marks.count("pqwrite run encode") == 2, marks


def test_a_pass_is_launched_at_most_twice_whatever_the_number_of_groups():
    """FDB_PROFILE=1 marks every pass it waits for. With 3 + 1 groups and with 70 + 1 every pass of the survey and encode sides is marked
    twice — the full groups' launch and the short last group's — and the compress, scan and gather passes once: the same marks for both."""
    seen = []
    for n_groups in (3, 70):
        r = subprocess.run([sys.executable, "-c", GROUP_PROFILE_SCRIPT, str(n_groups)], cwd=ROOT, env=dict(os.environ, FDB_PROFILE="1"), capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-2000:]
        marks = re.findall(r"^\[fdb\] (pqwrite [a-z ]+?)\s+[\d.]+ us$", r.stderr, flags=re.M)
        counts = {m: marks.count(m) for m in set(marks)}
        assert counts and all(v <= 2 for v in counts.values()), counts
        for name in ("pqwrite survey", "pqwrite stats", "pqwrite delta survey", "pqwrite dict present", "pqwrite dict remap", "pqwrite run survey", "pqwrite bloom insert", "pqwrite encode", "pqwrite delta encode", "pqwrite run encode"):
            assert counts.get(name) == 2, (name, counts)
        for name in ("pqwrite compress", "pqwrite scan", "pqwrite gather", "pqwrite copy"):
            assert counts.get(name) == 1, (name, counts)
        seen.append(counts)
    assert seen[0] == seen[1], seen


def test_everything_is_released():
    """Last in the module: whatever the tests above made — presence bitmaps, counts, re-keyed copies, images, returned bytes — is gone."""
    gc.collect()
    record = G.filtered_record(5000)
    rb = pp.ResidentBatch(record)
    for page_rows in (64, 0):
        rb.to_parquet(page_rows=page_rows, dictionaries="used", runs=True, encodings={"timestamp": "delta"}, compression="snappy", statistics="page", bloom_filters=["labels.wide"])
        rb.to_parquet(page_rows=page_rows, dictionaries="used")
    rb.close()
    gc.collect()
    assert all(v == 0 for v in pp.live_allocations().values()), pp.live_allocations()
