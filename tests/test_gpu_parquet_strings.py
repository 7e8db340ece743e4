"""PLAIN and DELTA_LENGTH_BYTE_ARRAY value pages on the device (ResidentBatch.to_parquet(strings=…)): the device's file byte for byte
against the host walk's (fdb_selftest_parquet_write_strings — which tests/test_parquet_strings_cpu.py holds against the page builder of
tests/parquet_strings_cases.py and pyarrow), at the edges of the byte survey and byte encode kernels (fdb_pqbytes.hip): rows 1, 63, 64,
65 and around one and two tiles, a page of two tiles, a tile of NULLs between tiles of values, a tile of empty values, the 70 001-byte
entry first, last and alone in a tile (an output range beyond one pass of the workgroup), values whose bytes start at every file offset
mod 4, more items than the grid has workgroups, 32 string columns in one call, a 65 537-entry dictionary, both forms beside
dictionary-form, DELTA, SNAPPY and LZ4_RAW columns, row groups with a short last one. pyarrow and from_parquet / from_parquet_many read
the files back; the chains from_parquet → filter() → to_parquet(strings="delta_length") and → sort → to_parquet(strings="plain",
sorting_columns=…) → from_parquet are held against the Sort's restatement; by the FDB_PROFILE marks each new pass is launched at most
twice whatever the number of row groups, and a call without a form launches neither."""
import gc
import os
import re
import subprocess
import sys

import numpy as np
import pyarrow as pa
import pytest

from frostdb_amd import physicalplan as pp
from frostdb_amd.logicalplan import Col, Sum
from tests import parquet_group_cases as G, parquet_runs_cases as R, parquet_strings_cases as Y, parquet_write_cases as cases, sort_oracle
from tests.parquet_util import row_group_chunks

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_GRID = int(re.search(r"^#define FDB_PQW_MAX_GRID (\d+)", open(os.path.join(ROOT, "frostdb_amd", "csrc", "fdb_pqwrite.h")).read(), flags=re.M).group(1))
TILE = 4096


def check(record: pa.RecordBatch, strings, page_rows: int = Y.PAGE, reread: bool = True, rules: bool = False, **kw) -> bytes:
    """to_parquet(strings=…) of the resident record == the host walk's file; pyarrow and from_parquet (with row groups: from_parquet_many)
    read it back by value — the reader's dictionary is first-seen. `rules`: the file is also held to the page builder."""
    rb = pp.ResidentBatch(record)
    made = []
    try:
        data = rb.to_parquet(page_rows=page_rows, strings=strings, **kw)
        want = pp.selftest_parquet_write(record, page_rows=page_rows, strings=strings, **kw)
        assert len(data) == len(want), (len(data), len(want))
        if data != want:
            diff = np.flatnonzero(np.frombuffer(data, dtype=np.uint8) != np.frombuffer(want, dtype=np.uint8))
            raise AssertionError("the device's file differs from the host walk's at %d bytes, first at %s" % (len(diff), diff[:8]))
        if rules:
            Y.assert_strings_file(record, data, strings, page_rows, kw.get("row_group_rows", 0))
        if reread:
            cases.assert_same_record(R.read_back(data), record)
            if record.num_rows > 0:
                gs = G.groups(data)
                made = pp.ResidentBatch.from_parquet_many([row_group_chunks(data, i) for i in range(len(gs))])
                whole, at = rb.to_arrow(), 0
                for g, back in zip(gs, made):
                    cases.assert_same_record(back.to_arrow(), whole.slice(at, g["rows"]))
                    at += g["rows"]
        return data
    finally:
        for back in made:
            back.close()
        rb.close()


# ---- 1. identity with the host walk at the kernels' edges ------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", Y.FORMS)
@pytest.mark.parametrize("pattern", cases.NULL_PATTERNS)
def test_the_four_kinds_under_every_null_pattern(form, pattern):
    for rows in (1, 63, 64, 65, 1000, TILE - 1, TILE, TILE + 1, 2 * TILE + 1):
        page_rows = Y.PAGE if rows <= 1000 else 2 * TILE   # (a page of two tiles, the second short)
        check(Y.kinds_record(rows, pattern, page=page_rows), form, page_rows=page_rows, rules=rows in (65, TILE + 1), reread=rows in (1, 1000, 2 * TILE + 1))


@pytest.mark.parametrize("form", Y.FORMS)
def test_a_tile_of_nulls_and_a_tile_of_empty_values_between_tiles_of_values(form):
    rows = 4 * TILE + 33
    r = np.arange(rows)
    valid = (r // TILE) != 1
    entries = [b""] + [Y._entry(i, 1 + i % 9) for i in range(1, 50)]
    idx = 1 + (r * 7) % 49
    idx[2 * TILE:3 * TILE] = 0   # a tile whose values are all empty
    record = pa.RecordBatch.from_arrays([Y._dict(idx, entries, valid), Y._dict(idx, entries, ~valid | (r % 5 == 0)), pa.array(r, mask=~valid)], names=["d", "d2", "i"])
    check(record, form, page_rows=4 * TILE, rules=True)
    check(record, form, page_rows=8192, compression="snappy", encodings={"i": "delta"}, statistics="page", runs=True, reread=False)


@pytest.mark.parametrize("form", Y.FORMS)
def test_the_long_entry_first_last_and_alone_in_a_tile(form):
    rows = 3 * TILE
    r = np.arange(rows)
    alone = r != TILE + 77
    alone[:TILE] = True
    alone[2 * TILE:] = True   # tile 1 holds one value: the long entry, alone
    record = Y.lengths_record(rows=rows, long_at=[0, TILE - 1, TILE + 77, 2 * TILE, rows - 1])
    valid = np.ones(rows, dtype=bool)
    valid[TILE:2 * TILE] = ~alone[TILE:2 * TILE]
    record = record.set_column(0, "labels.len", pa.DictionaryArray.from_arrays(pa.array(np.asarray(record.column(0).indices), type=pa.uint32(), mask=~valid), record.column(0).dictionary))
    check(record, form, page_rows=TILE, rules=True)
    check(record, form, page_rows=3 * TILE, reread=False)
    check(record, form, page_rows=TILE, compression={"labels.len": "lz4"}, reread=False)


@pytest.mark.parametrize("form", Y.FORMS)
def test_values_that_start_at_every_offset_mod_4(form):
    for shift in range(4):   # `shift` rows more, of 1, 2, 3 bytes, move every byte behind them
        record = Y.offsets_record(2 * Y.PAGE + shift)
        check(record, form, rules=True, reread=shift == 0)
        check(record, {"labels.a": form, "labels.b": "plain" if form == "delta_length" else "delta_length"}, optional={"labels.b": False}, reread=False)   # (a required column: no level bytes in front)


@pytest.mark.parametrize("form", Y.FORMS)
def test_more_items_than_workgroups(form):
    """1 094 pages of 64 rows × 17 columns: eighteen times as many (column, page, tile) items as a launch has workgroups, so every
    workgroup goes round its loop, and reuses its LDS staging, many times."""
    rows = 64 * 1094
    valid = R.clustered_valid(rows, 40)
    cols = [Y._dict((np.arange(rows) * (k + 3)) % (20 + k), [Y._entry(i + k, (i * (k + 1)) % 13) for i in range(20 + k)], valid if k % 2 else None) for k in range(17)]
    record = pa.RecordBatch.from_arrays(cols, names=["labels.c%02d" % k for k in range(17)])
    assert 17 * (rows // 64) > 16 * MAX_GRID
    check(record, form, reread=False)
    check(record.slice(0, 64 * 200), form, rules=True)   # (held to the builder and read back on fewer pages: their time is not this test's)


def test_32_string_columns_in_one_call():
    rows = 2 * TILE + 77
    valid = R.clustered_valid(rows, 129)
    cols = [Y._dict((np.arange(rows) * (k + 1)) % (7 * (k + 1)), cases.dict_entries(7 * (k + 1), k % 2 == 0), valid if k % 3 == 0 else None, pa.string() if k % 2 == 0 else pa.binary()) for k in range(32)]
    record = pa.RecordBatch.from_arrays(cols, names=["labels.c%02d" % k for k in range(32)])
    forms = [("plain", "delta_length", None)[k % 3] for k in range(32)]
    check(record, forms, page_rows=TILE, rules=True)
    check(record, forms, page_rows=2048, runs={"labels.c%02d" % k: ("levels" if forms[k] else True) for k in range(32)}, compression="snappy", statistics="page", reread=False)


@pytest.mark.parametrize("form", Y.FORMS)
def test_a_wide_dictionary_duplicates_empties_and_no_values(form):
    check(Y.wide_record(), form, rules=True)
    check(Y.wide_record(rows=TILE + 9, entries=65537), form, page_rows=TILE, bloom_filters=["labels.wide"], statistics="page")
    check(Y.duplicates_record(), form, rules=True)
    check(Y.empties_record(), form, rules=True)
    check(Y.null_page_record(), form, rules=True)
    check(cases.empty_dictionary_record(), form, rules=True)
    check(cases.mixed_record(130, "all"), form, rules=True)


@pytest.mark.parametrize("form", Y.FORMS)
def test_beside_dictionary_delta_snappy_and_lz4_columns(form):
    record = cases.mixed_record(TILE + 100, "alternate", dict_size=300)
    other = "plain" if form == "delta_length" else "delta_length"
    strings = {"labels.utf8": form, "labels.bin": "dictionary", "plain_str": other, "plain_bin": form}
    kw = dict(encodings={"timestamp": "delta", "dense": "delta"}, compression={"labels.utf8": "snappy", "plain_bin": "lz4", "labels.bin": "lz4", "timestamp": "snappy"},
              statistics="page", sorting_columns=[("labels.bin",)], bloom_filters=["labels.utf8", "plain_str"], dictionaries="used")
    check(record, strings, page_rows=1024, rules=True, **kw)
    check(record, strings, page_rows=2 * TILE, reread=False, **kw)


@pytest.mark.parametrize("form", Y.FORMS)
def test_row_groups_with_a_short_last_group(form):
    for rows, rg_rows, page_rows in ((64 * 5 + 9, 64, 64), (2 * TILE + 100, TILE, 1024)):
        record = Y.kinds_record(rows, "alternate", page=page_rows)
        opt = {n: True for n in record.schema.names}
        check(record, form, page_rows=page_rows, rules=True, row_group_rows=rg_rows, optional=opt)
        check(record, form, page_rows=page_rows, reread=False, row_group_rows=rg_rows, optional=opt, compression="snappy", statistics="page", bloom_filters=["labels.bin"], runs={"plain_str": "levels"})


# ---- 2. chains ----------------------------------------------------------------------------------------------------------------------------------
def test_from_parquet_filter_sort_to_parquet_strings():
    """from_parquet → filter() → to_parquet(strings="delta_length") and → sort → to_parquet(strings="plain", sorting_columns=…) →
    from_parquet equal the filter's and the Sort's restatement (tests/sort_oracle.py)."""
    rng = np.random.default_rng(72)
    n = 9000
    v = rng.integers(0, 1000, n).astype(np.int64)
    rec = pa.RecordBatch.from_arrays([pa.DictionaryArray.from_arrays(pa.array(rng.integers(0, 4, n).astype(np.uint32)), pa.array([b"c", b"a", b"d", b"b", b"unused"], type=pa.binary())),
                                      pa.DictionaryArray.from_arrays(pa.array((rng.integers(0, 25, n) * 2).astype(np.uint32), mask=rng.random(n) < 0.3), pa.array(["v%02d" % i * (1 + i % 3) for i in range(50)], type=pa.string())),
                                      pa.array(rng.permutation(n).astype(np.int64)), pa.array(v)], names=["labels.a", "labels.b", "timestamp", "v"])
    plan = pp.HashAggregatePlan(Col("v") > 300, [Sum(Col("v"))], [Col("labels.a")])
    made = []
    try:
        src = pp.ResidentBatch(rec)
        made.append(src)
        chunks, rows = row_group_chunks(src.to_parquet(strings="plain"), 0)
        loaded = pp.ResidentBatch.from_parquet(chunks, rows)
        made.append(loaded)
        filtered = plan.FilterResident(loaded)
        made.append(filtered)
        kept = rec.filter(pa.array(v > 300))
        data = filtered.to_parquet(page_rows=1024, strings="delta_length")
        assert data == pp.selftest_parquet_write(filtered.to_arrow(), page_rows=1024, strings="delta_length")
        Y.assert_strings_file(filtered.to_arrow(), data, "delta_length", 1024)
        cases.assert_same_record(R.read_back(data), kept)
        ordered = filtered.sort([("labels.a",), ("labels.b",), ("timestamp",)])
        made.append(ordered)
        kw = dict(page_rows=4096, statistics="page", sorting_columns=[("labels.a",), ("labels.b",), ("timestamp",)], bloom_filters="sorting")
        data = ordered.to_parquet(strings="plain", **kw)
        assert data == pp.selftest_parquet_write(ordered.to_arrow(), strings="plain", **kw)
        assert G.groups(data)[0]["sorting_columns"] == [(0, False, False), (1, False, False), (2, False, False)]
        chunks, rows = row_group_chunks(data, 0)
        again = pp.ResidentBatch.from_parquet(chunks, rows)
        made.append(again)
        want = kept.take(pa.array(sort_oracle.sort_indices(kept, [0, 1, 2])))
        cases.assert_same_record(again.to_arrow(), want)
        cases.assert_same_record(R.read_back(data), want)
    finally:
        plan.Close()
        for rb in made:
            rb.close()


# ---- 3. launches, refusals, allocations -----------------------------------------------------------------------------------------------------------
PROFILE_SCRIPT = """
import sys
from frostdb_amd import physicalplan as pp
from tests import parquet_strings_cases as Y
record = Y.kinds_record(64 * int(sys.argv[1]) + 9, "alternate")
rb = pp.ResidentBatch(record)
opt = {n: True for n in record.schema.names}
rb.to_parquet(page_rows=64, row_group_rows=64, optional=opt, strings={"labels.utf8": "plain", "plain_str": "delta_length"}, compression={"labels.utf8": "snappy"}, statistics="page")
print("[fdb] ---- without a form", file=sys.stderr, flush=True)
rb.to_parquet(page_rows=64, row_group_rows=64, optional=opt, encodings={"timestamp": "delta"})
rb.close()
"""


def test_each_new_pass_is_launched_at_most_twice_and_not_at_all_without_a_form():
    """FDB_PROFILE=1 marks every pass it waits for. With 4 + 1 groups and with 71 + 1 the byte survey and the byte encode pass are marked
    twice — the full groups' launch and the short last group's —, the same marks for both; the call without a form marks neither."""
    seen = []
    for n_groups in (4, 71):
        r = subprocess.run([sys.executable, "-c", PROFILE_SCRIPT, str(n_groups)], cwd=ROOT, env=dict(os.environ, FDB_PROFILE="1"), capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-2000:]
        with_form, without = r.stderr.split("[fdb] ---- without a form")
        marks = re.findall(r"^\[fdb\] (pqwrite [a-z ]+?)\s+[\d.]+ us$", with_form, flags=re.M)
        counts = {m: marks.count(m) for m in set(marks)}
        assert counts and all(c <= 2 for c in counts.values()), counts
        for name in ("pqwrite survey", "pqwrite bytes survey", "pqwrite delta survey", "pqwrite encode", "pqwrite delta encode", "pqwrite bytes encode"):
            assert counts.get(name) == 2, (name, counts)
        marks = re.findall(r"^\[fdb\] (pqwrite [a-z ]+?)\s+[\d.]+ us$", without, flags=re.M)
        assert marks.count("pqwrite survey") == 2 and marks.count("pqwrite delta encode") == 2 and not [m for m in marks if "bytes" in m], marks
        seen.append(counts)
    assert seen[0] == seen[1], seen


def test_refusals_leave_nothing_behind():
    record = cases.mixed_record(1000, "alternate", dict_size=300)
    rb = pp.ResidentBatch(record)
    try:
        assert rb.to_parquet(page_rows=64, strings={"labels.utf8": None}) == rb.to_parquet(page_rows=64) == pp.selftest_parquet_write(record, page_rows=64)
        before = pp.live_allocations()
        for kw, code in ((dict(strings="delta"), pp.FDB_ERR_INVALID), (dict(strings={"timestamp": "plain"}), pp.FDB_ERR_UNSUPPORTED), (dict(strings={"flag": "delta_length"}), pp.FDB_ERR_UNSUPPORTED),
                         (dict(strings={"labels.utf8": "plain"}, runs={"labels.utf8": "values"}), pp.FDB_ERR_UNSUPPORTED), (dict(strings="plain", page_rows=100), pp.FDB_ERR_INVALID),
                         (dict(strings="plain", row_group_rows=65), pp.FDB_ERR_INVALID)):
            with pytest.raises(pp.FdbError) as e:
                rb.to_parquet(**kw)
            assert e.value.code == code and pp.live_allocations() == before, kw
    finally:
        rb.close()
    # a page that would not fit its header: refused after the survey, before the image — nothing of the call stays
    big = pa.RecordBatch.from_arrays([Y._dict(np.zeros(2049, np.uint32), [b"\x5a" * (1 << 20)])], names=["labels.big"])
    rb = pp.ResidentBatch(big)
    try:
        before = pp.live_allocations()
        for form in Y.FORMS:
            with pytest.raises(pp.FdbError) as e:
                rb.to_parquet(page_rows=4096, strings=form)
            assert e.value.code == pp.FDB_ERR_INVALID and "page 0 of column labels.big" in str(e.value), str(e.value)
            assert pp.live_allocations()["device_bytes"] - before["device_bytes"] < (64 << 20), pp.live_allocations()
    finally:
        rb.close()


def test_everything_is_released():
    """Last in the module: whatever the tests above made — entry tables, lengths, byte tables, images, returned bytes — is gone."""
    gc.collect()
    record = Y.kinds_record(5000, "alternate")
    rb = pp.ResidentBatch(record)
    for page_rows in (64, 0):
        rb.to_parquet(page_rows=page_rows, strings="delta_length", runs=True, encodings={"timestamp": "delta"}, compression="snappy", statistics="page", bloom_filters=["labels.bin"])
        rb.to_parquet(page_rows=page_rows, strings="plain")
    rb.close()
    gc.collect()
    assert all(v == 0 for v in pp.live_allocations().values()), pp.live_allocations()
