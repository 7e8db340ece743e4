"""The device Sort of resident records (fdb_batch_sort_indices, fdb_batch_sort): indices compared EXACTLY with the Python restatement of
the reference's comparison (tests/sort_oracle.py, stable), sort() compared bit for bit with record.take(oracle indices).

Row counts: sort_keys_kernel gives a lane 4 consecutive rows, a wave 256, a 256-thread workgroup 1024, and reads the 4 validity bits of
a lane from one byte — so records of 0, 1, 2 rows (answered on the host / one partial lane), 63 / 64 / 65 (a validity word), 257 (a wave
+ 1 row), 1023 / 1025 (a workgroup ∓ 1 row), 4097 (several workgroups + 1 row: every full lane, one partial) and 100 003 (many
workgroups, rocPRIM off its single-block path), each with every direction × nulls_first combination (the restatement compares pairwise
in Python: ≈ 1 s per sort of 100 003 rows, the device's share is milliseconds).

Raw slots under NULLs hold distinct non-zero values — dictionary indices far outside the dictionary — so a kernel that used them would
order the NULL rows by them (the restatement keeps them in input order) or read outside a rank table."""
import gc

import numpy as np
import pyarrow as pa
import pytest

from frostdb_amd import physicalplan as pp
from frostdb_amd.logicalplan import Col, Sum
from tests import sort_oracle
from tests.golden.sort_cases import CASES as GOLDEN_CASES
from tests.test_gpu_take import assert_same
from tests.test_sort_cpu import golden_columns, golden_record

pytestmark = pytest.mark.gpu

ROWS = [0, 1, 2, 63, 64, 65, 257, 1023, 1025, 4097, 100_003]
BIG = 100_003
KINDS = ["dict_binary", "dict_utf8", "string", "int64", "uint64", "float64"]
COMBOS = [(False, False), (False, True), (True, False), (True, True)]  # (descending, nulls_first)
WORDS = [b"", b"a", b"ab", b"a\x00", b"B", b"b", b"\xff", b"\xc3\xa9", b"zz"]  # prefixes, an embedded NUL, bytes ≥ 0x80 (compared unsigned)
NEG_NAN = np.array([0xFFF8000000000000], dtype=np.uint64).view(np.float64)[0]
F_SPECIAL = np.array([np.nan, NEG_NAN, np.inf, -np.inf, -0.0, 0.0, 5e-324, 1.5, -1e308])


# ---- records -------------------------------------------------------------------------------------------------------------------------------
def null_mask(rng, n):
    m = rng.random(n) < 0.2
    if n:
        m[0] = True
    return m


def with_nulls(values: np.ndarray, mask, typ) -> pa.Array:
    """`values` as an Arrow array whose rows under `mask` are NULL — the raw slots stay what `values` holds there."""
    data = pa.py_buffer(np.ascontiguousarray(values).tobytes())
    if mask is None:
        return pa.Array.from_buffers(typ, len(values), [None, data], null_count=0)
    bits = pa.py_buffer(np.packbits(~mask, bitorder="little").tobytes())
    return pa.Array.from_buffers(typ, len(values), [bits, data], null_count=int(mask.sum()))


def dict_column(rng, n, mask, entries, typ=pa.binary()) -> pa.DictionaryArray:
    idx = rng.integers(0, len(entries), n).astype(np.uint32)
    if mask is not None:  # distinct, non-zero, far outside the dictionary
        idx[mask] = (0xF0000000 + np.arange(n, dtype=np.uint32) * 7 + 1)[::-1][mask]
    values = pa.array([e.decode() for e in entries], type=typ) if pa.types.is_string(typ) else pa.array(entries, type=typ)
    return pa.DictionaryArray.from_arrays(with_nulls(idx, mask, pa.uint32()), values, safe=False)


def make_column(kind: str, n: int, nullable: bool, seed: int = 0) -> pa.Array:
    rng = np.random.default_rng(1000 * n + 17 * KINDS.index(kind) + seed + (7 if nullable else 0))
    mask = null_mask(rng, n) if nullable else None
    junk = (np.arange(n, dtype=np.int64)[::-1] * 3 + 1)  # distinct and non-zero, descending: what the slots under NULLs hold
    if kind == "dict_binary":
        return dict_column(rng, n, mask, WORDS)
    if kind == "dict_utf8":
        return dict_column(rng, n, mask, [w for w in WORDS if w not in (b"\xff",)], pa.string())
    if kind == "string":  # a plain column (encoded to its distinct values on import)
        vals = [WORDS[k].decode("latin-1") * (1 + k % 2) for k in rng.integers(0, len(WORDS), n)]
        return pa.array(vals, type=pa.string(), mask=mask)
    if kind == "int64":
        v = np.where(rng.random(n) < 0.5, rng.integers(-3, 4, n), rng.integers(np.iinfo(np.int64).min, np.iinfo(np.int64).max, n, dtype=np.int64, endpoint=True))
        if n >= 3:
            v[n // 2], v[n - 1] = np.iinfo(np.int64).min, np.iinfo(np.int64).max
        if mask is not None:
            v[mask] = junk[mask]
        return with_nulls(v.astype(np.int64), mask, pa.int64())
    if kind == "uint64":
        v = np.where(rng.random(n) < 0.5, rng.integers(0, 5, n).astype(np.uint64) << np.uint64(62), rng.integers(0, 2**64 - 1, n, dtype=np.uint64, endpoint=True))
        if n >= 3:
            v[n // 2], v[n - 1] = 0, 2**64 - 1
        if mask is not None:
            v[mask] = junk.astype(np.uint64)[mask]
        return with_nulls(v.astype(np.uint64), mask, pa.uint64())
    assert kind == "float64"
    v = np.where(rng.random(n) < 0.5, rng.choice(F_SPECIAL, n), rng.standard_normal(n))
    if mask is not None:
        v[mask] = junk.astype(np.float64)[mask]
    return with_nulls(v.astype(np.float64), mask, pa.float64())


def record_of(cols: dict, n: int) -> pa.RecordBatch:
    cols = dict(cols)
    cols["row"] = pa.array(np.arange(n, dtype=np.int64))
    return pa.RecordBatch.from_arrays(list(cols.values()), names=list(cols.keys()))


def check_indices(rb, rec, columns, what=""):
    want = sort_oracle.sort_indices(rec, [(rec.schema.get_field_index(c[0]) if isinstance(c[0], str) else c[0],) + tuple(c[1:]) for c in columns])
    got = rb.sort_indices(columns)
    assert got.dtype == np.int32 and got.tolist() == want, (what, columns)
    return want


def check_sorted_record(rb, rec, columns, want, what=""):
    out = rb.sort(columns)
    try:
        assert out.num_rows == rec.num_rows
        assert_same(out.to_arrow(), rec.take(pa.array(want, type=pa.int32())), (what, columns))
    finally:
        out.close()


# ---- 1. single columns ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("nullable", [False, True], ids=["no_nulls", "nulls"])
@pytest.mark.parametrize("kind", KINDS)
def test_single_column(kind, nullable, rows):
    rec = record_of({"k": make_column(kind, rows, nullable)}, rows)
    rb = pp.ResidentBatch(rec)
    try:
        for descending, nulls_first in COMBOS:
            want = check_indices(rb, rec, [("k", descending, nulls_first)], (kind, nullable, rows))
            if (descending, nulls_first) == COMBOS[(KINDS.index(kind) + (2 if nullable else 0)) % 4]:
                check_sorted_record(rb, rec, [("k", descending, nulls_first)], want, (kind, nullable, rows))
        if rows == 65:
            assert rb.sort_indices("k").tolist() == rb.sort_indices([0]).tolist() == rb.sort_indices([("k", False, False)]).tolist()
    finally:
        rb.close()


# ---- 2. multi-column keys ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [65, 1025, 4097])
def test_narrow_dictionary_columns_share_a_word(rows):
    """Three dictionary columns — 9, 3 and 200 entries, two of them with NULLs — packed into one key word (4 + 1 + 2 + 1 + 8 bits), mixed
    directions and NULL placements."""
    rng = np.random.default_rng(rows)
    rec = record_of({"a": make_column("dict_binary", rows, True, seed=1),
                     "b": dict_column(rng, rows, None, [b"x", b"z", b"y"]),
                     "c": dict_column(rng, rows, null_mask(rng, rows), [b"e%03d" % ((k * 37) % 200) for k in range(200)], pa.string())}, rows)
    rb = pp.ResidentBatch(rec)
    try:
        for columns in ([("a", False, True), ("b", True), ("c", False, False)], [("b",), ("a", True, False), ("c", True, True)], [("c", True), ("b", False)]):
            want = check_indices(rb, rec, columns, rows)
        check_sorted_record(rb, rec, columns, want, rows)
    finally:
        rb.close()


@pytest.mark.parametrize("rows", [257, 4097])
def test_three_word_key_splits_the_null_bit_from_its_value(rows):
    """A nullable int64 (NULL bit in word 0, value in word 1), a float64 (word 2), a nullable dictionary (word 3): four passes. The first
    two columns draw from few values, so the later ones decide often."""
    rng = np.random.default_rng(rows + 5)
    mask = null_mask(rng, rows)
    i = rng.choice(np.array([np.iinfo(np.int64).min, -1, 0, np.iinfo(np.int64).max], dtype=np.int64), rows)
    i[mask] = (np.arange(rows, dtype=np.int64) + 1)[mask]
    f = rng.choice(F_SPECIAL, rows)
    rec = record_of({"i": with_nulls(i, mask, pa.int64()), "f": with_nulls(f, None, pa.float64()), "d": make_column("dict_binary", rows, True, seed=3)}, rows)
    rb = pp.ResidentBatch(rec)
    try:
        for columns in ([("i",), ("f",), ("d",)], [("i", True, True), ("f", True), ("d", False, True)], [("f",), ("i", False, True)]):
            want = check_indices(rb, rec, columns, rows)
        check_sorted_record(rb, rec, columns, want, rows)
    finally:
        rb.close()


def test_heavy_ties_are_decided_by_the_second_column_then_by_stability():
    rng = np.random.default_rng(8)
    rec = record_of({"a": dict_column(rng, BIG, None, [b"m", b"k", b"l"]), "v": pa.array(rng.integers(0, 1000, BIG), type=pa.int64())}, BIG)
    rb = pp.ResidentBatch(rec)
    try:
        want = check_indices(rb, rec, [("a", True), ("v",)])
        a, v, w = np.asarray(rec.column("a").indices), np.asarray(rec.column("v")), np.asarray(want)
        same = (a[w][1:] == a[w][:-1]) & (v[w][1:] == v[w][:-1])
        assert same.sum() > 90_000 and (np.diff(w)[same] > 0).all()  # ≈ 33 rows per (a, v): equal rows stay in input order
    finally:
        rb.close()


# ---- 3. stability, dictionaries ------------------------------------------------------------------------------------------------------------
def test_rows_equal_on_the_key_keep_their_input_order():
    rows = 4097
    rng = np.random.default_rng(2)
    rec = record_of({"k": pa.array(rng.integers(0, 2, rows) * 10 - 5, type=pa.int64())}, rows)
    rb = pp.ResidentBatch(rec)
    try:
        for descending in (False, True):
            got = rb.sort_indices([("k", descending)])
            k = np.asarray(rec.column("k"))[got]
            cut = int(np.flatnonzero(np.diff(k) != 0)[0]) + 1
            assert (np.diff(k) != 0).sum() == 1 and (k[0] < k[-1]) != descending
            assert (np.diff(got[:cut]) > 0).all() and (np.diff(got[cut:]) > 0).all()
            assert got.tolist() == sort_oracle.sort_indices(rec, [(0, descending)])
    finally:
        rb.close()


def test_dictionary_entries_with_equal_bytes_tie():
    """[b"b", b"a", b"b"]: entries 0 and 2 are equal, the second column orders their rows — positions among the sorted entries (0 → 1,
    2 → 2) would not."""
    rows = 65
    rng = np.random.default_rng(4)
    d = pa.DictionaryArray.from_arrays(pa.array(rng.integers(0, 3, rows), type=pa.uint32()), pa.array([b"b", b"a", b"b"], type=pa.binary()))
    rec = record_of({"d": d, "v": pa.array(rng.permutation(rows), type=pa.int64())}, rows)
    rb = pp.ResidentBatch(rec)
    try:
        for columns in ([("d",), ("v", True)], [("d", True), ("v",)]):
            want = check_indices(rb, rec, columns)
        idx = np.asarray(d.indices)[want]
        assert len(set(idx[idx != 1][:10].tolist())) == 2  # rows of both `b` entries interleave
    finally:
        rb.close()


def test_dictionary_with_more_than_65536_entries_and_unreferenced_ones():
    """70 001 entries in shuffled order, 4097 rows that reference a fraction of them: a 17-bit rank field, ranks counted over entries no
    row uses."""
    rows, entries = 4097, 70_001
    rng = np.random.default_rng(6)
    words = [b"k%06d" % k for k in rng.permutation(entries)]
    mask = null_mask(rng, rows)
    rec = record_of({"d": dict_column(rng, rows, mask, words), "t": dict_column(rng, rows, None, [b"q", b"p"])}, rows)
    rb = pp.ResidentBatch(rec)
    try:
        check_indices(rb, rec, [("d", True, True)])
        want = check_indices(rb, rec, [("t",), ("d",)])
        check_sorted_record(rb, rec, [("t",), ("d",)], want)
    finally:
        rb.close()


# ---- 4. the reference's vectors ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", GOLDEN_CASES, ids=[c["id"] for c in GOLDEN_CASES])
def test_golden_vectors(case):
    rec = golden_record(case["samples"])
    rb = pp.ResidentBatch(rec)
    try:
        if "error" in case:
            with pytest.raises(pp.FdbError) as e:
                rb.sort_indices(golden_columns(case))
            assert e.value.code == pp.FDB_ERR_INVALID and case["error"] in str(e.value)
            return
        assert rb.sort_indices(golden_columns(case)).tolist() == case["indices"], case["cite"]
    finally:
        rb.close()


# ---- 5. chaining ---------------------------------------------------------------------------------------------------------------------------
def test_filter_then_sort_feeds_an_ordered_plan():
    rows = 5000
    rng = np.random.default_rng(10)
    rec = pa.RecordBatch.from_arrays(
        [dict_column(rng, rows, null_mask(rng, rows), [b"c", b"a", b"d", b"b"]), dict_column(rng, rows, null_mask(rng, rows), [b"l%02d" % ((k * 7) % 23) for k in range(23)]),
         pa.array(rng.integers(0, 1000, rows), type=pa.int64())], names=["labels.a", "labels.b", "v"])
    groups, columns = [Col("labels.a"), Col("labels.b")], [("labels.a",), ("labels.b",)]
    filt = pp.HashAggregatePlan(Col("v") > 300, [Sum(Col("v"))], groups)
    on_device = pp.HashAggregatePlan(None, [Sum(Col("v"))], groups, ordered=True)
    on_host = pp.HashAggregatePlan(None, [Sum(Col("v"))], groups, ordered=True)
    rb = pp.ResidentBatch(rec)
    try:
        filtered = filt.FilterResident(rb)
        host_filtered = filtered.to_arrow()
        assert 0 < host_filtered.num_rows < rows
        ordered = filtered.sort(columns)
        filtered.close()  # the sorted record owns its bytes
        want = sort_oracle.sort_indices(host_filtered, [(0,), (1,)])
        host_sorted = host_filtered.take(pa.array(want, type=pa.int32()))
        assert_same(ordered.to_arrow(), host_sorted)
        on_device.Callback(ordered)
        ordered.close()
        on_host.Callback(host_sorted)
        a, b = on_device.Finish(), on_host.Finish()
        assert a.num_rows == b.num_rows > 50 and a.schema.names == b.schema.names
        assert [c.to_pylist() for c in a.columns] == [c.to_pylist() for c in b.columns]
        keys = list(zip(a.column(0).to_pylist(), a.column(1).to_pylist()))
        assert keys == sorted(keys, key=lambda k: tuple((x is None, x) for x in k))  # ascending, NULLs last: the order sort() produced
    finally:
        rb.close()
        for p in (filt, on_device, on_host):
            p.Close()


def test_sort_of_a_take_result_after_its_input_was_closed():
    rows = 300
    rec = record_of({"i": make_column("int64", rows, True), "d": make_column("dict_utf8", rows, True), "f": make_column("float64", rows, False)}, rows)
    rb = pp.ResidentBatch(rec)
    rev = np.arange(rows - 1, -1, -1)
    taken = rb.take(rev)
    rb.close()
    host = rec.take(pa.array(rev, type=pa.int32()))
    try:
        columns = [("d", True, True), ("f",), ("i",)]
        want = check_indices(taken, host, columns)
        out = taken.sort(columns)
    finally:
        taken.close()
    assert_same(out.to_arrow(), host.take(pa.array(want, type=pa.int32())))
    again = out.sort([("row",)])  # … and back into the original order
    out.close()
    assert_same(again.to_arrow(), rec)
    again.close()


# ---- 6. errors and edge cases --------------------------------------------------------------------------------------------------------------
def test_errors_are_answered_before_anything_is_launched():
    rows = 100
    rec = record_of({"k": make_column("int64", rows, True), "b": pa.array(np.arange(rows) % 2 == 0)}, rows)
    rb = pp.ResidentBatch(rec)
    try:
        gc.collect()
        before = pp.live_allocations()
        bad = [([], pp.FDB_ERR_INVALID, "at least one column is needed for sorting"),
               ([7], pp.FDB_ERR_INVALID, "index"), ([-1], pp.FDB_ERR_INVALID, "index"),
               ([pp.SortCol(0, 2, 0)], pp.FDB_ERR_INVALID, "direction"),
               ([("k",), ("b",)], pp.FDB_ERR_UNSUPPORTED, "unsupported column type for sorting")]
        for columns, code, text in bad:
            for call in (rb.sort_indices, rb.sort):
                with pytest.raises(pp.FdbError) as e:
                    call(columns)
                assert e.value.code == code and text in str(e.value), (columns, str(e.value))
                assert pp.live_allocations() == before, columns
        with pytest.raises(pp.UnsupportedError) as e:
            rb.sort("b")
        assert "for column b" in str(e.value)
        with pytest.raises(KeyError):  # a name the record lacks: refused before the call
            rb.sort_indices([("nope",)])
        assert pp.live_allocations() == before
    finally:
        rb.close()


@pytest.mark.parametrize("rows", [0, 1])
def test_zero_or_one_row_with_an_unsupported_column(rows):
    """sort.go:412-417: a record of 0 or 1 rows is answered without looking at the columns' types."""
    rec = record_of({"b": pa.array([True, None][:rows], type=pa.bool_())}, rows)
    rb = pp.ResidentBatch(rec)
    try:
        assert rb.sort_indices("b").tolist() == list(range(rows))
        assert rb.sort_indices([5]).tolist() == list(range(rows))  # not even the index
        out = rb.sort([("b", True, True)])
        assert_same(out.to_arrow(), rec)
        out.close()
        with pytest.raises(pp.FdbError) as e:  # … but "no columns" is checked first
            rb.sort_indices([])
        assert e.value.code == pp.FDB_ERR_INVALID
    finally:
        rb.close()


def test_everything_is_released():
    gc.collect()
    before = pp.live_allocations()
    rec = record_of({"i": make_column("int64", 3000, True), "d": make_column("dict_binary", 3000, True)}, 3000)
    rb = pp.ResidentBatch(rec)
    out = rb.sort([("d",), ("i", True)])
    rb.sort_indices([("i",)])
    assert pp.live_allocations()["device_bytes"] > before["device_bytes"]
    out.close()
    rb.close()
    assert pp.live_allocations() == before
