"""The device merge of resident records whose field lists differ (fdb_batches_merge_named, ResidentBatch.merge_named) and the
OrderedSynchronizer on top of it, compared with tests/osync_oracle.py: the reference's schema rules restated over pyarrow, absent columns
as real all-NULL arrays, the order by tests/merge_oracle.py's pairwise comparison. No code is shared with the library.

As in tests/test_gpu_merge.py every input carries `src` (its place in the call) and `row` (the row's place in the record), which are no
sorting columns, so the order of ties shows; the raw slots under the inputs' own NULLs hold junk; results are compared after dictionary
decode — NULL positions exactly, valid values bit for bit — together with null_count and the column order.

Row counts follow the kernels: 63 / 64 / 65 rows (a validity word of the gather: an input that lacks a column contributes `valid = false`
lanes to its wave's ballot), T - 1 / T + 1 with T = merge_tile_rows(words) (a merge tile ∓ a row), a record of 1 and of 3 rows (the key
kernel's last lane, whose four rows are all marked NULL when the column is absent), five 64-bit sorting columns (the run-time-W merge
kernel). An input is ordered by the sorting columns it HAS: in a column it lacks all its rows tie as NULLs."""
import ctypes
import gc
import threading

import numpy as np
import pyarrow as pa
import pytest

from frostdb_amd import physicalplan as pp
from frostdb_amd.logicalplan import Col, DynCol
from tests import osync_oracle, sort_oracle
from tests.golden.osync_cases import ENSURE_SAME_SCHEMA, ORDERED_SYNCHRONIZER
from tests.test_gpu_merge import assert_decoded_same, junk_under_nulls
from tests.test_gpu_sort import COMBOS, dict_column, null_mask, with_nulls

pytestmark = pytest.mark.gpu


def tile(words=1):
    return pp.merge_tile_rows(words)


@pytest.fixture(scope="module", autouse=True)
def allocations_before_this_module():
    gc.collect()
    return pp.live_allocations()


# ---- records ---------------------------------------------------------------------------------------------------------------------------------
def ordered_inputs(records, order_by):
    """Every record put by the oracle into the order of the unified sorting columns it has, junk under its NULLs, tagged with src and row."""
    schema, columns = osync_oracle.unify(records, order_by)
    out = []
    for s, rec in enumerate(records):
        own = [(rec.schema.get_field_index(schema.names[k]), d, nf) for k, d, nf in columns if schema.names[k] in rec.schema.names]
        if own:
            rec = rec.take(pa.array(sort_oracle.sort_indices(rec, own), type=pa.int64()))
        n = rec.num_rows
        cols = [junk_under_nulls(c) for c in rec.columns] + [pa.array(np.full(n, s, dtype=np.int64)), pa.array(np.arange(n, dtype=np.int64))]
        out.append(pa.RecordBatch.from_arrays(cols, names=rec.schema.names + ["src", "row"]))
    return out


def merged_on_device(records, order_by, limit=0):
    rbs = [pp.ResidentBatch(r) for r in records]
    try:
        out = pp.ResidentBatch.merge_named(rbs, order_by, limit)
    finally:
        for rb in rbs:
            rb.close()  # the result owns its bytes
    try:
        assert out.column_names == out.to_arrow().schema.names
        return out.to_arrow()
    finally:
        out.close()


def check_named(records, order_by, limit=0, what=""):
    """`records`: ordered host records. Column order, rows, NULL positions, values and null_count against the oracle."""
    got = merged_on_device(records, order_by, limit)
    want = osync_oracle.merge(records, order_by, limit)
    assert_decoded_same(got, want, what)
    for name in want.schema.names:
        assert got.column(name).null_count == want.column(name).null_count, (what, name)
        if want.column(name).null_count == 0 and want.num_rows:
            assert got.column(name).buffers()[0] is None, (what, name, "a column without a NULL carries no bitmap")
    return got


def raw_slots(col: pa.Array) -> np.ndarray:
    """the value buffer as the library exported it (8-byte columns)"""
    return np.frombuffer(col.buffers()[1], dtype=np.uint64)[: len(col)]


def keys(rng, n, distinct=40):
    return pa.array(np.sort(rng.integers(0, distinct, n)), type=pa.int64())


def small_merge_works():
    recs = ordered_inputs([pa.RecordBatch.from_arrays([pa.array([1, 3], type=pa.int64())], names=["k"]),
                           pa.RecordBatch.from_arrays([pa.array([2], type=pa.int64()), pa.array([7.0])], names=["k", "f"])], ["k"])
    got = check_named(recs, ["k"])
    assert got.column("k").to_pylist() == [1, 2, 3] and got.column("f").to_pylist() == [None, 7.0, None]


# ---- 1. the reference's vector -----------------------------------------------------------------------------------------------------------------
def vector_records():
    return [pa.RecordBatch.from_arrays([pa.array([row[k] for row in rec["rows"]], type=pa.int64()) for k in range(len(rec["fields"]))], names=rec["fields"])
            for rec in ENSURE_SAME_SCHEMA["records"]]


@pytest.mark.parametrize("order_by", [["Field1"], ["Field1", "Field2", "Field3"]], ids=["by_field1", "by_all_three"])
def test_ensure_same_schema_vector(order_by):
    records = ordered_inputs(vector_records(), order_by)
    for r, rec in zip(records, vector_records()):
        assert r.column("row").to_pylist() == list(range(rec.num_rows)), ENSURE_SAME_SCHEMA["cite"]  # the reference's records ARE ordered
    got = check_named(records, order_by, 0, order_by)
    # the sorting columns, then the rest first seen first: record1's Field2 and tags come before record2's Field3
    assert got.schema.names == (["Field1", "Field2", "src", "row", "Field3"] if order_by == ["Field1"] else ENSURE_SAME_SCHEMA["fields"] + ["src", "row"])
    expected = ENSURE_SAME_SCHEMA["expected"]
    if order_by == ["Field1"]:  # ties in record order: the reference's expected rows, the (2, 2, 2) of record3 last anyway
        assert [tuple(got.column(f)[i].as_py() for f in ENSURE_SAME_SCHEMA["fields"]) for i in range(6)] == expected, ENSURE_SAME_SCHEMA["cite"]
    assert sorted(map(repr, (tuple(got.column(f)[i].as_py() for f in ENSURE_SAME_SCHEMA["fields"]) for i in range(6)))) == sorted(map(repr, expected))
    for name in ("Field2", "Field3"):  # the raw slot under an absent field reads 0, as the reference's reader shows it
        col = got.column(name)
        assert (raw_slots(col)[np.asarray(col.is_null())] == ENSURE_SAME_SCHEMA["value_under_absent"]).all(), name


# ---- 2. an absent column that is no sorting column ---------------------------------------------------------------------------------------------
def other_columns(rng, n, nullable):
    mask = (lambda: null_mask(rng, n)) if nullable else (lambda: None)
    return {"c_int64": with_nulls(rng.integers(-5, 5, n).astype(np.int64), mask(), pa.int64()),
            "c_uint64": with_nulls(rng.integers(0, 2**63, n).astype(np.uint64) * np.uint64(2) + np.uint64(1), mask(), pa.uint64()),
            "c_float64": with_nulls(rng.choice(np.array([np.nan, -0.0, 1.5, np.inf]), n), mask(), pa.float64()),
            "c_dict": dict_column(rng, n, mask(), [b"p", b"", b"q\x00", b"\xff"]),
            "c_string": pa.array(["s%d" % v for v in rng.integers(0, 5, n)], type=pa.string(), mask=mask())}


def absent_non_sorting_inputs(n, nullable):
    rng = np.random.default_rng(100 + n + (1 if nullable else 0))
    recs = []
    for s in range(3):
        cols = {"k": keys(rng, n)}
        if s != 1:  # the middle input lacks every other column
            cols.update(other_columns(rng, n, nullable))
        recs.append(pa.RecordBatch.from_arrays(list(cols.values()), names=list(cols.keys())))
    return ordered_inputs(recs, ["k"])


def row_counts():
    return [1, 63, 64, 65, tile(1) - 1, tile(1) + 1]


@pytest.mark.parametrize("nullable", [True, False], ids=["nulls", "no_nulls_elsewhere"])
@pytest.mark.parametrize("n", row_counts())
def test_absent_non_sorting_column_of_every_kind(n, nullable):
    records = absent_non_sorting_inputs(n, nullable)
    got = check_named(records, ["k"], 0, (n, nullable))
    assert got.schema.names == ["k", "c_int64", "c_uint64", "c_float64", "c_dict", "c_string", "src", "row"]
    from_middle = np.asarray(got.column("src")) == 1
    assert from_middle.sum() == n
    for name in ("c_int64", "c_uint64", "c_float64", "c_dict", "c_string"):
        col = got.column(name)
        assert col.buffers()[0] is not None and np.asarray(col.is_null())[from_middle].all(), name  # the bitmap appears, whatever the other inputs hold
        if not nullable:
            assert col.null_count == n, name
    for name in ("c_int64", "c_uint64", "c_float64"):
        assert (raw_slots(got.column(name))[from_middle] == 0).all(), name
    assert (np.frombuffer(got.column("c_dict").indices.buffers()[1], dtype=np.uint32)[: got.num_rows][from_middle] == 0).all()


def test_the_old_entry_point_still_refuses_differing_field_lists():
    rbs = [pp.ResidentBatch(r) for r in absent_non_sorting_inputs(65, True)]
    try:
        with pytest.raises(pp.FdbError) as e:
            pp.ResidentBatch.merge(rbs, ["k"])
        assert e.value.code == pp.FDB_ERR_INVALID and "record 1" in str(e.value)
    finally:
        for rb in rbs:
            rb.close()


# ---- 3. an absent SORTING column ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["first", "second"])
def test_absent_sorting_column_of_two(which):
    """Three inputs of 65, T + 1 and 3 rows; the second lacks `a` (the first sorting column) or `b` (the second): its rows sit where the
    column's NULLs sit, ordered among themselves by the other column."""
    counts = [65, tile(2) + 1, 3]
    rng = np.random.default_rng(31)
    raw = []
    for s, n in enumerate(counts):
        cols = {"a": with_nulls(rng.integers(0, 6, n).astype(np.int64), null_mask(rng, n), pa.int64()),
                "b": with_nulls(rng.integers(-3, 3, n).astype(np.int64), null_mask(rng, n), pa.int64())}
        if s == 1:
            del cols["a" if which == "first" else "b"]
        raw.append(pa.RecordBatch.from_arrays(list(cols.values()), names=list(cols.keys())))
    lacking = "a" if which == "first" else "b"
    for descending, nulls_first in COMBOS:
        order_by = [(Col("a"), descending, nulls_first), (Col("b"), not descending, nulls_first)]
        got = check_named(ordered_inputs(raw, order_by), order_by, 0, (which, descending, nulls_first))
        assert got.schema.names[:2] == ["a", "b"]
        nulls = np.asarray(got.column(lacking).is_null())
        src = np.asarray(got.column("src"))
        assert nulls[src == 1].all()
        if which == "first":  # the NULLs of the first column are one block, at the head or at the tail; the lacking input's rows are inside it
            block = np.flatnonzero(nulls)
            assert block.size and (block == np.arange(block[0], block[0] + block.size)).all() and (block[0] == 0 if nulls_first else block[-1] == len(nulls) - 1)
        # … and among themselves they are in the order of the column they have (their own row order: the input was ordered by it)
        assert (np.diff(np.asarray(got.column("row"))[src == 1]) > 0).all()


def test_absent_sorting_column_of_a_five_column_dynamic_key():
    """DynCol("k") over k.a … k.e, 64 bits each (with the NULL bit of the column one input lacks: six key words — the run-time-W kernel),
    2 T + 1 rows in all."""
    T = tile(5)
    counts = [T + 1, T - 3, 3]
    assert sum(counts) == 2 * T + 1
    rng = np.random.default_rng(32)
    raw = []
    for s, n in enumerate(counts):
        names = ["k.e", "k.a", "k.c", "k.b", "k.d"]
        if s == 1:
            names.remove("k.c")
        raw.append(pa.RecordBatch.from_arrays([pa.array(rng.integers(0, 3, n), type=pa.int64()) for _ in names], names=names))
    for order_by in ([DynCol("k")], [(DynCol("k"), True, True)]):
        got = check_named(ordered_inputs(raw, order_by), order_by, 0, order_by)
        assert got.schema.names == ["k.a", "k.b", "k.c", "k.d", "k.e", "src", "row"]
        assert got.column("k.c").null_count == counts[1]


# ---- 4. dynamic order-by, dictionaries ---------------------------------------------------------------------------------------------------------
def label_records(rng, counts, entries):
    """{labels.a, labels.c}, {labels.b}, {labels.a, labels.b, labels.c}, each with a timestamp; entries[s][label] = the dictionary"""
    have = [["labels.c", "labels.a"], ["labels.b"], ["labels.b", "labels.c", "labels.a"]]
    recs = []
    for s, n in enumerate(counts):
        cols = {"timestamp": pa.array(rng.integers(0, 50, n), type=pa.int64())}
        for name in have[s]:
            cols[name] = dict_column(rng, n, null_mask(rng, n), entries[s][name])
        recs.append(pa.RecordBatch.from_arrays(list(cols.values()), names=list(cols.keys())))
    return recs


def test_dynamic_order_by_with_differing_dictionaries():
    rng = np.random.default_rng(41)
    entries = [{"labels.a": [b"m", b"a", b"z"], "labels.c": [b"c1", b"c0"]},
               {"labels.b": [b"y", b"x"]},
               {"labels.a": [b"z", b"k", b"m"], "labels.b": [b"x", b"w", b"y"], "labels.c": [b"c0", b"c2"]}]
    for order_by in ([DynCol("labels"), Col("timestamp")], [(DynCol("labels"), True, True), (Col("timestamp"), True)]):
        records = ordered_inputs(label_records(rng, [300, 65, tile(1) + 1], entries), order_by)
        got = check_named(records, order_by, 0, order_by)
        assert got.schema.names == ["labels.a", "labels.b", "labels.c", "timestamp", "src", "row"]
        # the union in first-seen order over the inputs that HAVE the column
        assert got.column("labels.a").dictionary.to_pylist() == [b"m", b"a", b"z", b"k"]
        assert got.column("labels.b").dictionary.to_pylist() == [b"y", b"x", b"w"]
        assert got.column("labels.c").dictionary.to_pylist() == [b"c1", b"c0", b"c2"]


def test_inputs_that_have_the_column_share_one_dictionary():
    """labels.a has the same entries in both inputs that carry it (a duplicate and an unused entry included): the output carries that
    dictionary untranslated, although a third input lacks the column."""
    rng = np.random.default_rng(42)
    shared = [b"q", b"c", b"x", b"c", b"never-used"]
    entries = [{"labels.a": shared, "labels.c": [b"1"]}, {"labels.b": [b"y", b"x"]}, {"labels.a": shared, "labels.b": [b"x"], "labels.c": [b"2"]}]
    order_by = [DynCol("labels"), Col("timestamp")]
    recs = label_records(rng, [70, 65, 300], entries)
    for s in (0, 2):  # indices 0 … 3 only: the last entry stays unreferenced
        k = recs[s].schema.get_field_index("labels.a")
        n = recs[s].num_rows
        idx = with_nulls(rng.integers(0, 4, n).astype(np.uint32), null_mask(rng, n), pa.uint32())
        recs[s] = recs[s].set_column(k, "labels.a", pa.DictionaryArray.from_arrays(idx, pa.array(shared, type=pa.binary())))
    got = check_named(ordered_inputs(recs, order_by), order_by)
    assert got.column("labels.a").dictionary.to_pylist() == shared


# ---- 5. expressions that match nothing ---------------------------------------------------------------------------------------------------------
def test_an_expression_that_matches_nothing():
    rng = np.random.default_rng(51)
    counts = [65, tile(1) + 1, 3]
    raw = [pa.RecordBatch.from_arrays([keys(rng, n)] + ([pa.array(rng.random(n))] if s != 2 else []), names=["k", "f"][: 2 if s != 2 else 1]) for s, n in enumerate(counts)]
    order_by = [Col("missing"), (Col("k"), True), DynCol("k")]
    got = check_named(ordered_inputs(raw, order_by), order_by)
    assert got.schema.names == ["k", "f", "src", "row"]
    # no expression matches at all: the empty key — the concatenation in input order, cut to the limit
    nothing = [Col("missing"), DynCol("nope"), Col("K")]
    records = ordered_inputs(raw, ["k"])
    for limit in (0, 1, 65, 66, sum(counts) + 1):
        got = check_named(records, nothing, limit, ("empty key", limit))
        n = sum(counts) if limit == 0 else min(limit, sum(counts))
        assert got.column("src").to_pylist() == ([0] * counts[0] + [1] * counts[1] + [2] * counts[2])[:n]
        assert got.schema.names == ["k", "f", "src", "row"]


# ---- 6. inputs without rows --------------------------------------------------------------------------------------------------------------------
def empty_of(schema: pa.Schema) -> pa.RecordBatch:
    return pa.RecordBatch.from_arrays([pa.array([], type=f.type) if not pa.types.is_dictionary(f.type) else
                                       pa.DictionaryArray.from_arrays(pa.array([], type=pa.uint32()), pa.array([b"e0", b"e1"], type=pa.binary())) for f in schema], schema=schema)


def test_fields_of_inputs_without_rows_take_part_in_the_schema():
    rng = np.random.default_rng(61)
    only = empty_of(pa.schema([("only_i", pa.int64()), ("k", pa.int64()), ("only_d", pa.dictionary(pa.uint32(), pa.binary())), ("only_f", pa.float64())]))
    only = only.append_column("src", pa.array([], type=pa.int64())).append_column("row", pa.array([], type=pa.int64()))
    with_rows = ordered_inputs([pa.RecordBatch.from_arrays([keys(rng, n)], names=["k"]) for n in (65, 70)], ["k"])
    records = [with_rows[0], only, with_rows[1]]
    got = check_named(records, ["k", "only_d"])
    assert got.schema.names == ["k", "only_d", "src", "row", "only_i", "only_f"]  # sorting columns, then first seen first
    for name in ("only_i", "only_d", "only_f"):
        assert got.column(name).null_count == 135 == got.num_rows
    assert got.column("only_d").dictionary.to_pylist() == [b"e0", b"e1"]  # the zero-row input's dictionary
    assert (raw_slots(got.column("only_i")) == 0).all() and (raw_slots(got.column("only_f")) == 0).all()
    # zero-row inputs at the ends, and one input with rows among them
    got = check_named([only, with_rows[0], only], ["k"])
    assert got.schema.names == ["k", "only_i", "only_d", "only_f", "src", "row"] and got.num_rows == 65
    # no rows at all: the unified schema
    other = empty_of(pa.schema([("z", pa.float64()), ("k", pa.int64())]))
    got = check_named([only, other], [Col("k"), Col("z")])
    assert got.num_rows == 0 and got.schema.names == ["k", "z", "only_i", "only_d", "only_f", "src", "row"]
    got = check_named([other], ["k"], 5)
    assert got.num_rows == 0 and got.schema.names == ["k", "z"]


# ---- 7. K = 1 and limits -----------------------------------------------------------------------------------------------------------------------
def test_one_record_is_rearranged_and_limited_without_a_look_at_its_order():
    rng = np.random.default_rng(71)
    n = tile(1) + 1
    rec = pa.RecordBatch.from_arrays([pa.array(rng.random(n)), dict_column(rng, n, null_mask(rng, n), [b"b", b"a"]), pa.array(rng.integers(0, 9, n), type=pa.int64()),
                                      dict_column(rng, n, None, [b"x"])], names=["v", "labels.b", "k", "labels.a"])  # (not ordered by anything)
    for limit in (0, 1, 65, n, n + 1):
        got = check_named([rec], [Col("k"), DynCol("labels")], limit, limit)
        assert got.schema.names == ["k", "labels.a", "labels.b", "v"] and got.num_rows == (n if limit == 0 else min(limit, n))


def test_limits_on_three_records_of_differing_schemas():
    T = tile(1)
    rng = np.random.default_rng(72)
    counts = [T + 1, 70, 2 * T + 3]
    total = sum(counts)
    raw = [pa.RecordBatch.from_arrays([pa.array(rng.integers(0, 300, n), type=pa.int64())] + ([pa.array(rng.random(n))] if s == 1 else []), names=["k", "f"][: 2 if s == 1 else 1])
           for s, n in enumerate(counts)]
    order_by = [(Col("k"), True)]
    records = ordered_inputs(raw, order_by)
    want_all = osync_oracle.merge(records, order_by)
    rbs = [pp.ResidentBatch(r) for r in records]
    try:
        for limit in (1, T, total, total + 1):
            out = pp.ResidentBatch.merge_named(rbs, order_by, limit)
            got = out.to_arrow()
            out.close()
            assert got.num_rows == min(limit, total)
            assert_decoded_same(got, want_all.slice(0, min(limit, total)), limit)
            assert got.column("f").null_count == want_all.slice(0, min(limit, total)).column("f").null_count
    finally:
        for rb in rbs:
            rb.close()


# ---- 8. / 9. refusals ------------------------------------------------------------------------------------------------------------------------
def test_an_unordered_input_is_named_by_its_place_in_the_call():
    T = tile(1)
    rng = np.random.default_rng(81)
    good = ordered_inputs([pa.RecordBatch.from_arrays([keys(rng, 65, 1000), pa.array(rng.random(65))], names=["k", "f"]),
                           pa.RecordBatch.from_arrays([keys(rng, 70, 1000)], names=["k"])], ["k"])
    k = np.sort(rng.integers(0, 1000, T + 1))
    k[1500], k[1501] = k[1501] + 5, k[1500]  # row 1501 sorts before row 1500 — and nothing earlier is out of order
    assert (np.diff(k[:1501]) >= 0).all() and k[1501] < k[1500]
    unordered = pa.RecordBatch.from_arrays([pa.array(k, type=pa.int64()), pa.array(np.arange(T + 1, dtype=np.int64))], names=["k", "other"])
    empty = pa.RecordBatch.from_arrays([pa.array([], type=pa.int64())], names=["k"])
    rbs = [pp.ResidentBatch(r) for r in (good[0], empty, unordered, good[1])]
    try:
        gc.collect()
        before = pp.live_allocations()
        with pytest.raises(pp.FdbError) as e:  # (the record without rows does not shift the numbering)
            pp.ResidentBatch.merge_named(rbs, [Col("k"), Col("missing")])
        assert e.value.code == pp.FDB_ERR_INVALID and "record 2" in str(e.value) and "row 1501" in str(e.value), str(e.value)
        assert pp.live_allocations() == before
        out = pp.ResidentBatch.merge_named([rbs[0], rbs[1], rbs[3]], ["k"])  # the next call on the same device
        assert_decoded_same(out.to_arrow(), osync_oracle.merge([good[0], empty, good[1]], ["k"]))
        out.close()
        assert pp.live_allocations() == before
    finally:
        for rb in rbs:
            rb.close()


def test_refusals_name_their_reason_and_leave_the_device_usable():
    i64 = lambda v: pa.array(v, type=pa.int64())  # noqa: E731
    recs = {"g0": pa.RecordBatch.from_arrays([i64([1, 3])], names=["k"]),
            "g1": pa.RecordBatch.from_arrays([i64([2]), pa.array([0.5])], names=["k", "f"]),
            "twice": pa.RecordBatch.from_arrays([i64([1]), i64([2]), i64([3])], names=["k", "dup", "dup"]),
            "float_k": pa.RecordBatch.from_arrays([pa.array([1.0])], names=["k"]),
            "flag0": pa.RecordBatch.from_arrays([pa.array([False, True]), i64([1, 2])], names=["b", "v"]),
            "flag1": pa.RecordBatch.from_arrays([pa.array([True]), pa.array([1.5])], names=["b", "w"]),
            "utf8": pa.RecordBatch.from_arrays([pa.DictionaryArray.from_arrays(pa.array([0, 1], type=pa.uint32()), pa.array(["a", "b"], type=pa.string()))], names=["d"]),
            "binary": pa.RecordBatch.from_arrays([pa.DictionaryArray.from_arrays(pa.array([0, 1], type=pa.uint32()), pa.array([b"a", b"b"], type=pa.binary())), i64([1, 2])], names=["d", "x"]),
            "big": pa.RecordBatch.from_arrays([pa.array(np.zeros(1 << 20, dtype=np.int64))], names=["k"])}
    made = {name: pp.ResidentBatch(r) for name, r in recs.items()}
    L = pp.lib()
    try:
        gc.collect()
        before = pp.live_allocations()
        bad = [(["g0", "twice"], ["k"], pp.FDB_ERR_INVALID, ["found multiple fields", "for name dup"]),
               (["g0", "g1", "float_k"], ["k"], pp.FDB_ERR_INVALID, ["record 0", "record 2"]),
               (["flag0", "flag1"], ["b"], pp.FDB_ERR_UNSUPPORTED, []),
               (["utf8", "binary"], ["d"], pp.FDB_ERR_UNSUPPORTED, []),
               (["utf8", "binary"], ["x"], pp.FDB_ERR_UNSUPPORTED, []),  # (also where the field is no sorting column)
               ([], ["k"], pp.FDB_ERR_INVALID, []),
               (["g0", "g1"], [], pp.FDB_ERR_INVALID, ["order expression"]),
               (["g0", "g1"], [pp.OrderCol(None, 0, 0, 0)], pp.FDB_ERR_INVALID, ["name"]),
               (["g0", "g1"], [pp.OrderCol(b"k", 0, 2, 0)], pp.FDB_ERR_INVALID, ["direction"]),
               (["big"] * 2048, ["k"], pp.FDB_ERR_INVALID, ["2^31 - 1"])]
        for names, order_by, code, texts in bad:
            with pytest.raises(pp.FdbError) as e:
                pp.ResidentBatch.merge_named([made[n] for n in names], order_by)
            assert e.value.code == code, (names, order_by, str(e.value))
            for text in texts:
                assert text in str(e.value), (names, order_by, str(e.value))
            assert pp.live_allocations() == before, (names, order_by)
            small_merge_works()
        # what the binding cannot express: a null record, a null order list, a null result pointer
        out = ctypes.c_void_p()
        one = (pp.OrderCol * 1)(pp.OrderCol(b"k", 0, 0, 0))
        handles = (ctypes.c_void_p * 2)(made["g0"].handle, None)
        assert L.fdb_batches_merge_named(handles, 2, one, 1, 0, ctypes.byref(out)) == pp.FDB_ERR_INVALID and b"record 1 is null" in L.fdb_last_error()
        handles = (ctypes.c_void_p * 2)(made["g0"].handle, made["g1"].handle)
        assert L.fdb_batches_merge_named(handles, 2, None, 1, 0, ctypes.byref(out)) == pp.FDB_ERR_INVALID
        assert L.fdb_batches_merge_named(handles, 2, one, -1, 0, ctypes.byref(out)) == pp.FDB_ERR_INVALID
        assert L.fdb_batches_merge_named(handles, 2, one, 1, 0, None) == pp.FDB_ERR_INVALID
        assert not out.value
        if pp.device_count() > 1:  # records on different devices
            far = pp.ResidentBatch(recs["g1"], device=1)
            try:
                with pytest.raises(pp.FdbError) as e:
                    pp.ResidentBatch.merge_named([made["g0"], far], ["k"])
                assert e.value.code == pp.FDB_ERR_INVALID and "different device" in str(e.value)
            finally:
                far.close()
        small_merge_works()
        assert pp.live_allocations() == before
    finally:
        for rb in made.values():
            rb.close()


# ---- 11. OrderedSynchronizer -------------------------------------------------------------------------------------------------------------------
SOURCE = 600


def one_row(name, value):
    return pa.RecordBatch.from_arrays([pa.array([value], type=pa.int64())], names=[name])


def test_ordered_synchronizer_round_robin_like_the_reference_test():
    """TestOrderedSynchronizer driven from one thread: inputs 0 and 4 finish without pushing, the other six draw consecutive values and
    push one-row records. Nothing is emitted before a round is complete; everything emitted, concatenated, is the source in order."""
    inputs, name = ORDERED_SYNCHRONIZER["inputs"], ORDERED_SYNCHRONIZER["order_by"]
    idle = ORDERED_SYNCHRONIZER["finish_without_pushing"]
    osync, rounds = pp.OrderedSynchronizer(inputs, [Col(name)]), osync_oracle.Rounds(inputs)
    emitted, held, cursor = [], [], 0
    try:
        for i in idle:
            merged, done = osync.Finish(i)
            assert (merged, done) == rounds.finish(i) == (None, False)
        pushing = [i for i in range(inputs) if i not in idle]
        while cursor < SOURCE:
            for i in pushing:
                rb = pp.ResidentBatch(one_row(name, cursor))
                held.append(rb)
                cursor += 1
                merged, want = osync.Callback(i, rb), rounds.push(i, cursor - 1)
                assert (merged is None) == (want is None), (i, cursor)
                if merged is not None:
                    emitted += merged.to_arrow().column(name).to_pylist()
                    assert emitted[-len(want):] == [v for _, v in want]
                    merged.close()
                    for h in held:
                        h.close()
                    held = []
        assert cursor == SOURCE and emitted == list(range(SOURCE))
        for k, i in enumerate(pushing):
            merged, done = osync.Finish(i)
            assert merged is None and done == (k == len(pushing) - 1) and (None, done) == rounds.finish(i)
        with pytest.raises(pp.FdbError) as e:
            osync.Finish(pushing[0])
        assert e.value.code == pp.FDB_ERR_STATE and "too many OrderedSynchronizer Finish calls" in str(e.value)
    finally:
        osync.Close()
        for h in held:
            h.close()


def test_ordered_synchronizer_from_six_threads():
    """The same with one thread per pushing input. The library does not block: a barrier after every push stands where the reference's
    wait channel stands, so each round holds one record per thread — whichever thread arrives last completes it."""
    inputs, name = ORDERED_SYNCHRONIZER["inputs"], ORDERED_SYNCHRONIZER["order_by"]
    idle = ORDERED_SYNCHRONIZER["finish_without_pushing"]
    pushing = [i for i in range(inputs) if i not in idle]
    osync = pp.OrderedSynchronizer(inputs, [Col(name)])
    lock, barrier = threading.Lock(), threading.Barrier(len(pushing))
    state = {"cursor": 0, "done": 0}
    emitted, errors = [], []

    def run(i):
        try:
            mine = []
            while True:
                with lock:
                    v = state["cursor"]
                    state["cursor"] += 1
                if v >= SOURCE:
                    merged, done = osync.Finish(i)
                    assert merged is None
                    with lock:
                        state["done"] += int(done)
                    return
                rb = pp.ResidentBatch(one_row(name, v))
                mine.append(rb)
                merged = osync.Callback(i, rb)
                if merged is not None:
                    with lock:
                        emitted.append(merged.to_arrow().column(name).to_pylist())
                    merged.close()
                barrier.wait()  # the round is merged: everyone's record is their own again
                for h in mine:
                    h.close()
                mine = []
        except BaseException as e:  # noqa: BLE001
            errors.append(e)
            barrier.abort()

    try:
        for i in idle:
            assert osync.Finish(i) == (None, False)
        threads = [threading.Thread(target=run, args=(i,)) for i in pushing]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        assert not errors, errors
        assert state["done"] == 1  # `done` on the last finish only
        assert all(r == sorted(r) and len(r) == len(pushing) for r in emitted)
        assert [v for r in sorted(emitted, key=lambda r: r[0]) for v in r] == list(range(SOURCE))
    finally:
        osync.Close()


def test_ordered_synchronizer_rounds_finishes_schemas_and_errors():
    rng = np.random.default_rng(111)
    order_by = [DynCol("labels"), (Col("t"), True)]

    def rec(n, labels):
        cols = {"t": pa.array(rng.integers(0, 20, n), type=pa.int64())}
        for name in labels:
            cols["labels." + name] = dict_column(rng, n, null_mask(rng, n), [b"u", b"v" + name.encode(), b"w"])
        return pa.RecordBatch.from_arrays(list(cols.values()), names=list(cols.keys()))

    made = []

    def resident(record):
        made.append(pp.ResidentBatch(record))
        return made[-1]

    def emitted(merged, records):
        assert merged is not None
        made.append(merged)
        got = merged.to_arrow()
        want = osync_oracle.merge(records, order_by)
        assert_decoded_same(got, want)
        return got

    osync = pp.OrderedSynchronizer(3, order_by)
    try:
        # round 1: schemas differ between the inputs; the records are merged in INPUT order, whoever arrives first
        r1 = ordered_inputs([rec(65, "ac"), rec(tile(1) + 1, "b"), rec(3, "abc")], order_by)
        assert osync.Callback(2, resident(r1[2])) is None and osync.Callback(0, resident(r1[0])) is None
        with pytest.raises(pp.FdbError) as e:  # a second push of an input that already waits
            osync.Callback(0, resident(r1[0]))
        assert e.value.code == pp.FDB_ERR_STATE and "input 0" in str(e.value)
        got = emitted(osync.Callback(1, resident(r1[1])), r1)
        assert got.schema.names == ["labels.a", "labels.b", "labels.c", "t", "src", "row"]
        # round 2: other schemas than round 1's; completed by a Finish (running == waiting)
        r2 = ordered_inputs([rec(70, "d"), rec(64, "")], order_by)
        assert osync.Callback(0, resident(r2[0])) is None and osync.Callback(1, resident(r2[1])) is None
        merged, done = osync.Finish(2)
        got = emitted(merged, r2)
        assert not done and got.schema.names == ["labels.d", "t", "src", "row"]
        with pytest.raises(pp.FdbError) as e:  # a push after the input's finish
            osync.Callback(2, resident(r2[0]))
        assert e.value.code == pp.FDB_ERR_STATE and "finished" in str(e.value)
        with pytest.raises(pp.FdbError) as e:
            osync.Finish(2)
        assert e.value.code == pp.FDB_ERR_STATE
        with pytest.raises(pp.FdbError) as e:
            osync.Callback(3, resident(r2[0]))
        assert e.value.code == pp.FDB_ERR_INVALID
        # round 3 fails: input 1's record is not ordered — the error goes to the completing call, the round is discarded
        t = np.arange(65, dtype=np.int64)  # ascending, the order asks for descending
        unordered = pa.RecordBatch.from_arrays([pa.array(t), pa.array(np.ones(65, dtype=np.int64)), pa.array(t)], names=["t", "src", "row"])
        assert osync.Callback(0, resident(r2[0])) is None
        with pytest.raises(pp.FdbError) as e:
            osync.Callback(1, resident(unordered))
        assert e.value.code == pp.FDB_ERR_INVALID and "record 1" in str(e.value) and "row 1 " in str(e.value), str(e.value)
        # … and the synchronizer goes on: round 4, then the finishes
        r4 = ordered_inputs([rec(5, "a"), rec(9, "e")], order_by)
        assert osync.Callback(1, resident(r4[1])) is None
        emitted(osync.Callback(0, resident(r4[0])), r4)
        assert osync.Callback(0, resident(r4[0])) is None
        merged, done = osync.Finish(1)  # input 0 waits alone: its record comes out as the round
        emitted(merged, r4[:1])
        assert not done
        assert osync.Finish(0) == (None, True)
        with pytest.raises(pp.FdbError) as e:
            osync.Finish(0)
        assert e.value.code == pp.FDB_ERR_STATE and "too many OrderedSynchronizer Finish calls" in str(e.value)
    finally:
        osync.Close()
        for rb in made:
            rb.close()
    # bad constructions
    for inputs, order in ((0, ["t"]), (2, []), (2, [pp.OrderCol(None, 0, 0, 0)]), (2, [pp.OrderCol(b"t", 0, 2, 0)])):
        with pytest.raises(pp.FdbError) as e:
            pp.OrderedSynchronizer(inputs, order)
        assert e.value.code == pp.FDB_ERR_INVALID, (inputs, order)


# ---- 12. nothing is left behind ----------------------------------------------------------------------------------------------------------------
def test_everything_is_released(allocations_before_this_module):
    small_merge_works()
    gc.collect()
    assert pp.live_allocations() == allocations_before_this_module
