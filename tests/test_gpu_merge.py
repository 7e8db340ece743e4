"""The device MergeRecords over resident records (fdb_batches_merge, ResidentBatch.merge): the result compared with the stable order of the
concatenation as tests/merge_oracle.py gives it (the reference's comparison restated pairwise in Python; no code shared with the library).

Every input carries two int64 columns that are no sorting columns — `src`, the record's place in the call, and `row`, the row's place in
the record — so the order of ties is visible in the result: equal rows must come out in record order, then row order. Results are
compared column by column after dictionary decode: NULL positions exactly, values bit for bit (float64 by its bits, on the valid rows).

Row counts follow the kernels: with T = merge_tile_rows(W) the output tile of the merge kernel (2048 rows for keys of one or two words,
512 for five), records of 0, 1, 2 rows, 63 / 64 / 65 (a validity word of the gather), T - 1 / T / T + 1 (a tile ∓ one row) and 3 T + 1
(several tiles and a one-row tail); K = 1 (no merge), 2, 3 and 5 (an odd run sits out a round and changes buffers), 8 (three full
rounds). Inputs are ordered beforehand by the oracle, and the raw slots under their NULLs are then filled with junk — distinct, non-zero,
dictionary indices far outside the dictionary — which a kernel that looked at them would sort by, or index a table with."""
import gc

import numpy as np
import pyarrow as pa
import pytest

from frostdb_amd import physicalplan as pp
from frostdb_amd.logicalplan import Col, Sum
from tests import merge_oracle, sort_oracle
from tests.golden.merge_cases import CASES as GOLDEN_CASES
from tests.test_gpu_sort import COMBOS, KINDS, dict_column, make_column, null_mask, with_nulls
from tests.test_merge_cpu import golden_columns, golden_record

pytestmark = pytest.mark.gpu


def tile(words=1):
    return pp.merge_tile_rows(words)


# ---- records ---------------------------------------------------------------------------------------------------------------------------------
def junk_under_nulls(col: pa.Array) -> pa.Array:
    """`col` with the raw slots under its NULLs overwritten: distinct non-zero values, dictionary indices far outside the dictionary."""
    if col.null_count == 0:
        return col
    n = len(col)
    mask = np.asarray(col.is_null())
    if pa.types.is_dictionary(col.type):
        idx = np.asarray(col.indices.fill_null(0)).astype(np.uint32)
        idx[mask] = (0xF0000000 + np.arange(n, dtype=np.uint32) * 7 + 1)[::-1][mask]
        return pa.DictionaryArray.from_arrays(with_nulls(idx, mask, pa.uint32()), col.dictionary, safe=False)
    if pa.types.is_string(col.type) or pa.types.is_binary(col.type):
        return col  # (a plain column has no slot under a NULL)
    fill = 0.0 if pa.types.is_floating(col.type) else 0
    v = np.asarray(col.fill_null(fill)).copy()
    v[mask] = (np.arange(n)[::-1] * 3 + 1).astype(v.dtype)[mask]
    return with_nulls(v, mask, col.type)


def ordered_inputs(records, columns):
    """Every record put into the order of `columns` (by position) by the oracle, junk under its NULLs, tagged with src and row."""
    out = []
    for s, rec in enumerate(records):
        order = sort_oracle.sort_indices(rec, columns)
        rec = rec.take(pa.array(order, type=pa.int64()))
        cols = [junk_under_nulls(c) for c in rec.columns]
        n = rec.num_rows
        cols += [pa.array(np.full(n, s, dtype=np.int64)), pa.array(np.arange(n, dtype=np.int64))]
        out.append(pa.RecordBatch.from_arrays(cols, names=rec.schema.names + ["src", "row"]))
    return out


def assert_decoded_same(got: pa.RecordBatch, want: pa.RecordBatch, what=""):
    assert got.schema.names == want.schema.names, what
    assert got.num_rows == want.num_rows, (what, got.num_rows, want.num_rows)
    for name in want.schema.names:
        g, w = merge_oracle.decoded(got.column(name)), merge_oracle.decoded(want.column(name))
        assert g.type == w.type, (what, name, g.type, w.type)
        gn, wn = np.asarray(g.is_null()), np.asarray(w.is_null())
        assert (gn == wn).all(), (what, name, "NULL positions", np.flatnonzero(gn != wn)[:5])
        if pa.types.is_binary(g.type):
            assert g.to_pylist() == w.to_pylist(), (what, name)
            continue
        fill = 0.0 if pa.types.is_floating(g.type) else 0
        gv = np.asarray(g.fill_null(fill)).view(np.uint64)[~gn]
        wv = np.asarray(w.fill_null(fill)).view(np.uint64)[~wn]
        assert (gv == wv).all(), (what, name, np.flatnonzero(gv != wv)[:5])


def check_merge(records, columns, limit=0, what=""):
    """`records`: ordered host records; `columns`: (position[, descending[, nulls_first]]). Returns the merged record on the host."""
    rbs = [pp.ResidentBatch(r) for r in records]
    try:
        out = pp.ResidentBatch.merge(rbs, columns, limit)
    finally:
        for rb in rbs:
            rb.close()  # the result owns its bytes
    try:
        got = out.to_arrow()
    finally:
        out.close()
    assert_decoded_same(got, merge_oracle.merge(records, columns, limit), what)
    return got


def int_records(counts, seed, distinct=9):
    rng = np.random.default_rng(seed)
    return [pa.RecordBatch.from_arrays([pa.array(rng.integers(-distinct // 2, distinct // 2 + 1, n), type=pa.int64())], names=["k"]) for n in counts]


# ---- 1. the reference's vectors ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", GOLDEN_CASES, ids=[c["id"] for c in GOLDEN_CASES])
def test_golden_vectors(case):
    columns = golden_columns(case)
    records = [golden_record(rows) for rows in case["records"]]
    tagged = ordered_inputs(records, columns)
    for r, t in zip(records, tagged):
        assert t.column("row").to_pylist() == list(range(r.num_rows)), case["cite"]  # the reference's inputs ARE ordered
    got = check_merge(tagged, columns, case["limit"], case["id"])
    want = golden_record(case["expected"])
    assert got.column("number").to_pylist() == want.column("number").to_pylist(), case["cite"]
    assert got.column("text").to_pylist() == want.column("text").to_pylist(), case["cite"]


# ---- 2. K and row counts -----------------------------------------------------------------------------------------------------------------------
def count_cases():
    T = tile(1)  # (host arithmetic: collecting the cases touches no device)
    return [("k1", [T + 1]), ("k1_empty", [0]), ("k2", [T - 1, 65]), ("k2_all_empty", [0, 0]), ("k3", [3 * T + 1, 1, T]), ("k5", [2, 63, 64, 0, T + 1]),
            ("k5_one_among_empty", [0, 0, T + 1, 0, 0]), ("k8", [0, 1, 2, 63, 64, 65, T - 1, T]), ("k8_last_empty", [T, 1, 65, 2, T + 1, 64, 63, 0])]


@pytest.mark.parametrize("name,counts", count_cases(), ids=[c[0] for c in count_cases()])
def test_record_counts_and_row_counts(name, counts):
    records = ordered_inputs(int_records(counts, seed=len(counts) * 100 + sum(counts)), [(0,)])
    got = check_merge(records, [(0,)], 0, name)
    assert got.num_rows == sum(counts)
    if sum(counts):  # ties in record order, then row order
        k, s, r = (np.asarray(got.column(c)) for c in ("k", "src", "row"))
        same = k[1:] == k[:-1]
        assert ((s[1:] > s[:-1]) | ((s[1:] == s[:-1]) & (r[1:] > r[:-1])))[same].all()


# ---- 3. column kinds ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nullable", [False, True], ids=["no_nulls", "nulls"])
@pytest.mark.parametrize("kind", KINDS)
def test_every_sorting_column_kind_at_k3(kind, nullable):
    counts = [tile(1) + 1, 65, 300]
    raw = [pa.RecordBatch.from_arrays([make_column(kind, n, nullable, seed=31 * s)], names=["k"]) for s, n in enumerate(counts)]
    for descending, nulls_first in COMBOS:
        columns = [(0, descending, nulls_first)]
        check_merge(ordered_inputs(raw, columns), columns, 0, (kind, nullable, descending, nulls_first))


def test_nulls_in_one_input_only():
    """The NULL bit is in every input's keys as soon as ONE input has a NULL in the column."""
    raw = [pa.RecordBatch.from_arrays([make_column("int64", n, nullable, seed=s), make_column("dict_binary", n, not nullable, seed=s)], names=["i", "d"])
           for s, (n, nullable) in enumerate([(300, False), (65, True), (tile(2) + 1, False)])]
    for columns in ([(0, False, True), (1, True, False)], [(1, False, True), (0, True, True)]):
        check_merge(ordered_inputs(raw, columns), columns, 0, columns)


# ---- 4. ties -----------------------------------------------------------------------------------------------------------------------------------
def test_all_keys_equal_is_pure_record_order():
    n = tile(1) + 1
    records = ordered_inputs([pa.RecordBatch.from_arrays([pa.array(np.full(n, 42, dtype=np.int64))], names=["k"]) for _ in range(3)], [(0,)])
    got = check_merge(records, [(0,)])
    assert got.column("src").to_pylist() == [0] * n + [1] * n + [2] * n
    assert got.column("row").to_pylist() == list(range(n)) * 3


def test_single_valued_dictionary_key_has_no_key_words():
    """One distinct entry, no NULLs: the key has no bits at all, everything ties, the result is the concatenation."""
    counts = [70, tile(0) + 1, 3]
    records = ordered_inputs([pa.RecordBatch.from_arrays([pa.DictionaryArray.from_arrays(pa.array(np.zeros(n, dtype=np.uint32)), pa.array([b"only"], type=pa.binary()))], names=["d"])
                              for n in counts], [(0,)])
    got = check_merge(records, [(0, True)])
    assert got.column("src").to_pylist() == [0] * counts[0] + [1] * counts[1] + [2] * counts[2]


def test_first_column_ties_across_a_tile_boundary():
    """Two int64 columns (two key words): the first has three long stretches of equal values, one of them over the first tile boundary of
    the output, so the partition's diagonal search is decided by the second word there."""
    T = tile(2)
    rng = np.random.default_rng(5)
    counts = [T + 1, T - 1, 130]
    raw = [pa.RecordBatch.from_arrays([pa.array(rng.integers(0, 3, n), type=pa.int64()), pa.array(rng.integers(0, 50, n), type=pa.int64())], names=["a", "b"]) for n in counts]
    for columns in ([(0,), (1,)], [(0, True), (1,)], [(0,), (1, True)]):
        check_merge(ordered_inputs(raw, columns), columns, 0, columns)


def test_key_of_five_words():
    """nullable int64, nullable int64, int64: NULL bit | value | NULL bit | value | value — five words, the run-time-W merge kernel."""
    T = tile(5)
    assert T < tile(1)
    rng = np.random.default_rng(6)
    counts = [T + 1, T - 1, 70, 3 * T + 1]
    few = np.array([np.iinfo(np.int64).min, -1, 0, np.iinfo(np.int64).max], dtype=np.int64)
    raw = []
    for n in counts:
        cols = [with_nulls(rng.choice(few, n), null_mask(rng, n), pa.int64()), with_nulls(rng.choice(few[:2], n), null_mask(rng, n), pa.int64()),
                pa.array(rng.integers(0, 4, n), type=pa.int64())]
        raw.append(pa.RecordBatch.from_arrays(cols, names=["a", "b", "c"]))
    for columns in ([(0,), (1,), (2,)], [(0, True, True), (1, False, True), (2, True)]):
        check_merge(ordered_inputs(raw, columns), columns, 0, columns)


# ---- 5. dictionaries ---------------------------------------------------------------------------------------------------------------------------
def dict_record(rng, n, entries, other_entries, typ=pa.binary()):
    """a dictionary sorting column `d` and a dictionary column `o` that is no sorting column (only the gather translates it)"""
    return pa.RecordBatch.from_arrays([dict_column(rng, n, null_mask(rng, n), entries, typ), dict_column(rng, n, null_mask(rng, n), other_entries, typ)], names=["d", "o"])


def merged_dictionary(records, columns, name):
    rbs = [pp.ResidentBatch(r) for r in records]
    out = pp.ResidentBatch.merge(rbs, columns)
    for rb in rbs:
        rb.close()
    got = out.to_arrow()
    out.close()
    assert_decoded_same(got, merge_oracle.merge(records, columns))
    return got.column(name).dictionary.to_pylist()


@pytest.mark.parametrize("descending", [False, True], ids=["asc", "desc"])
def test_disjoint_and_overlapping_dictionaries(descending):
    rng = np.random.default_rng(11)
    columns = [(0, descending, descending)]
    # disjoint entries; byte order interleaves the records' entries
    sets = [[b"b", b"e", b"h"], [b"a", b"d", b"g", b"\xff"], [b"c", b"f", b""]]
    records = ordered_inputs([dict_record(rng, n, e, [b"o%d" % s, b"shared"]) for s, (n, e) in enumerate(zip([tile(1) + 1, 300, 65], sets))], columns)
    assert merged_dictionary(records, columns, "d") == sets[0] + sets[1] + sets[2]  # the union, first seen first
    assert merged_dictionary(records, columns, "o") == [b"o0", b"shared", b"o1", b"o2"]
    # overlapping entries in different index orders
    sets = [[b"m", b"a", b"z"], [b"z", b"m", b"k"], [b"k", b"a", b"m", b"z"]]
    records = ordered_inputs([dict_record(rng, n, e, e[::-1]) for n, e in zip([300, tile(1) + 1, 65], sets)], columns)
    assert merged_dictionary(records, columns, "d") == [b"m", b"a", b"z", b"k"]
    assert merged_dictionary(records, columns, "o") == [b"z", b"a", b"m", b"k"]


def test_a_dictionary_with_duplicate_entries():
    """[b"b", b"a", b"b"]: entries 0 and 2 hold the same bytes — they tie, the second column decides; the union holds b"b" once."""
    rng = np.random.default_rng(12)
    columns = [(0,), (1, True)]
    recs = []
    for n, entries in [(300, [b"b", b"a", b"b"]), (tile(1) + 1, [b"a", b"c"]), (65, [b"c", b"b"])]:
        d = pa.DictionaryArray.from_arrays(pa.array(rng.integers(0, len(entries), n), type=pa.uint32()), pa.array(entries, type=pa.binary()))
        recs.append(pa.RecordBatch.from_arrays([d, pa.array(rng.integers(0, 5, n), type=pa.int64())], names=["d", "v"]))
    records = ordered_inputs(recs, columns)
    assert merged_dictionary(records, columns, "d") == [b"b", b"a", b"c"]


def test_one_shared_dictionary_is_the_outputs_untranslated():
    rng = np.random.default_rng(13)
    entries = [b"q", b"c", b"x", b"c", b"never-used"]  # a duplicate and an unreferenced entry: they stay, nothing is rebuilt
    columns = [(0, True, True)]
    recs = []
    for n in (65, tile(1) + 1, 300):
        idx = rng.integers(0, 4, n).astype(np.uint32)
        recs.append(pa.RecordBatch.from_arrays([pa.DictionaryArray.from_arrays(with_nulls(idx, null_mask(rng, n), pa.uint32()), pa.array(entries, type=pa.binary()))], names=["d"]))
    records = ordered_inputs(recs, columns)
    assert merged_dictionary(records, columns, "d") == entries
    # utf8 in one record, binary in another: refused
    mixed = [pa.RecordBatch.from_arrays([pa.DictionaryArray.from_arrays(pa.array([0, 1], type=pa.uint32()), pa.array(["a", "b"], type=t))], names=["d"]) for t in (pa.string(), pa.binary())]
    rbs = [pp.ResidentBatch(r) for r in mixed]
    try:
        with pytest.raises(pp.UnsupportedError):
            pp.ResidentBatch.merge(rbs, ["d"])
    finally:
        for rb in rbs:
            rb.close()


# ---- 6. limit ----------------------------------------------------------------------------------------------------------------------------------
def test_limits():
    T = tile(1)
    counts = [T + 1, 2 * T + 3, 65]
    total = sum(counts)
    records = ordered_inputs(int_records(counts, seed=21, distinct=200), [(0, True)])
    rbs = [pp.ResidentBatch(r) for r in records]
    try:
        want_all = merge_oracle.merge(records, [(0, True)])
        for limit in (1, T, total - 1, total, total + 5):
            out = pp.ResidentBatch.merge(rbs, [("k", True)], limit)
            got = out.to_arrow()
            out.close()
            assert got.num_rows == min(limit, total)
            assert_decoded_same(got, want_all.slice(0, min(limit, total)), limit)
        one = pp.ResidentBatch.merge(rbs[:1], ["k"], 7)  # K == 1: Limit of the record
        assert_decoded_same(one.to_arrow(), records[0].slice(0, 7))
        one.close()
    finally:
        for rb in rbs:
            rb.close()


# ---- 7. refusals -------------------------------------------------------------------------------------------------------------------------------
def test_refusals_name_their_reason_and_leave_the_device_usable():
    T = tile(1)
    good = ordered_inputs(int_records([300, T + 1, 65], seed=31), [(0,)])
    k = np.sort(np.random.default_rng(32).integers(0, 1000, T + 1))
    k[1500], k[1501] = k[1501] + 5, k[1500]  # row 1501 sorts before row 1500 — and nothing earlier is out of order
    assert (np.diff(k[:1501]) >= 0).all() and k[1501] < k[1500]
    unordered = pa.RecordBatch.from_arrays([pa.array(k, type=pa.int64()), pa.array(np.ones(T + 1, dtype=np.int64)), pa.array(np.arange(T + 1, dtype=np.int64))], names=["k", "src", "row"])
    renamed = pa.RecordBatch.from_arrays(good[2].columns, names=["k", "source", "row"])
    other_kind = pa.RecordBatch.from_arrays([good[2].column(0).cast(pa.float64())] + good[2].columns[1:], names=good[2].schema.names)
    shorter = pa.RecordBatch.from_arrays(good[2].columns[:2], names=["k", "src"])
    flags = [pa.RecordBatch.from_arrays([pa.array(np.arange(n) >= n // 2), pa.array(np.arange(n, dtype=np.int64))], names=["b", "v"]) for n in (10, 20)]
    made = {name: pp.ResidentBatch(r) for name, r in [("g0", good[0]), ("g1", good[1]), ("g2", good[2]), ("unordered", unordered), ("renamed", renamed), ("other_kind", other_kind),
                                                      ("shorter", shorter), ("f0", flags[0]), ("f1", flags[1])]}
    try:
        gc.collect()
        before = pp.live_allocations()
        bad = [(["g0", "unordered", "g2"], ["k"], pp.FDB_ERR_INVALID, ["record 1", "row 1501"]),
               (["g0", "g1", "renamed"], ["k"], pp.FDB_ERR_INVALID, ["record 2"]),
               (["g0", "other_kind"], ["k"], pp.FDB_ERR_INVALID, ["record 1"]),
               (["g0", "shorter"], ["k"], pp.FDB_ERR_INVALID, ["record 1"]),
               (["f0", "f1"], ["b"], pp.FDB_ERR_UNSUPPORTED, []),
               ([], ["k"], pp.FDB_ERR_INVALID, []),
               (["g0", "g1"], [], pp.FDB_ERR_INVALID, ["at least one column"]),
               (["g0", "g1"], [7], pp.FDB_ERR_INVALID, ["index"]),
               (["g0", "g1"], [pp.SortCol(0, 2, 0)], pp.FDB_ERR_INVALID, ["direction"])]
        for names, columns, code, texts in bad:
            with pytest.raises(pp.FdbError) as e:
                pp.ResidentBatch.merge([made[n] for n in names], columns)
            assert e.value.code == code, (names, columns, str(e.value))
            for text in texts:
                assert text in str(e.value), (names, columns, str(e.value))
            assert pp.live_allocations() == before, (names, columns)
        out = pp.ResidentBatch.merge([made["g0"], made["g1"], made["g2"]], ["k"])  # a later valid call on the same device
        assert_decoded_same(out.to_arrow(), merge_oracle.merge(good, [(0,)]))
        out.close()
        assert pp.live_allocations() == before
    finally:
        for rb in made.values():
            rb.close()


# ---- 8. chaining -------------------------------------------------------------------------------------------------------------------------------
def test_filter_sort_merge_equals_sort_of_the_whole_and_feeds_an_ordered_plan():
    rng = np.random.default_rng(41)
    counts = [3000, tile(1) + 1, 900]

    def shard(n):
        return pa.RecordBatch.from_arrays(
            [dict_column(rng, n, null_mask(rng, n), [b"c", b"a", b"d", b"b"]), dict_column(rng, n, null_mask(rng, n), [b"l%02d" % ((k * 7) % 23) for k in range(23)]),
             pa.array(rng.integers(0, 1000, n), type=pa.int64())], names=["labels.a", "labels.b", "v"])

    shards = [shard(n) for n in counts]
    whole = pa.RecordBatch.from_arrays([pa.concat_arrays([s.column(k) for s in shards]) for k in range(3)], names=shards[0].schema.names)
    groups, columns = [Col("labels.a"), Col("labels.b")], [("labels.a",), ("labels.b",)]
    filt = pp.HashAggregatePlan(Col("v") > 300, [Sum(Col("v"))], groups)
    on_device = pp.HashAggregatePlan(None, [Sum(Col("v"))], groups, ordered=True)
    on_host = pp.HashAggregatePlan(None, [Sum(Col("v"))], groups, ordered=True)
    made = []
    try:
        ordered = []
        for s in shards + [whole]:
            rb = pp.ResidentBatch(s)
            filtered = filt.FilterResident(rb)
            rb.close()
            ordered.append(filtered.sort(columns))
            filtered.close()
            made.append(ordered[-1])
        merged = pp.ResidentBatch.merge(ordered[:3], columns)
        made.append(merged)
        host_merged, host_whole = merged.to_arrow(), ordered[3].to_arrow()
        assert 0 < host_whole.num_rows < sum(counts)
        assert_decoded_same(host_merged, host_whole)  # sort of the whole == merge of the sorted shards (both stable)
        keep = np.flatnonzero(np.asarray(whole.column("v")) > 300)
        host_filtered = whole.take(pa.array(keep))
        want = host_filtered.take(pa.array(sort_oracle.sort_indices(host_filtered, [(0,), (1,)]), type=pa.int64()))
        assert_decoded_same(host_merged, want)
        on_device.Callback(merged)
        on_host.Callback(want)
        a, b = on_device.Finish(), on_host.Finish()
        assert a.num_rows == b.num_rows > 50 and a.schema.names == b.schema.names
        assert [c.to_pylist() for c in a.columns] == [c.to_pylist() for c in b.columns]
    finally:
        for rb in made:
            rb.close()
        for p in (filt, on_device, on_host):
            p.Close()


def test_everything_is_released():
    gc.collect()
    before = pp.live_allocations()
    records = ordered_inputs(int_records([3000, 70, 5000], seed=51), [(0,)])
    rbs = [pp.ResidentBatch(r) for r in records]
    out = pp.ResidentBatch.merge(rbs, ["k"])
    assert pp.live_allocations()["device_bytes"] > before["device_bytes"]
    for rb in rbs + [out]:
        rb.close()
    assert pp.live_allocations() == before
