"""Take, Limit and the reservoir Sampler on resident records (fdb_batch_take, fdb_batch_limit, fdb_sampler_*): take against
pyarrow.RecordBatch.take, limit against the reference's exec/limit vectors and pyarrow's slice, the Sampler against the Python
restatement of its selection (tests/sampler_oracle.py) with every kept row compared to its source row, dictionary unions, dynamic
columns, chaining into filter() and the aggregate, errors and allocations.

Row counts: take_kernel and scatter_kernel run 256-thread workgroups and a wave writes one 64-bit validity word, so output lengths sit
on the byte (31 / 32 / 33), wave (63 / 64 / 65) and workgroup (257) edges and at 4097 (several workgroups + 1 row); sources of 1, 64, 65
and 5000 rows."""
import gc

import numpy as np
import pyarrow as pa
import pytest

from frostdb_amd import physicalplan as pp
from frostdb_amd.logicalplan import Col, Count, Sum
from tests import sampler_oracle
from tests.golden.limit_cases import CASES as LIMIT_CASES, TABLE as LIMIT_TABLE
from tests.test_sampler_cpu import SHAPES
from tests.util import arrow_to_pydict, dict_array, record_from_rows

pytestmark = pytest.mark.gpu

SOURCE_ROWS = [1, 64, 65, 5000]
OUT_LENGTHS = [0, 1, 31, 32, 33, 63, 64, 65, 257, 4097]


# ---- records and comparison ------------------------------------------------------------------------------------------------------------
def make_record(n: int, seed: int = 3, first_id: int = 0, words=None, extra=None) -> pa.RecordBatch:
    """Dictionary, plain-string, int64, uint64, float64 and bool columns, each with NULLs (first row NULL, ≈ 20 % of the others) and
    without, and `id` numbering the rows from `first_id`."""
    rng = np.random.default_rng(seed + 1000 * n)
    words = words or [b"w%d" % i for i in range(7)]

    def mask():
        m = rng.random(n) < 0.2
        if n:
            m[0] = True
        return m

    fspecial = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, 5e-324, 1.5, -1e308])
    cols = {"id": pa.array(np.arange(first_id, first_id + n, dtype=np.int64))}
    for suffix, nullable in (("", True), ("0", False)):
        m = mask() if nullable else None
        pick = rng.integers(0, len(words), n)
        cols["d" + suffix] = pa.DictionaryArray.from_arrays(pa.array(pick.astype(np.uint32), mask=m), pa.array(words, type=pa.binary()))
        cols["s" + suffix] = pa.array([f"s{k % 5}" * (k % 3) for k in rng.integers(0, 50, n)], type=pa.string(), mask=m)
        cols["i" + suffix] = pa.array(rng.integers(np.iinfo(np.int64).min, np.iinfo(np.int64).max, n, dtype=np.int64), mask=m)
        cols["u" + suffix] = pa.array(rng.integers(0, 2**64 - 1, n, dtype=np.uint64, endpoint=True), mask=m)
        cols["f" + suffix] = pa.array(np.where(rng.random(n) < 0.5, rng.choice(fspecial, n), rng.standard_normal(n)), mask=m)
        cols["b" + suffix] = pa.array(rng.random(n) < 0.5, mask=m)
    if extra:
        cols.update(extra)
    return pa.RecordBatch.from_arrays(list(cols.values()), names=list(cols.keys()))


def assert_same(got: pa.RecordBatch, want: pa.RecordBatch, what=""):
    """Same fields, same values bit for bit (float64 by its bits), same NULLs; a validity bitmap is present only when a NULL is."""
    assert got.schema.names == want.schema.names, what
    assert got.num_rows == want.num_rows, what
    for name, g, w in zip(want.schema.names, got.columns, want.columns):
        where = (what, name)
        assert g.null_count == w.null_count, where
        assert (g.buffers()[0] is not None) == (g.null_count > 0), where
        if pa.types.is_dictionary(w.type):
            assert pa.types.is_dictionary(g.type), where
            g, w = g.dictionary_decode(), w.dictionary_decode()
        assert g.type == w.type or (pa.types.is_binary(g.type) and pa.types.is_binary(w.type)), (where, g.type, w.type)
        if pa.types.is_floating(w.type):
            valid = np.asarray(w.is_valid())
            assert np.array_equal(np.asarray(g.is_valid()), valid), where
            gb = np.asarray(g.fill_null(0.0)).view(np.uint64)[valid]
            wb = np.asarray(w.fill_null(0.0)).view(np.uint64)[valid]
            assert np.array_equal(gb, wb), where
        else:
            assert g.to_pylist() == w.to_pylist(), where


@pytest.fixture(scope="module")
def sources():
    recs = {n: make_record(n) for n in SOURCE_ROWS}
    rbs = {n: pp.ResidentBatch(r) for n, r in recs.items()}
    yield recs, rbs
    for rb in rbs.values():
        rb.close()


# ---- 1. take -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", SOURCE_ROWS)
def test_take_equals_pyarrow_take(sources, rows):
    recs, rbs = sources
    rec, rb = recs[rows], rbs[rows]
    rng = np.random.default_rng(rows)
    for n in OUT_LENGTHS:
        orders = {"shuffled": rng.integers(0, rows, n), "reversed": np.resize(np.arange(rows - 1, -1, -1), n), "all-equal": np.full(n, rows - 1)}
        for order, idx in orders.items():
            out = rb.take(idx)
            try:
                assert out.num_rows == n
                assert_same(out.to_arrow(), rec.take(pa.array(idx, type=pa.int32())), (rows, n, order))
            finally:
                out.close()


def test_take_outlives_its_input_and_chains():
    rec = make_record(300, seed=9)
    rb = pp.ResidentBatch(rec)
    first = rb.take(np.arange(299, -1, -1))
    rb.close()  # the output owns its bytes
    second = first.take([5, 5, 0, 299])
    first.close()
    assert_same(second.to_arrow(), rec.take(pa.array([294, 294, 299, 0], type=pa.int32())))
    second.close()


def test_take_refuses_indices_outside_the_record(sources):
    _, rbs = sources
    for rows in (1, 65):
        for bad in ([-1], [rows], [0, rows, 0], [0, -1]):
            with pytest.raises(pp.FdbError) as e:
                rbs[rows].take(bad)
            assert e.value.code == pp.FDB_ERR_INVALID, bad
            assert "take" in str(e.value)


# ---- 2. limit ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", LIMIT_CASES, ids=[c["id"] for c in LIMIT_CASES])
def test_limit_golden_vectors(case):
    rec = record_from_rows(LIMIT_TABLE["cols"], [list(r) for r in LIMIT_TABLE["rows"]])
    plan = pp.Projection([Col(c) for c in case["select"]])
    limiter = pp.Limiter(case["count"])
    assert limiter.Draw() == "Limit(%d)" % case["count"]
    want = [tuple(None if v is None else v.encode() for v in row) for row in case["expected"]]
    rb = pp.ResidentBatch(rec)
    try:
        projected = plan.ProjectResident(rb)
        limited = limiter.CallbackResident(projected)
        projected.close()
        got = limited.to_arrow()
        limited.close()
        host = limiter.Callback(plan.Callback(rec))
        for out in (got, host):
            assert out.schema.names == case["select"]
            d = arrow_to_pydict(out)
            assert [tuple(d[c][i] for c in case["select"]) for i in range(out.num_rows)] == want
    finally:
        rb.close()
        plan.Close()


def test_limit_applies_to_each_record():
    """limit.go:63-98 never decrements its count: two records in turn keep `count` rows EACH."""
    limiter = pp.Limiter(5)
    for seed in (1, 2):
        rec = make_record(40, seed=seed)
        assert_same(limiter.Callback(rec), rec.slice(0, 5))


@pytest.mark.parametrize("count", [0, 1, 7, 8, 9, 64, 65, 100, 101, 2**63])
def test_limit_equals_slice(count):
    rec = make_record(100, seed=5)
    rb = pp.ResidentBatch(rec)
    out = pp.Limiter(count).CallbackResident(rb)
    rb.close()  # the output owns its bytes, whole-record copies included
    try:
        assert out.num_rows == min(count, 100)
        want = rec.slice(0, min(count, 100))
        assert_same(out.to_arrow(), pa.RecordBatch.from_arrays([pa.concat_arrays([c]) for c in want.columns], names=want.schema.names), count)
    finally:
        out.close()


def test_limit_of_a_zero_row_record():
    rec = make_record(0)
    rb = pp.ResidentBatch(rec)
    for count in (0, 3):
        out = pp.Limiter(count).CallbackResident(rb)
        got = out.to_arrow()
        out.close()
        assert got.num_rows == 0 and got.schema.names == rec.schema.names
    rb.close()


# ---- 3. sampler --------------------------------------------------------------------------------------------------------------------------
def sampler_records(lens, words_of=None):
    """Records of `lens` rows whose `id` numbers all rows; record r's dictionary differs from and overlaps its neighbours'."""
    recs, first = [], 0
    for r, n in enumerate(lens):
        words = [b"w%d" % (r + k) for k in range(4)] if words_of is None else words_of(r)
        recs.append(make_record(n, seed=17 + r, first_id=first, words=words))
        first += n
    return recs


def expected_rows(recs, ids):
    whole = pa.Table.from_batches([r for r in recs if r.num_rows] or recs[:1]).combine_chunks()
    taken = whole.take(pa.array(ids, type=pa.int64())).combine_chunks()
    return taken.to_batches()[0] if taken.num_rows else None


@pytest.mark.parametrize("size,lens", SHAPES, ids=[f"K{k}-{'_'.join(map(str, l))}" for k, l in SHAPES])
def test_sampler_keeps_the_restatements_rows(size, lens):
    """The ids in slot order equal the restatement's, every other column holds its source row's values. (3, [3, 5000]) draws ≈ 22
    replacements for 3 slots out of ONE record — the same slot several times in one launch, which the host's last-pair pass resolves."""
    recs = sampler_records(lens)
    rbs = [pp.ResidentBatch(r) for r in recs]
    try:
        for seed in (0, 1, 7):
            ids = sampler_oracle.sample(seed, size, lens)
            s = pp.ReservoirSampler(size, seed)
            assert s.Draw() == "Reservoir Sampler (%d)" % size
            try:
                for rec, rb in zip(recs, rbs):
                    if seed == 1:
                        s.Callback(rec)           # host records, staged
                    else:
                        s.CallbackResident(rb)
                got = s.Finish()
                res = s.FinishResident()
                again = res.to_arrow()
                res.close()
            finally:
                s.Close()
            if not ids:
                assert got.num_rows == 0 and got.num_columns == 0 and again.num_rows == 0 and again.num_columns == 0
                continue
            assert got.column("id").to_pylist() == ids, (seed, size, lens)
            want = expected_rows(recs, ids)
            want = want.select(sorted(want.schema.names, key=lambda s: s.encode()))
            # a column whose kept rows hold no NULL loses its bitmap in `got`; pyarrow's take keeps none either
            assert_same(got, want, (seed, size, lens))
            assert_same(again, want, (seed, size, lens))
    finally:
        for rb in rbs:
            rb.close()


def test_sampler_dictionaries_union_and_conflict():
    lens = [6, 9, 30]
    recs = sampler_records(lens, words_of=lambda r: [[b"a", b"b", b"c"], [b"c", b"d", b"a", b"e"], [b"x", b"b"]][r])
    s = pp.ReservoirSampler(8, 4)
    try:
        for r in recs:
            s.Callback(r)
        got = s.Finish()
        ids = sampler_oracle.sample(4, 8, lens)
        assert got.column("id").to_pylist() == ids
        want = expected_rows(recs, ids)
        assert got.column("d").dictionary_decode().to_pylist() == want.column("d").dictionary_decode().to_pylist()
        # first-seen order, entries compared by their bytes; entries no kept row references may stay
        entries = got.column("d").dictionary.to_pylist()
        assert entries[:5] == [b"a", b"b", b"c", b"d", b"e"] and len(set(entries)) == len(entries)
        # the same field as utf8 where it was binary: refused, the sampler's rows untouched
        clash = make_record(5, first_id=1000)
        k = clash.schema.get_field_index("d")
        clash = clash.set_column(k, "d", dict_array(["a", "b", "a", None, "c"], pa.dictionary(pa.uint32(), pa.string())))
        with pytest.raises(pp.UnsupportedError):
            s.Callback(clash)
        k = clash.schema.get_field_index("i")
        with pytest.raises(pp.UnsupportedError):  # int64 against float64
            s.Callback(make_record(5, first_id=1000).set_column(k, "i", pa.array([1.0] * 5)))
        assert s.Finish().column("id").to_pylist() == ids
    finally:
        s.Close()


def test_sampler_dynamic_columns():
    """A field only some records have, and one first seen after the reservoir filled: NULL in the rows of records without it, the
    fields of the records that have rows in the reservoir, sorted by name."""
    lens, size = [4, 3, 50], 6

    def rec(r, first, n):
        cols = {"id": pa.array(np.arange(first, first + n, dtype=np.int64))}
        if r != 2:
            cols["labels.a"] = dict_array([f"a{k % 3}" for k in range(n)])
        if r == 1:
            cols["labels.x"] = dict_array([None if k == 1 else f"x{k}" for k in range(n)])
        if r == 2:
            cols["labels.z"] = dict_array([f"z{k % 4}" for k in range(n)])
            cols["Value"] = pa.array(np.arange(n, dtype=np.float64))
        return pa.RecordBatch.from_arrays(list(cols.values()), names=list(cols.keys()))

    recs = [rec(0, 0, 4), rec(1, 4, 3), rec(2, 7, 50)]
    of_record = lambda i: 0 if i < 4 else 1 if i < 7 else 2  # noqa: E731
    seeds = [sd for sd in range(100) if {of_record(i) for i in sampler_oracle.sample(sd, size, lens)} == {0, 1, 2}][:2]
    only_late = [sd for sd in range(400) if {of_record(i) for i in sampler_oracle.sample(sd, size, lens)} == {2}][:1]
    assert len(seeds) == 2 and len(only_late) == 1
    for seed in seeds + only_late:
        ids = sampler_oracle.sample(seed, size, lens)
        s = pp.ReservoirSampler(size, seed)
        try:
            for r in recs:
                s.Callback(r)
            got = s.Finish()
        finally:
            s.Close()
        names = sorted({n for i in ids for n in recs[of_record(i)].schema.names}, key=lambda n: n.encode())
        assert got.schema.names == names, seed
        assert names[0] == "Value"  # bytewise: the capital sorts first (record 2 has rows in the reservoir for every seed chosen)
        if seed in only_late:
            assert names == ["Value", "id", "labels.z"]  # no row of a record with labels.a / labels.x is left
        rows = {}
        for r in recs:
            d = arrow_to_pydict(r)
            for k in range(r.num_rows):
                rows[d["id"][k]] = {n: d[n][k] for n in r.schema.names}
        d = arrow_to_pydict(got)
        for slot, i in enumerate(ids):
            for n in names:
                assert d[n][slot] == rows[i].get(n), (seed, slot, i, n)


def test_sampler_same_seed_same_record_and_empty_cases():
    lens = [10, 300, 7]
    recs = sampler_records(lens)
    outs = []
    for _ in range(2):
        s = pp.ReservoirSampler(16, 99)
        for r in recs:
            s.Callback(r)
        s.Callback(make_record(0))  # a zero-row push is a no-op
        outs.append(s.Finish())
        s.Close()
    assert outs[0].num_rows == 16
    assert_same(outs[0], outs[1])  # (bit for bit: RecordBatch.equals would call two equal NaNs of column f different)
    for name in outs[0].schema.names:  # … and where no NaN is involved, pyarrow's own comparison agrees
        if not pa.types.is_floating(outs[0].column(name).type):
            assert outs[0].column(name).equals(outs[1].column(name)), name
    other = pp.ReservoirSampler(16, 100)
    for r in recs:
        other.Callback(r)
    assert other.Finish().column("id").to_pylist() != outs[0].column("id").to_pylist()
    other.Close()
    # nothing pushed; size 0
    for s in (pp.ReservoirSampler(4, 1), pp.ReservoirSampler(0, 1)):
        if s.size == 0:
            s.Callback(recs[0])
        got = s.Finish()
        res = s.FinishResident()
        assert got.num_rows == 0 and got.num_columns == 0 and res.num_rows == 0
        res.close()
        s.Close()
    with pytest.raises(pp.FdbError):
        pp.ReservoirSampler(-1, 0)


def test_sampler_output_feeds_filter_and_aggregate():
    lens = [500, 1500]
    recs = sampler_records(lens)
    s = pp.ReservoirSampler(400, 5)
    for r in recs:
        s.Callback(r)
    res = s.FinishResident()
    s.Close()
    host = res.to_arrow()
    aggs, groups = [Sum(Col("i0")), Count(Col("id"))], [Col("d"), Col("s0")]
    on_device = pp.HashAggregatePlan(Col("id") > 100, aggs, groups)
    on_host = pp.HashAggregatePlan(Col("id") > 100, aggs, groups)
    try:
        filtered = on_device.FilterResident(res)
        assert_same(filtered.to_arrow(), on_host.Filter(host))
        filtered.close()
        on_device.Callback(res)
        on_host.Callback(host)
        a, b = on_device.Finish(), on_host.Finish()
        assert a.schema.names == b.schema.names
        da, db = arrow_to_pydict(a), arrow_to_pydict(b)
        rows = lambda d, t: sorted((tuple(d[n][k] for n in t.schema.names) for k in range(t.num_rows)), key=repr)  # noqa: E731
        assert rows(da, a) == rows(db, b) and a.num_rows > 1
    finally:
        res.close()
        on_device.Close()
        on_host.Close()


# ---- 4. allocations ----------------------------------------------------------------------------------------------------------------------
def test_everything_is_released():
    gc.collect()
    before = pp.live_allocations()
    recs = sampler_records([300, 3000])
    rbs = [pp.ResidentBatch(r) for r in recs]
    taken = rbs[1].take(np.arange(0, 3000, 3))
    limited = [pp.Limiter(c).CallbackResident(rbs[0]) for c in (0, 10, 300)]
    s = pp.ReservoirSampler(2000, 3)  # the reservoir grows past its first allocation
    for rb in rbs:
        s.CallbackResident(rb)
    res = s.FinishResident()
    assert pp.live_allocations()["device_bytes"] > before["device_bytes"]
    with pytest.raises(pp.FdbError):
        rbs[0].take([300])
    for o in [taken, res] + limited + rbs:
        o.close()
    s.Close()
    assert pp.live_allocations() == before
