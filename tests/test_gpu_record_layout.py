"""The layout contract of resident records (frostdb_amd/csrc/fdb_record.h), through the public API, for every operator that produces one:
content against pyarrow, a validity bitmap present iff the column holds a NULL, and `device_bytes` against the slot formula

    values slot = align_up(rows * width + 256, 256)        width: 4 for dictionary indices, 8 for everything else (bool is widened)
    bitmap slot = align_up((rows + 63) / 64 * 8 + 256, 256)  only for a column that may hold NULLs

restated here — never read back from the library. Where an operator sizes some block for the worst case (the generated filter(), the
projection of several records, the aggregate's Finish) `device_bytes` is only bounded from below by the slots of its own columns.

Rows: 32 / 33 and 64 / 65 are the 256-byte edge of 8-byte and 4-byte values, 64 is one validity word, 2048 rows make a bitmap of
exactly 256 bytes; 1 and 63 / 2047 / 2049 sit around them."""
import numpy as np
import pyarrow as pa
import pytest

from frostdb_amd import physicalplan as pp
from frostdb_amd.logicalplan import Col, Count, Sum
from tests.parquet_util import row_group_chunks, write_parquet
from tests.test_gpu_take import assert_same

pytestmark = pytest.mark.gpu

ROWS = [1, 32, 33, 63, 64, 65, 2047, 2048, 2049]
WIDTH = {"i": 8, "u": 8, "f": 8, "b": 8, "d": 4, "x": 8}  # by the first letter of a column's name
WORDS = [b"w%d" % i for i in range(7)]


def align_up(v: int) -> int:
    return (v + 255) // 256 * 256


def values_slot(rows: int, width: int) -> int:
    return align_up(rows * width + 256)


def bitmap_slot(rows: int) -> int:
    return align_up((rows + 63) // 64 * 8 + 256)


def record_bytes(rows: int, names, bitmaps) -> int:
    """Σ slots of a record of `rows` rows; a record without rows holds no buffers."""
    if rows == 0:
        return 0
    return sum(values_slot(rows, WIDTH[n[0]]) + (bitmap_slot(rows) if n in bitmaps else 0) for n in names)


def make_record(n: int, first: int = 0) -> pa.RecordBatch:
    """int64, uint64, float64, bool and dictionary columns with NULLs (i, u, f, b, d: row 0 is NULL, ≈ 20 % of the others too — `b`
    only in row 0) and without (i0 numbers the rows from `first`, u0, f0, b0, d0)."""
    rng = np.random.default_rng(11 + n + 7 * first)

    def mask(only_first=False):
        m = np.zeros(n, dtype=bool) if only_first else rng.random(n) < 0.2
        m[0] = True
        return m

    cols = {}
    for suffix in ("", "0"):
        m = (lambda **kw: None) if suffix else mask
        cols["i" + suffix] = pa.array(np.arange(first, first + n, dtype=np.int64) if suffix else rng.integers(-2**62, 2**62, n, dtype=np.int64), mask=m())
        cols["u" + suffix] = pa.array(rng.integers(0, 2**64 - 1, n, dtype=np.uint64, endpoint=True), mask=m())
        cols["f" + suffix] = pa.array(rng.standard_normal(n), mask=m())
        cols["b" + suffix] = pa.array(rng.random(n) < 0.5, mask=m(only_first=True))
        cols["d" + suffix] = pa.DictionaryArray.from_arrays(pa.array(rng.integers(0, len(WORDS), n).astype(np.uint32), mask=m()), pa.array(WORDS, type=pa.binary()))
    return pa.RecordBatch.from_arrays(list(cols.values()), names=list(cols.keys()))


def with_nulls(rec: pa.RecordBatch) -> set:
    return {n for n, c in zip(rec.schema.names, rec.columns) if c.null_count > 0}


def check(rb, want: pa.RecordBatch, bitmaps, what, exact=True):
    """Content and NULLs as `want`, a validity buffer iff a NULL (assert_same), and the record's bytes: the slots of its columns, a bitmap
    slot for the names in `bitmaps`."""
    try:
        got = rb.to_arrow()
        assert rb.num_rows == want.num_rows, what
        assert_same(got, want, what)
        if exact:
            assert rb.device_bytes == record_bytes(want.num_rows, want.schema.names, bitmaps), (what, sorted(bitmaps))
        else:
            assert rb.device_bytes >= record_bytes(want.num_rows, want.schema.names, with_nulls(got)), what
    finally:
        rb.close()


def in_order(parts, key="i0") -> pa.RecordBatch:
    """The rows of `parts` (same fields) as one record ordered by `key`."""
    whole = pa.Table.from_batches(parts).combine_chunks()
    return whole.take(pa.array(np.argsort(np.asarray(whole.column(key).to_numpy()), kind="stable"))).combine_chunks().to_batches()[0]


def halves(rec: pa.RecordBatch):
    """Two records with rows, each ordered by i0: the even and the odd rows of `rec` (one row: the record and a second one after it)."""
    n = rec.num_rows
    if n == 1:
        return [rec, make_record(1, first=1)]
    return [rec.take(pa.array(np.arange(k, n, 2), type=pa.int32())) for k in (0, 1)]


@pytest.fixture(scope="module")
def sources():
    recs = {n: make_record(n) for n in ROWS}
    rbs = {n: pp.ResidentBatch(r) for n, r in recs.items()}
    yield recs, rbs
    for rb in rbs.values():
        rb.close()


@pytest.mark.parametrize("rows", ROWS)
def test_import(sources, rows):
    rec = sources[0][rows]
    check(pp.ResidentBatch(rec), rec, with_nulls(rec), rows)


@pytest.mark.parametrize("rows", ROWS)
def test_parquet_row_group(sources, rows):
    """PLAIN values, dictionary-encoded strings; i, u, f, b, d optional, the others required: an optional column has a bitmap slot."""
    rec = sources[0][rows]
    schema = pa.schema([pa.field(f.name, f.type, nullable=not f.name.endswith("0")) for f in rec.schema])
    data = write_parquet(pa.Table.from_arrays(rec.columns, schema=schema))
    chunks, n = row_group_chunks(data, 0)
    assert n == rows and [c[2] for c in chunks] == [0 if f.name.endswith("0") else 1 for f in rec.schema]
    check(pp.ResidentBatch.from_parquet(chunks, n), rec, {f.name for f in rec.schema if not f.name.endswith("0")}, rows)


@pytest.mark.parametrize("generated", [False, True], ids=["interpreting", "generated"])
@pytest.mark.parametrize("rows", ROWS)
def test_filter(sources, rows, generated, monkeypatch):
    """Everything selected, and everything but row 0 (`b` keeps its bitmap slot and loses its only NULL; one row: nothing is left). The
    interpreting path allocates the exact slots; the generated one-pass path keeps worst-case blocks."""
    recs, rbs = sources
    rec, rb = recs[rows], rbs[rows]
    if generated:
        monkeypatch.delenv("FDB_NO_JIT", raising=False)
        monkeypatch.setenv("FDB_SELECT_ONE_PASS", "1")
    else:
        monkeypatch.setenv("FDB_NO_JIT", "1")
    for lo in (0, 1):
        plan = pp.HashAggregatePlan(Col("i0") >= lo)
        try:
            out = plan.FilterResident(rb)
            if generated:
                assert "fdb_select_kernel" in plan.last_kernel(), plan.last_kernel()
            elif rows > lo:
                assert plan.last_kernel() == "compact_col_kernel", plan.last_kernel()
            check(out, rec.slice(lo), with_nulls(rec), (rows, lo), exact=not generated)
        finally:
            plan.Close()


@pytest.mark.parametrize("rows", ROWS)
def test_take_and_sort(sources, rows):
    recs, rbs = sources
    rec, rb = recs[rows], rbs[rows]
    back = np.arange(rows - 1, -1, -1)
    want = rec.take(pa.array(back, type=pa.int32()))
    check(rb.take(back), want, with_nulls(rec), (rows, "take"))
    check(rb.sort([("i0", True)]), want, with_nulls(rec), (rows, "sort"))


@pytest.mark.parametrize("rows", ROWS)
def test_limit(sources, rows):
    """Below the row count: a prefix (one row: the schema alone, no buffers); above it: the whole record, copied."""
    recs, rbs = sources
    rec, rb = recs[rows], rbs[rows]
    check(pp.Limiter(rows - 1).CallbackResident(rb), rec.slice(0, rows - 1), with_nulls(rec), (rows, "prefix"))
    check(pp.Limiter(rows + 5).CallbackResident(rb), rec, with_nulls(rec), (rows, "copy"))


@pytest.mark.parametrize("rows", ROWS)
def test_sampler_finish(sources, rows):
    """A reservoir larger than the record keeps every row in order; its fields leave sorted by name. The reservoir holds a validity byte
    per slot for every field, so every column of the result has a bitmap slot."""
    recs, rbs = sources
    rec = recs[rows]
    s = pp.ReservoirSampler(rows + 3, 1)
    try:
        s.CallbackResident(rbs[rows])
        names = sorted(rec.schema.names)
        check(s.FinishResident(), rec.select(names), set(names), rows)
    finally:
        s.Close()


@pytest.mark.parametrize("rows", ROWS)
def test_merge(sources, rows):
    """A column has a bitmap slot iff an input has a bitmap for it."""
    parts = halves(sources[0][rows])
    ins = [pp.ResidentBatch(p) for p in parts]
    try:
        check(pp.ResidentBatch.merge(ins, ["i0"]), in_order(parts), with_nulls(parts[0]) | with_nulls(parts[1]), rows)
    finally:
        for r in ins:
            r.close()


@pytest.mark.parametrize("rows", ROWS)
def test_merge_named_with_a_lacking_column(sources, rows):
    """The second record lacks `f` and `d0`: its rows are NULL there, and both columns get a bitmap slot. The sorting column leaves first."""
    a, b = halves(sources[0][rows])
    lacking = ["f", "d0"]
    ins = [pp.ResidentBatch(a), pp.ResidentBatch(b.select([n for n in b.schema.names if n not in lacking]))]
    names = ["i0"] + [n for n in a.schema.names if n != "i0"]
    b_full = pa.RecordBatch.from_arrays([pa.nulls(b.num_rows, a.schema.field(n).type) if n in lacking else b.column(n) for n in names], names=names)
    try:
        check(pp.ResidentBatch.merge_named(ins, [Col("i0")]), in_order([a.select(names), b_full]), with_nulls(a) | with_nulls(b) | set(lacking), rows)
    finally:
        for r in ins:
            r.close()


@pytest.mark.parametrize("rows", ROWS)
def test_project(sources, rows):
    """One field passed through with its NULLs, one computed."""
    recs, rbs = sources
    rec = recs[rows]
    plan = pp.Projection([Col("d"), (Col("i0") + Col("i0")).Alias("x")])
    try:
        want = pa.RecordBatch.from_arrays([rec.column("d"), pa.array(2 * np.arange(rows, dtype=np.int64))], names=["d", "x"])
        check(plan.ProjectResident(rbs[rows]), want, set(), rows, exact=False)
    finally:
        plan.Close()


@pytest.mark.parametrize("rows", ROWS)
def test_resident_aggregate_finish(sources, rows):
    recs, rbs = sources
    rec = recs[rows]
    want = {}
    for d, b, v in zip(rec.column("d").dictionary_decode().to_pylist(), rec.column("b").to_pylist(), rec.column("i0").to_pylist()):
        acc = want.setdefault((d, b), [0, 0])
        acc[0] += v
        acc[1] += 1
    plan = pp.HashAggregatePlan(None, [Sum(Col("i0")), Count(Col("i0"))], [Col("b"), Col("d")])
    try:
        plan.CallbackResident([rbs[rows]])
        res = plan.FinishResident()
        got = res.to_arrow()
        assert got.schema.names == ["b", "d", "sum(i0)", "count(i0)"]
        for c in got.columns:
            assert (c.buffers()[0] is not None) == (c.null_count > 0)
        keys = zip(got.column("d").dictionary_decode().to_pylist(), got.column("b").to_pylist())
        assert {k: [s, c] for k, s, c in zip(keys, got.column(2).to_pylist(), got.column(3).to_pylist())} == want
        assert res.num_rows == len(want)
        assert res.device_bytes >= record_bytes(len(want), ["b", "d", "i_sum", "i_count"], with_nulls(got))
        res.close()
    finally:
        plan.Close()


def test_a_merged_bool_column_counts_as_bits(sources):
    """A scan's algorithmic bytes count a bool column as Arrow's bits, whichever operator produced the record: COUNT filtered on a bool
    column reports the same bytes over a merged record and over take(identity) of the same rows."""
    rec = sources[0][2049]
    ins = [pp.ResidentBatch(p) for p in halves(rec)]
    merged = pp.ResidentBatch.merge(ins, ["i0"])
    taken = sources[1][2049].take(np.arange(2049))
    seen = []
    try:
        for rb in (merged, taken):
            plan = pp.HashAggregatePlan(Col("b0") == True, [Count(Col("i0"))], [])  # noqa: E712
            plan.CallbackResident([rb])
            counted = plan.Finish().column(0).to_pylist()
            seen.append((plan.stats()["algorithmic_bytes"], counted))
            plan.Close()
        assert seen[0] == seen[1] and seen[0][0] > 0
    finally:
        for r in ins + [merged, taken]:
            r.close()
