"""Exact float64 sums (fdb_plan_set_exact_sums) on the device: every group's SUM(float64) is the correctly rounded exact sum — checked
BIT FOR BIT against float(sum(Fraction(v))) — on every key shape of the hash table, with and without the run-time specialised kernel,
and the bits do not depend on row order, record split, push style or merge order."""
from fractions import Fraction

import numpy as np
import pyarrow as pa
import pytest

from frostdb_amd.logicalplan import Col, Count, DynCol, Max, Sum

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pp():
    from frostdb_amd import physicalplan
    assert physicalplan.device_count() >= 1, "no HIP device visible"
    yield physicalplan
    assert physicalplan.live_allocations()["device_blocks"] == 0


@pytest.fixture(params=["jit", "nojit"])
def jit_mode(request, monkeypatch):
    if request.param == "nojit":
        monkeypatch.setenv("FDB_NO_JIT", "1")  # (read when a plan is created: the ahead-of-time scan_hash_kernel)
    return request.param


def f64_bits(x):
    return int(np.float64(x).view(np.uint64))


def wild_values(rng, n):
    """Values over 1e-300 … 1e300, both signs, some exact cancellations; roughly 5 % NULL."""
    mant = rng.uniform(1.0, 10.0, n) * rng.choice([-1.0, 1.0], n)
    v = mant * np.power(10.0, rng.integers(-300, 301, n).astype(np.float64))
    v[: n // 8] = -v[n // 8: 2 * (n // 8)]  # (exact cancellations, between rows that may or may not share a group)
    mask = rng.random(n) < 0.05
    return v, mask


def dict_col(rng, n, names, null_frac=0.0):
    idx = rng.integers(0, len(names), n).astype(np.uint32)
    mask = rng.random(n) < null_frac if null_frac > 0 else None
    return pa.DictionaryArray.from_arrays(pa.array(idx, type=pa.uint32(), mask=mask), pa.array(names, type=pa.binary()))


def make_records(rng, n, n_records=3, n_label_cols=2, extra=None):
    """Records of labels.l00 … (dictionary), labels.path (dictionary), timestamp (int64 time buckets), value (float64 with NULLs)."""
    recs = []
    for _ in range(n_records):
        v, mask = wild_values(rng, n)
        arrays, names = [], []
        for c in range(n_label_cols):
            arrays.append(dict_col(rng, n, [b"v%d" % i for i in range(2 if n_label_cols > 8 else 5)], 0.02))
            names.append("labels.l%02d" % c)
        arrays.append(dict_col(rng, n, [b"/p%03d" % i for i in range(40)], 0.02))
        names.append("labels.path")
        arrays.append(pa.array((rng.integers(0, 50, n) * 60_000).astype(np.int64)))
        names.append("timestamp")
        arrays.append(pa.array(v, mask=mask))
        names.append("value")
        if extra:
            for k, col in extra(rng, n).items():
                arrays.append(col)
                names.append(k)
        recs.append(pa.RecordBatch.from_arrays(arrays, names=names))
    return recs


def exact_reference(recs, keys, value_of):
    """{key tuple: exact rational sum} over the records (NULL values contribute 0, like the plan)."""
    acc = {}
    for r in recs:
        cols = [r.column(r.schema.get_field_index(k)).to_pylist() for k in keys]
        vals = value_of(r)
        for i, v in enumerate(vals):
            t = tuple(c[i] for c in cols)
            acc[t] = acc.get(t, Fraction(0)) + (Fraction(v) if v is not None else 0)
    return {t: float(s) + 0.0 for t, s in acc.items()}


def result_sums(out, n_keys, agg_index=0):
    keys = [out.column(i).to_pylist() for i in range(n_keys)]
    sums = out.column(n_keys + agg_index).to_pylist()
    return {tuple(k[i] for k in keys): s for i, s in enumerate(sums)}


def assert_exact(got, want):
    assert set(got) == set(want), (len(got), len(want))
    bad = [(k, got[k], want[k]) for k in want if f64_bits(got[k]) != f64_bits(want[k])]
    assert not bad, bad[:5]


def run_plan(pp, recs, aggs, groups, style="host", exact=True, **kw):
    plan = pp.HashAggregatePlan(None, aggs, groups, **kw)
    if exact:
        plan.set_exact_sums(True)
    rbs = []
    try:
        if style == "host":
            for r in recs:
                plan.Callback(r)
        elif style == "small":  # small host records: queued and scanned together
            for r in recs:
                for off in range(0, r.num_rows, 700):
                    plan.Callback(r.slice(off, 700))
        else:
            rbs = [pp.ResidentBatch(r) for r in recs]
            plan.CallbackResident(rbs)
        out = plan.Finish()
        kernel = plan.last_kernel()
    finally:
        plan.Close()
        for b in rbs:
            b.close()
    return out, kernel


def values(r, col="value"):
    return r.column(r.schema.get_field_index(col)).to_pylist()


def raw_values(r, col="value"):
    """The values buffer as it is, NULL slots included: a computed input (a pre-aggregate Projection) reads the slot of a NULL row too."""
    c = r.column(r.schema.get_field_index(col))
    return np.frombuffer(c.buffers()[1], dtype=np.float64)[c.offset:c.offset + len(c)].tolist()


@pytest.mark.parametrize("shape", ["path", "cfg5_32_columns", "int64_time_bucket", "no_groups", "computed", "sum_and_count"])
def test_exact_sums_match_the_rational_reference(pp, jit_mode, shape):
    rng = np.random.default_rng(len(shape) * 7 + ord(shape[0]))
    n_label = 32 if shape == "cfg5_32_columns" else 2
    recs = make_records(rng, 20_000, n_label_cols=n_label)
    if shape == "path":
        groups, keys = [Col("labels.path")], ["labels.path"]
    elif shape == "cfg5_32_columns":
        keys = ["labels.l%02d" % c for c in range(32)]
        groups = [Col(k) for k in keys]
    elif shape == "int64_time_bucket":
        groups, keys = [Col("timestamp")], ["timestamp"]
    else:
        groups, keys = [Col("labels.path")] if shape != "no_groups" else [], ["labels.path"] if shape != "no_groups" else []
    aggs = [Sum(Col("value"))]
    value_of = values
    if shape == "computed":
        if jit_mode == "nojit":
            pytest.skip("computed inputs need the run-time specialised kernel (the interpreting kernels refuse them)")
        aggs = [Sum(Col("value") * 3.0)]
        value_of = lambda r: [v * 3.0 for v in raw_values(r)]  # noqa: E731  (the product is rounded per row, as the kernel does)
    if shape == "sum_and_count":  # AVG = SUM + COUNT
        aggs = [Count(Col("value")), Sum(Col("value")), Max(Col("value"))]
    out, kernel = run_plan(pp, recs, aggs, groups)
    assert kernel == ("scan_hash_kernel" if jit_mode == "nojit" else "fdb_hash_kernel"), kernel
    want = exact_reference(recs, keys, value_of)
    got = result_sums(out, len(keys), agg_index=1 if shape == "sum_and_count" else 0)
    assert_exact(got, want)
    if shape == "sum_and_count":
        counts = result_sums(out, len(keys), agg_index=0)
        assert sum(counts.values()) == sum(r.num_rows for r in recs)  # (COUNT counts the group's rows)


def test_dynamic_final_stage_and_ordered_plans(pp, jit_mode):
    rng = np.random.default_rng(5)
    extra = lambda rng, n: {"foo.a": pa.array(wild_values(rng, n)[0]), "foo.b": pa.array(wild_values(rng, n)[0])}  # noqa: E731
    recs = make_records(rng, 10_000, extra=extra)
    # dynamic sum(foo.*) by labels.path
    out, _ = run_plan(pp, recs, [Sum(DynCol("foo"))], [Col("labels.path")])
    names = out.schema.names
    for col in ("foo.a", "foo.b"):
        want = exact_reference(recs, ["labels.path"], lambda r: values(r, col))
        got = result_sums(out, 1, agg_index=names.index(col) - 1)
        assert_exact(got, want)
    # final stage over partial results: two partial plans, their outputs pushed into one final plan
    parts = [run_plan(pp, recs[i:i + 1], [Sum(Col("value"))], [Col("labels.path")])[0] for i in range(len(recs))]
    fin, _ = run_plan(pp, parts, [Sum(Col("value"))], [Col("labels.path")], final_stage=True)
    partial_want = [exact_reference(recs[i:i + 1], ["labels.path"], values) for i in range(len(recs))]
    want = {}
    for pw in partial_want:
        for k, v in pw.items():
            want[k] = want.get(k, Fraction(0)) + Fraction(v)
    assert_exact(result_sums(fin, 1), {k: float(v) + 0.0 for k, v in want.items()})
    # ordered: the result comes sorted by the group column
    out, kernel = run_plan(pp, recs, [Sum(Col("value"))], [Col("labels.path")], ordered=True)
    assert "runs" not in kernel, kernel
    keys = out.column(0).to_pylist()
    assert keys == sorted(keys, key=lambda k: (k is None, k or b""))
    assert_exact(result_sums(out, 1), exact_reference(recs, ["labels.path"], values))


def test_bits_do_not_depend_on_order_split_or_push_style(pp):
    rng = np.random.default_rng(11)
    rec = pa.Table.from_batches(make_records(rng, 30_000, n_records=2)).combine_chunks().to_batches()[0]
    groups = [Col("labels.path")]
    want = exact_reference([rec], ["labels.path"], values)
    seen = []
    for trial, (perm_seed, n_parts, style) in enumerate([(0, 1, "host"), (1, 7, "host"), (2, 64, "resident"), (3, 7, "small"), (4, 64, "host"), (5, 1, "resident")]):
        perm = np.random.default_rng(perm_seed).permutation(rec.num_rows)
        shuffled = rec.take(pa.array(perm))
        cuts = sorted(set([0, rec.num_rows] + list(np.random.default_rng(perm_seed).integers(1, rec.num_rows, n_parts - 1))))
        pieces = [shuffled.slice(a, b - a) for a, b in zip(cuts, cuts[1:])]
        out, _ = run_plan(pp, pieces, [Sum(Col("value"))], groups, style=style)
        got = result_sums(out, 1)
        assert_exact(got, want)
        seen.append({k: f64_bits(v) for k, v in got.items()})
    assert all(s == seen[0] for s in seen)


def test_merge_order_does_not_change_the_bits(pp):
    rng = np.random.default_rng(21)
    recs = make_records(rng, 8_000, n_records=8)
    groups = [Col("labels.path"), Col("timestamp")]
    keys = ["labels.path", "timestamp"]
    want = exact_reference(recs, keys, values)

    def plan_of(r):
        p = pp.HashAggregatePlan(None, [Sum(Col("value"))], groups)
        p.set_exact_sums(True)
        p.Callback(r)
        return p

    def finish(p):
        out = p.Finish()
        p.Close()
        return result_sums(out, 2)

    a, b = plan_of(recs[0]), plan_of(recs[1])
    a.Merge(b)
    b.Close()
    ab = finish(a)
    a, b = plan_of(recs[0]), plan_of(recs[1])
    b.Merge(a)
    a.Close()
    ba = finish(b)
    assert_exact(ab, exact_reference(recs[:2], keys, values))
    assert {k: f64_bits(v) for k, v in ab.items()} == {k: f64_bits(v) for k, v in ba.items()}
    results = []
    for order in (list(range(8)), [5, 2, 7, 0, 3, 6, 1, 4]):
        plans = [plan_of(r) for r in recs]
        # a chain: pairs first, then the pairs' results into the first of the order
        for i in range(0, 8, 2):
            plans[order[i]].Merge(plans[order[i + 1]])
            plans[order[i + 1]].Close()
        for i in range(2, 8, 2):
            plans[order[0]].Merge(plans[order[i]])
            plans[order[i]].Close()
        results.append(finish(plans[order[0]]))
    assert_exact(results[0], want)
    assert {k: f64_bits(v) for k, v in results[0].items()} == {k: f64_bits(v) for k, v in results[1].items()}


def test_a_growing_table_stays_exact(pp, jit_mode):
    """Distinct int64 keys arriving in growing waves: the table (65 536 slots at first) is rehashed several times, limb rows move with it."""
    rng = np.random.default_rng(31)
    recs = []
    base = 0
    for n in (20_000, 60_000, 200_000, 500_000):
        keys = np.concatenate([np.arange(base, base + n // 2), rng.integers(0, base + n // 2, n - n // 2)]).astype(np.int64)
        base += n // 2
        v, mask = wild_values(rng, n)
        recs.append(pa.RecordBatch.from_arrays([pa.array(keys), pa.array(v, mask=mask)], names=["k", "value"]))
    out, _ = run_plan(pp, recs, [Sum(Col("value"))], [Col("k")], style="resident")
    want = {}
    for r in recs:
        for k, v in zip(r.column(0).to_numpy(), r.column(1).to_pylist()):
            want[int(k)] = want.get(int(k), Fraction(0)) + (Fraction(v) if v is not None else 0)
    assert out.num_rows == base
    got = dict(zip(out.column(0).to_pylist(), out.column(1).to_pylist()))
    assert_exact({(k,): v for k, v in got.items()}, {(k,): float(s) + 0.0 for k, s in want.items()})


def test_normalizing_often_changes_nothing(pp, monkeypatch):
    rng = np.random.default_rng(41)
    recs = make_records(rng, 30_000, n_records=3)
    monkeypatch.setenv("FDB_TEST_EXACT_NORMALIZE_ROWS", "1024")
    for jit in (True, False):
        if not jit:
            monkeypatch.setenv("FDB_NO_JIT", "1")
        out, _ = run_plan(pp, recs, [Sum(Col("value"))], [Col("labels.path")], style="resident")
        assert_exact(result_sums(out, 1), exact_reference(recs, ["labels.path"], values))
        # merges normalize too
        a = pp.HashAggregatePlan(None, [Sum(Col("value"))], [Col("labels.path")])
        b = pp.HashAggregatePlan(None, [Sum(Col("value"))], [Col("labels.path")])
        a.set_exact_sums(True)
        b.set_exact_sums(True)
        a.Callback(recs[0])
        b.Callback(recs[1])
        b.Callback(recs[2])
        a.Merge(b)
        b.Close()
        out = a.Finish()
        a.Close()
        assert_exact(result_sums(out, 1), exact_reference(recs, ["labels.path"], values))


def test_digits_near_two_to_the_32_across_many_normalizes(pp, monkeypatch):
    """Values whose three digits are all close to 2^32, into two groups: with a small normalize threshold the limbs are carried many
    times in one scan; the result is the closed-form exact sum."""
    monkeypatch.setenv("FDB_TEST_EXACT_NORMALIZE_ROWS", "4096")
    n = 1 << 20
    # m = 2^53 − 1 shifted by 31: digits 2^32 − 2^31 … ≈ 2^32; a second value with its own exponent for the other group
    x0 = float((2**53 - 1) * 2**(31 - 1074 + 32 * 10))
    x1 = -float((2**53 - 1) * 2**(30 - 1074 + 32 * 20))
    k = np.arange(n, dtype=np.int64) & 1
    v = np.where(k == 0, x0, x1)
    rec = pa.RecordBatch.from_arrays([pa.array(k), pa.array(v)], names=["k", "value"])
    out, _ = run_plan(pp, [rec, rec, rec], [Sum(Col("value"))], [Col("k")], style="resident")
    got = dict(zip(out.column(0).to_pylist(), out.column(1).to_pylist()))
    want = {0: float(Fraction(x0) * (3 * n // 2)), 1: float(Fraction(x1) * (3 * n // 2))}
    assert {k: f64_bits(v) for k, v in got.items()} == {k: f64_bits(v) for k, v in want.items()}


def test_contract_edges(pp):
    rng = np.random.default_rng(51)
    rec = make_records(rng, 2_000, n_records=1)[0]
    aggs, groups = [Sum(Col("value"))], [Col("labels.path")]
    # switching after the first push is a state error
    p = pp.HashAggregatePlan(None, aggs, groups)
    p.Callback(rec)
    with pytest.raises(pp.FdbError) as e:
        p.set_exact_sums(True)
    assert e.value.code == pp.FDB_ERR_STATE
    p.Close()
    # exact + non-exact do not merge
    a = pp.HashAggregatePlan(None, aggs, groups)
    a.set_exact_sums(True)
    b = pp.HashAggregatePlan(None, aggs, groups)
    a.Callback(rec)
    b.Callback(rec)
    with pytest.raises(pp.FdbError) as e:
        a.Merge(b)
    assert e.value.code == pp.FDB_ERR_INVALID
    with pytest.raises(pp.FdbError):
        b.Merge(a)
    # raw state / export / exchange entry points refuse an exact plan
    with pytest.raises(pp.UnsupportedError, match="exact sums"):
        a.state_signature()
    with pytest.raises(pp.UnsupportedError, match="exact sums"):
        a.state_array_ops()
    with pytest.raises(pp.UnsupportedError, match="exact sums"):
        a.group_schema()
    with pytest.raises(pp.UnsupportedError, match="exact sums"):
        a.hash_export(a, 2)
    # partial results are the rounded sums
    assert a.num_groups() > 0
    assert "exact float64 sums" in a.Draw()
    a.Close()
    b.Close()
    # fdb_plan_set_deterministic alone keeps refusing the hash table; with exact sums as well, nothing is refused
    recs = make_records(rng, 5_000, n_records=1, n_label_cols=32)
    groups32 = [Col("labels.l%02d" % c) for c in range(32)]
    d = pp.HashAggregatePlan(None, aggs, groups32)
    d.set_deterministic(True)
    with pytest.raises(pp.UnsupportedError):
        d.Callback(recs[0])
        d.Finish()
    d.Close()
    d = pp.HashAggregatePlan(None, aggs, groups32)
    d.set_deterministic(True)
    d.set_exact_sums(True)
    d.Callback(recs[0])
    out = d.Finish()
    d.Close()
    assert_exact(result_sums(out, 32), exact_reference(recs, ["labels.l%02d" % c for c in range(32)], values))
