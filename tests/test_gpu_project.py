"""The device Projection operator (fdb_plan_project*, physicalplan.Projection): the reference's exec/projection vectors, a differential
test against a numpy restatement of physicalplan/project.go:163-399 (the Add / Sub / Mul / Div loops and the boolean, convert, isnull
and if projections around them), pass-through fields, chaining with filter() and the aggregate, AVG finished on the device, several
records per launch, errors and allocations.

Every row count of the differential test is a record of ONE ProjectResidentMany call per expression set, so an expression set costs one
kernel compilation and one launch; row counts are the byte, wave (256 rows) and tile (1 024 rows) edges of the kernel's 256-thread
workgroups (a lane owns 4 rows), 4 099 (several tiles + 3 rows) and 70 001 (more tiles than one pass of a small grid)."""
import numpy as np
import pyarrow as pa
import pytest

from frostdb_amd import physicalplan as pp
from frostdb_amd.logicalplan import (OP_ADD, OP_AND, OP_DIV, OP_EQ, OP_GT, OP_GT_EQ, OP_LT, OP_LT_EQ, OP_MUL, OP_NOT_EQ, OP_OR, OP_SUB, AliasExpr,  # noqa: F401
                                     BinaryExpr, Col, Column, Convert, ConvertExpr, Count, DynCol, IfExpr, IsNullExpr, Literal, Sum, expr_name)
from tests.golden.projection_cases import DIFF_CASES, VECTORS
from tests.util import dict_array

pytestmark = pytest.mark.gpu

ROW_COUNTS = [0, 1, 7, 8, 9, 63, 64, 255, 256, 257, 1023, 1024, 1025, 4099, 70001]
I64_MIN, I64_MAX = np.iinfo(np.int64).min, np.iinfo(np.int64).max


# ---- test records ---------------------------------------------------------------------------------------------------------------------
def _nullable(values: np.ndarray, valid: np.ndarray, typ) -> pa.Array:
    """An Arrow array whose NULL slots keep the raw values of `values` (pa.array would zero them)."""
    n = len(values)
    if n == 0:
        return pa.array([], type=typ)
    if valid.all():
        return pa.Array.from_buffers(typ, n, [None, pa.py_buffer(np.ascontiguousarray(values))])
    bits = np.packbits(valid, bitorder="little")
    return pa.Array.from_buffers(typ, n, [pa.py_buffer(bits), pa.py_buffer(np.ascontiguousarray(values))], null_count=int((~valid).sum()))


def _mask(rng, n, nullable=True):
    v = rng.random(n) >= 0.2 if nullable else np.ones(n, dtype=bool)
    if nullable and n:
        v[0] = False  # every record of a nullable column carries a bitmap: one kernel shape for every row count
    return v


def make_data(n: int, seed: int = 7) -> dict:
    """name → (raw values, validity, kind). Raw slots under NULLs are whatever the generator put there — non-zero on purpose."""
    rng = np.random.default_rng(seed + n)
    ispecial = np.array([I64_MIN, -1, 0, 1, I64_MAX, I64_MIN + 1, 2, -2, 3, -7, 1000, -1000], dtype=np.int64)
    a = np.where(rng.random(n) < 0.5, rng.choice(ispecial, n), rng.integers(I64_MIN, I64_MAX, n, dtype=np.int64, endpoint=True))
    b = np.where(rng.random(n) < 0.7, rng.choice(ispecial, n), rng.integers(-50, 50, n, dtype=np.int64))
    c = rng.integers(-10**12, 10**12, n, dtype=np.int64)
    fspecial = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, 5e-324, -5e-324, 2.2250738585072014e-308 / 4, 1.0, -1.5, 1e308, -1e308, 3.0, 0.1], dtype=np.float64)
    f = np.where(rng.random(n) < 0.5, rng.choice(fspecial, n), rng.standard_normal(n) * 1e3)
    g = np.where(rng.random(n) < 0.6, rng.choice(fspecial, n), rng.standard_normal(n))
    h = rng.standard_normal(n) * 10
    uspecial = np.array([0, 1, 2, 3, 2**63, 2**63 + 5, 2**64 - 1, 2**64 - 2, 10**19], dtype=np.uint64)
    u = np.where(rng.random(n) < 0.6, rng.choice(uspecial, n), rng.integers(0, 2**64 - 1, n, dtype=np.uint64, endpoint=True))
    v = np.where(rng.random(n) < 0.6, rng.choice(uspecial, n), rng.integers(0, 100, n, dtype=np.uint64))
    return {
        "a": (a, _mask(rng, n), "i"), "b": (b, _mask(rng, n), "i"), "c": (c, _mask(rng, n, False), "i"),
        "f": (f, _mask(rng, n), "f"), "g": (g, _mask(rng, n), "f"), "h": (h, _mask(rng, n, False), "f"),
        "u": (u, _mask(rng, n, False), "u"), "v": (v, _mask(rng, n, False), "u"),
        "d": (rng.integers(0, 5, n).astype(np.uint32), _mask(rng, n), "d"),      # dictionary v0 … v4, with NULLs
        "w": (rng.integers(0, 100, n).astype(np.uint32), _mask(rng, n, False), "w"),  # dictionary w0 … w99: its truth table lives in LDS
        "s": (rng.integers(0, 3, n).astype(np.uint32), _mask(rng, n, False), "s"),    # plain utf8 s0 … s2
    }


_D_VALUES = {"d": [f"v{i}".encode() for i in range(5)], "w": [f"w{i}".encode() for i in range(100)], "s": [f"s{i}" for i in range(3)]}


def make_record(data: dict) -> pa.RecordBatch:
    arrays, names = [], []
    for name, (raw, valid, kind) in data.items():
        names.append(name)
        if kind in "iuf":
            arrays.append(_nullable(raw, valid, {"i": pa.int64(), "u": pa.uint64(), "f": pa.float64()}[kind]))
        elif kind == "s":
            arrays.append(pa.array([_D_VALUES["s"][i] for i in raw], type=pa.string()))
        else:
            arrays.append(pa.DictionaryArray.from_arrays(_nullable(raw, valid, pa.uint32()), pa.array(_D_VALUES[kind], type=pa.binary())))
    return pa.RecordBatch.from_arrays(arrays, names=names)


# ---- numpy restatement of project.go ---------------------------------------------------------------------------------------------------
def _go_div_i64(a, b):
    """DivInt64s (project.go:347-363): NULL where the divisor is 0, else Go's quotient — truncated toward zero, MinInt64 / -1 wraps."""
    valid = b != 0
    bs = np.where(valid, b, 1)
    neg1 = bs == -1
    bs2 = np.where(neg1, 1, bs)
    q = a // bs2
    r = a - q * bs2
    q = q + ((r != 0) & ((a < 0) != (bs2 < 0)))
    q = np.where(neg1, (np.uint64(0) - a.view(np.uint64)).view(np.int64), q)
    return np.where(valid, q, 0), valid


def evaluate(e, data):
    """(raw values, validity, kind 'i' 'u' 'f' 'b') of expression `e` over the record — only the outermost operation's validity survives."""
    n = len(data["a"][0])
    true = np.ones(n, dtype=bool)
    if isinstance(e, AliasExpr):
        return evaluate(e.expr, data)
    if isinstance(e, Column):
        return data[e.name]
    if isinstance(e, Literal):
        if isinstance(e.value, float):
            return np.full(n, e.value, dtype=np.float64), true, "f"
        return np.full(n, e.value, dtype=np.int64), true, "i"
    if isinstance(e, ConvertExpr):
        raw, _, kind = evaluate(e.expr, data)
        assert kind == "i"
        return raw.astype(np.float64), true, "f"  # float64(c.Value(i)): the raw slot (project.go:523-535)
    if isinstance(e, IsNullExpr):
        return ~evaluate(e.expr, data)[1], true, "b"
    if isinstance(e, IfExpr):
        cr, cv, _ = evaluate(e.cond, data)
        return np.where(cr & cv, evaluate(e.then, data)[0], evaluate(e.els, data)[0]), true, "i"
    assert isinstance(e, BinaryExpr), e
    if e.op in (OP_AND, OP_OR):
        l, r = evaluate(e.left, data)[0], evaluate(e.right, data)[0]
        return (l & r) if e.op == OP_AND else (l | r), true, "b"
    lr, lv, lk = evaluate(e.left, data)
    if lk in "dws":  # a dictionary / string column against a string literal: a NULL row does not match
        lit = e.right.value.encode() if isinstance(e.right.value, str) else e.right.value
        want = [x if isinstance(x, bytes) else x.encode() for x in _D_VALUES[lk]].index(lit)
        assert e.op == OP_EQ
        return lv & (lr == want), true, "b"
    rr, rv, rk = evaluate(e.right, data)
    with np.errstate(all="ignore"):
        if OP_EQ <= e.op <= OP_GT_EQ:
            if lk != rk:
                lr, rr = lr.astype(np.float64), rr.astype(np.float64)
            cmp = {OP_EQ: np.equal, OP_NOT_EQ: np.not_equal, OP_LT: np.less, OP_LT_EQ: np.less_equal, OP_GT: np.greater, OP_GT_EQ: np.greater_equal}[e.op]
            return lv & rv & cmp(lr, rr), true, "b"  # a NULL operand compares false
        assert lk == rk, "operands of one type"
        if e.op == OP_DIV:
            if lk == "i":
                q, valid = _go_div_i64(lr, rr)
            elif lk == "u":
                valid = rr != 0
                q = np.where(valid, lr // np.where(valid, rr, np.uint64(1)), np.uint64(0)).astype(np.uint64)
            else:
                valid = rr != 0  # (so -0.0 too)
                q = np.where(valid, lr / np.where(valid, rr, 1.0), 0.0)
            return q, valid, lk
        if lk == "f":
            return {OP_ADD: np.add, OP_SUB: np.subtract, OP_MUL: np.multiply}[e.op](lr, rr), true, "f"
        ul, ur = lr.view(np.uint64), rr.view(np.uint64)  # + - * wrap modulo 2^64, on the RAW slots
        res = {OP_ADD: np.add, OP_SUB: np.subtract, OP_MUL: np.multiply}[e.op](ul, ur)
        return res.view(np.int64) if lk == "i" else res, true, lk


def check_column(col: pa.Array, exp_raw, exp_valid, kind, what):
    n = len(exp_raw)
    assert len(col) == n, what
    if kind == "b":
        assert col.type == pa.bool_() and col.null_count == 0, what
        got = np.asarray(col.to_numpy(zero_copy_only=False), dtype=bool) if n else np.zeros(0, dtype=bool)
        np.testing.assert_array_equal(got, exp_raw.astype(bool), err_msg=str(what))
        return
    assert col.type == {"i": pa.int64(), "u": pa.uint64(), "f": pa.float64()}[kind], (what, col.type)
    if n == 0:
        return
    bufs = col.buffers()
    # validity: bit for bit, the zero tail bits of the last byte included; no buffer at all when nothing is NULL
    if exp_valid.all():
        assert bufs[0] is None and col.null_count == 0, (what, "a column without NULLs carries no validity buffer")
    else:
        assert bufs[0] is not None, what
        got_bits = np.frombuffer(bufs[0], dtype=np.uint8)[: (n + 7) // 8]
        np.testing.assert_array_equal(got_bits, np.packbits(exp_valid, bitorder="little"), err_msg=f"{what}: validity bitmap")
        assert col.null_count == int((~exp_valid).sum()), what
    got = np.frombuffer(bufs[1], dtype=np.uint64)[:n]
    exp = np.ascontiguousarray(exp_raw).view(np.uint64)
    same = got == exp
    if kind == "f":
        same = same | (np.isnan(got.view(np.float64)) & np.isnan(exp.view(np.float64)))
    bad = np.flatnonzero(exp_valid & ~same)
    assert bad.size == 0, (what, "row", int(bad[0]), hex(int(got[bad[0]])), hex(int(exp[bad[0]])))


@pytest.fixture(scope="module")
def records():
    """One record per row count, host and resident; built once, shared and left unchanged."""
    datas = [make_data(n) for n in ROW_COUNTS]
    recs = [make_record(d) for d in datas]
    rbs = [pp.ResidentBatch(r) for r in recs]
    yield datas, recs, rbs
    for rb in rbs:
        rb.close()


# ---- 1. golden vectors -----------------------------------------------------------------------------------------------------------------
def _vector_record(v) -> pa.RecordBatch:
    arrays = []
    for k, (_, typ) in enumerate(v["cols"]):
        vals = [r[k] for r in v["rows"]]
        arrays.append(dict_array(vals) if typ == "dict" else pa.array(vals, type={"int64": pa.int64(), "float64": pa.float64(), "bool": pa.bool_()}[typ]))
    return pa.RecordBatch.from_arrays(arrays, names=[c for c, _ in v["cols"]])


def _rows_of(rec: pa.RecordBatch):
    cols = []
    for c in rec.columns:
        vals = c.to_pylist()
        cols.append([x.decode() if isinstance(x, bytes) else x for x in vals])
    return [tuple(r) for r in zip(*cols)] if cols else []


@pytest.mark.parametrize("v", VECTORS, ids=[v["id"] for v in VECTORS])
def test_golden_vectors(v):
    rec = _vector_record(v)
    plan = pp.Projection(v["select"], filter_expr=v["where"])
    rb = pp.ResidentBatch(rec)
    try:
        src = plan.FilterResident(rb) if v["where"] is not None else rb
        out = plan.ProjectResident(src)
        got = out.to_arrow()
        assert got.schema.names == v["out"], v["cite"]
        assert _rows_of(got) == v["expected"], v["cite"]
        host_in = src.to_arrow() if v["where"] is not None else rec
        host = plan.Callback(host_in)
        assert host.schema.names == v["out"] and _rows_of(host) == v["expected"], v["cite"]
        out.close()
        if src is not rb:
            src.close()
    finally:
        rb.close()
        plan.Close()


# ---- 2. differential -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", DIFF_CASES, ids=[c["id"] for c in DIFF_CASES])
def test_differential_against_numpy(records, case):
    datas, recs, rbs = records
    plan = pp.Projection(case["exprs"])
    try:
        outs = plan.ProjectResidentMany(rbs)
        assert plan.last_kernel() == "fdb_project_kernel"
        for n, data, out in zip(ROW_COUNTS, datas, outs):
            got = out.to_arrow()
            out.close()
            assert got.num_rows == n and got.schema.names == [expr_name(e) for e in case["exprs"]]
            for k, e in enumerate(case["exprs"]):
                raw, valid, kind = evaluate(e, data)
                check_column(got.column(k), raw, valid, kind, (case["id"], expr_name(e), n))
        # the host-record entry point over one of the records (several tiles + a ragged tail)
        k = ROW_COUNTS.index(4099)
        host = plan.Callback(recs[k])
        for j, e in enumerate(case["exprs"]):
            raw, valid, kind = evaluate(e, datas[k])
            check_column(host.column(j), raw, valid, kind, (case["id"], expr_name(e), "host"))
    finally:
        plan.Close()


def test_division_properties(records):
    """What the differential data must contain for the division rules to be exercised at all."""
    datas, _, _ = records
    a, av, _ = datas[-1]["a"]
    b, bv, _ = datas[-1]["b"]
    assert ((a == I64_MIN) & (b == -1)).any(), "MinInt64 / -1"
    assert ((b == 0) & bv).any() and ((b == 0) & ~bv).any() and ((b != 0) & ~bv).any(), "zero divisors, valid and under a NULL; non-zero raw slots under NULLs"
    q, _ = _go_div_i64(a, b)
    assert (q < 0).any() and ((a % np.where(b == 0, 1, b) != 0) & (q < 0)).any(), "negative quotients that truncate"
    g = datas[-1]["g"][0]
    assert (np.signbit(g) & (g == 0)).any(), "-0.0 as a divisor"
    f = datas[-1]["f"][0]
    assert np.isnan(f).any() and np.isinf(f).any() and ((f != 0) & (np.abs(f) < 2.3e-308)).any(), "NaN, Inf, denormals"
    assert (datas[-1]["u"][0] > np.uint64(2**63)).any()


# ---- 3. pass-through -------------------------------------------------------------------------------------------------------------------
def _labels_record(n=1500, seed=3):
    rng = np.random.default_rng(seed)
    valid = rng.random(n) >= 0.3
    cols = {
        "labels.zone": dict_array([None if rng.random() < 0.2 else f"z{rng.integers(0, 4)}" for _ in range(n)]),
        "value": _nullable(rng.integers(-9, 9, n, dtype=np.int64), valid, pa.int64()),
        "labels.app": dict_array([f"a{rng.integers(0, 7)}" for _ in range(n)]),
        "flag": pa.array([None if rng.random() < 0.1 else bool(rng.integers(0, 2)) for _ in range(n)], type=pa.bool_()),
        "fv": _nullable(rng.standard_normal(n), rng.random(n) >= 0.1, pa.float64()),
        "timestamp": pa.array(rng.integers(0, 10**9, n, dtype=np.int64)),
        "labels.node": dict_array([None if i % 97 else "n0" for i in range(n)]),
    }
    return pa.RecordBatch.from_arrays(list(cols.values()), names=list(cols.keys()))


def _same_column(got: pa.Array, exp: pa.Array, what):
    assert len(got) == len(exp) and got.null_count == exp.null_count, what
    if pa.types.is_dictionary(exp.type):
        assert got.to_pylist() == exp.to_pylist(), what  # (indices leave as uint32 whatever they came as)
        assert got.dictionary.to_pylist() == exp.dictionary.to_pylist(), what
        return
    assert got.type == exp.type, what
    assert got.is_valid().to_pylist() == exp.is_valid().to_pylist(), what
    if pa.types.is_boolean(exp.type):
        assert got.to_pylist() == exp.to_pylist(), what
        return
    n = len(exp)
    g = np.frombuffer(got.buffers()[1], dtype=np.uint64)[:n]
    x = np.frombuffer(exp.buffers()[1], dtype=np.uint64)[exp.offset: exp.offset + n]
    np.testing.assert_array_equal(g, x, err_msg=str(what))  # bit for bit, the raw slots under NULLs included


def test_pass_through_and_item_kinds():
    rec = _labels_record()
    rb = pp.ResidentBatch(rec)
    V, T = Col("value"), Col("timestamp")
    try:
        # the order of a dynamic set is the RECORD's field order; a plain column the record lacks is skipped; computed items share inputs
        plan = pp.Projection([Col("fv"), DynCol("labels"), Col("absent"), V * T, Col("flag"), V + T, Col("value"), DynCol("nothing")])
        for got in (plan.ProjectResident(rb), plan.Callback(rec)):
            rec_out = got.to_arrow() if isinstance(got, pp.ResidentBatch) else got
            assert rec_out.schema.names == ["fv", "labels.zone", "labels.app", "labels.node", "value * timestamp", "flag", "value + timestamp", "value"]
            for name in ("fv", "labels.zone", "labels.app", "labels.node", "flag", "value"):
                _same_column(rec_out.column(name), rec.column(name), name)
            v = np.frombuffer(rec.column("value").buffers()[1], dtype=np.int64)[: rec.num_rows]
            t = np.asarray(rec.column("timestamp"))
            np.testing.assert_array_equal(np.frombuffer(rec_out.column("value * timestamp").buffers()[1], dtype=np.int64)[: rec.num_rows], v * t)
            np.testing.assert_array_equal(np.frombuffer(rec_out.column("value + timestamp").buffers()[1], dtype=np.int64)[: rec.num_rows], v + t)
            assert rec_out.column("value * timestamp").null_count == 0
            if isinstance(got, pp.ResidentBatch):
                got.close()
        plan.Close()
        # the output does not depend on the input's lifetime
        plan = pp.Projection([Col("value"), Col("labels.app")])
        rb2 = pp.ResidentBatch(rec)
        out = plan.ProjectResident(rb2)
        rb2.close()
        got = out.to_arrow()
        _same_column(got.column("value"), rec.column("value"), "value after release")
        _same_column(got.column("labels.app"), rec.column("labels.app"), "labels.app after release")
        out.close()
        # kind 3 (every field) and the zero-field call, through the C ABI's item list
        items = (pp.ProjectCol * 1)()
        items[0].kind, items[0].name = pp.PROJECT_ALL, None
        plan._items, plan._n_items = items, 1
        out = plan.ProjectResident(rb)
        got = out.to_arrow()
        out.close()
        assert got.schema.names == rec.schema.names
        for name in rec.schema.names:
            _same_column(got.column(name), rec.column(name), name)
        plan._n_items = 0
        out = plan.ProjectResident(rb)
        got = out.to_arrow()
        assert (out.num_rows, got.num_columns, got.num_rows) == (0, 0, 0)
        out.close()
        plan.Close()
        plan = pp.Projection([Col("absent")])  # …also when every item expands to nothing
        out = plan.ProjectResident(rb)
        assert (out.num_rows, out.to_arrow().num_columns) == (0, 0)
        out.close()
        plan.Close()
    finally:
        rb.close()


# ---- 4. chaining -----------------------------------------------------------------------------------------------------------------------
def test_filter_then_project_and_project_then_aggregate():
    rec = _labels_record(n=5000, seed=11)
    rb = pp.ResidentBatch(rec)
    V, T = Col("value"), Col("timestamp")
    plan = pp.Projection([Col("labels.app"), V * T], filter_expr=T > 500_000_000)
    fused = pp.HashAggregatePlan(None, [Sum(V * T)], [Col("labels.app")])
    split = pp.HashAggregatePlan(None, [Sum(Col("value * timestamp"))], [Col("labels.app")])
    try:
        filtered = plan.FilterResident(rb)
        out = plan.ProjectResident(filtered)
        got = out.to_arrow()
        v = np.frombuffer(rec.column("value").buffers()[1], dtype=np.int64)[: rec.num_rows]
        t = np.asarray(rec.column("timestamp"))
        keep = t > 500_000_000
        assert got.num_rows == int(keep.sum())
        np.testing.assert_array_equal(np.frombuffer(got.column(1).buffers()[1], dtype=np.int64)[: got.num_rows], (v * t)[keep])
        assert got.column(0).to_pylist() == [x for x, k in zip(rec.column("labels.app").to_pylist(), keep) if k]
        filtered.close()
        out.close()
        # Projection → HashAggregate equals the fused chain, bit for bit (int64 sums)
        projected = plan.ProjectResident(rb)
        split.Callback(projected)
        fused.Callback(rb)
        a, b = split.Finish(), fused.Finish()
        projected.close()
        assert a.schema.names == b.schema.names == ["labels.app", "sum(value * timestamp)"]
        assert dict(zip(a.column(0).to_pylist(), a.column(1).to_pylist())) == dict(zip(b.column(0).to_pylist(), b.column(1).to_pylist()))
        assert a.num_rows == 7
    finally:
        for p in (plan, fused, split):
            p.Close()
        rb.close()


def test_zero_row_records_without_buffers():
    """A filter that selects nothing returns a record without any buffer, and so does a projection of it: both project to zero-row
    columns of the right types — alone, and as one record of a ProjectResidentMany call."""
    rec = _labels_record(n=3000, seed=2)
    rb = pp.ResidentBatch(rec)
    V, T = Col("value"), Col("timestamp")
    exprs = [Col("labels.app"), V * T, V / T, Col("labels.app") == "a1", Col("fv")]
    names = [expr_name(e) for e in exprs]
    types = [rec.schema.field("labels.app").type.value_type, pa.int64(), pa.int64(), pa.bool_(), pa.float64()]
    plan = pp.Projection(exprs, filter_expr=T < 0)  # selects no row
    try:
        empty = plan.FilterResident(rb)
        assert empty.num_rows == 0
        out = plan.ProjectResident(empty)
        again = pp.Projection([Col("value * timestamp") + Col("value / timestamp"), Col("fv")])
        out2 = again.ProjectResident(out)  # a zero-row projected batch, projected again
        many = plan.ProjectResidentMany([rb, empty, rb])
        for o in (out, many[1]):
            got = o.to_arrow()
            assert got.num_rows == 0 and got.schema.names == names
            for k, t in enumerate(types):
                ft = got.schema.field(k).type
                assert (ft.value_type if pa.types.is_dictionary(ft) else ft) == t, (names[k], ft)
        got2 = out2.to_arrow()
        assert got2.num_rows == 0 and got2.schema.names == ["value * timestamp + value / timestamp", "fv"]
        assert [f.type for f in got2.schema] == [pa.int64(), pa.float64()]
        a, b = many[0].to_arrow(), many[2].to_arrow()
        assert a.num_rows == b.num_rows == rec.num_rows and a.equals(b)
        for o in [empty, out, out2] + many:
            o.close()
        again.Close()
    finally:
        plan.Close()
        rb.close()


# ---- 5. AVG on the device --------------------------------------------------------------------------------------------------------------
def test_avg_finishes_on_the_device():
    """avg(x) = sum(x) / convert(count(x), float64) behind the final aggregate (logicalplan/builder.go:205-238): every quotient is the
    correctly rounded IEEE quotient of the Finish's own two columns."""
    n, groups = 40_000, 3001
    rng = np.random.default_rng(5)
    rec = pa.RecordBatch.from_arrays([dict_array([f"/p/{i}" for i in rng.integers(0, groups, n)]), pa.array(rng.standard_normal(n) * 1e3 + rng.random(n) / 3)],
                                     names=["labels.path", "value"])
    agg = pp.HashAggregatePlan(None, [Sum(Col("value")), Count(Col("value"))], [Col("labels.path")])
    avg = (Col("sum(value)") / Convert(Col("count(value)"), "float64")).Alias("avg(value)")
    plan = pp.Projection([Col("labels.path"), avg])
    try:
        agg.Callback(rec)
        fin = agg.FinishResident()
        out = plan.ProjectResident(fin)
        f, got = fin.to_arrow(), out.to_arrow()
        fin.close()
        out.close()
        assert got.schema.names == ["labels.path", "avg(value)"] and got.num_rows == f.num_rows > 1000
        assert got.column(0).to_pylist() == f.column("labels.path").to_pylist()
        exp = np.asarray(f.column("sum(value)")) / np.asarray(f.column("count(value)")).astype(np.float64)
        assert got.column(1).null_count == 0 and got.column(1).buffers()[0] is None
        np.testing.assert_array_equal(np.asarray(got.column(1)).view(np.uint64), exp.view(np.uint64))
    finally:
        agg.Close()
        plan.Close()


# ---- 6. several records in one launch --------------------------------------------------------------------------------------------------
def test_many_records_equal_one_by_one(records):
    _, _, rbs = records
    pick = [ROW_COUNTS.index(n) for n in (1025, 0, 7, 70001, 256)]
    A, B, C = Col("a"), Col("b"), Col("c")
    plan = pp.Projection([Col("d"), (A / B) + C, A / B, Col("f")])
    try:
        many = plan.ProjectResidentMany([rbs[k] for k in pick])
        for k, m in zip(pick, many):
            one = plan.ProjectResident(rbs[k])
            x, y = m.to_arrow(), one.to_arrow()
            m.close()
            one.close()
            assert x.num_rows == ROW_COUNTS[k] and x.schema == y.schema
            for j in range(x.num_columns):
                assert x.column(j).null_count == y.column(j).null_count
                bx, by = x.column(j).buffers(), y.column(j).buffers()
                for p, q in zip(bx[:2], by[:2]):
                    assert (p is None) == (q is None) and (p is None or p.to_pybytes() == q.to_pybytes()), (ROW_COUNTS[k], j)
        assert plan.ProjectResidentMany([]) == []
    finally:
        plan.Close()


# ---- 7. errors -------------------------------------------------------------------------------------------------------------------------
def test_errors(records, monkeypatch):
    _, recs, rbs = records
    rb = rbs[ROW_COUNTS.index(257)]
    A, F = Col("a"), Col("f")
    plan = pp.Projection([A * F])  # int64 × float64: the reference type-asserts the right array to the left one's type
    with pytest.raises(pp.FdbError) as ei:
        plan.ProjectResident(rb)
    assert ei.value.code == pp.FDB_ERR_INVALID
    with pytest.raises(pp.FdbError):
        plan.Callback(recs[ROW_COUNTS.index(257)])
    plan.Close()
    plan = pp.Projection([Col("nope") * A])
    with pytest.raises(pp.FdbError) as ei:
        plan.ProjectResident(rb)
    assert ei.value.code == pp.FDB_ERR_NOT_FOUND
    plan.Close()
    plan = pp.Projection([A + A])
    plan._names[0] = b"a - a"  # a computed item that names no projection of the plan
    plan._items[0].name = plan._names[0]
    with pytest.raises(pp.FdbError) as ei:
        plan.ProjectResident(rb)
    assert ei.value.code == pp.FDB_ERR_INVALID
    plan._items[0].kind = 9
    with pytest.raises(pp.FdbError):
        plan.ProjectResident(rb)
    plan.Close()
    # a filter-only plan still refuses push
    plan = pp.Projection([A + A])
    with pytest.raises(pp.FdbError) as ei:
        plan._check(pp.lib().fdb_plan_push_batch(plan.handle, rb.handle))
    assert ei.value.code == pp.FDB_ERR_STATE
    plan.Close()
    # without the run-time compiler: computed items are refused, pass-through-only calls work
    monkeypatch.setenv("FDB_NO_JIT", "1")
    plan = pp.Projection([Col("d"), A + A])
    with pytest.raises(pp.UnsupportedError):
        plan.ProjectResident(rb)
    plan.Close()
    plan = pp.Projection([Col("d"), Col("a")])
    out = plan.ProjectResident(rb)
    got = out.to_arrow()
    out.close()
    plan.Close()
    _same_column(got.column("a"), recs[ROW_COUNTS.index(257)].column("a"), "a without the compiler")
    monkeypatch.delenv("FDB_NO_JIT")


# ---- 8. allocations --------------------------------------------------------------------------------------------------------------------
def test_every_output_is_released(records):
    import gc
    _, _, rbs = records
    gc.collect()
    before = pp.live_allocations()
    plan = pp.Projection([Col("a") / Col("b"), Col("d"), Col("f") * Col("g")])
    outs = plan.ProjectResidentMany(rbs)
    assert pp.live_allocations()["device_bytes"] > before["device_bytes"]
    for o in outs:
        o.close()
    plan.Close()
    assert pp.live_allocations() == before
