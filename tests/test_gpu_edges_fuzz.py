"""Edge values through filters, merges and exchanges: int64 at INT64_MIN / INT64_MAX and sums that wrap, uint64 at and above 2^63,
float64 subnormals, ±DBL_MIN, huge values, ±inf, NaN and ±0.0, bools and NULLs in every column — pushed through every way the
operator is composed (one plan, chains folded with Merge, partial plans feeding a final stage, ranks merged by the aligned all-reduce
or by the exchange, exact sums, the interpreting kernels) and checked against a plain Python reference written here AND the oracle.
A second part runs every numeric leaf kind with every operator over edge literals through every filter path.

Fixed seeds: every case is reproducible by its id."""
import math
import struct

import numpy as np
import pyarrow as pa
import pytest

from frostdb_amd.logicalplan import (OP_EQ, OP_GT, OP_GT_EQ, OP_LT, OP_LT_EQ, OP_NOT_EQ, OP_AND, OP_OR, And, AndAgg, BinaryExpr, Col,
                                     Count, DynCol, Literal, Max, Min, Or, Sum, UInt64, Unique)
from tests.test_exact_sums_cpu import reference as exact_reference
from tests.util import arrow_to_pydict

pytestmark = pytest.mark.gpu

I64_MIN, I64_MAX = -(2**63), 2**63 - 1
I64_EDGES = [I64_MIN, I64_MIN + 1, -1, 0, 1, I64_MAX - 1, I64_MAX, 2**53, -(2**53), 2**53 + 1, -(2**53 + 1)]
U64_EDGES = [0, 1, 2**63 - 1, 2**63, 2**63 + 1, 2**64 - 2, 2**64 - 1]
SUB_MIN, SUB_MAX, DBL_MIN = 5e-324, 2.225073858507201e-308, 2.2250738585072014e-308
F64_EDGES = [0.0, -0.0, SUB_MIN, -SUB_MIN, SUB_MAX, -SUB_MAX, DBL_MIN, -DBL_MIN, 1e308, -1e308, math.inf, -math.inf, math.nan]
UQ_POOL = [I64_MAX, I64_MIN, 0, -1, 7, I64_MAX - 1, I64_MIN + 1, 2**53 + 1]
EPS = 2.0**-52

# special groups of the dictionary key (k00000 … k00004): what the accumulators' identities and the float atomics could get wrong
G_SUBNORMAL, G_WRAP, G_ALL_MAX, G_ALL_MIN, G_ALL_NAN = range(5)


@pytest.fixture(scope="module")
def pp():
    from frostdb_amd import physicalplan
    assert physicalplan.device_count() >= 1
    return physicalplan


@pytest.fixture(scope="module")
def fcomm():
    from frostdb_amd import comm
    return comm


def bits(x: float) -> int:
    return struct.unpack("<Q", struct.pack("<d", x))[0]


# ---- data ------------------------------------------------------------------------------------------------------------------------

def key_names(card):
    return [b"k%05d" % i for i in range(card)]


def edge_record(rng, n, card, exact, same_dict=False, drop=()):
    """One record mixing friendly values with the edge pools at random rates (per column and per record). `card`: distinct dictionary
    keys (the record draws from a random prefix of them, so chains and ranks hold dense and hash tables side by side); `same_dict`: the
    full dictionary in key order (ranks whose layouts agree); `exact`: huge float64 magnitudes allowed (a non-exact SUM keeps
    Σ|x| < DBL_MAX per group so that no summation order overflows)."""
    names = key_names(card)
    if same_dict:
        dvals, hi = names, card
    else:
        hi = card if rng.random() < 0.5 else max(8, int(card * rng.uniform(0.05, 1.0)))
        dvals = [names[i] for i in rng.permutation(hi)]
    pos = {v: i for i, v in enumerate(dvals)}
    kid = rng.integers(0, hi, size=n)
    if card >= 16 and rng.random() < 0.7:  # weight the special groups so that they always have rows
        sp = rng.random(n) < 0.15
        kid[sp] = rng.integers(0, 5, size=int(sp.sum()))
    idx = np.array([pos[names[k]] for k in kid], dtype=np.uint32)
    knull = rng.random(n) < rng.choice([0.0, 0.02, 0.1])
    cols = {"labels.k": pa.DictionaryArray.from_arrays(pa.array(idx, type=pa.uint32(), mask=knull), pa.array(dvals, type=pa.binary()))}
    special = ~knull & (card >= 16)

    def mix(friendly, pool, rate):
        pick = rng.random(n) < rate
        out = list(friendly)
        for i in np.flatnonzero(pick):
            out[i] = pool[int(rng.integers(0, len(pool)))]
        return out

    def nulls(rate):
        return rng.random(n) < rate

    ik = mix(rng.integers(-3, 4, size=n).tolist(), I64_EDGES, rng.uniform(0.0, 0.5))
    cols["ikey"] = pa.array(ik, type=pa.int64(), mask=nulls(0.05))
    uk = mix(rng.integers(0, 4, size=n).tolist(), U64_EDGES, rng.uniform(0.0, 0.6))
    cols["ukey"] = pa.array(uk, type=pa.uint64(), mask=nulls(0.05))
    cols["flag"] = pa.array((rng.random(n) < rng.uniform(0.5, 1.0)).tolist(), type=pa.bool_(), mask=nulls(rng.choice([0.0, 0.1, 0.5])))

    big = [int(x) for x in rng.integers(I64_MIN, I64_MAX, size=64, endpoint=True)]
    iv = mix(rng.integers(-20, 20, size=n).tolist(), I64_EDGES + big, rng.choice([0.0, 0.05, 0.3]))
    imask = nulls(rng.choice([0.0, 0.1]))
    fpool = F64_EDGES if exact else [1e300 if x == 1e308 else -1e300 if x == -1e308 else x for x in F64_EDGES]
    fv = mix(rng.uniform(-5, 5, size=n).tolist(), fpool, rng.choice([0.0, 0.05, 0.3]))
    fmask = nulls(rng.choice([0.0, 0.1]))
    uq = [UQ_POOL[k % len(UQ_POOL)] for k in kid]
    uqmask = np.zeros(n, dtype=bool)
    for i in range(n):
        if special[i] and kid[i] == G_SUBNORMAL:
            fv[i] = float(rng.integers(-(2**52), 2**52)) * SUB_MIN if rng.random() < 0.9 else SUB_MAX
            fmask[i] = False
        elif special[i] and kid[i] == G_WRAP:
            iv[i] = int(rng.integers(2**61, 2**62)) * (1 if rng.random() < 0.9 else -1)  # Σ wraps once several rows come together
            imask[i] = False
        elif special[i] and kid[i] == G_ALL_MAX:
            iv[i], imask[i] = I64_MAX, False
            fv[i], fmask[i] = (math.inf if exact else 1e300), False
        elif special[i] and kid[i] == G_ALL_MIN:
            iv[i], imask[i] = I64_MIN, False
            fv[i], fmask[i] = -0.0, False
        elif special[i] and kid[i] == G_ALL_NAN:
            fv[i], fmask[i] = math.nan, False
        if kid[i] % 11 == 5 and rng.random() < 0.01:  # a few keys lose UNIQUE to a second value or a NULL
            if rng.random() < 0.5:
                uq[i] = uq[i] ^ 1
            else:
                uqmask[i] = True
    cols["ival"] = pa.array(iv, type=pa.int64(), mask=imask)
    cols["fval"] = pa.array(fv, type=pa.float64(), mask=fmask)
    cols["uq"] = pa.array(uq, type=pa.int64(), mask=uqmask)
    for d in drop:
        cols.pop(d, None)
    return pa.RecordBatch.from_arrays(list(cols.values()), names=list(cols.keys()))


# ---- plans -----------------------------------------------------------------------------------------------------------------------

def random_numeric_leaf(rng):
    k = int(rng.integers(0, 9))
    op = [OP_EQ, OP_NOT_EQ, OP_LT, OP_LT_EQ, OP_GT, OP_GT_EQ][int(rng.integers(0, 6))]
    if k == 0:
        return BinaryExpr(Col("ival"), op, Literal(I64_EDGES[int(rng.integers(0, len(I64_EDGES)))] if rng.random() < 0.5 else int(rng.integers(-20, 20))))
    if k == 1:
        return BinaryExpr(Col("ival"), op, Literal([2.0**63, -(2.0**63), 2.0**53, 0.5, -3.5, math.inf, math.nan][int(rng.integers(0, 7))]))
    if k == 2:
        return BinaryExpr(Col("fval"), op, Literal([0.0, -0.0, SUB_MIN, -DBL_MIN, 1.5, -2.0, math.inf, math.nan][int(rng.integers(0, 8))]))
    if k == 3:
        return BinaryExpr(Col("ukey"), op, Literal(UInt64(U64_EDGES[int(rng.integers(0, len(U64_EDGES)))])))
    if k == 4:
        return BinaryExpr(Col("ukey"), op, Literal(int(rng.integers(0, 4))))
    if k == 5:
        return BinaryExpr(Col("flag"), op, Literal(bool(rng.random() < 0.5)))
    if k == 6:
        return BinaryExpr(Col("ikey"), op, Literal(I64_EDGES[int(rng.integers(0, len(I64_EDGES)))]))
    if k == 7:
        return BinaryExpr(Col("fval"), op, Literal(int(rng.integers(-3, 3))))
    return Col("labels.k") == "k%05d" % rng.integers(0, 8) if rng.random() < 0.5 else Col("labels.k") != "k00001"


def random_numeric_filter(rng, depth=0):
    r = rng.random()
    if depth >= 2 or r < 0.5:
        return random_numeric_leaf(rng)
    return (And if r < 0.8 else Or)(random_numeric_filter(rng, depth + 1), random_numeric_filter(rng, depth + 1))


AGG_POOL = [Sum(Col("ival")), Min(Col("ival")), Max(Col("ival")), Count(Col("ival")), Sum(Col("fval")), Min(Col("fval")),
            Max(Col("fval")), Unique(Col("uq")), AndAgg(Col("flag")), Count(Col("fval"))]
GROUP_POOL = [[Col("labels.k")], [Col("labels.k"), Col("flag")], [Col("ikey")], [Col("ukey")], [Col("labels.k"), Col("ikey")],
              [Col("flag")], [], [Col("ukey"), Col("flag")], [Col("labels.k"), Col("ukey")]]


def random_aggs(rng):
    aggs = [AGG_POOL[i] for i in sorted(rng.choice(len(AGG_POOL), size=int(rng.integers(1, 7)), replace=False))]
    if not any(a.Name() == "sum(fval)" for a in aggs) and rng.random() < 0.5:
        aggs.append(Sum(Col("fval")))  # (the float SUM is where the atomics and the exact limbs live: most cases carry one)
    return aggs


# ---- the reference ---------------------------------------------------------------------------------------------------------------

def np_select(expr, rec):
    """numpy's rows for a predicate of numeric / bool leaves (None if it holds another kind of leaf or a column the record lacks)."""
    if isinstance(expr, BinaryExpr) and expr.op in (OP_AND, OP_OR):
        a, b = np_select(expr.left, rec), np_select(expr.right, rec)
        if a is None or b is None:
            return None
        return (a & b) if expr.op == OP_AND else (a | b)
    name, lit = expr.left.name, expr.right.value
    if name not in rec.schema.names:
        return None
    col = rec.column(name)
    if pa.types.is_dictionary(col.type):
        return None
    valid = np.asarray(col.is_valid())
    if pa.types.is_boolean(col.type):
        v = np.asarray(col.fill_null(False)).astype(np.int64)
        lv = np.int64(int(lit))
    elif pa.types.is_uint64(col.type):
        v = np.asarray(col.fill_null(0))
        lv = np.uint64(int(lit))
    elif pa.types.is_int64(col.type) and isinstance(lit, float):
        v = np.asarray(col.fill_null(0)).astype(np.float64)  # the column converted to double, compared with the float literal
        lv = np.float64(lit)
    elif pa.types.is_int64(col.type):
        v = np.asarray(col.fill_null(0))
        lv = np.int64(lit)
    else:
        v = np.asarray(col.fill_null(0.0))
        lv = np.float64(lit)
    with np.errstate(invalid="ignore"):
        r = {OP_EQ: v == lv, OP_NOT_EQ: v != lv, OP_LT: v < lv, OP_LT_EQ: v <= lv, OP_GT: v > lv, OP_GT_EQ: v >= lv}[expr.op]
    return r & valid


def oracle_select(filt, rec):
    from oracle import OraclePlan
    o = OraclePlan(filt)
    try:
        out, idx = o.filter(rec)
        if out is not None:
            out.close()
        return idx
    finally:
        o.close()


def selected_rows(filt, recs):
    """[(record, selected row indices)]: the oracle's filter(); for numeric predicates numpy must agree."""
    out = []
    for r in recs:
        if filt is None:
            out.append((r, np.arange(r.num_rows)))
            continue
        idx = oracle_select(filt, r)
        want = np_select(filt, r)
        if want is not None:
            assert list(idx) == list(np.flatnonzero(want)), ("oracle and numpy disagree", str(filt))
        out.append((r, idx))
    return out


def key_of(v, typ):
    if typ in ("i", "u") and v == 0:
        return None  # int64 / uint64 key 0 ≡ NULL (the reference's hash identity)
    return v


class Group:
    __slots__ = ("n", "vals", "valid")

    def __init__(self, n_aggs):
        self.n = 0
        self.vals = [[] for _ in range(n_aggs)]
        self.valid = [[] for _ in range(n_aggs)]


def py_reference(sel, aggs, groups):
    """{key tuple: Group} over the selected rows in arrival order. A NULL contributes the builder's zeroed slot (0 / 0.0) to SUM, MIN
    and MAX."""
    gnames = [g.name for g in groups]
    out = {}
    for rec, idx in sel:
        names = rec.schema.names
        keys = []
        for g in gnames:
            if g not in names:
                keys.append([None] * len(idx))
                continue
            c = rec.column(g)
            typ = "i" if pa.types.is_int64(c.type) else "u" if pa.types.is_uint64(c.type) else "o"
            if pa.types.is_dictionary(c.type):
                c = c.dictionary_decode()
            vals = c.take(pa.array(idx, type=pa.int64())).to_pylist()
            keys.append([key_of(v, typ) for v in vals])
        ins = [rec.column(a.expr.name).take(pa.array(idx, type=pa.int64())).to_pylist() for a in aggs]
        for i in range(len(idx)):
            k = tuple(kc[i] for kc in keys)
            grp = out.get(k)
            if grp is None:
                grp = out[k] = Group(len(aggs))
            grp.n += 1
            for j, a in enumerate(aggs):
                v = ins[j][i]
                grp.valid[j].append(v is not None)
                grp.vals[j].append(v)
    return out


def want_value(a, grp, j, exact):
    """What the device must return for aggregation `a` of a group, by its documented rule."""
    vals, valid = grp.vals[j], grp.valid[j]
    fn, col = a.Name().split("(")[0], a.expr.name
    if fn == "count":
        return grp.n
    if fn == "unique":
        return vals[0] if all(valid) and all(v == vals[0] for v in vals) else None
    if fn == "and":
        return all(v for v in vals if v is not None)
    if col == "ival":
        z = [v if v is not None else 0 for v in vals]
        if fn == "sum":
            s = sum(z) % 2**64
            return s - 2**64 if s >= 2**63 else s
        return min(z) if fn == "min" else max(z)
    z = [v if v is not None else 0.0 for v in vals]
    if fn == "sum":
        return exact_reference(z) if exact else ("fsum", z)
    nn = [v for v in z if not math.isnan(v)]
    if not nn:
        return math.nan
    return (min(nn) if fn == "min" else max(nn)) + 0.0  # (+ 0.0: −0.0 is reported as +0.0)


def check_float_sum(got, z, ctx):
    has_nan = any(math.isnan(v) for v in z) or (math.inf in z and -math.inf in z)
    if has_nan:
        assert math.isnan(got), ctx
        return
    if math.inf in z or -math.inf in z:
        assert got == (math.inf if math.inf in z else -math.inf), ctx
        return
    exact = math.fsum(z)
    bound = 4 * len(z) * EPS * math.fsum(abs(v) for v in z)
    assert math.isfinite(got) and abs(got - exact) <= bound, (ctx, got, exact, bound)


def canon_result(d, gnames, gtypes):
    """Device / oracle result → {key tuple: {agg name: value}}; int64 / uint64 key 0 folded into NULL."""
    n = len(next(iter(d.values()))) if d else 0
    out = {}
    for i in range(n):
        k = tuple(key_of(d[g][i], gtypes[g]) if g in d else None for g in gnames)
        assert k not in out, ("a group appears twice", k)
        out[k] = {c: d[c][i] for c in d if c not in gnames}
    return out


def group_types(recs, groups):
    t = {}
    for g in groups:
        for r in recs:
            if g.name in r.schema.names:
                ty = r.schema.field(g.name).type
                t[g.name] = "i" if pa.types.is_int64(ty) else "u" if pa.types.is_uint64(ty) else "o"
    return {g.name: t.get(g.name, "o") for g in groups}


def first_value(grp, j):
    return grp.vals[j][0] if grp.vals[j][0] is not None else 0.0


def compare(got, recs, filt, aggs, groups, exact, oracle=True):
    """The device result against the Python reference (every value, by the documented rules) and the oracle (every value whose
    reference answer does not depend on row order)."""
    sel = selected_rows(filt, recs)
    ref = py_reference(sel, aggs, groups)
    gnames = [g.name for g in groups]
    gt = group_types(recs, groups)
    dev = canon_result(got, gnames, gt)
    if not ref:
        assert not dev, ("nothing selected, yet groups came back", len(dev))
        return
    assert dev.keys() == ref.keys(), (len(dev), len(ref), sorted(set(dev) ^ set(ref), key=repr)[:5])
    for k, grp in ref.items():
        for j, a in enumerate(aggs):
            name = a.Name()
            w, g = want_value(a, grp, j, exact), dev[k][name]
            ctx = (k, name, str(filt))
            if isinstance(w, tuple):
                check_float_sum(g, w[1], ctx)
            elif isinstance(w, float):
                assert (math.isnan(w) and math.isnan(g)) or (g == w and bits(g) == bits(w)), (ctx, g, w)
            else:
                assert g == w and type(g) is type(w), (ctx, g, w)
    if not oracle:
        return
    from oracle import OraclePlan
    o = OraclePlan(filt, aggs, groups, nchains=1)
    try:
        for r in recs:
            o.push(r)
        want = o.finish().to_pydict()
    finally:
        o.close()
    orc = canon_result(want, gnames, gt)
    assert orc.keys() == ref.keys(), (len(orc), len(ref))
    for k, grp in ref.items():
        for j, a in enumerate(aggs):
            name = a.Name()
            w, g = orc[k][name], dev[k][name]
            fn = name.split("(")[0]
            if a.expr.name == "fval" and fn in ("min", "max"):
                if math.isnan(first_value(grp, j)):
                    continue  # the reference keeps a NaN only as the group's FIRST value: order-dependent, the device rule applies
                assert (math.isnan(w) and math.isnan(g)) or w == g, (k, name, g, w)  # (== : which signed zero it keeps is order-dependent)
            elif a.expr.name == "fval" and fn == "sum":
                z = [v if v is not None else 0.0 for v in grp.vals[j]]
                if exact and sum(abs(v) for v in z if math.isfinite(v)) >= 1e307:
                    continue  # the oracle adds in row order and may overflow where the exact sum does not
                check_float_sum(w, z, (k, name, "oracle"))
            else:
                assert w == g, (k, name, g, w)


# ---- composition modes -----------------------------------------------------------------------------------------------------------

def run_ranks(n, fn):
    from tests.test_gpu_comm import run_ranks as rr
    return rr(n, fn)


def push(pp, plan, recs, resident, keep):
    if resident:
        rbs = [pp.ResidentBatch(r) for r in recs]
        keep += rbs
        if rbs:
            plan.CallbackResident(rbs)
    else:
        for r in recs:
            plan.Callback(r)


def split(rng, recs, k):
    """Records sliced at random points and dealt to k chains (every chain gets at least one slice)."""
    pieces = []
    for r in recs:
        cuts = sorted(set(int(x) for x in rng.integers(0, r.num_rows + 1, size=int(rng.integers(0, 3)))))
        lo = 0
        for c in cuts + [r.num_rows]:
            if c > lo:
                pieces.append(r.slice(lo, c - lo))
            lo = c
    while len(pieces) < k:
        pieces.append(recs[0].slice(0, 0))
    order = rng.permutation(len(pieces))
    parts = [[] for _ in range(k)]
    for i, p in enumerate(order):
        parts[i % k if i < k else int(rng.integers(0, k))].append(pieces[p])
    return parts


def make_plan(pp, filt, aggs, groups, exact, final_stage=False):
    p = pp.HashAggregatePlan(filt, aggs, groups, final_stage=final_stage)
    if exact:
        p.set_exact_sums(True)
    return p


def run_single(pp, rng, recs, filt, aggs, groups, exact):
    resident = rng.random() < 0.5
    plan = make_plan(pp, filt, aggs, groups, exact)
    keep = []
    try:
        push(pp, plan, recs, resident, keep)
        if resident and rng.random() < 0.5:
            rb = plan.FinishResident()
            keep.append(rb)
            return arrow_to_pydict(rb.to_arrow())
        return arrow_to_pydict(plan.Finish())
    finally:
        plan.Close()
        for k in keep:
            k.close()


def run_chains(pp, rng, recs, filt, aggs, groups, exact):
    k = int(rng.integers(2, 6))
    parts = split(rng, recs, k)
    plans, keep = [], []
    try:
        for part in parts:
            plans.append(make_plan(pp, filt, aggs, groups, exact))
            push(pp, plans[-1], part, rng.random() < 0.5, keep)
        live = list(plans)
        while len(live) > 1:  # fold in a random tree order
            i, j = rng.choice(len(live), size=2, replace=False)
            live[i].Merge(live[j])
            live.pop(j)
        return arrow_to_pydict(live[0].Finish())
    finally:
        for p in plans:
            p.Close()
        for x in keep:
            x.close()


def run_final(pp, rng, recs, filt, aggs, groups, exact):
    k = int(rng.integers(1, 4))
    parts = split(rng, recs, k)
    final = make_plan(pp, None, aggs, groups, False, final_stage=True)
    keep = []
    try:
        for part in parts:
            p = make_plan(pp, filt, aggs, groups, False)
            try:
                push(pp, p, part, rng.random() < 0.5, keep)
                if rng.random() < 0.5:
                    rb = p.FinishResident()
                    keep.append(rb)
                    if rb.num_rows:
                        final.Callback(rb)
                else:
                    for r in p.FinishAll():
                        if r.num_rows:
                            final.Callback(r)
            finally:
                p.Close()
        return arrow_to_pydict(final.Finish())
    finally:
        final.Close()
        for x in keep:
            x.close()


def run_ranks_mode(pp, fcomm, rng, shards, filt, aggs, groups, exact, aligned):
    world = len(shards)
    comms = fcomm.Comm.init_local([0] * world)
    resident = [rng.random() < 0.5 for _ in range(world)]

    def rank_fn(r):
        plan = make_plan(pp, filt, aggs, groups, exact)
        keep = []
        try:
            push(pp, plan, shards[r], resident[r], keep)
            ok = comms[r].allreduce(plan)
            assert ok is aligned, (r, ok)
            if ok:
                return arrow_to_pydict(plan.Finish())
            shard = comms[r].merge_alltoall(plan)
            try:
                return arrow_to_pydict(shard.Finish())
            finally:
                shard.Close()
        finally:
            plan.Close()
            for x in keep:
                x.close()

    try:
        return run_ranks(world, rank_fn)
    finally:
        for c in comms:
            c.close()


def union_of_shards(parts, gnames, gtypes):
    """The exchange's shards are disjoint and their union is the result."""
    seen = set()
    merged = {}
    for p in parts:
        n = len(next(iter(p.values()))) if p else 0
        for k in canon_result(p, gnames, gtypes):
            assert k not in seen, ("a group is in two shards", k)
            seen.add(k)
        for c in p:
            merged.setdefault(c, [])
        for c in merged:
            merged[c] += p.get(c, [None] * n)
    return merged


MODES = ["single", "chains", "final", "allreduce", "exchange", "exact_single", "exact_chains", "exact_exchange", "interpreted"]
CASES = [(MODES[s % len(MODES)], s) for s in range(64)]


def edge_case(pp, fcomm, mode, seed, monkeypatch):
    rng = np.random.default_rng(70_000 + seed)
    exact = mode.startswith("exact")
    if mode == "interpreted":
        monkeypatch.setenv("FDB_NO_JIT", "1")
    else:
        monkeypatch.delenv("FDB_NO_JIT", raising=False)
    filt = random_numeric_filter(rng) if rng.random() < 0.6 else None
    aggs = random_aggs(rng)
    ranks = mode in ("allreduce", "exchange", "exact_exchange")
    if mode == "allreduce":
        groups = [Col("labels.k")]
        card = int(rng.choice([16, 40, 300]))
    else:  # (through the exchange: a key that keeps the ranks' layouts apart — their own dictionaries, or a hash table)
        pool = [g for g in GROUP_POOL if any(c.name in ("labels.k", "ikey", "ukey") for c in g)] if ranks else GROUP_POOL
        groups = pool[int(rng.integers(0, len(pool)))]
        card = int(rng.choice([16, 40, 300, 5_000, 100_000], p=[0.3, 0.2, 0.2, 0.2, 0.1]))
    big = card == 100_000
    n_rec = int(rng.integers(1, 4))
    world = int(rng.integers(2, 4))
    n_parts = world if ranks else n_rec
    recs = []
    for _ in range(n_parts):
        n = int(rng.integers(1, 60_000 if big else 12_000))
        drop = [c for c in ("labels.k", "ikey", "ukey") if not ranks and rng.random() < 0.08]
        recs.append(edge_record(rng, n, card, exact, same_dict=mode == "allreduce", drop=drop))
    gnames = [g.name for g in groups]
    gt = group_types(recs, groups)
    if mode in ("single", "exact_single", "interpreted"):
        got = run_single(pp, rng, recs, filt, aggs, groups, exact)
    elif mode in ("chains", "exact_chains"):
        got = run_chains(pp, rng, recs, filt, aggs, groups, exact)
    elif mode == "final":
        got = run_final(pp, rng, recs, filt, aggs, groups, exact)
    else:
        aligned = mode == "allreduce"
        parts = run_ranks_mode(pp, fcomm, rng, [[r] for r in recs], filt, aggs, groups, exact, aligned)
        if aligned:
            for p in parts[1:]:  # every rank holds the merged table
                assert canon_result(p, gnames, gt).keys() == canon_result(parts[0], gnames, gt).keys()
                compare(p, recs, filt, aggs, groups, exact, oracle=False)
            got = parts[0]
        else:
            got = union_of_shards(parts, gnames, gt)
    compare(got, recs, filt, aggs, groups, exact)


@pytest.mark.parametrize("mode,seed", CASES, ids=[f"{m}-{s}" for m, s in CASES])
def test_edges_fuzz(pp, fcomm, mode, seed, monkeypatch):
    edge_case(pp, fcomm, mode, seed, monkeypatch)


# ---- hand-picked edges -----------------------------------------------------------------------------------------------------------

def small_record(keys, ivals, fvals, uq=None, flags=None, reverse=False):
    n = len(keys)
    d = key_names(8)[::-1] if reverse else key_names(8)
    return pa.RecordBatch.from_arrays(
        [pa.DictionaryArray.from_arrays(pa.array([d.index(k) for k in keys], type=pa.uint32()), pa.array(d, type=pa.binary())),
         pa.array(ivals, type=pa.int64()), pa.array(fvals, type=pa.float64()), pa.array(uq if uq is not None else [7] * n, type=pa.int64()),
         pa.array(flags if flags is not None else [True] * n, type=pa.bool_())],
        names=["labels.k", "ival", "fval", "uq", "flag"])


@pytest.mark.parametrize("how", ["one_plan", "merge", "final_stage", "allreduce", "exchange"])
def test_identities_and_wraps_survive_every_merge(pp, fcomm, how, monkeypatch):
    """Groups whose true MIN is INT64_MAX, whose MAX is INT64_MIN, whose UNIQUE is either, whose float MIN / MAX is ±inf, whose
    float values are all NaN or all subnormal, whose int64 SUM wraps only once the halves meet, and a group that only one half has:
    the answers must not turn into the accumulators' identities or into 'empty' on any path."""
    monkeypatch.delenv("FDB_NO_JIT", raising=False)
    K = key_names(8)
    a = small_record([K[0], K[1], K[2], K[3], K[4], K[5]], [I64_MAX, I64_MIN, 2**62 + 3, I64_MAX, 1, 2],
                     [math.inf, -math.inf, SUB_MIN, math.nan, SUB_MAX, 1.0], uq=[I64_MAX, I64_MIN, 5, 5, 1, 2])
    b = small_record([K[0], K[1], K[2], K[3], K[4], K[6]], [I64_MAX, I64_MIN, 2**62 + 5, I64_MAX, -1, 3],
                     [math.inf, -math.inf, 3 * SUB_MIN, math.nan, SUB_MAX, -1.0], uq=[I64_MAX, I64_MIN, 5, 6, 1, 3],
                     reverse=how == "exchange")  # (its own dictionary order: the ranks' layouts differ, the exchange runs)
    aggs = [Min(Col("ival")), Max(Col("ival")), Sum(Col("ival")), Unique(Col("uq")), Min(Col("fval")), Max(Col("fval")),
            Sum(Col("fval"))]  # (8 accumulators, the most a plan has: UNIQUE takes two)
    groups = [Col("labels.k")]
    if how == "one_plan":
        got = run_single(pp, np.random.default_rng(0), [a, b], None, aggs, groups, False)
    elif how == "merge":
        p, q = pp.HashAggregatePlan(None, aggs, groups), pp.HashAggregatePlan(None, aggs, groups)
        try:
            p.Callback(a); q.Callback(b)
            p.Merge(q)
            got = arrow_to_pydict(p.Finish())
        finally:
            p.Close(); q.Close()
    elif how == "final_stage":
        fin = pp.HashAggregatePlan(None, aggs, groups, final_stage=True)
        try:
            for r in (a, b):
                p = pp.HashAggregatePlan(None, aggs, groups)
                try:
                    p.Callback(r)
                    fin.Callback(p.Finish())
                finally:
                    p.Close()
            got = arrow_to_pydict(fin.Finish())
        finally:
            fin.Close()
    else:
        parts = run_ranks_mode(pp, fcomm, np.random.default_rng(1), [[a], [b]], None, aggs, groups, False, how == "allreduce")
        got = parts[0] if how == "allreduce" else union_of_shards(parts, ["labels.k"], {"labels.k": "o"})
    compare(got, [a, b], None, aggs, groups, False)
    d = {k: i for i, k in enumerate(got["labels.k"])}
    i0, i1, i2 = d[K[0]], d[K[1]], d[K[2]]
    assert got["min(ival)"][i0] == I64_MAX and got["unique(uq)"][i0] == I64_MAX and got["max(fval)"][i0] == math.inf
    assert got["max(ival)"][i1] == I64_MIN and got["unique(uq)"][i1] == I64_MIN and got["min(fval)"][i1] == -math.inf
    assert got["sum(ival)"][i2] == 2**63 + 8 - 2**64 and got["sum(fval)"][i2] == 4 * SUB_MIN  # a wrap; subnormals kept by the float SUM


def test_subnormal_float_sums_are_not_flushed(pp, monkeypatch):
    """Float64 SUM over subnormals only, one group per path (dense table, hash table, interpreting kernel, exact sums): while every
    partial sum stays subnormal each addition is exact, so every path must give fsum's answer bit for bit, whatever the order — a float
    atomic that flushed subnormals to zero would not."""
    rng = np.random.default_rng(3)
    n = 50_000
    vals = (rng.integers(-(2**36), 2**36, size=n) * SUB_MIN).tolist()  # |any partial sum| < 50 000 · 2^36 · 2^-1074 < DBL_MIN
    key = rng.integers(0, 8, size=n)
    rec = pa.RecordBatch.from_arrays([pa.DictionaryArray.from_arrays(pa.array(key.astype(np.uint32)), pa.array(key_names(8), type=pa.binary())),
                                      pa.array(key.astype(np.int64) * 1_000_003), pa.array(vals, type=pa.float64())], names=["labels.k", "ikey", "fval"])
    want = {}
    for k, v in zip(key.tolist(), vals):
        want.setdefault(k, []).append(v)
    want = {k: math.fsum(v) for k, v in want.items()}
    assert all(0 < abs(w) < DBL_MIN for w in want.values())
    for path, groups, env, exact in (("dense", [Col("labels.k")], None, False), ("hash", [Col("ikey")], None, False),
                                     ("interpreted", [Col("labels.k")], "FDB_NO_JIT", False), ("exact", [Col("ikey")], None, True)):
        if env:
            monkeypatch.setenv(env, "1")
        else:
            monkeypatch.delenv("FDB_NO_JIT", raising=False)
        for resident in (False, True):
            plan = make_plan(pp, None, [Sum(Col("fval"))], groups, exact)
            keep = []
            try:
                push(pp, plan, [rec.slice(0, 20_000), rec.slice(20_000)], resident, keep)
                got = arrow_to_pydict(plan.Finish())
            finally:
                plan.Close()
                for x in keep:
                    x.close()
            kcol = got[groups[0].name]
            for kv, s in zip(kcol, got["sum(fval)"]):
                k = int(kv[1:]) if isinstance(kv, bytes) else kv // 1_000_003
                assert bits(s) == bits(want[k]), (path, resident, k, s, want[k])


# ---- contract refusals -----------------------------------------------------------------------------------------------------------

def test_refusals_at_the_edges(pp, fcomm):
    """Combinations the contract refuses are refused, by the device path and the oracle alike: a uint64 column against a negative
    int64 literal, and a dynamic aggregation through the exchange."""
    from oracle import OraclePlan
    rng = np.random.default_rng(9)
    rec = edge_record(rng, 1000, 16, False)
    filt = Col("ukey") > -1
    plan = pp.HashAggregatePlan(filt, [Count(Col("ival"))], [Col("labels.k")])
    try:
        with pytest.raises(pp.FdbError):
            plan.Callback(rec)
            plan.Finish()
    finally:
        plan.Close()
    o = OraclePlan(filt, [Count(Col("ival"))], [Col("labels.k")])
    try:
        with pytest.raises(Exception):
            o.push(rec)
            o.finish()
    finally:
        o.close()
    comms = fcomm.Comm.init_local([0, 0])
    errs = []

    dyn = rec.append_column("dv.a", rec.column("ival")).append_column("dv.b", rec.column("ival"))

    def rank_fn(r):
        plan = pp.HashAggregatePlan(None, [Sum(DynCol("dv"))], [Col("labels.k")])
        try:
            plan.Callback(dyn)
            try:
                comms[r].merge_alltoall(plan).Close()
            except pp.FdbError as e:
                errs.append(e.code)
        finally:
            plan.Close()

    try:
        run_ranks(2, rank_fn)
    finally:
        for c in comms:
            c.close()
    assert errs == [pp.FDB_ERR_UNSUPPORTED] * 2, errs


# ---- the numeric-leaf matrix -----------------------------------------------------------------------------------------------------

OPS = [(OP_EQ, "=="), (OP_NOT_EQ, "!="), (OP_LT, "<"), (OP_LT_EQ, "<="), (OP_GT, ">"), (OP_GT_EQ, ">=")]
LEAF_LITERALS = {
    "i64": ("i", [I64_MIN, I64_MAX, 2**53 + 1, -(2**53 + 1), 0, -1]),
    "i64_vs_f64": ("i", [2.0**63, -(2.0**63), math.inf, -math.inf, math.nan, -0.0, float(2**53 + 1)]),
    "u64": ("u", [UInt64(2**63), UInt64(2**64 - 1), UInt64(0), 2**63 - 1]),
    "f64": ("f", [2.0**63, -(2.0**63), math.inf, -math.inf, math.nan, -0.0, SUB_MIN, -DBL_MIN, I64_MAX]),
    "bool": ("b", [True, False]),
}


def leaf_record(rng, n, nulls):
    """One record holding every edge pool: `i` int64, `u` uint64, `f` float64, `b` bool (with validity bitmaps when `nulls`), a small
    dictionary key (dense table) and a high-cardinality int64 key (hash table)."""
    i = rng.choice(np.array(I64_EDGES + [2, -2, 2**53 - 1, 2**62], dtype=object), size=n).tolist()
    u = rng.choice(np.array(U64_EDGES, dtype=object), size=n).tolist()
    f = rng.choice(np.array(F64_EDGES + [float(2**53 + 1), 2.0**63, -(2.0**63), 1.5], dtype=object), size=n).tolist()
    b = (rng.random(n) < 0.5).tolist()
    m = (lambda: rng.random(n) < 0.1) if nulls else (lambda: None)
    small = rng.integers(0, 6, size=n).astype(np.uint32)
    wide = rng.integers(0, 20_000, size=n).astype(np.int64) * 7919 + 1
    return pa.RecordBatch.from_arrays(
        [pa.array(i, type=pa.int64(), mask=m()), pa.array(u, type=pa.uint64(), mask=m()), pa.array(f, type=pa.float64(), mask=m()),
         pa.array(b, type=pa.bool_(), mask=m()),
         pa.DictionaryArray.from_arrays(pa.array(small), pa.array([b"s%d" % k for k in range(6)], type=pa.binary())),
         pa.array(wide)],
        names=["i", "u", "f", "b", "labels.s", "hk"])


def same_rows(got, want):
    """Two records hold the same rows (dictionaries decoded; floats bit for bit, so NaN rows count)."""
    assert got.num_rows == want.num_rows and got.schema.names == want.schema.names, (got.num_rows, want.num_rows)
    for name, g, w in zip(want.schema.names, got.columns, want.columns):
        if pa.types.is_floating(w.type):
            gv, wv = np.asarray(g.is_valid()), np.asarray(w.is_valid())
            assert (gv == wv).all(), name
            gb, wb = np.asarray(g.fill_null(0.0)).view(np.uint64), np.asarray(w.fill_null(0.0)).view(np.uint64)
            assert (gb[gv] == wb[wv]).all(), name
        else:
            assert arrow_to_pydict(pa.RecordBatch.from_arrays([g], names=[name])) == arrow_to_pydict(pa.RecordBatch.from_arrays([w], names=[name])), name
    return True


def group_counts(rec, sel, key):
    c = rec.column(key)
    keys = (c.dictionary_decode() if pa.types.is_dictionary(c.type) else c).to_pylist()
    out = {}
    for r in np.flatnonzero(sel):
        out[keys[r]] = out.get(keys[r], 0) + 1
    return out


@pytest.mark.parametrize("nulls", [False, True], ids=["no_validity", "validity"])
@pytest.mark.parametrize("kind", list(LEAF_LITERALS))
def test_numeric_leaf_matrix_on_every_filter_path(pp, kind, nulls, monkeypatch):
    """Every numeric leaf kind × every operator × edge literals, through the aggregate scan (generated fdb_plan_kernel and the
    interpreting scan_slots_kernel), the hash scan, Select, Filter and FilterResident (one-pass, three-launch and the stall fallback):
    the selected rows equal the oracle's and numpy's, row for row."""
    for v in ("FDB_NO_JIT", "FDB_SELECT_ONE_PASS", "FDB_SELECT_TWO_PASS", "FDB_TEST_SELECT_STALL"):
        monkeypatch.delenv(v, raising=False)
    rng = np.random.default_rng(list(LEAF_LITERALS).index(kind) * 2 + nulls)
    rec = leaf_record(np.random.default_rng(11 + nulls), 4099, nulls)
    col, lits = LEAF_LITERALS[kind]
    rb = pp.ResidentBatch(rec)
    try:
        for lit in lits:
            for op, sym in OPS:
                filt = BinaryExpr(Col(col), op, Literal(lit))
                ctx = (kind, sym, lit, nulls)
                sel = np_select(filt, rec)
                want_idx = np.flatnonzero(sel)
                assert list(oracle_select(filt, rec)) == list(want_idx), ("oracle", ctx)
                # aggregate scans: generated, interpreting, hash
                for tuning, kernel, key in ((0, "fdb_plan_kernel", "labels.s"), (4 << 25, "scan_slots_kernel", "labels.s"), (0, "fdb_hash_kernel", "hk")):
                    plan = pp.HashAggregatePlan(filt, [Count(Col("f"))], [Col(key)])
                    if tuning:
                        plan.set_tuning(0, tuning)
                    try:
                        if rng.random() < 0.5:
                            plan.Callback(rec)
                        else:
                            plan.CallbackResident([rb])
                        assert plan.last_kernel().startswith(kernel), (ctx, plan.last_kernel())
                        got = arrow_to_pydict(plan.Finish())
                    finally:
                        plan.Close()
                    assert dict(zip(got.get(key, []), got.get("count(f)", []))) == group_counts(rec, sel, key), (ctx, kernel)
                plan = pp.HashAggregatePlan(filt)
                try:
                    assert list(plan.Select(rec)) == list(want_idx), ("Select", ctx)
                    out = plan.Filter(rec)
                    if len(want_idx) == 0:
                        assert out is None, ("Filter", ctx)
                    else:
                        assert same_rows(out, rec.take(pa.array(want_idx))), ("Filter", ctx)
                finally:
                    plan.Close()
                for path, env in (("one_pass", "FDB_SELECT_ONE_PASS"), ("three_launch", "FDB_SELECT_TWO_PASS"), ("stall", "FDB_TEST_SELECT_STALL")):
                    monkeypatch.setenv(env, "1")
                    if path == "stall":
                        monkeypatch.setenv("FDB_SELECT_ONE_PASS", "1")
                    plan = pp.HashAggregatePlan(filt)
                    try:
                        out = plan.FilterResident(rb)
                        lk = plan.last_kernel()
                        try:
                            got = out.to_arrow()
                        finally:
                            out.close()
                    finally:
                        plan.Close()
                        for e in ("FDB_SELECT_ONE_PASS", "FDB_SELECT_TWO_PASS", "FDB_TEST_SELECT_STALL"):
                            monkeypatch.delenv(e, raising=False)
                    if path == "one_pass" and not nulls:
                        assert "fdb_select_kernel" in lk, (ctx, lk)
                    elif path != "one_pass":
                        assert "fdb_select_kernel" not in lk, (ctx, path, lk)
                    assert got.num_rows == len(want_idx), (path, ctx, got.num_rows, len(want_idx))
                    assert same_rows(got, rec.take(pa.array(want_idx))), (path, ctx)
    finally:
        rb.close()
