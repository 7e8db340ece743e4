"""Exact float64 sums (fdb_plan_set_exact_sums) across ranks: the exchange of fdb_plan_exchange carries every group's limb row from the
exporting rank to the owner, so the union of the shards' SUM(float64) is the correctly rounded exact sum — checked BIT FOR BIT against
float(sum(Fraction(v))) and against one exact plan over all rows — on 2, 3 or 8 ranks, for any split of the rows and any rank order.

The ranks are threads of the in-process transport (fdb_comm_init_local, all on device 0); the RCCL transport runs through the
test-only librccl stand-in in a child process, as in tests/test_gpu_fake_rccl.py."""
import json
import math
import os
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pyarrow as pa
import pytest

from frostdb_amd.logicalplan import Col, Count, Max, Min, Sum
from tests.test_gpu_comm import run_ranks
from tests.test_gpu_exact_sums import assert_exact, exact_reference, f64_bits, make_records, result_sums, run_plan, values, wild_values

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def pp():
    from frostdb_amd import physicalplan
    assert physicalplan.device_count() >= 1, "no HIP device visible"
    yield physicalplan
    assert physicalplan.live_allocations()["device_blocks"] == 0


@pytest.fixture(scope="module")
def fcomm():
    from frostdb_amd import comm
    return comm


@pytest.fixture(params=["jit", "nojit"])
def jit_mode(request, monkeypatch):
    if request.param == "nojit":
        monkeypatch.setenv("FDB_NO_JIT", "1")
    return request.param


def exchange(pp, fcomm, shards, aggs, groups, exact=True):
    """Every rank pushes its records into a plan and exchanges it; returns each rank's shard Finish(). `exact`: a bool, or one per rank."""
    world = len(shards)
    flags = exact if isinstance(exact, (list, tuple)) else [exact] * world
    comms = fcomm.Comm.init_local([0] * world)

    def rank_fn(r):
        plan = pp.HashAggregatePlan(None, aggs, groups)
        if flags[r]:
            plan.set_exact_sums(True)
        try:
            for rec in shards[r]:
                plan.Callback(rec)
            shard = comms[r].merge_alltoall(plan)
            try:
                return shard.Finish()
            finally:
                shard.Close()
        finally:
            plan.Close()

    try:
        return run_ranks(world, rank_fn)
    finally:
        for c in comms:
            c.close()


def union(outs, n_keys, agg_index=0):
    """{key tuple: value} over the shards; a group lives on exactly one shard."""
    got = {}
    for out in outs:
        part = result_sums(out, n_keys, agg_index)
        assert not (set(part) & set(got)), "a group on two shards"
        got.update(part)
    return got


def split(rng, rec, world, empty_rank=None):
    """The rows of `rec` in a random order, cut at random points into `world` shares (one or two records each); `empty_rank` gets none."""
    perm = rng.permutation(rec.num_rows)
    shuffled = rec.take(pa.array(perm))
    takers = [r for r in range(world) if r != empty_rank]
    cuts = sorted(rng.choice(np.arange(1, rec.num_rows), len(takers) - 1, replace=False).tolist())
    bounds = [0] + cuts + [rec.num_rows]
    shards = [[] for _ in range(world)]
    for r, a, b in zip(takers, bounds, bounds[1:]):
        mid = int(rng.integers(a, b + 1))
        shards[r] = [s for s in (shuffled.slice(a, mid - a), shuffled.slice(mid, b - mid)) if s.num_rows > 0]
    return shards


SHAPES = {
    "path": ["labels.path"],
    "cfg5_32_columns": ["labels.l%02d" % c for c in range(32)],
    "int64_time_bucket": ["timestamp"],
    "no_groups": [],
}
_REFS = {}


def shape_data(shape):
    if shape not in _REFS:
        rng = np.random.default_rng(100 + len(shape))
        recs = make_records(rng, 12_000, n_records=3, n_label_cols=32 if shape == "cfg5_32_columns" else 2)
        rec = pa.Table.from_batches(recs).combine_chunks().to_batches()[0]
        _REFS[shape] = (rec, exact_reference([rec], SHAPES[shape], values))
    return _REFS[shape]


@pytest.mark.parametrize("world", [2, 3, 8])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_exchanged_exact_sums_match_the_rational_reference_bit_for_bit(pp, fcomm, jit_mode, shape, world):
    rec, want = shape_data(shape)
    keys = SHAPES[shape]
    groups = [Col(k) for k in keys]
    aggs = [Sum(Col("value"))]
    rng = np.random.default_rng(world * 31 + len(shape))
    shards = split(rng, rec, world, empty_rank=world - 1)
    got = union(exchange(pp, fcomm, shards, aggs, groups), len(keys))
    assert_exact(got, want)
    single, _ = run_plan(pp, [rec], aggs, groups)
    assert {k: f64_bits(v) for k, v in got.items()} == {k: f64_bits(v) for k, v in result_sums(single, len(keys)).items()}


def test_split_and_rank_order_do_not_change_the_bits(pp, fcomm):
    rec, want = shape_data("path")
    groups, aggs = [Col("labels.path")], [Sum(Col("value"))]
    seen = []
    for seed, order in ((1, [0, 1, 2, 3]), (2, [3, 1, 0, 2]), (3, [2, 3, 1, 0])):
        shards = split(np.random.default_rng(seed), rec, 4, empty_rank=1 if seed == 3 else None)
        got = union(exchange(pp, fcomm, [shards[o] for o in order], aggs, groups), 1)
        assert_exact(got, want)
        seen.append({k: f64_bits(v) for k, v in got.items()})
    assert all(s == seen[0] for s in seen)


def test_carries_across_rank_imports(pp, fcomm, monkeypatch):
    """Digits close to 2^32 in every limb a value reaches, 8 ranks that all hold every group, and a normalize threshold (1 024 rows)
    that the owner's rank-by-rank imports pass several times: the limbs are carried between imports, the sums stay exact."""
    monkeypatch.setenv("FDB_TEST_EXACT_NORMALIZE_ROWS", "1024")
    world, n_groups, per_group = 8, 4096, 3
    x0 = float((2**53 - 1) * 2**(31 - 1074 + 32 * 10))
    x1 = -float((2**53 - 1) * 2**(30 - 1074 + 32 * 20))
    k = np.tile(np.arange(n_groups, dtype=np.int64), per_group)
    v = np.where(k % 2 == 0, x0, x1)
    rec = pa.RecordBatch.from_arrays([pa.array(k), pa.array(v)], names=["k", "value"])
    got = union(exchange(pp, fcomm, [[rec]] * world, [Sum(Col("value"))], [Col("k")]), 1)
    n = world * per_group
    want = {(g,): float(Fraction(x0 if g % 2 == 0 else x1) * n) for g in range(n_groups)}
    assert {k: f64_bits(v) for k, v in got.items()} == {k: f64_bits(v) for k, v in want.items()}


def test_non_finite_values_travel(pp, fcomm):
    inf, nan = float("inf"), float("nan")
    # group: values per rank (rank 0, 1, 2)
    rows = {
        0: ([nan, 1.0], [2.0], [3.0]),       # NaN on one rank
        1: ([1.0], [inf], [-inf, 5.0]),      # +inf and -inf on different ranks
        2: ([1e300], [inf], [-1e300]),       # +inf on one rank only
        3: ([-inf], [], [1.0]),              # -inf on one rank only
        4: ([1e308], [1e308], [-1e308]),     # finite, past DBL_MAX on the way
    }
    shards = []
    for r in range(3):
        ks = [g for g, per in rows.items() for _ in per[r]]
        vs = [x for per in rows.values() for x in per[r]]
        shards.append([pa.RecordBatch.from_arrays([pa.array(ks, type=pa.int64()), pa.array(vs, type=pa.float64())], names=["k", "value"])])
    got = union(exchange(pp, fcomm, shards, [Sum(Col("value"))], [Col("k")]), 1)
    assert set(got) == {(g,) for g in rows}
    assert math.isnan(got[(0,)]) and math.isnan(got[(1,)])
    assert got[(2,)] == inf and got[(3,)] == -inf
    assert f64_bits(got[(4,)]) == f64_bits(1e308)


def test_mixed_aggregations(pp, fcomm):
    """SUM(int64), SUM(float64), COUNT, MIN, MAX (AVG = SUM + COUNT) in one exact plan: every column but the float64 SUM equals the plain
    exchange's; the float64 SUM is exact."""
    rng = np.random.default_rng(7)
    recs = make_records(rng, 15_000, n_records=2, extra=lambda rng, n: {"ivalue": pa.array(rng.integers(-2**40, 2**40, n))})
    rec = pa.Table.from_batches(recs).combine_chunks().to_batches()[0]
    keys = ["labels.path", "timestamp"]
    groups = [Col(k) for k in keys]
    aggs = [Sum(Col("ivalue")), Sum(Col("value")), Count(Col("value")), Min(Col("value")), Max(Col("value"))]
    shards = split(np.random.default_rng(8), rec, 3)
    exact_outs = exchange(pp, fcomm, shards, aggs, groups, exact=True)
    plain_outs = exchange(pp, fcomm, shards, aggs, groups, exact=False)
    assert_exact(union(exact_outs, 2, 1), exact_reference([rec], keys, values))
    for j in (0, 2, 3, 4):
        e, p = union(exact_outs, 2, j), union(plain_outs, 2, j)
        assert set(e) == set(p)
        assert {k: f64_bits(v) if isinstance(v, float) else v for k, v in e.items()} == {k: f64_bits(v) if isinstance(v, float) else v for k, v in p.items()}, j


def test_allreduce_declines_and_merge_takes_the_exchange(pp, fcomm):
    """An exact plan lives in the hash table: Comm.allreduce() answers False and leaves the plan as it was (its Finish is the exact sum
    of its own rows); Comm.merge() falls through to the exchange and returns the exact shards."""
    rec, want = shape_data("path")
    groups, aggs = [Col("labels.path")], [Sum(Col("value"))]
    world = 3
    shards = split(np.random.default_rng(9), rec, world)
    comms = fcomm.Comm.init_local([0] * world)

    def plan_of(r):
        plan = pp.HashAggregatePlan(None, aggs, groups)
        plan.set_exact_sums(True)
        for s in shards[r]:
            plan.Callback(s)
        return plan

    def rank_fn(r):
        plan = plan_of(r)
        try:
            assert comms[r].allreduce(plan) is False
            own = result_sums(plan.Finish(), 1)
        finally:
            plan.Close()
        plan = plan_of(r)
        try:
            return own, comms[r].merge(plan)
        finally:
            plan.Close()

    try:
        outs = run_ranks(world, rank_fn)
    finally:
        for c in comms:
            c.close()
    for r, (own, _) in enumerate(outs):
        assert_exact(own, exact_reference(shards[r], ["labels.path"], values))
    assert_exact(union([o for _, o in outs], 1), want)


def test_ranks_that_disagree_on_exact_sums_all_fail(pp, fcomm):
    rec, _ = shape_data("path")
    world = 3
    shards = split(np.random.default_rng(10), rec, world)
    comms = fcomm.Comm.init_local([0] * world)
    errors = [None] * world

    def rank_fn(r):
        plan = pp.HashAggregatePlan(None, [Sum(Col("value"))], [Col("labels.path")])
        if r == 0:
            plan.set_exact_sums(True)
        try:
            for s in shards[r]:
                plan.Callback(s)
            try:
                comms[r].merge_alltoall(plan).Close()
            except pp.FdbError as e:
                errors[r] = e
        finally:
            plan.Close()

    try:
        run_ranks(world, rank_fn)  # (asserts that no rank is left in a collective)
    finally:
        for c in comms:
            c.close()
    assert all(e is not None and e.code == pp.FDB_ERR_INVALID for e in errors), errors
    assert "exact sums" in str(errors[0])


RCCL_CHILD = r'''
import json, sys
from fractions import Fraction
import numpy as np
import pyarrow as pa
sys.path.insert(0, %(root)r)
from frostdb_amd import physicalplan as pp, comm as fcomm
from frostdb_amd.logicalplan import Col, Sum
from tests.test_gpu_comm import run_ranks
from tests.test_gpu_exact_sums import f64_bits, wild_values

world, n_groups = int(sys.argv[1]), int(sys.argv[2])
rng = np.random.default_rng(2024)
keys = np.concatenate([rng.permutation(n_groups), rng.integers(0, n_groups, n_groups // 4)]).astype(np.int64)
v, mask = wild_values(rng, len(keys))
cuts = np.sort(rng.choice(np.arange(1, len(keys)), world - 1, replace=False))
bounds = [0] + cuts.tolist() + [len(keys)]
shards = [pa.RecordBatch.from_arrays([pa.array(keys[a:b]), pa.array(v[a:b], mask=mask[a:b])], names=["k", "value"]) for a, b in zip(bounds, bounds[1:])]
comms = fcomm.Comm.init_all([0] * world)
def rank_fn(r):
    plan = pp.HashAggregatePlan(None, [Sum(Col("value"))], [Col("k")])
    plan.set_exact_sums(True)
    try:
        plan.Callback(shards[r])
        shard = comms[r].merge_alltoall(plan)
        try:
            out = shard.Finish()
            return dict(zip(out.column(0).to_pylist(), out.column(1).to_pylist()))
        finally:
            shard.Close()
    finally:
        plan.Close()
parts = run_ranks(world, rank_fn)
for c in comms: c.close()
want = {}
for k, x, m in zip(keys.tolist(), v.tolist(), mask.tolist()):
    want[k] = want.get(k, Fraction(0)) + (0 if m else Fraction(x))
got = {}
for p in parts:
    assert not (set(p) & set(got))
    got.update(p)
assert set(got) == set(want), (len(got), len(want))
bad = [k for k in want if f64_bits(got[k]) != f64_bits(float(want[k]) + 0.0)]
print("REPORT " + json.dumps({"groups": len(got), "bad": len(bad), "shard_groups": [len(p) for p in parts]}))
'''


@pytest.mark.timeout(600)
def test_rccl_transport_exchanges_exact_sums_across_slices():
    """4 ranks of the RCCL transport (the librccl stand-in), 240 000 exact groups, slices of 1 MiB: each rank's rows for one peer
    (~60 000 rows of ~300 bytes) cross several slices."""
    sys.path.insert(0, os.path.join(ROOT, "tests", "fake_rccl"))
    import importlib
    fake = importlib.import_module("build").build()
    env = dict(os.environ)
    env.update({"FDB_RCCL_LIB": fake, "FDB_EXCHANGE_SLICE_BYTES": str(1 << 20), "PYTHONPATH": ROOT + os.pathsep + env.get("PYTHONPATH", ""),
                "HSA_ENABLE_IPC_MODE_LEGACY": "0"})
    p = subprocess.run([sys.executable, "-c", RCCL_CHILD % {"root": ROOT}, "4", "240000"], capture_output=True, text=True, timeout=550, env=env, cwd=ROOT)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("REPORT ")]
    assert p.returncode == 0 and lines, p.stderr[-3000:]
    rep = json.loads(lines[-1][7:])
    assert rep["groups"] == 240_000 and rep["bad"] == 0, rep
    assert all(n > 0 for n in rep["shard_groups"]), rep
