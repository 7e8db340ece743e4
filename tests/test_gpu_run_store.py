"""The table-free OrderedAggregate at its stage, chunk and segment edges: every case of tests/run_store_cases.py — each one claims there
which events of a wave's (rb, rp, ps) state, which run record and how many runs it makes, and tests/test_run_store_cases_cpu.py holds the
families to covering all of them — through ONE ordered plan of the Python binding (HashAggregatePlan(ordered=True): Callback per host
record or CallbackResident of a list, Merge for the translate family, Finish), once per reducer and per grid: set_tuning(8, 1) and (8, 2)
force one and two workgroups, so that a wave walks dozens of tiles, carries its stage across them, fills it and changes chunks; 0 is the
default grid, where a wave sees one tile.

Every expected value is the numpy group-by of run_store_cases.py (`reference`), compared row for row IN ORDER on key ranks and values:
counts, int64 SUM / MIN / MAX, float MIN / MAX and float sums of integer-valued (or otherwise exactly summable) data exactly (with ==:
−0.0 and +0.0 are one value), the one family of general floats within (n − 1) · 2^-53 · Σ|v| of math.fsum per group — the
bound of a sum in any order. After every push the kernel's name is the one the case's run record claims; after Finish the sorted Finish's
kernels are named exactly when the keys did not arrive in order.

The module prints how many kernels it compiled: the families share shapes (row counts, run layouts and grids are not part of one)."""
import gc
import time

import numpy as np
import pyarrow as pa
import pytest

from frostdb_amd.logicalplan import Col
from tests import run_store_cases as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pp():
    from frostdb_amd import physicalplan
    assert physicalplan.device_count() >= 1, "no HIP device visible"
    return physicalplan


@pytest.fixture(autouse=True)
def _runs_on_small_shapes(monkeypatch):
    """Ordered plans over small key spaces keep the dense table (Plan::runs_wanted); these tests are about the run store."""
    monkeypatch.setenv("FDB_RUNS_ALWAYS", "1")


@pytest.fixture(scope="module", autouse=True)
def compile_cost(pp):
    before, t0 = pp.jit_stats(), time.time()
    yield
    after = pp.jit_stats()
    print("\n[test_gpu_run_store] kernels compiled: %d (%.1f s of hiprtc), loaded from the disk cache: %d, module wall time %.1f s"
          % (after["compiled"] - before["compiled"], (after["compile_ms"] - before["compile_ms"]) / 1e3, after["disk_loads"] - before["disk_loads"], time.time() - t0))


def push_all(pp, plan, c, records, pushes, formats, keep):
    for how, what in pushes:
        idx = [what] if how == "host" else list(what)
        if how == "host":
            plan.Callback(records[what])
        else:
            rbs = [pp.ResidentBatch(records[i]) for i in idx]
            keep.extend(rbs)
            plan.CallbackResident(rbs)
        live = [i for i in idx if records[i].num_rows > 0]
        if not live:
            continue
        fmt = formats[live[-1]]
        if fmt is not None:
            assert plan.last_kernel() == R.KERNEL[fmt], (c.id, how, what, plan.last_kernel())
        else:  # the run store was left (or never entered): no run kernel scanned this record
            assert "runs" not in plan.last_kernel(), (c.id, how, what, plan.last_kernel())


def run(pp, c, agg, grid):
    """→ (result record, last_kernel() after Finish)"""
    groups = [Col(n) for n in c.names]
    plans, keep = [], []
    try:
        plan = pp.HashAggregatePlan(c.filter_expr(), [R.AGGS[agg]], groups, ordered=True, final_stage=False)
        plans.append(plan)
        if grid:
            plan.set_tuning(8, grid)
        push_all(pp, plan, c, c.records, c.pushes, c.formats, keep)
        if c.source:
            src = pp.HashAggregatePlan(c.filter_expr(), [R.AGGS[agg]], groups, ordered=True, final_stage=False)
            plans.append(src)
            sc = R.Case("source", c.family, c.source)
            push_all(pp, src, sc, sc.records, sc.pushes, sc.formats, keep)
            plan.Merge(src)
            assert plan.last_kernel() == R.TRANSLATE, (c.id, plan.last_kernel())
        out = plan.Finish()
        return out, plan.last_kernel()
    finally:
        for p in plans:
            p.Close()
        for k in keep:
            k.close()


def key_ranks_of(out, name, shown):
    """The result's column as ranks among the reference's values of that column (NULL = the largest), from indices and dictionary"""
    a = out.column(out.schema.get_field_index(name))
    rank = {v: r for r, v in enumerate(shown[:-1])}
    if not pa.types.is_dictionary(a.type):
        a = a.dictionary_encode()
    lut = np.array([rank.get(v, -1) for v in a.dictionary.to_pylist()] + [len(shown) - 1], np.int64)
    return lut[a.indices.fill_null(len(lut) - 1).to_numpy(zero_copy_only=False).astype(np.int64)]


def check(c, agg, grid, out, after):
    what = (c.id, agg, "grid %d" % grid)
    keys, shown, acc = c.want(agg)
    col = "f" if agg in ("sum_f", "max") else "v"
    assert out.schema.names == c.names + [col], (what, out.schema.names)  # (a partial-stage OrderedAggregate names its result after the column)
    assert out.num_rows == len(acc), (what, out.num_rows, len(acc))
    if not c.leaves_the_path:
        assert (after == R.SORTED_FINISH) == (not c.in_order), (what, after)
    for n, k, s in zip(c.names, keys, shown):
        got = key_ranks_of(out, n, s)
        bad = np.flatnonzero(got != k)
        assert len(bad) == 0, (what, n, "first wrong row", int(bad[0]), "of", len(k), "got rank", int(got[bad[0]]), "want", int(k[bad[0]]), "wrong rows", len(bad))
    a = out.column(out.num_columns - 1)
    assert a.null_count == 0 and a.type == (pa.float64() if col == "f" and agg != "count" else pa.int64()), (what, a.type, a.null_count)
    got = a.to_numpy(zero_copy_only=False)
    if c.fsum and agg == "sum_f":
        bound = R.fsum_bounds(c.records, c.names, c.filt)
        err = np.abs(got - acc)
        print("\n[%s] float sums against fsum: largest error / bound = %.3g over %d groups" % (c.id, float(np.max(err / np.maximum(bound, 1e-300))), len(acc)))
        bad = np.flatnonzero(~(err <= bound))
    else:
        bad = np.flatnonzero(~(got == acc))
    assert len(bad) == 0, (what, "first wrong row", int(bad[0]), "of", len(acc), "got", got[bad[0]], "want", acc[bad[0]], "wrong rows", len(bad))


def run_family(pp, monkeypatch, c):
    if c.force:
        monkeypatch.setenv("FDB_RUNS_WIDE", c.force)
    for grid in c.grids:
        for agg in c.aggs:
            out, after = run(pp, c, agg, grid)
            check(c, agg, grid, out, after)


def ids(family):
    return [c.id for c in R.cases(family)]


@pytest.mark.parametrize("c", R.cases("per_tile_k"), ids=ids("per_tile_k"))
def test_per_tile_k(pp, monkeypatch, c):
    """Every wave tile ends exactly k runs: stages that fill on a known tile, chunks that are exactly full, abandoned with slots to spare,
    changed with runs pending; every second wave edge cuts a group in two."""
    run_family(pp, monkeypatch, c)


@pytest.mark.parametrize("c", R.cases("edges"), ids=ids("edges"))
def test_edges(pp, monkeypatch, c):
    run_family(pp, monkeypatch, c)


@pytest.mark.parametrize("c", R.cases("filter"), ids=ids("filter"))
def test_filter(pp, monkeypatch, c):
    """v > 0 with the dropped rows placed: the wave's writer lane and flush stride follow the lanes that are still in the tile"""
    run_family(pp, monkeypatch, c)


@pytest.mark.parametrize("c", R.cases("formats"), ids=ids("formats"))
def test_formats(pp, monkeypatch, c):
    run_family(pp, monkeypatch, c)


@pytest.mark.parametrize("c", R.cases("segments"), ids=ids("segments"))
def test_segments(pp, monkeypatch, c):
    """64 segments stay table-free, the 65th push leaves the path mid-scan (no assertion on Finish's kernels there): the same rows either way"""
    run_family(pp, monkeypatch, c)


@pytest.mark.parametrize("c", R.cases("extremes"), ids=ids("extremes"))
def test_extremes(pp, monkeypatch, c):
    run_family(pp, monkeypatch, c)


@pytest.mark.parametrize("c", R.cases("run_counts"), ids=ids("run_counts"))
def test_run_counts(pp, monkeypatch, c):
    run_family(pp, monkeypatch, c)


@pytest.mark.parametrize("c", R.cases("violation"), ids=ids("violation"))
def test_violation(pp, monkeypatch, c):
    """Exactly one pair out of order: the sorted Finish ran and the rows are the reference's; in order: its kernels are not named"""
    run_family(pp, monkeypatch, c)


@pytest.mark.parametrize("c", R.cases("translate"), ids=ids("translate"))
def test_translate(pp, monkeypatch, c):
    run_family(pp, monkeypatch, c)


def test_many_runs(pp, monkeypatch):
    """2^20 + 1 runs: more than 1 024 blocks of 1 024 in the scans of run counts and group flags (scan_u64_single_kernel's second round, with
    its carry). Compared on indices and dictionaries. Kept at its full size: the claim does not hold below it."""
    c, = R.cases("many_runs")
    run_family(pp, monkeypatch, c)


def test_the_grids_are_the_ones_the_claims_assume(pp, monkeypatch, capfd):
    """set_tuning(8, 1) and (8, 2) launch the run kernel with one and two workgroups, and the default grid has at least the workgroups up
    to which run_store_cases.py takes it for "one per tile" — read from the launch line $FDB_JIT_DEBUG prints (fdb_hash.cpp, push_hash)."""
    import re
    monkeypatch.setenv("FDB_JIT_DEBUG", "1")
    c = R.cases("per_tile_k")[0]
    seen = {}
    for grid in (1, 2, 0):
        capfd.readouterr()
        run(pp, c, "sum_i", grid)
        m = re.findall(r"hash kernel \(runs\): (\d+) workgroups", capfd.readouterr().err)
        assert len(m) == 1, (grid, m)
        seen[grid] = int(m[0])
    assert seen[1] == 1 and seen[2] == 2 and seen[0] >= R.DEFAULT_GRID_AT_LEAST, seen


def test_the_segment_limit_gives_the_same_rows_on_both_sides(pp):
    """(what the two segments tests compare against is each case's own reference; the 64 and 65 record cuts of one generator differ in seed,
    so here one case is pushed whole, as 64 records and as 65 records)"""
    c = R.cases("segments")[0]
    whole = pa.Table.from_batches(c.records).combine_chunks().to_batches()[0]
    want = c.want("sum_i")
    for n in (64, 65):
        cuts = np.linspace(0, whole.num_rows, n + 1).astype(int)[1:-1]
        cc = R.Case("segments-whole_in_%d" % n, "segments", R.cut(whole, cuts), aggs=("sum_i",))
        assert cc.leaves_the_path == (n == 65)
        out, after = run(pp, cc, "sum_i", 0)
        check(cc, "sum_i", 0, out, after)
        assert np.array_equal(cc.want("sum_i")[2], want[2])


def test_nothing_is_left_on_the_device(pp):
    gc.collect()
    assert all(v == 0 for v in pp.live_allocations().values()), pp.live_allocations()
