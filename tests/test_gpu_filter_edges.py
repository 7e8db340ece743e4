"""filter() on resident records over constructed selection and NULL patterns (tests/filter_cases.py), on every route:

  one_pass        fdb_select_kernel + compact_multi_kernel — the default for `sel > 0`; `selk == "y"` and `seln > 0` under FDB_SELECT_ONE_PASS
  two_pass        fdb_flags_kernel + compact_multi_kernel under FDB_SELECT_TWO_PASS (and by default for `seln > 0`, which cannot be fused)
  interp          the interpreting flags kernel + compact_col_kernel per column under FDB_NO_JIT
  select          the selection vector of SelectResident against numpy.flatnonzero
  … with set_tuning(grid_blocks=1) and (=3): one worker walks every share / the look-back crosses workers at every share.

The whole (rows x selection pattern) grid is packed as the records of ONE FilterResidentMany call per route and validity pattern.
The reference is pyarrow's RecordBatch.filter with the mask the case was built from: row count, row order, positions of NULLs,
null_count and the values at valid positions, per column (a value under a NULL is unspecified). One record per route is also put
through the oracle's filter(), so the two references are seen to agree."""
import gc

import numpy as np
import pyarrow as pa
import pytest

from frostdb_amd import physicalplan as pp
from frostdb_amd.logicalplan import Col

from tests import filter_cases as fc
from tests.util import arrow_to_pydict

pytestmark = pytest.mark.gpu

SELECT_MULTI = "fdb_select_kernel + compact_multi_kernel"
FLAGS_MULTI = "fdb_flags_kernel + compact_multi_kernel"
# route → (predicate column, environment, kernel, grid_blocks)
ROUTES = {
    "one_pass": ("sel", {}, SELECT_MULTI, 0),
    "one_pass_selk": ("selk", {"FDB_SELECT_ONE_PASS": "1"}, SELECT_MULTI, 0),
    "one_pass_seln": ("seln", {"FDB_SELECT_ONE_PASS": "1"}, SELECT_MULTI, 0),
    "one_pass_grid1": ("sel", {}, SELECT_MULTI, 1),
    "one_pass_grid3": ("sel", {}, SELECT_MULTI, 3),
    "two_pass": ("sel", {"FDB_SELECT_TWO_PASS": "1"}, FLAGS_MULTI, 0),
    "two_pass_seln": ("seln", {}, FLAGS_MULTI, 0),
    "two_pass_grid1": ("sel", {"FDB_SELECT_TWO_PASS": "1"}, FLAGS_MULTI, 1),
    "two_pass_grid3": ("sel", {"FDB_SELECT_TWO_PASS": "1"}, FLAGS_MULTI, 3),
    "interp": ("sel", {"FDB_NO_JIT": "1"}, "compact_col_kernel", 0),
}
ENV = ("FDB_NO_JIT", "FDB_SELECT_ONE_PASS", "FDB_SELECT_TWO_PASS", "FDB_TEST_SELECT_STALL")


def predicate(column):
    return (Col("selk") == "y") if column == "selk" else (Col(column) > 0)


class Packed:
    """The records of one packed launch, resident, and what pyarrow's filter makes of them (computed once per predicate column)."""

    def __init__(self, recs):
        self.recs = recs
        self.rbs = [pp.ResidentBatch(r) for r in recs]
        self._want = {}

    def want(self, column):
        if column not in self._want:
            self._want[column] = [r.filter(pa.array(fc.mask_of(r, column))) for r in self.recs]
        return self._want[column]

    def close(self):
        for rb in self.rbs:
            rb.close()
        self.rbs = []


_packed = {}


def grid_records(validity_of):
    """The grid's records; validity_of(j) names the validity pattern of record j."""
    return [fc.record(j, c.mask, fc.validity(validity_of(j), c.rows, c.mask)) for j, c in enumerate(fc.grid())]


def packed(name):
    if name not in _packed:
        if name == "mixed":  # records of different validity patterns: a column has a bitmap in some records and none in others
            _packed[name] = Packed(grid_records(lambda j: fc.VALIDITIES[j % len(fc.VALIDITIES)]))
        elif name == "single":
            mask = fc.selection("bernoulli_50", 6145)
            _packed[name] = Packed([fc.record(0, mask, fc.validity("bernoulli_3", 6145, mask))])
        elif name == "threshold":
            recs = []
            for n in (5000, 8193):
                for count in fc.threshold_counts(n):
                    mask = fc.spread_mask(n, count)
                    recs.append(fc.record(len(recs), mask, fc.validity("bernoulli_3", n, mask)))
            _packed[name] = Packed(recs)
        else:
            _packed[name] = Packed(grid_records(lambda j: name))
    return _packed[name]


def assert_same_record(got, want, what):
    assert got.num_rows == want.num_rows, (what, got.num_rows, want.num_rows)
    assert got.schema.names == want.schema.names, what
    for name in want.schema.names:
        g, w = got.column(name), want.column(name)
        if pa.types.is_dictionary(g.type):
            g = g.dictionary_decode()
        if pa.types.is_dictionary(w.type):
            w = w.dictionary_decode()
        assert g.type == w.type, (what, name, g.type, w.type)
        g_valid, w_valid = np.asarray(g.is_valid()), np.asarray(w.is_valid())
        bad = np.flatnonzero(g_valid != w_valid)
        assert len(bad) == 0, (what, name, "NULLs differ at output rows", bad[:8])
        assert g.null_count == w.null_count, (what, name, g.null_count, w.null_count)
        gv, wv = g.drop_null(), w.drop_null()
        if not gv.equals(wv):
            at = next(i for i in range(len(wv)) if gv[i] != wv[i])
            raise AssertionError((what, name, "valid value", at, gv[at], wv[at]))


def set_route(monkeypatch, route):
    column, env, kernel, grid_blocks = ROUTES[route]
    for v in ENV:
        monkeypatch.delenv(v, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    plan = pp.HashAggregatePlan(predicate(column))
    if grid_blocks:
        plan.set_tuning(grid_blocks=grid_blocks)
    return plan, column, kernel


def run_route(monkeypatch, route, P, many=True):
    """The records of `P` through `route`: (Arrow results, device bytes of the results, predicate column)."""
    plan, column, kernel = set_route(monkeypatch, route)
    try:
        outs = plan.FilterResidentMany(P.rbs) if many else [plan.FilterResident(P.rbs[0])]
        try:
            assert plan.last_kernel() == kernel, (route, plan.last_kernel())
            got = [o.to_arrow() for o in outs]
            assert [o.num_rows for o in outs] == [g.num_rows for g in got]
            sizes = [o.device_bytes for o in outs]
        finally:
            for o in outs:
                o.close()
    finally:
        plan.Close()
    return got, sizes, column


def check_route(monkeypatch, route, name):
    P = packed(name)
    got, _, column = run_route(monkeypatch, route, P)
    cases = fc.grid()
    for j, (g, w) in enumerate(zip(got, P.want(column))):
        assert_same_record(g, w, (route, name, j, cases[j].rows, cases[j].selection, cases[j].lead))
    return got


@pytest.mark.parametrize("validity", fc.VALIDITIES)
@pytest.mark.parametrize("route", list(ROUTES))
def test_packed_grid(monkeypatch, route, validity):
    check_route(monkeypatch, route, validity)


@pytest.mark.parametrize("route", list(ROUTES))
def test_packed_grid_of_mixed_validity_patterns(monkeypatch, route):
    P = packed("mixed")
    for c in fc.NULLABLE_COLUMNS:  # some records carry a bitmap in the column and some do not
        has = {r.column(c).null_count > 0 for r in P.recs}
        assert has == {True, False}
    check_route(monkeypatch, route, "mixed")


@pytest.mark.parametrize("validity", fc.VALIDITIES + ["mixed"])
def test_one_pass_and_two_pass_results_are_the_same_arrow_records(monkeypatch, validity):
    P = packed(validity)
    one, _, _ = run_route(monkeypatch, "one_pass", P)
    two, _, _ = run_route(monkeypatch, "two_pass", P)
    for j, (a, b) in enumerate(zip(one, two)):
        assert a.equals(b), (validity, j)


@pytest.mark.parametrize("route", list(ROUTES))
def test_single_record(monkeypatch, route):
    """FilterResident of one record (6 145 rows, every second row selected at random, 3 % NULLs) — against pyarrow and the oracle."""
    from oracle import OraclePlan
    P = packed("single")
    got, _, column = run_route(monkeypatch, route, P, many=False)
    assert_same_record(got[0], P.want(column)[0], (route, "single"))
    o = OraclePlan(predicate(column))
    out, idx = o.filter(P.recs[0])
    try:
        assert np.array_equal(np.asarray(idx), np.flatnonzero(fc.mask_of(P.recs[0], column)))
        want = out.to_pydict()
    finally:
        out.close()
        o.close()
    g = arrow_to_pydict(got[0])
    for name in fc.COLUMNS:
        assert g[name] == want[name], (route, name)


@pytest.mark.parametrize("column", ["sel", "selk", "seln"])
def test_selection_vectors(monkeypatch, column):
    import torch
    for v in ENV:
        monkeypatch.delenv(v, raising=False)
    P = packed("no_bitmap")
    buf = torch.empty(max(fc.ROWS) + 64, dtype=torch.int32, device="cuda:0")
    plan = pp.HashAggregatePlan(predicate(column))
    try:
        for j, (rec, rb) in enumerate(zip(P.recs, P.rbs)):
            want = np.flatnonzero(fc.mask_of(rec, column)).astype(np.uint32)
            k = plan.SelectResident(rb, buf.data_ptr(), rec.num_rows)
            assert k == len(want), (column, j, rec.num_rows, k, len(want))
            assert np.array_equal(buf[:k].cpu().numpy().view(np.uint32), want), (column, j, rec.num_rows)
        assert plan.last_kernel() == "compact_col_kernel"
    finally:
        plan.Close()


def test_repack_threshold(monkeypatch):
    """The fused column's worst-case block is kept from ⌈0.4 n⌉ selected rows on and repacked into the exact arena below: results on both
    sides of the boundary, and a repacked result holds fewer device bytes than a kept one."""
    P = packed("threshold")
    got, sizes, column = run_route(monkeypatch, "one_pass", P)
    at = 0
    for n in (5000, 8193):
        counts = fc.threshold_counts(n)
        for j, count in enumerate(counts):
            assert got[at + j].num_rows == count
            assert_same_record(got[at + j], P.want(column)[at + j], ("threshold", n, count))
        none, below, exactly, above, everything = sizes[at:at + 5]
        assert none < below < exactly <= above <= everything, (n, sizes[at:at + 5])
        # (the block of n 8-byte values against one of the exact size, either rounded up to at most 256 bytes)
        assert exactly - below >= 8 * (n - counts[2]) - 256, (n, below, exactly)
        at += len(counts)
    two, _, _ = run_route(monkeypatch, "two_pass", P)
    for a, b in zip(got, two):
        assert a.equals(b)


def test_everything_is_released():
    for P in _packed.values():
        P.close()
    _packed.clear()
    gc.collect()
    assert pp.live_allocations() == {"device_blocks": 0, "device_bytes": 0, "pinned_blocks": 0}
