"""What feeds the hash table and what empties it, at their edges: every case of tests/hash_scan_cases.py — each one claims there which
branch of the scan, the table's growth and its Finish it takes, and tests/test_hash_scan_cases_cpu.py holds the families to covering
every branch — runs through the Python binding (HashAggregatePlan, resident records, one Callback per record, Finish, FinishResident,
partial_keys / partial_state) in BOTH variants of the scan: the specialised fdb_hash_kernel and, under FDB_NO_JIT, the interpreting
scan_hash_kernel. The result is compared with the case's expected rows as multisets, exactly, float columns included (all values are
integers); the expected rows come from the numpy group-by of hash_scan_cases.py, which the CPU module holds to the oracle.

After every push the observable part of the claim is asserted: the kernel's name, the number of launches so far (= chunks), the number
of groups. The growth cases read the group count only at their end: num_groups() refreshes the bound push_hash works with, and the
claimed chunk walk is that of undisturbed pushes.

The module reads fdb_jit_stats before and after itself and prints how many kernels it compiled; the families share shapes (the row
count and the run layout are not part of one), so the number is that of the column layouts, not of the cases."""
import time

import numpy as np
import pyarrow as pa
import pytest

from tests import hash_scan_cases as S
from tests.hash_merge_cases import record_rows

pytestmark = pytest.mark.gpu

MAX_COMPILED = 64  # the distinct (columns, validity, LUT placement, filter, reducers, exact) shapes the families were laid out to share


@pytest.fixture(scope="module")
def pp():
    from frostdb_amd import physicalplan
    assert physicalplan.device_count() >= 1, "no HIP device visible"
    return physicalplan


@pytest.fixture(scope="module", autouse=True)
def compile_cost(pp):
    before, t0 = pp.jit_stats(), time.time()
    yield
    after = pp.jit_stats()
    compiled = after["compiled"] - before["compiled"]
    print("\n[test_gpu_hash_scan] kernels compiled: %d (%.1f s of hiprtc), loaded from the disk cache: %d, module wall time %.1f s"
          % (compiled, (after["compile_ms"] - before["compile_ms"]) / 1e3, after["disk_loads"] - before["disk_loads"], time.time() - t0))
    assert compiled <= MAX_COMPILED, compiled


class Plans:
    """The plans and resident records of one run, closed on the way out whatever happened"""

    def __init__(self, pp):
        self.pp, self.plans, self.keep = pp, [], []

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for p in self.plans:
            p.Close()
        for k in self.keep:
            k.close()

    def plan(self, case):
        p = self.pp.HashAggregatePlan(case.filt, case.aggs, case.matchers)
        self.plans.append(p)
        if case.exact:
            p.set_exact_sums(True)
        return p

    def resident(self, batch):
        rb = self.pp.ResidentBatch(batch)
        self.keep.append(rb)
        return rb


def assert_rows(got, want, what):
    missing, extra = want - got, got - want
    assert not missing and not extra, (what, sum(got.values()), sum(want.values()), "missing", list(missing.items())[:3], "extra", list(extra.items())[:3])


def set_variant(monkeypatch, case, variant):
    for k, v in case.env.items():
        monkeypatch.setenv(k, v)
    if variant == "interp":
        monkeypatch.setenv("FDB_NO_JIT", "1")
    else:
        monkeypatch.delenv("FDB_NO_JIT", raising=False)


def scan(pp, ps, case, variant):
    """Every record through one plan, the claims asserted push by push → the plan (None where the variant refuses the case, as claimed)"""
    p = ps.plan(case)
    for i, b in enumerate(case.records):
        rb = ps.resident(b)
        if case.kernels[variant] == "unsupported":
            with pytest.raises(pp.FdbError) as e:
                p.Callback(rb)
            assert e.value.code == pp.FDB_ERR_UNSUPPORTED, str(e.value)
            return None
        p.Callback(rb)
        claim = case.pushes[i]
        assert p.last_kernel() == case.kernels[variant], (case.id, i, p.last_kernel())
        assert p.stats()["launches"] == claim["launches"], (case.id, i, p.stats()["launches"], claim["chunks"])
        if case.family != "growth" or i == len(case.records) - 1:
            assert p.num_groups() == case.groups_after[i], (case.id, i)
    return p


def check_record(case, rec, what):
    """→ the rows. Exact equality with the expected rows; the schema and the NULL count of every column, from the expected rows alone"""
    cols = case.out_columns()
    got = case.normalise(record_rows(rec, cols))
    assert_rows(got, case.want, (case.id, what))
    assert rec.num_rows == case.finish["groups"]
    if rec.num_rows == 0:
        return got
    assert rec.schema.names == cols, (case.id, rec.schema.names)
    want_rows = list(case.want.elements())
    for c, name in enumerate(cols):
        a = rec.column(c)
        if c >= len(case.names):
            assert a.null_count == 0 and a.type == (pa.float64() if "floatvalue" in name and not name.startswith("count(") else pa.int64()), (case.id, name, a.type)
            continue
        if name.startswith("labels."):
            assert pa.types.is_dictionary(a.type) and a.type.index_type == pa.uint32() and a.type.value_type == pa.binary(), (case.id, name, a.type)
        if not case.null_or_zero:
            assert a.null_count == sum(1 for r in want_rows if r[c] is None), (case.id, name, a.null_count)
            assert (a.null_count > 0) == (name in case.finish["bitmaps"])
    if "null_row" in case.finish:  # the case put its one NULL group on this row of the result (slot order; hash_scan_cases.home_slot)
        assert np.flatnonzero(rec.column(0).is_null().to_numpy(zero_copy_only=False)).tolist() == [case.finish["null_row"]], case.id
    return got


def run_case(pp, monkeypatch, case, variant, through):
    set_variant(monkeypatch, case, variant)
    with Plans(pp) as ps:
        p = scan(pp, ps, case, variant)
        if p is None:
            return None
        if through == "finish":
            return check_record(case, p.Finish(), variant)
        if through == "resident":
            rb = p.FinishResident()
            ps.keep.append(rb)
            assert rb.num_rows == case.finish["groups"]
            return check_record(case, rb.to_arrow(), variant + ", resident")
        # partial keys and states (hash_compact_kernel): two calls on an unchanged table line up row by row, with each other and with the states
        keys, again = p.partial_keys(), p.partial_keys()
        n = keys.num_rows
        assert n == case.finish["groups"] and again.equals(keys)
        cols = [keys.column(keys.schema.get_field_index(c)) for c in case.names]
        cols = [(a.dictionary_decode() if pa.types.is_dictionary(a.type) else a).to_pylist() for a in cols]
        for j in range(len(case.aggs)):
            buf = np.zeros(n, dtype=np.float64 if p.agg_format(j) == "g" else np.int64)
            p.partial_state_into(j, buf.ctypes.data, n * 8)
            cols.append(buf.tolist())
        got = type(case.want)(zip(*cols))
        assert_rows(got, case.want, (case.id, variant, "partial"))
        return got


def params(family):
    return [pytest.param(c, v, t, id="%s-%s-%s" % (c.id, v, t)) for c in S.cases(family) for v in c.variants for t in c.through]


@pytest.mark.parametrize("case,variant,through", params("rows"))
def test_rows_at_lane_wave_and_tile_edges(pp, monkeypatch, case, variant, through):
    run_case(pp, monkeypatch, case, variant, through)


@pytest.mark.parametrize("case,variant,through", params("runs"))
def test_runs_fold_without_losing_or_doubling_a_row(pp, monkeypatch, case, variant, through):
    """Beside equality with the reference: the count of every group is the one the run layout gives by construction"""
    got = run_case(pp, monkeypatch, case, variant, through)
    counts = {k[:2]: k[2] for k in got}
    assert counts == case.counts, (case.id, variant, {k: (v, case.counts.get(k)) for k, v in counts.items() if case.counts.get(k) != v})


@pytest.mark.parametrize("case,variant,through", params("columns"))
def test_columns_in_groups_of_eight_quads_and_wide_keys(pp, monkeypatch, case, variant, through):
    run_case(pp, monkeypatch, case, variant, through)


@pytest.mark.parametrize("case,variant,through", params("luts"))
def test_key_id_luts_identity_lds_and_global(pp, monkeypatch, case, variant, through):
    run_case(pp, monkeypatch, case, variant, through)


@pytest.mark.parametrize("case,variant,through", params("growth"))
def test_chunks_growth_and_rehash_keep_every_group(pp, monkeypatch, case, variant, through):
    """The two records of 2^20 rows and more are checked against the numpy reference only (hash_scan_cases.reference; the oracle is not asked).
    Where the case re-hashes (`before_rehash`: the push that does), every group that was in the table before and gets no row afterwards is
    still there with the aggregates it had."""
    got = run_case(pp, monkeypatch, case, variant, through)
    if case.before_rehash is None:
        return
    k, nk = case.before_rehash, len(case.names)
    before = S.reference(case.records[:k], case.names, case.aggs)[0]
    later = {r[:nk] for r in S.reference(case.records[k:], case.names, case.aggs)[0]}
    untouched = type(before)({r: n for r, n in before.items() if r[:nk] not in later})
    assert len(untouched) >= 10000
    keys = {r[:nk] for r in untouched}
    assert_rows(type(before)({r: n for r, n in got.items() if r[:nk] in keys}), untouched, (case.id, "the groups from before the re-hash"))


@pytest.mark.parametrize("case,variant,through", params("finish"))
def test_finish_group_counts_slices_widths_and_bitmaps(pp, monkeypatch, case, variant, through):
    run_case(pp, monkeypatch, case, variant, through)
