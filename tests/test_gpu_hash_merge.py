"""hash_merge_wave_kernel<TABLE_SRC>, hash_partition_wave_kernel<PASS> and partition_bases_kernel (fdb_merge.hip) at their wave edges:
every case of tests/hash_merge_cases.py — each one claims a launch shape there, and tests/test_hash_merge_cases_cpu.py holds the
families to covering every branch — runs through the Python binding (HashAggregatePlan, Callback, Merge, clone_empty, seed_groups,
hash_export, hash_import, Finish, num_groups) and is compared with the oracle over all records of the case, as multisets of rows.
Everything is exact, float64 sums included: the float values are small integers, so their sum is the same in any order.

The oracle gets the key columns of every record in one order (hash_merge_cases.Case.all_records says why: the reference's group hash
depends on the field order, the library's groups on the columns' names).

The scan is not under test: the module runs with FDB_NO_JIT, the interpreting kernels, so that no shape pays a compile at run time;
the plain 12-column merge runs once more with the specialised kernel."""
import numpy as np
import pytest

from frostdb_amd.logicalplan import Col, Count, DynCol, Sum
from tests import hash_merge_cases as H

pytestmark = pytest.mark.gpu

HASH_SCANS = ("scan_hash_kernel", "fdb_hash_kernel")


@pytest.fixture(scope="module")
def pp():
    from frostdb_amd import physicalplan
    assert physicalplan.device_count() >= 1, "no HIP device visible"
    return physicalplan


@pytest.fixture(autouse=True)
def interpreted_scan(monkeypatch):
    monkeypatch.setenv("FDB_NO_JIT", "1")


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
        p = self.pp.HashAggregatePlan(case.filt, case.aggs, case.matchers, final_stage=case.final_stage)
        self.plans.append(p)
        return p

    def own(self, plan):
        self.plans.append(plan)
        return plan

    def scan(self, plan, recs):
        """record by record, each resident and scanned at its own Callback (a host record would wait for the next ones)"""
        for r in recs:
            rb = self.pp.ResidentBatch(r.batch)
            self.keep.append(rb)
            plan.Callback(rb)


def assert_rows(got, want, what):
    missing, extra = want - got, got - want
    assert not missing and not extra, (what, sum(got.values()), sum(want.values()), "missing", list(missing.items())[:3], "extra", list(extra.items())[:3])


def by_id(family, id):
    return next(c for c in H.cases(family) if c.id == id)


# ---- merges: table → table, packed rows of a dense source → table ---------------------------------------------------------------------
def merge_both_ways(pp, case):
    want = H.oracle_rows(case)
    for swapped in (False, True):
        with Plans(pp) as ps:
            a, b = ps.plan(case), ps.plan(case)
            ps.scan(a, case.dst)
            ps.scan(b, case.srcs[0])
            assert a.num_groups() == case.dst_groups and b.num_groups() == case.src_groups[0], case.id
            if case.dst:
                assert a.last_kernel() in HASH_SCANS, a.last_kernel()
            if case.srcs[0]:  # the source holds what the case claims: a hash table, or the dense table whose slots leave as packed rows
                assert (b.last_kernel() in HASH_SCANS) == (case.op == "merge"), b.last_kernel()
            dst, src = (b, a) if swapped else (a, b)
            dst.Merge(src)
            assert dst.num_groups() == case.groups, (case.id, swapped)
            got = H.record_rows(dst.Finish(), case.out_columns())
        assert_rows(got, want, (case.id, "swapped" if swapped else "as stated"))


MERGES = [c for f in ("widths", "layouts", "counts", "reducers") for c in H.cases(f)] + [c for c in H.cases("packed") if c.op == "dense_into_hash"]


@pytest.mark.parametrize("case", MERGES, ids=repr)
def test_merge_equals_the_oracle_in_both_directions(pp, case):
    merge_both_ways(pp, case)


def test_plain_merge_behind_the_specialised_scan(pp, monkeypatch):
    monkeypatch.delenv("FDB_NO_JIT")
    merge_both_ways(pp, by_id("widths", "widths-12_dict"))


def test_a_widened_destination_keeps_its_groups_and_their_aggregates(pp):
    """The source brings a 13th dictionary column: the destination's 16-word tuples are re-hashed into 20 words. Every group it held is
    still there with the aggregates it had, its new column NULL (the words a tuple gains come out zero: a stray id there would make it
    another group, or give it a value); the source's groups all carry a value in the new column."""
    case = by_id("layouts", "layouts-source_brings_a_13th_column")
    cols = case.out_columns()
    before = H.oracle_rows_of([r.batch for r in case.dst], None, case.aggs, case.matchers, cols)
    assert len(before) == case.dst_groups == 3000
    with Plans(pp) as ps:
        a, b = ps.plan(case), ps.plan(case)
        ps.scan(a, case.dst)
        ps.scan(b, case.srcs[0])
        assert a.num_groups() == 3000
        a.Merge(b)
        got = H.record_rows(a.Finish(), cols)
    new = cols.index("labels.l12")
    assert_rows(type(got)({r: n for r, n in got.items() if r[new] is None}), before, "the groups from before the widening")
    assert sum(1 for r in got if r[new] is not None) == case.src_groups[0]


def test_a_column_that_lands_on_the_tuples_padding_is_null_in_the_groups_from_before(pp, monkeypatch):
    """Nine dictionary columns use 13 of a tuple's 16 words; a source with a 10th column puts it on word 13, tail padding until then. The
    specialised scan does not write a canonical tuple's padding (the table remembers its used prefix instead), so whatever the key store's
    block held before shows through unless hash_layout clears the words the new column lands on. A plan of 12 columns and 32 768 groups
    runs and closes first: the caching allocator hands its 4 MiB key store — ids in words 13 … 15 of half the slots — to the destination.
    (tests/test_gpu_edges_fuzz.py::test_edges_fuzz[chains-55] met this with a uint64 key beside a dictionary column: a key id of 14 in
    a dictionary of 10 values, depending on what ran before it.)"""
    monkeypatch.delenv("FDB_NO_JIT")
    case = by_id("layouts", "layouts-source_brings_a_10th_column_onto_the_padding")
    before = by_id("counts", "counts-32768_into_empty")
    cols = case.out_columns()
    with Plans(pp) as ps:
        p = ps.plan(before)
        ps.scan(p, before.srcs[0])
        assert p.num_groups() == 32768 and p.last_kernel() == "fdb_hash_kernel"
    with Plans(pp) as ps:
        a, b = ps.plan(case), ps.plan(case)
        ps.scan(a, case.dst)
        ps.scan(b, case.srcs[0])
        assert a.last_kernel() == "fdb_hash_kernel" and a.num_groups() == 3000
        a.Merge(b)
        assert a.num_groups() == case.groups
        got = H.record_rows(a.Finish(), cols)
    assert_rows(got, H.oracle_rows(case), case.id)
    old = H.oracle_rows_of([r.batch for r in case.dst], None, case.aggs, case.matchers, cols)
    assert_rows(type(got)({r: n for r, n in got.items() if r[cols.index("labels.l09")] is None}), old, "the groups from before the new column")


# ---- migration: the dense table's slots leave as packed rows ----------------------------------------------------------------------------
@pytest.mark.parametrize("case", [c for c in H.cases("packed") if c.op == "migrate"], ids=repr)
def test_migration_equals_the_oracle(pp, case):
    first, second = case.dst
    with Plans(pp) as ps:
        a = ps.plan(case)
        ps.scan(a, [first])
        assert a.last_kernel() not in HASH_SCANS, a.last_kernel()  # a dense table so far
        assert a.num_groups() == H.distinct_groups([first], case.names)
        ps.scan(a, [second])
        assert a.last_kernel() in HASH_SCANS, a.last_kernel()
        assert a.num_groups() == case.groups
        got = H.record_rows(a.Finish(), case.out_columns())
    assert_rows(got, H.oracle_rows(case), case.id)


# ---- the hash-partitioned export and the import of its regions --------------------------------------------------------------------------
def export_import(pp, ps, case, sources=None, schema=None):
    """→ (every owner's Finish, every source's counts per partition). Every source plan exports for the case's owners, owner p imports
    region p of every source."""
    from frostdb_amd import distributed as fd
    plans = []
    for recs in (case.srcs if sources is None else sources):
        p = ps.plan(case)
        ps.scan(p, recs)
        plans.append(p)
    if schema is None:
        schema = fd.unify_group_schemas([fd._schema_to_obj(p.group_schema()) for p in plans])
    owners = []
    for _ in range(case.n_parts):
        o = ps.own(plans[0].clone_empty())
        o.seed_groups(schema)
        owners.append(o)
    all_counts = []
    for p in plans:
        n = p.num_groups()
        ptr, counts, row_bytes = p.hash_export(owners[0], case.n_parts)
        assert len(counts) == case.n_parts and min(counts) >= 0 and sum(counts) == n, (case.id, n, counts)
        row = 0
        for o, c in zip(owners, counts):
            o.hash_import(ptr + row * row_bytes, c)
            row += c
        all_counts.append(counts)
    return [o.Finish() for o in owners], all_counts, schema


def check_owners(case, recs, all_counts):
    keys = [H.record_rows(r, case.names) for r in recs]
    union = type(keys[0])()
    for k in keys:
        assert all(n == 1 for n in k.values())
        union.update(k)
    assert all(n == 1 for n in union.values()), (case.id, "a group on two owners", [k for k, n in union.items() if n > 1][:3])
    got = type(union)()
    for r in recs:
        got.update(H.record_rows(r, case.out_columns()))
    assert_rows(got, H.oracle_rows(case), case.id)
    if len(case.srcs) == 1:
        assert [r.num_rows for r in recs] == all_counts[0]
    for n, counts in zip(case.src_groups, all_counts):
        assert sum(counts) == n
        if n >= 32768:  # a uniform hash: binomial spread, 6 standard deviations (√(n/P · (1 − 1/P)) < √(n/P)); the inputs are seeded
            mean = n / case.n_parts
            assert all(abs(c - mean) <= 6 * np.sqrt(mean) for c in counts), (case.id, mean, min(counts), max(counts))


@pytest.mark.parametrize("case", H.cases("exports"), ids=repr)
def test_export_and_import_equal_the_oracle_on_disjoint_owners(pp, case):
    with Plans(pp) as ps:
        for p_src, n in zip(case.srcs, case.src_groups):
            assert n == H.distinct_groups(p_src, case.names)
        recs, all_counts, _ = export_import(pp, ps, case)
        if case.src_groups[0] <= 65 and case.n_parts == 64:
            assert sum(1 for c in all_counts[0] if c == 0) >= 64 - case.src_groups[0]  # most partitions are empty, and that works
        check_owners(case, recs, all_counts)


def test_dictionary_order_does_not_change_a_groups_owner(pp):
    """The same 3 000 groups in two plans that differ only in the order (and size) of their dictionaries, exported into one layout for 17
    owners: partition by partition the same keys."""
    sp = H.space(12)
    names = H.column_names(sp)
    g = H.rows_over(np.arange(3000), 3, 5)
    natural, permuted = H.make_record(sp, g, 6), H.make_record(sp, g, 6, dict_order="permuted")
    case = H.Case("same groups, two dictionary orders", "exports", "export_import", names, srcs=[[natural], [permuted]], n_parts=17)
    assert [s["same_ids"] for s in case.shapes if s["why"] == "export"] == [1, 0]
    with Plans(pp) as ps:
        recs_a, counts_a, schema = export_import(pp, ps, case, sources=[[natural]])
        recs_b, counts_b, _ = export_import(pp, ps, case, sources=[[permuted]], schema=schema)
        # (the first run's schema holds the natural order only; the permuted plan's two unused values are appended to it by the export)
        assert counts_a == counts_b
        for p, (ra, rb) in enumerate(zip(recs_a, recs_b)):
            assert_rows(H.record_rows(rb, case.out_columns()), H.record_rows(ra, case.out_columns()), ("partition", p))


def test_exact_sums_travel_through_the_exchange_of_local_ranks(pp):
    """fdb_plan_hash_import refuses exact plans: their limb rows travel through fdb_plan_exchange, here on three ranks of the in-process
    transport (three partitions, every rank both exports and imports). 12 dictionary columns, half of a rank's groups are the next one's."""
    from frostdb_amd import comm
    from tests.test_gpu_exact_exchange import exchange
    sp = H.space(12)
    names = H.column_names(sp)
    aggs = [Sum(Col("floatvalue")), Count(Col("value")), Sum(Col("value"))]
    shards = [[H.make_record(sp, H.rows_over(np.arange(1500 * r, 1500 * r + 3000), 3, 40 + r), 50 + r, dict_order="permuted" if r == 1 else "natural").batch] for r in range(3)]
    cols = names + [a.Name() for a in aggs]
    want = H.oracle_rows_of([b for s in shards for b in s], None, aggs, [DynCol("labels")], cols)
    assert len(want) == 6000
    outs = exchange(pp, comm, shards, aggs, [DynCol("labels")])
    got = type(want)()
    for out in outs:
        assert out.num_rows > 1500  # (6 000 groups over three owners)
        got.update(H.record_rows(out, cols))
    assert_rows(got, want, "exact exchange")


def test_refusals_return_their_codes_and_leave_the_plans_usable(pp):
    case = by_id("exports", "exports-3000_groups_2_parts")
    with Plans(pp) as ps:
        p = ps.plan(case)
        ps.scan(p, case.srcs[0])
        owner = ps.own(p.clone_empty())
        owner.seed_groups(p.group_schema())
        for n_parts in (0, H.MAX_PARTS + 1):
            with pytest.raises(pp.FdbError) as e:
                p.hash_export(owner, n_parts)
            assert e.value.code == pp.FDB_ERR_INVALID, (n_parts, str(e.value))
        other = ps.own(pp.HashAggregatePlan(None, [Count(Col("value"))], case.matchers))  # one aggregation, not two
        with pytest.raises(pp.FdbError) as e:
            p.hash_export(other, 2)
        assert e.value.code == pp.FDB_ERR_INVALID
        with pytest.raises(pp.FdbError) as e:
            p.Merge(other)
        assert e.value.code == pp.FDB_ERR_INVALID
        with pytest.raises(pp.FdbError) as e:
            p.Merge(p)
        assert e.value.code == pp.FDB_ERR_INVALID
        exact = ps.own(p.clone_empty())
        exact.set_exact_sums(True)
        with pytest.raises(pp.FdbError) as e:
            exact.hash_import(0, 0)
        assert e.value.code == pp.FDB_ERR_UNSUPPORTED
        # both plans still do their work
        ptr, counts, row_bytes = p.hash_export(owner, 2)
        assert sum(counts) == p.num_groups() == 3000
        owner.hash_import(ptr, counts[0])
        owner.hash_import(ptr + counts[0] * row_bytes, counts[1])
        assert owner.num_groups() == 3000
        assert_rows(H.record_rows(owner.Finish(), case.out_columns()), H.oracle_rows(case), "after the refusals")
        assert_rows(H.record_rows(p.Finish(), case.out_columns()), H.oracle_rows(case), "the source after the refusals")
