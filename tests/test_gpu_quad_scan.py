"""The quad form of the dense generated scan (fdb_jit.h, JitShape::quad): a launch with a narrow slot counts its work in units of
block x 16 rows, a wave takes a block of 1 024 rows as four sub-steps and reads a full block's narrow indices with 16-byte loads of the
wave-interleaved cache (fdb_record.h, scan_cache_position); the record's last, partial block is read in row order.

The tables, the numpy restatement of the query and the checks are those of tests/test_gpu_narrow_scan.py (counts and int64 MIN / MAX
exact, float64 sums to 1e-9 relative, algorithmic bytes at the widths scanned): per-group sums of random `v` catch any row that meets
another row's index. T = 1 Mi rows is the smallest record that gets a cache. Rows: T + {255, 256} (the last sub-step of a wave's block
partial / just full), T + {4095, 4096, 4097} around the unit of a 256-thread workgroup, T + {16383, 16384, 16385} around the unit of
1 024 threads (variant 3); variant 2 (256 threads) once. T itself is a multiple of every unit."""
import numpy as np
import pytest

from frostdb_amd import physicalplan as pp
from tests import test_gpu_narrow_scan as ns
from tests.test_gpu_narrow_scan import T, Table

pytestmark = pytest.mark.gpu

DICTS = {"f": 5, "g": 200, "h": 300, "k": 65537}  # 1 byte, 1 byte, 2 bytes, and one that stays at 4
WIDTHS = {name: ns.width_of(entries) for name, entries in DICTS.items()}
CASES = [(T + d, 0) for d in (255, 256, 4095, 4096, 4097)] + [(T + d, 3) for d in (16383, 16384, 16385)] + [(T + 4097, 2)]


def run(tables, filt, groups, variant=0, **kw):
    """ns.run with the plan's kernel variant set (fdb_plan_set_tuning: 2 = 256, 3 = 1 024 threads per workgroup)."""
    plain = pp.HashAggregatePlan

    class Tuned(plain):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            self.set_tuning(0, variant << 25)

    pp.HashAggregatePlan = Tuned if variant else plain
    try:
        return ns.run(tables, filt, groups, WIDTHS, **kw)
    finally:
        pp.HashAggregatePlan = plain


def table(rows, nulls, seed, **kw):
    return Table(rows, {name: (entries, nulls) for name, entries in DICTS.items()}, seed=seed, **kw)


@pytest.mark.parametrize("rows,variant", CASES, ids=["T+%d-v%d" % (r - T, v) for r, v in CASES])
def test_rows_and_shapes(rows, variant):
    for nulls in (False, True):
        t = table(rows, nulls, seed=rows + variant + nulls)
        try:
            run([t], "f", [], variant, with_i=True)          # filter only
            run([t], None, ["h"], variant)                   # group only
            run([t], "f", ["h"], variant)                    # both (single-phase: the headline's shape)
            run([t], "f", ["g", "h"], variant, with_i=True)  # two group columns of 1 + 2 bytes (two-phase)
            run([t], "f", ["k"], variant)                    # a 4-byte slot beside a narrow one (a table too big for LDS)
            assert t.rb.scan_cache_bytes == sum(ns.values_slot(rows, WIDTHS[c]) for c in "fgh")
        finally:
            t.close()


def test_one_launch_over_records_that_end_mid_unit():
    """Every record ends inside a unit (T + 1025, T + 4097) or on one (T), and the next starts at a fresh unit of its own."""
    tables = [table(T + 1025, True, 31), table(T, True, 32), table(T + 4097, True, 33)]
    try:
        run(tables, "f", ["h"])
        run(tables, "f", ["g", "h"], with_i=True)
    finally:
        for t in tables:
            t.close()


def test_ordered_plan_over_a_sorted_record():
    """Sorted by the group column: the rows a wave selects in a sub-step fall into one slot (the uniform fold inside the sub-step loop)."""
    t = table(T + 4097, False, 34, sort_by="h")
    try:
        assert np.all(np.diff(t.idx["h"]) >= 0)
        run([t], "f", ["h"], ordered=True)
    finally:
        t.close()
