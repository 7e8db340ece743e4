"""The quad form of the dense scan issues every early load of a wave's 1 024-row block in front of sub-step 0's filter (Gen::block_loads,
frostdb_amd/csrc/fdb_jitgen.cpp). The branches those loads used to hide behind are taken here on purpose: tables built from explicit arrays
whose filter column selects nothing in chosen sub-steps of 256 rows — sub-step 0 of every fourth block, later sub-steps of the others, one
whole block — with NULLs in the group column at a block's rows 0 to 3 and at its last row.

Records of 2^20 + {0, 1, 1023, 1025} rows: full blocks only, and a last block of 1, 1 023 and 1 025 rows (a full block and one row). Each
size runs with the group column sorted (a wave's selected rows fall into one slot: the uniform fold) and, unsorted, with
set_deterministic (per-wave tables); SUM(float64) alone (single-phase) and SUM + COUNT + MIN / MAX(int64) (two-phase). The query
restatement, the byte formulas and the tolerances are those of tests/test_gpu_narrow_scan.py."""
import numpy as np
import pyarrow as pa
import pytest

from frostdb_amd import physicalplan as pp
from frostdb_amd.logicalplan import Col, Count, Max, Min, Sum
from tests.test_gpu_narrow_scan import T, dictionary, expected, scanned_bytes, values_slot

pytestmark = pytest.mark.gpu

ROWS = [T + d for d in (0, 1, 1023, 1025)]
DICTS = {"f": (5, True), "g": (1024, True)}
WIDTHS = {"f": 1, "g": 2}
EMPTY_BLOCK = 5


class Explicit:
    """A record of `rows` rows with the attributes tests.test_gpu_narrow_scan.expected reads (rows, dicts, idx, v, i), from explicit arrays."""

    def __init__(self, rows: int, sort: bool):
        rng = np.random.default_rng(rows + sort)
        row = np.arange(rows)
        block, sub = row // 1024, (row % 1024) // 256
        # f: 5 entries, the filter keeps the last one; ≈ 10 % NULL rows whose index slots hold something above every narrow range
        f = rng.integers(0, 5, rows, dtype=np.uint32)
        f[rng.random(rows) < 0.25] = 4
        f[-1] = 4
        f_null = rng.random(rows) < 0.1
        f_null[-1] = False
        nothing = ((block % 4 == 0) & (sub == 0)) | ((block % 4 == 1) & (sub == 2)) | ((block % 4 == 2) & ((sub == 1) | (sub == 3))) | (block == EMPTY_BLOCK)
        nothing[-1] = False  # (the record's last row stays selected: the partial block's tail lane has work)
        f[nothing & (f == 4)] = 0
        f = np.where(f_null, np.uint32(70000) + (f & np.uint32(0xFFF)), f).astype(np.uint32)
        # g: 1 024 entries; sorted: one entry per block (the tail rows share the last block's)
        g = np.minimum(block, 1023).astype(np.uint32) if sort else rng.integers(0, 1024, rows, dtype=np.uint32)
        g_null = (block % 3 == 0) & ((row % 1024 < 4) | (row % 1024 == 1023))
        g = np.where(g_null, np.uint32(70000) + (g & np.uint32(0xFFF)), g).astype(np.uint32)
        self.rows, self.dicts = rows, DICTS
        self.idx = {"f": np.where(f_null, -1, f.astype(np.int64)), "g": np.where(g_null, -1, g.astype(np.int64))}
        self.v = 1.0 - rng.random(rows)
        self.i = rng.integers(-2**40, 2**40, rows, dtype=np.int64)
        sel = self.idx["f"] == 4
        assert not sel[nothing].any() and sel[(block % 4 == 0) & (sub == 1)].any() and sel[-1]
        assert (self.idx["g"][sel] == -1).any()  # (selected rows with a NULL group key exist)
        self.record = pa.RecordBatch.from_arrays(
            [pa.DictionaryArray.from_arrays(pa.array(f, mask=f_null), dictionary(5, "f")), pa.DictionaryArray.from_arrays(pa.array(g, mask=g_null), dictionary(1024, "g")),
             pa.array(self.v), pa.array(self.i)], names=["f", "g", "v", "i"])
        self.rb = pp.ResidentBatch(self.record)


def run(t, with_i: bool, deterministic: bool):
    aggs = [Sum(Col("v"))] + ([Count(Col("v")), Min(Col("i")), Max(Col("i"))] if with_i else [])
    plan = pp.HashAggregatePlan(Col("f") == "f4", aggs, [Col("g")])
    try:
        if deterministic:
            plan.set_deterministic()
        plan.CallbackResident([t.rb])
        assert plan.last_kernel() == "fdb_plan_kernel", plan.last_kernel()
        assert plan.stats()["algorithmic_bytes"] == scanned_bytes([t], "f", ["g"], WIDTHS, with_i)
        out = plan.Finish()
    finally:
        plan.Close()
    keys, sums, counts, mins, maxs = expected([t], "f", ["g"], with_i)
    assert out.num_rows == len(keys), (out.num_rows, len(keys))
    c = out.column("g")
    entry = np.array([int(x.decode()[1:]) for x in c.dictionary.to_pylist()] + [-1], dtype=np.int64)
    flat = entry[c.indices.fill_null(len(entry) - 1).to_numpy(zero_copy_only=False).astype(np.int64)] + 1
    order = np.argsort(flat, kind="stable")
    assert np.array_equal(flat[order], keys)  # the same groups, each once
    got = out.column("sum(v)").to_numpy()[order]
    assert np.all(np.abs(got - sums) <= 1e-9 * np.abs(sums)), float(np.max(np.abs(got - sums) / np.abs(sums)))
    if with_i:
        assert np.array_equal(out.column("count(v)").to_numpy()[order], counts)
        assert np.array_equal(out.column("min(i)").to_numpy()[order], mins) and np.array_equal(out.column("max(i)").to_numpy()[order], maxs)


@pytest.mark.parametrize("rows", ROWS, ids=["T+%d" % (r - T) for r in ROWS])
def test_blocks_whose_sub_steps_select_nothing(rows):
    for sort in (True, False):
        t = Explicit(rows, sort)
        try:
            run(t, with_i=False, deterministic=not sort)
            run(t, with_i=True, deterministic=not sort)
            assert t.rb.scan_cache_bytes == values_slot(rows, 1) + values_slot(rows, 2)
        finally:
            t.rb.close()
