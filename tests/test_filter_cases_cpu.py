"""The case builders of tests/filter_cases.py, checked on the host: the patterns select what their names say, the NULL patterns are
what the device tests rely on, and the packed launch stays small."""
import numpy as np
import pyarrow as pa
import pytest

from tests import filter_cases as fc


@pytest.mark.parametrize("name", fc.SELECTIONS)
def test_selected_counts_in_closed_form(name):
    for n in fc.ROWS + [5000, fc.LEAD_ROWS]:
        mask = fc.selection(name, n)
        assert mask.dtype == bool and len(mask) == n
        want = fc.selected_count(name, n)
        if want is not None:
            assert int(mask.sum()) == want, (name, n)
        else:  # a fixed seed: the same mask every time, within six standard deviations of its mean
            p = fc.BERNOULLI[name]
            assert np.array_equal(mask, fc.selection(name, n))
            assert abs(int(mask.sum()) - p * n) <= 6 * np.sqrt(n * p * (1 - p)) + 1, (name, n)
    for lead in fc.LEADS:
        assert int(fc.selection("runs_65_63", fc.LEAD_ROWS, lead).sum()) == fc.selected_count("runs_65_63", fc.LEAD_ROWS, lead)


def test_patterns_reach_the_edges_they_are_named_for():
    n = 6145  # three tiles and one row
    assert np.flatnonzero(fc.selection("tile_first_rows", n)).tolist() == [0, 2048, 4096, 6144]
    assert np.flatnonzero(fc.selection("tile_last_rows", n)).tolist() == [2047, 4095, 6143, 6144]
    assert np.flatnonzero(~fc.selection("all_but_one_per_tile", n)).tolist() == [1000, 3048, 5096]
    alt = fc.selection("alternate_tiles", n)
    assert alt[:2048].all() and not alt[2048:4096].any() and alt[4096:6144].all() and not alt[6144]
    runs = fc.selection("runs_65_63", 8193)
    assert runs[:65].all() and not runs[65:128].any() and runs[128:193].all()
    # tiles and steps that select nothing, in the same record as ones that do
    for step in fc.STEPS:
        per_step = np.add.reduceat(fc.selection("tile_first_rows", 8193).astype(int), np.arange(0, 8193, step))
        assert (per_step == 0).any() and (per_step > 0).any()
    # the last partial 32-row word and the last partial group of a record
    assert {n % fc.WORD for n in fc.ROWS} >= {0, 1, 31} and {n % fc.GROUP for n in fc.ROWS} >= {0, 1, 63}
    # a share of four tiles whose last tiles lie past the record's end
    assert {-(-n // fc.TILE) % fc.SHARE_TILES for n in fc.ROWS} == {0, 1, 2, 3}


def test_null_where_selected_and_where_not_partition_the_rows():
    for c in fc.grid():
        a = fc.validity("null_where_selected", c.rows, c.mask)
        b = fc.validity("null_where_unselected", c.rows, c.mask)
        assert np.array_equal(~a, c.mask) and np.array_equal(~b, ~c.mask)
        assert np.array_equal(a ^ b, np.ones(c.rows, dtype=bool))  # every row is NULL in exactly one of the two


def test_validity_patterns():
    for c in fc.grid():
        one = fc.validity("one_null_unselected", c.rows, c.mask)
        if c.mask.all():
            assert one is None
        else:
            assert int((~one).sum()) == 1 and not c.mask[~one].any()  # a bitmap, and no NULL among the selected rows
        assert fc.validity("no_bitmap", c.rows, c.mask) is None
        assert not fc.validity("all_null", c.rows, c.mask).any()
        assert np.flatnonzero(~fc.validity("group_last_rows", c.rows, c.mask)).tolist() == list(range(63, c.rows, 64))
    v = fc.validity("bernoulli_3", 8193, fc.selection("all", 8193))
    assert 150 < int((~v).sum()) < 350


def test_runs_walk_the_output_bit_offset_through_all_64_shifts():
    """The validity bits of a step are shifted by the output's bit offset at the step's start. Runs of 65 / 63 alone cannot move it off
    the multiples of 4 — a step of 512 rows holds four whole runs, 260 rows —; behind 0 … 63 selected rows they reach every offset, at
    both step sizes, in records of at most 8 193 rows."""
    assert fc.LEAD_ROWS <= 8193
    for step in fc.STEPS:
        alone = fc.step_start_offsets(fc.selection("runs_65_63", 8193), step)
        assert alone <= set(range(0, 64, 4))
        seen = set()
        for c in fc.grid():
            if c.selection == "runs_65_63":
                seen |= fc.step_start_offsets(c.mask, step)
        assert seen == set(range(64)), (step, sorted(set(range(64)) - seen))


def test_the_packed_launch_stays_small():
    cases = fc.grid()
    assert len(cases) == len(fc.ROWS) * len(fc.SELECTIONS) + len(fc.LEADS) - 1
    assert sum(c.rows for c in cases) < 1_000_000
    assert max(c.rows for c in cases) == 8193


def test_records_follow_the_layout():
    n = 4097
    mask = fc.selection("bernoulli_50", n)
    valid = fc.validity("bernoulli_3", n, mask)
    rec = fc.record(3, mask, valid)
    assert rec.schema.names == fc.COLUMNS and rec.num_rows == n
    for name in ("sel", "selk", "k", "f"):
        assert rec.column(name).null_count == 0
    assert np.array_equal(fc.mask_of(rec, "sel"), mask) and np.array_equal(fc.mask_of(rec, "selk"), mask)
    assert np.array_equal(fc.mask_of(rec, "seln"), mask & ~fc.SELN_NULL(n))
    for name in fc.NULLABLE_COLUMNS:
        assert np.array_equal(np.asarray(rec.column(name).is_valid()), valid), name
    r = np.arange(n)
    assert rec.column("i").fill_null(-1).to_numpy()[valid].tolist() == (3 * 2**20 + r[valid]).tolist()
    assert rec.column("f").to_numpy().tolist() == (3 * 2**20 + r + 0.5).tolist()
    assert rec.column("plain").type == pa.binary() and rec.column("flag").type == pa.bool_()
    assert rec.column("plain")[int(np.flatnonzero(valid)[5])].as_py() == b"p%d" % (int(np.flatnonzero(valid)[5]) % 97)
    assert rec.column("d").type == fc.DICT_TYPE and len(rec.column("d").dictionary) == 251
    no_bitmap = fc.record(0, mask, None)
    assert all(no_bitmap.column(c).null_count == 0 for c in fc.NULLABLE_COLUMNS)


def test_threshold_counts_sit_on_the_repack_boundary():
    for n in (5000, 8193):
        none, below, exactly, above, everything = fc.threshold_counts(n)
        assert (none, everything) == (0, n) and below + 1 == exactly == above - 1
        assert float(below) < 0.4 * float(n) <= float(exactly)  # (the library's own comparison, in doubles)
        for count in fc.threshold_counts(n):
            m = fc.spread_mask(n, count)
            assert int(m.sum()) == count


def test_the_oracle_and_pyarrow_filter_alike():
    """The two references of the device tests agree on records of the layout (NULLs in the predicate column included)."""
    from frostdb_amd.logicalplan import Col
    from oracle import OraclePlan
    from tests.util import arrow_to_pydict
    for n, s, v in [(6145, "bernoulli_50", "bernoulli_3"), (2049, "runs_65_63", "null_where_selected"), (65, "group_edges", "group_last_rows")]:
        mask = fc.selection(s, n)
        rec = fc.record(1, mask, fc.validity(v, n, mask))
        for column in ("sel", "selk", "seln"):
            o = OraclePlan((Col("selk") == "y") if column == "selk" else (Col(column) > 0))
            out, idx = o.filter(rec)
            try:
                assert np.array_equal(np.asarray(idx), np.flatnonzero(fc.mask_of(rec, column)))
                got = out.to_pydict()
            finally:
                out.close()
                o.close()
            assert got == arrow_to_pydict(rec.filter(pa.array(fc.mask_of(rec, column))))
