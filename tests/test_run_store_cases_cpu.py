"""tests/run_store_cases.py held to account without a device: its restatement of the run kernels' per-wave state (wave_model) on claims
worked out by hand, the families to claiming every event of that state, every format boundary and both sides of the segment limit, every
launch to fitting the segment push_hash sizes for it, the numpy reference to the oracle's OrderedAggregate (tests/ordered_oracle.py) on every
case of at most 5 000 rows and to the reference's own vectors (tests/golden/ordered_cases.py), and the data to the properties the cases
rely on."""
import numpy as np
import pyarrow as pa
import pytest

from tests import run_store_cases as R
from tests.golden.ordered_cases import ORDERED_CASES
from tests.ordered_oracle import COUNT, MAX, MIN, SUM, OrderedAggregate

SMALL = [c for c in R.all_cases() if c.rows() <= 5000]


def case(id):
    return next(c for c in R.all_cases() if c.id == id)


# ---- the state machine, worked by hand -------------------------------------------------------------------------------------------------------
def test_k_256_by_hand():
    """k = 256, 34 tiles, grid 1: wave w sees its 256 rows of every tile, 256 runs each, narrow records (CAP = 256).
    tile 0: (rb, rp, ps) = (0, 4096, 4096): rp + 256 > 4096 — the first chunk (not an event: every test takes it); rp = 256, 256 runs staged.
    tile 1: (256 − 0) + 256 > 256: the stage is full with 256 pending → flush_stage_full; ps = 256, rp = 512. … every tile flushes the one before.
    tile 16: rp = 4096 = the chunk, exactly: rp + 256 > 4096 with rp = 4096 → switch_exact_fit, the 256 runs of tile 15 still staged →
    switch_with_runs_pending. tile 32: the same. After tile 33 the 256 runs of that tile wait → final_flush_pending. All 64 lanes are active
    and lane 0 writes throughout; nothing is direct (narrow)."""
    c = case("per_tile_k-256_runs_over_34_tiles")
    assert c.events(1) == {"flush_stage_full", "switch_exact_fit", "switch_with_runs_pending", "final_flush_pending"}
    (_, r), = c.launches(1)
    assert r["runs"] == 34 * 1024 and r["chunks"] == 4 * 3 and set(r["n_w"]) == {256}
    # grid 2: a wave sees 17 tiles — one change of chunks, at its 17th
    (_, r2), = c.launches(2)
    assert c.events(2) == c.events(1) and r2["chunks"] == 8 * 2
    # the default grid: one tile per wave — what every test before these reached
    assert c.events(0) == {"final_flush_pending"}


def test_k_255_by_hand():
    """k = 255: after 16 tiles rp = 16 · 255 = 4 080; tile 16: 4 080 + 255 > 4 096 → the chunk changes with 16 slots left unused →
    switch_abandoning (255 runs pending: switch_with_runs_pending); tile 1 already has (255 − 0) + 255 > 256 → flush_stage_full."""
    c = case("per_tile_k-255_runs_over_34_tiles_joined")
    assert c.events(1) == {"flush_stage_full", "switch_abandoning", "switch_with_runs_pending", "final_flush_pending"}
    (_, r), = c.launches(1)
    assert r["chunks"] == 4 * 3 and set(r["n_w"]) == {255}
    # joined: wave tiles 2 m and 2 m + 1 share a key across their edge — 34 · 4 · 255 runs, 34 · 2 fewer groups
    keys, _, _ = c.want("count")
    assert len(keys[0]) == 34 * 4 * 255 - 34 * 2


def test_emptied_lanes_by_hand():
    """4 tiles, every wave tile 128 runs of 2 rows, grid 1, wave 0: tile 0 stages 128 runs, tile 1 128 more (256 = CAP, no flush yet: 256 > 256 is
    false); tile 2 has its first 5 lanes emptied by the filter: lanes 5 … 63 hold 59 · 2 = 118 runs, (256 − 0) + 118 > 256 → the stage leaves,
    copied by 59 lanes → flush_stage_full + flush_with_fewer_than_64_active_lanes, and lane 5 is the first active one → writer_lane_not_0."""
    c = case("filter-first_5_lanes_of_a_wave_tile_emptied")
    assert c.events(1) == {"flush_stage_full", "flush_with_fewer_than_64_active_lanes", "writer_lane_not_0", "final_flush_pending"}
    (_, r), = c.launches(1)
    assert r["n_w"][2 * 4 + 0] == 118 and r["runs"] == 16 * 128 - 10
    # at the default grid the wave of that tile has nothing staged: lane 5 still writes the state and the directory entry
    assert c.events(0) == {"writer_lane_not_0", "final_flush_pending"}
    # 63 lanes emptied: lane 63 alone copies a full stage out
    assert case("filter-first_63_lanes_of_a_wave_tile_emptied").launches(1)[0][1]["n_w"][8] == 2


def test_run_ends_by_hand():
    """One wave, keys a a a a | a b b b | (lane 2 dropped) | b b c c: lane 0 hands its run to lane 1 (row 3 does not end one), row 4 ends a,
    row 7 ends b — lane 2 has left the tile, so the run is cut there — and b goes on in lane 3: rows 13 and 15 end runs."""
    sel = np.ones(16, bool)
    sel[8:12] = False
    ends, active = R.run_ends(sel, np.array([0, 0, 0, 0, 0, 1, 1, 1, 1, 1, 1, 1, 1, 1, 2, 2]))
    assert np.flatnonzero(ends).tolist() == [4, 7, 13, 15] and active[:4].tolist() == [True, True, False, True]
    # middle rows dropped inside a lane: rows 0 and 3 are not adjacent, two runs of one key
    ends, _ = R.run_ends(np.array([True, False, False, True]), np.zeros(4, np.int64))
    assert np.flatnonzero(ends).tolist() == [0, 3]
    # lane 63 never hands on to lane 0 of the next wave
    ends, _ = R.run_ends(np.ones(512, bool), np.zeros(512, np.int64))
    assert np.flatnonzero(ends).tolist() == [255, 511]


def test_stage_capacities():
    assert [R.stage_cap(0, 3), R.stage_cap(1, 3), R.stage_cap(2, 3), R.stage_cap(2, 13), R.stage_cap(2, 40)] == [256, 153, 256, 128, 64]


# ---- coverage ------------------------------------------------------------------------------------------------------------------------------
def test_every_event_is_claimed_by_a_case_the_gpu_module_runs():
    seen = {}
    for c in R.all_cases(R.SCAN_FAMILIES):
        for g in c.grids:
            for e in c.events(g) or ():
                seen.setdefault(e, []).append((c.id, g))
    assert set(seen) == set(R.EVENTS), sorted(set(R.EVENTS) - set(seen))
    # … and beyond the first chunk only where a grid is forced: what the default grid reaches is what the suite reached before
    for e in ("switch_exact_fit", "switch_abandoning", "switch_with_runs_pending", "direct_and_switch_same_tile", "flush_stage_full", "wave_tile_without_runs"):
        assert all(g != 0 for _, g in seen[e]), e
    for c in R.all_cases():
        for name in c.claims:
            if name in R.EVENTS:
                assert name in c.events(1), (c.id, name)


def test_every_format_boundary_and_both_sides_of_the_segment_limit():
    fmt = {c.id: c.formats for c in R.cases("formats")}
    assert fmt["formats-largest_column_of_254_values"] == [0] and fmt["formats-largest_column_of_255_values"] == [1]
    assert fmt["formats-largest_column_of_65534_values"] == [1] and fmt["formats-largest_column_of_65535_values"] == [2]
    assert fmt["formats-32_group_columns"] == [0] and fmt["formats-33_group_columns"] == [2]
    assert fmt["formats-narrow_then_medium_then_wide_segments_in_key_order"] == [0, 1, 2]
    for c in R.all_cases():
        for name in c.claims:
            if name.startswith("format_"):
                assert int(name[7:]) in c.formats, (c.id, name, c.formats)
    at, beyond = [c for c in R.cases("segments") if "segments_at_limit" in c.claims], [c for c in R.cases("segments") if "segments_beyond_limit" in c.claims]
    assert len(at) == 2 and len(beyond) == 2
    for c in at:
        assert not c.leaves_the_path and c.formats == [0] * R.MAX_SEGMENTS
    host, resident = beyond
    assert host.leaves_the_path and host.formats == [0] * R.MAX_SEGMENTS + [None]   # 64 segments, the 65th push leaves the path mid-scan
    assert resident.leaves_the_path and resident.formats == [None] * 65            # 65 records in one call never enter it
    assert {len(c.records) for c in at} == {64} and {len(c.records) for c in beyond} == {65}


def test_run_counts_and_chunks_are_what_the_cases_say():
    for c in R.all_cases(("run_counts", "translate")):
        for name in c.claims:
            if name.startswith("runs="):
                assert c.runs(0) == int(name[5:]), (c.id, c.runs(0))
            if name.startswith("source_runs="):
                src = R.Case("src", "translate", c.source)
                assert src.runs(0) == src.rows() == int(name[12:]) and src.formats == [0]
            if name == "two_chunks":  # the two runs of the one group lie in the chunks of two different waves
                e = int(c.id.rsplit("_", 1)[1])
                (_, r), = c.launches(0)
                a, b = r["chunk_of"][(e - 1) // 256], r["chunk_of"][e // 256]
                assert a is not None and b is not None and a != b, (c.id, a, b)
                assert c.runs(0) - len(c.want("count")[2]) == 1
    assert sorted({c.runs(0) for c in R.cases("run_counts") if c.id.endswith("_runs")}) == list(R.RUN_COUNTS)
    c = case("run_counts-a_one_run_group_between_many_run_groups")
    assert c.want("count")[2].tolist() == [600, 1, 700, 1, 1, 300]  # groups of 3, 1, 4, 1, 1 and 2 runs
    c = case("run_counts-a_group_in_two_segments")
    assert [r["runs"] for _, r in c.launches(0)] == [300, 725] and len(c.want("count")[2]) == 1024
    m, = R.cases("many_runs")
    assert m.rows() == 1024 * 1024 + 1 > 1024 * 1024  # more than 1 024 scan blocks of 1 024 runs: scan_u64_single_kernel's second round


def test_every_launch_fits_the_segment_push_hash_sizes_for_it():
    """A wave that changes chunks takes the next one from the segment's cursor: the chunks a launch takes must be within what push_hash
    allocated, or the kernel writes out of bounds. (Checked here, before any of this runs on a device.)"""
    for c in R.all_cases():
        if c.family == "many_runs":
            continue
        for g in c.grids:
            for i, r in c.launches(g):
                if r["chunks"] is not None:
                    assert r["chunks"] <= R.segment_chunks(c.records[i].num_rows, g), (c.id, g, i)


# ---- the reference -------------------------------------------------------------------------------------------------------------------------
FUNC = {"sum_i": SUM, "sum_f": SUM, "min": MIN, "max": MAX, "count": COUNT}


def oracle_rows(c, agg):
    col = "f" if agg in ("sum_f", "max") else "v"
    o = OrderedAggregate(FUNC[agg], col, [(n, False) for n in c.names], final_stage=False)
    for b in c.all_records():
        keep = np.flatnonzero(R.selected(b, c.filt))
        if len(keep) == 0:
            continue
        b = b.take(pa.array(keep))
        rec = {n: b.column(b.schema.get_field_index(n)).dictionary_decode().to_pylist() for n in c.names if b.schema.get_field_index(n) >= 0}
        rec[col] = b.column(b.schema.get_field_index(col)).to_pylist()
        o.callback(rec)
    out = o.finish()
    if out is None:
        return []
    idx = [out["columns"].index(n) for n in c.names] + [len(out["columns"]) - 1]
    return [tuple(r[i] for i in idx) for r in out["rows"]]


def folded(rows, agg):
    red = {"sum_i": lambda a, b: (a + b + 2 ** 63) % 2 ** 64 - 2 ** 63, "sum_f": lambda a, b: a + b, "count": lambda a, b: a + b, "min": min, "max": max}[agg]
    out = {}
    for r in rows:
        out[r[:-1]] = red(out[r[:-1]], r[-1]) if r[:-1] in out else r[-1]
    return out


@pytest.mark.parametrize("c", SMALL, ids=[c.id for c in SMALL])
def test_the_numpy_reference_is_the_oracle(c):
    """Row for row, in order, wherever no key is NULL. Rows with a NULL key: the reference's merge stops comparing at the first column that is
    NULL on both sides (merge.go:91-98), so such a group can come out in several rows, not in key order — the device and the numpy reference
    bring it out whole: those rows are folded per key before they are compared. (Python's int sums do not wrap: folded modulo 2^64.)"""
    for agg in c.aggs:
        if c.fsum:
            continue  # (general floats: the oracle's sum has an order of its own; test_fsum_bound_is_not_empty covers the case)
        want, got = c.want_rows(agg), oracle_rows(c, agg)
        if agg == "sum_i":
            got = [r[:-1] + ((r[-1] + 2 ** 63) % 2 ** 64 - 2 ** 63,) for r in got]
        whole = lambda rows: [r for r in rows if None not in r[:-1]]  # noqa: E731
        assert whole(got) == whole(want), (c.id, agg)
        assert folded(got, agg) == folded(want, agg), (c.id, agg)
        assert len(folded(want, agg)) == len(want)  # the reference's own rows are whole groups


def test_the_numpy_reference_on_the_reference_vectors():
    for case_ in ORDERED_CASES:
        recs = []
        for groups, vals in case_["records"]:
            arrays, names = [], []
            for i, col in enumerate(groups):
                if col:
                    arrays.append(pa.array([g.encode() if g else None for g in col], type=pa.binary()).dictionary_encode()); names.append("labels.g%d" % i)
            arrays += [pa.array(vals, type=pa.int64()), pa.array([float(v) for v in vals])]
            recs.append(pa.RecordBatch.from_arrays(arrays, names=names + ["v", "f"]))
        names = ["labels.g%d" % i for i in range(case_["ncols"])]
        want = [tuple(x.encode() if isinstance(x, str) else x for x in r) for r in case_["expected"]]
        assert R.reference_rows(recs, names, "sum_i") == want, case_["cite"]
        assert [r[:-1] + (int(r[-1]),) for r in R.reference_rows(recs, names, "sum_f")] == want


def test_fsum_bound_is_not_empty():
    c = case("extremes-general_floats_against_fsum")
    exact, plain = c.want("sum_f")[2], R.reference(c.records, c.names, "sum_f")[2]
    bound = R.fsum_bounds(c.records, c.names)
    assert np.all(np.abs(plain - exact) <= bound) and np.any(plain != exact)  # numpy's own sum: within the bound, and not the same number
    assert np.all(bound[c.want("count")[2] > 1] > 0) and np.all(bound < 1e-3 * np.maximum(np.abs(exact), 1e-300) + 1e-3)


# ---- the data ------------------------------------------------------------------------------------------------------------------------------
def descents(c):
    """The pairs of adjacent selected rows, over all records of the FIRST plan in push order, whose keys are out of order"""
    ranks, shown = R.key_ranks(c.records, c.names)
    sel = np.concatenate([R.selected(b, c.filt) for b in c.records])
    code = R.group_codes(ranks, shown)[sel]
    return int((np.diff(code) < 0).sum())


def test_data_properties():
    for c in R.all_cases():
        if c.family == "many_runs":
            continue
        # in order, or — family violation — exactly ONE pair out of order
        if c.family == "violation":
            assert descents(c) == (0 if c.in_order else 1), c.id
        elif c.family != "translate":
            assert c.in_order and descents(c) == 0, c.id
        for b in c.all_records():
            for n in c.names:
                i = b.schema.get_field_index(n)
                if i >= 0:
                    d = b.column(i).dictionary.to_pylist()
                    assert len(set(d)) == len(d)
                    if c.family != "translate" and len(d) > 1:
                        assert d == sorted(d, reverse=True), (c.id, n)  # descending: an index, and the key id made of it, is no rank
    # per_tile_k: every wave tile ends exactly k runs, at every grid
    for c in R.cases("per_tile_k"):
        k = int(c.id.split("-")[1].split("_")[0])
        for g in c.grids:
            (_, r), = c.launches(g)
            assert set(r["n_w"].tolist()) == {k}, c.id
    # translate: the dictionaries of the two plans differ in order and content; the source's keys interleave with the destination's
    for c in R.cases("translate"):
        d0, s0 = c.records[0].column(1).dictionary.to_pylist(), c.source[0].column(1).dictionary.to_pylist()
        assert set(d0) != set(s0) and d0 != sorted(d0) and s0 != sorted(s0)
        assert len(c.want("count")[2]) < c.runs(0) + c.source[0].num_rows  # … and share groups with them
    # filter: the emptied lanes are lanes of the tile whose runs make the stage flush; the removed record is all of one record
    c = case("filter-all_of_a_record_removed")
    assert [int(R.selected(b, c.filt).sum()) for b in c.records] == [1000, 0, 972]
    c = case("filter-middle_rows_of_a_lane_removed")
    assert c.runs(0) == case("per_tile_k-3_runs_over_172_tiles_joined").launches(1)[0][1]["n_w"][:12].sum() + 3  # three lanes' runs cut in two
    # extremes: the sums wrap, a group is all NULL, nothing is NaN
    c = case("extremes-int64_limits_and_special_floats")
    v = c.records[0].column(3).to_numpy()
    assert (v == R.I64_MAX).sum() > 2 and (v == R.I64_MIN).sum() > 2 and not np.isnan(c.records[0].column(4).to_numpy()).any()
    assert np.isinf(c.want("sum_f")[2]).sum() == 4 and not np.isnan(c.want("sum_f")[2]).any()
    c = case("extremes-nulls_in_the_aggregated_column")
    cnt, s = c.want("count")[2], c.want("sum_i")[2]
    assert s[12] == 0 and cnt[12] > 0 and c.want("min")[2][12] == 0 and c.records[0].column(3).null_count > 100
    # many_runs: three narrow columns, every row its own key, in order (checked on the indices: the dictionary is descending)
    m, = R.cases("many_runs")
    b = m.records[0]
    idx = [101 - b.column(i).indices.to_numpy().astype(np.int64) for i in range(3)]
    code = (idx[0] * 102 + idx[1]) * 102 + idx[2]
    assert np.array_equal(code, np.arange(R.MANY_RUNS)) and m.formats == [0]
