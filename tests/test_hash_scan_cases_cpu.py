"""The cases of tests/hash_scan_cases.py are what they say: the numpy reference that supplies every expected row equals the oracle on
every case, the families together claim every side of every branch of the hash scan, the table's growth and its Finish, four claims
worked out by hand pin the restatement, and the fdb_hash_kernel sources of the column counts the cases use compile for gfx950 without
scratch. No GPU is touched.

The claims are a Python RESTATEMENT of the host arithmetic and can drift from the C++ they restate:
  Plan::hash_layout (fdb_hash.cpp:36-61), Plan::hash_reserve (:71-96), push_hash (:246-453: the key-id LUTs :293-317, `canonical`
  :306-308, the chunk walk :381-450), the transport widths of finish_columns_hash (:555-563, :709-718) and its slices (:549-553), the
  mode decision of Plan::push_batches (fdb_plan.cpp:1418-1427), resolve_batch's column order (:1203-1237) and the quads of
  HashGen::emit_tuple_stores (fdb_jitgen.cpp). Whoever changes how those shape a push or a Finish changes hash_scan_cases.py with them."""
import os
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

from tests import hash_scan_cases as S
from tests.jit_corpus import HASH_CASES
from tests.test_jit_sources_cpu import HIPCC, ROOT, jit_dump  # noqa: F401  (the fixture that builds tools/jit_dump.cpp)


def by_id(id):
    return next(c for c in S.cases(id.split("-")[0]) if c.id == id)


def claims(families=S.FAMILIES):
    """(case, push claim | None, finish claim | None): one entry per push and one per Finish"""
    out = []
    for f in families:
        for c in S.cases(f):
            out += [(c, p, None) for p in c.pushes]
            out.append((c, None, c.finish))
    return out


def push(hit):
    return lambda c, p, f: p is not None and hit(c, p)


def fin(hit):
    return lambda c, p, f: f is not None and hit(c, f)


def rows_left(p):
    """rows of the record's last tile, 1 … 1 024"""
    r0, r1 = p["chunks"][-1]
    return (r1 - r0 - 1) % 1024 + 1


COVERED = [
    # 4 rows per lane, 256 per wave, 1 024 per tile
    ("a last lane with 1 row", push(lambda c, p: rows_left(p) % 4 == 1)),
    ("a last lane with 3 rows", push(lambda c, p: rows_left(p) % 4 == 3)),
    ("a last lane that is full", push(lambda c, p: rows_left(p) % 4 == 0)),
    ("a record of one full wave", push(lambda c, p: p["rows"] == 256)),
    ("a record one row short of a wave", push(lambda c, p: p["rows"] == 255)),
    ("a record one row past a wave", push(lambda c, p: p["rows"] == 257)),
    ("a record of one full tile", push(lambda c, p: p["rows"] == 1024)),
    ("a record one row short of a tile", push(lambda c, p: p["rows"] == 1023)),
    ("a record one row past a tile", push(lambda c, p: p["rows"] == 1025)),
    ("a record of more than four tiles", push(lambda c, p: p["rows"] == 4097)),
    ("a record that starts where another ended, off a multiple of 4", push(lambda c, p: len(c.records) > 1 and c.records[0].num_rows % 4 != 0)),
    ("a filter that selects nothing", push(lambda c, p: c.filt is not None and c.selected == 0)),
    ("a filter that selects every row", push(lambda c, p: c.family == "rows" and c.filt is not None and c.selected == 2049 - 6)),
    ("a filter that empties whole lanes and waves", push(lambda c, p: c.id == "rows-filter_selects_nothing_in_whole_lanes_and_waves")),
    # run folding
    ("runs given by construction", push(lambda c, p: c.counts is not None and not c.exact)),
    ("runs under exact sums: nothing folds", push(lambda c, p: c.counts is not None and c.exact)),
    ("a run of 256 rows", push(lambda c, p: c.counts is not None and 256 in c.counts.values())),
    ("a run of 1 500 rows, the whole record", push(lambda c, p: c.counts is not None and 1500 in c.counts.values() and p["rows"] == 1500)),
    ("a run that loses rows to the filter", push(lambda c, p: c.counts is not None and c.selected < sum(r.num_rows for r in c.records))),
    ("a run across two records", push(lambda c, p: c.counts is not None and len(c.records) == 2)),
    ("NULL and 0 in one group", push(lambda c, p: c.null_or_zero)),
    # columns in groups of 8
    ("fewer than 8 columns", push(lambda c, p: 0 < p["n_cols"] < 8)),
    ("8 columns", push(lambda c, p: p["n_cols"] == 8)),
    ("9 columns", push(lambda c, p: p["n_cols"] == 9)),
    ("16 columns", push(lambda c, p: p["n_cols"] == 16)),
    ("17 columns", push(lambda c, p: p["n_cols"] == 17)),
    ("64 columns, specialised", push(lambda c, p: p["n_cols"] == 64 and "jit" in c.variants)),
    ("64 columns, interpreted", push(lambda c, p: p["n_cols"] == 64 and "interp" in c.variants)),
    ("no quad", push(lambda c, p: p["canonical"] and p["quads"] == [])),
    ("a last group of 8 with one quad and a rest", push(lambda c, p: p["canonical"] and p["n_cols"] % 8 in (5, 6, 7) and p["quads"] and p["quads"][-1] == p["n_cols"] // 8 * 8)),
    ("dictionary columns behind the last quad", push(lambda c, p: p["canonical"] and p["quads"] and p["quads"][-1] + 4 < p["n_cols"])),
    ("a record that is not canonical", push(lambda c, p: p["canonical"] is False)),
    ("not canonical for lacking columns", push(lambda c, p: p["canonical"] is False and p["n_cols"] < len(c.names))),
    ("not canonical for its field order", push(lambda c, p: p["canonical"] is False and p["n_cols"] == len(c.names))),
    ("an int64 key at word 4", push(lambda c, p: 4 in p["wide_words"])),
    ("an int64 key at word 5", push(lambda c, p: 5 in p["wide_words"])),
    ("an int64 key at word 6", push(lambda c, p: 6 in p["wide_words"])),
    ("an int64 key at word 7", push(lambda c, p: 7 in p["wide_words"])),
    ("vmask bit 31", push(lambda c, p: 31 in p["vmask_bits"])),
    ("vmask bit 32", push(lambda c, p: 32 in p["vmask_bits"])),
    ("vmask bit 63", push(lambda c, p: 63 in p["vmask_bits"])),
    ("two wide keys", push(lambda c, p: len(p["wide_words"]) == 2)),
    ("a computed key", push(lambda c, p: bool(c.computed))),
    ("key words grow, 16 -> 20", push(lambda c, p: p["layout_rehash"] and (p["kw_before"], p["kw_after"]) == (16, 20))),
    ("a new column on the tuples' padding", push(lambda c, p: p["layout_rehash"] and p["kw_before"] == p["kw_after"] and p["used_after"] > p["used_before"])),
    # key-id LUTs
    ("an identity LUT", push(lambda c, p: "identity" in p["lut"])),
    ("a LUT in LDS", push(lambda c, p: "lds" in p["lut"])),
    ("a LUT in global memory", push(lambda c, p: "global" in p["lut"])),
    ("a LUT of 8 192 bytes in LDS", push(lambda c, p: c.id.startswith("luts-2048") and p["lut"] == ["lds", "lds"])),
    ("a LUT of 8 196 bytes in global memory", push(lambda c, p: c.id.startswith("luts-2049") and p["lut"] == ["global", "global"])),
    ("LDS and global LUTs in one record, by the 60 KiB total", push(lambda c, p: p["lut"] == ["lds"] * 7 + ["global"])),
    ("a filter leaf beside key-id LUTs", push(lambda c, p: c.family == "luts" and c.filt is not None and "lds" in p["lut"])),
    # chunks and growth
    ("a push of one chunk", push(lambda c, p: len(p["chunks"]) == 1)),
    ("a push of two chunks", push(lambda c, p: len(p["chunks"]) == 2)),
    ("a chunk boundary inside a record, at 2^20", push(lambda c, p: len(p["chunks"]) == 2 and p["chunks"][0] == (0, 1 << 20))),
    ("a second chunk of more than one tile", push(lambda c, p: len(p["chunks"]) == 2 and p["chunks"][1][1] - p["chunks"][1][0] > 1024)),
    ("a table at load 0.5", push(lambda c, p: p["cap_after"] == 65536 and c.groups_after[0] == 32768)),
    ("the bound refreshed and room found", push(lambda c, p: p["refreshed"] and not p["rehash"])),
    ("the bound refreshed and the table re-hashed, two steps at once", push(lambda c, p: p["refreshed"] and p["rehash"] and p["cap_after"] == 262144)),
    ("a re-hash after a column was added", push(lambda c, p: p["rehash"] and p["layout_rehash"])),
    ("a re-hash under exact sums", push(lambda c, p: p["rehash"] and c.exact)),
    ("a table that never grows", push(lambda c, p: p["cap_after"] == 65536 and not p["rehash"])),
    # Finish
    ("1 group", fin(lambda c, f: f["groups"] == 1)),
    ("63 groups", fin(lambda c, f: f["groups"] == 63)),
    ("64 groups", fin(lambda c, f: f["groups"] == 64)),
    ("65 groups", fin(lambda c, f: f["groups"] == 65)),
    ("127 groups", fin(lambda c, f: f["groups"] == 127)),
    ("128 groups", fin(lambda c, f: f["groups"] == 128)),
    ("129 groups", fin(lambda c, f: f["groups"] == 129)),
    ("4 097 groups", fin(lambda c, f: f["groups"] == 4097)),
    ("no group at all", fin(lambda c, f: f["groups"] == 0)),
    ("a resident Finish", fin(lambda c, f: "resident" in c.through)),
    ("partial keys and states", fin(lambda c, f: "partial" in c.through)),
    ("2 slices", fin(lambda c, f: f["slices"] == 2)),
    ("3 slices, the last one short", fin(lambda c, f: f["slices"] == 3 and f["groups"] % f["slice_rows"] != 0)),
    ("1 slice of exactly 64 rows", fin(lambda c, f: f["slices"] == 1 and f["groups"] == 64 and "FDB_FINISH_SLICE_SHIFT" in c.env)),
    ("width -2 at 4 entries and -4 at 5", fin(lambda c, f: f["width_before"][:2] == [-2, -4])),
    ("width -4 at 16 entries and 1 at 17", fin(lambda c, f: f["width_before"][2:4] == [-4, 1])),
    ("width 1 at 256 entries and 2 at 257", fin(lambda c, f: f["width_before"][4:6] == [1, 2])),
    ("width 4 at 65 537 entries", fin(lambda c, f: 4 in f["width_before"])),
    ("present ids: 2 -> -2 at 4 and -4 at 5", fin(lambda c, f: f["width_before"][:2] == [2, 2] and f["width_after"][:2] == [-2, -4])),
    ("present ids: 2 -> -4 at 16 and 1 at 17", fin(lambda c, f: f["width_before"][2:4] == [2, 2] and f["width_after"][2:4] == [-4, 1])),
    ("present ids: 2 -> 1 at 256, stays 2 at 257", fin(lambda c, f: f["width_before"][4:6] == [2, 2] and f["width_after"][4:6] == [1, 2])),
    ("present ids: nothing gained", fin(lambda c, f: "FDB_PRESENT_IDS_MIN_BYTES" in c.env and f["width_before"] == f["width_after"] and 1 in f["width_before"])),
    ("present ids switched off", fin(lambda c, f: "FDB_NO_PRESENT_IDS" in c.env and f["width_before"] == f["width_after"] == [2] * 6 + [8])),
    ("present ids: a column of NULLs only", fin(lambda c, f: f["bitmaps"] == ["labels.l01"] and f["width_after"][1] == -2)),
    ("a bitmap shipped beside one that is not", fin(lambda c, f: f["bitmaps"] == ["labels.l00"] and len(c.names) == 3)),
    ("the one NULL group on row 0", fin(lambda c, f: f.get("null_row") == 0)),
    ("the one NULL group on row 63, the last of a validity word", fin(lambda c, f: f.get("null_row") == 63 and f["groups"] > 64)),
    ("the one NULL group on row 64, the first of the next word", fin(lambda c, f: f.get("null_row") == 64 and f["groups"] > 65)),
    ("the one NULL group on the last row", fin(lambda c, f: f.get("null_row") == f["groups"] - 1 and f["groups"] in (65, 130))),
    ("no bitmap shipped", fin(lambda c, f: f["groups"] > 0 and f["bitmaps"] == [])),
]
# which family a value comes from: taking the family out of the generator must leave it uncovered
FAMILY_OWNS = {
    "rows": "a record one row past a tile",
    "runs": "a run of 256 rows",
    "columns": "vmask bit 63",
    "luts": "a LUT of 8 196 bytes in global memory",
    "growth": "a chunk boundary inside a record, at 2^20",
    "finish": "3 slices, the last one short",
}


def uncovered(families):
    found = claims(families)
    return [name for name, hit in COVERED if not any(hit(*x) for x in found)]


def test_every_branch_is_claimed_by_some_case():
    missing = uncovered(S.FAMILIES)
    assert not missing, "no case claims: " + "; ".join(missing)
    ids = [c.id for c in S.all_cases()]
    assert len(set(ids)) == len(ids)
    assert all(c.why_hash for c in S.all_cases())


@pytest.mark.parametrize("family", S.FAMILIES)
def test_without_a_family_a_value_goes_uncovered_and_is_named(family):
    missing = uncovered([f for f in S.FAMILIES if f != family])
    assert FAMILY_OWNS[family] in missing, (family, missing)


def test_the_families_hold_the_shapes_the_edges_ask_for():
    ids = {c.id for c in S.all_cases()}
    for tag in ("plain", "nulls"):
        for n in S.ROW_COUNTS:
            assert "rows-%s_%d" % (tag, n) in ids
            if n >= 3:
                assert "rows-%s_%d_in_two" % (tag, n) in ids
            if n >= 4:
                assert "rows-%s_%d_in_three" % (tag, n) in ids
    for c in S.cases("rows"):  # record boundaries that are no multiple of 4 (the last record ends where the rows do)
        assert all(r.num_rows % 4 != 0 for r in c.records[:-1]), c.id
    for c in S.cases("runs"):  # one or two shapes: every case has the one filter and no validity bitmap but the NULL-or-0 case's
        assert c.filt is not None and c.counts is not None
        assert sum(c.counts.values()) == c.selected, c.id
        got = {k[:2]: k[2] for k in c.want}  # count(value) is the first aggregation
        assert got == c.counts, c.id
    for n in (1, 7, 8):
        assert "columns-%d_dict_and_int64" % n in ids
    for n in (9, 12, 16, 17, 31, 32, 33, 63, 64):
        assert "columns-%d_dict" % n in ids
    assert sum(1 for c in S.cases("columns") if "jit" in c.variants and any(p["n_cols"] == 64 for p in c.pushes)) == 1  # its compile is the slowest
    for c in S.all_cases():
        if c.oracle is False:
            assert c.family == "growth" and c.records[0].num_rows > 1 << 20


def test_restatement_on_four_claims_worked_out_by_hand():
    # (a) 32 768 rows of 32 768 groups into a plan without state: switch_to_hash reserves next_pow2(max(2 * 1, 65 536)) = 65 536 slots; room 32 768
    #   is what the first chunk asks for — one launch, no growth, load 0.5. Then one row of a new group: room 65 536 / 2 − (0 + 32 768) = 0 < 1, the
    #   bound is stale → refreshed to 32 768, still 0 → hash_reserve(1): next_pow2(2 * 32 769) = 131 072, a table with groups and no estimate
    #   grows two steps: 262 144. Key words 4 + 2 = 6 → 8.
    c = by_id("growth-32768_groups_fill_half_of_65536_then_one_more")
    a, b = c.pushes
    assert (a["chunks"], a["cap_after"], a["rehash"], a["refreshed"], a["kw_after"], a["launches"]) == ([(0, 32768)], 65536, False, False, 8, 1), a
    assert (b["chunks"], b["cap_after"], b["rehash"], b["refreshed"], b["kw_before"], b["kw_after"], b["launches"]) == ([(0, 1)], 262144, True, True, 8, 8, 2), b
    assert c.groups_after == [32768, 32769]
    # (b) four records of 10 000 rows, 40 000 groups: the pessimistic bound runs 10 000, 20 000, 30 000; the fourth push finds room 32 768 − 30 000 = 2 768
    #   < 10 000, the refresh reads 30 000 (every row was a group), hash_reserve(10 000): next_pow2(2 * 40 000) = 131 072, doubled: 262 144. 4 launches.
    c = by_id("growth-four_records_of_10000_distinct_groups")
    assert [(p["chunks"], p["cap_after"], p["rehash"], p["refreshed"]) for p in c.pushes] == [([(0, 10000)], 65536, False, False)] * 3 + [([(0, 10000)], 262144, True, True)]
    assert c.pushes[-1]["launches"] == 4 and c.groups_after == [10000, 20000, 30000, 40000]
    #   … with 10 groups in all the refresh reads 10: room 32 758, no re-hash
    c = by_id("growth-four_records_of_10000_rows_in_10_groups")
    assert [(p["cap_after"], p["rehash"], p["refreshed"]) for p in c.pushes] == [(65536, False, False)] * 3 + [(65536, False, True)]
    # (c) a dictionary of 2 048 entries listed in another order: a LUT of 8 192 bytes, the last size that goes to LDS (two of them: 16 384 bytes);
    #   2 049 entries: 8 196 bytes, read from global memory, no LDS. The first record of either IS the plan's value list: identity.
    c = by_id("luts-2048_entries_identity_then_two_permutations")
    assert [(p["lut"], p["lds_lut_bytes"]) for p in c.pushes] == [(["identity"] * 2, 0)] + [(["lds"] * 2, 16384)] * 2
    c = by_id("luts-2049_entries_identity_then_two_permutations")
    assert [(p["lut"], p["lds_lut_bytes"]) for p in c.pushes] == [(["identity"] * 2, 0)] + [(["global"] * 2, 0)] * 2
    # (d) one record of 2^20 + 1 025 rows into a plan without state: 65 536 slots from switch_to_hash, room 32 768 < the first chunk's 2^20 →
    #   hash_reserve(2^20): 2^21 slots (the bound is 0: one step), room 2^20 < 1 049 601 rows left → rounded down to 1 024: it is one already. The
    #   second chunk: room 0, the bound is refreshed to the 1 001 groups there are (1 000 buckets and NULL), room 1 047 575 ≥ 1 025: the rest.
    c = by_id("growth-a_record_of_2^20_plus_1025_rows_in_two_chunks")
    (p,) = c.pushes
    assert (p["chunks"], p["cap_after"], p["refreshed"], p["launches"]) == ([(0, 1 << 20), (1 << 20, (1 << 20) + 1025)], 1 << 21, True, 2), p
    assert c.finish["groups"] == 1001


@pytest.mark.parametrize("family", S.FAMILIES)
def test_the_numpy_reference_equals_the_oracle(family):
    """As multisets of rows, every column exact. The oracle gets every record's key columns in the case's one order; in the NULL-or-0 case both
    sides show such a key as one value. The two records of 2^20 rows and more are left to the numpy reference alone (the oracle appends to
    a builder per group and row: tens of seconds there)."""
    for c in S.cases(family):
        if not c.oracle:
            continue
        want = c.normalise(S.oracle_rows(c))
        assert sum(c.want.values()) == len(c.want) == c.finish["groups"] == c.groups_after[-1], c.id
        missing, extra = want - c.want, c.want - want
        assert not missing and not extra, (c.id, len(want), len(c.want), list(missing.items())[:2], list(extra.items())[:2])


# jit_dump's arguments: N dictionary columns with validity (the first 8 LUTs in LDS), SUM(float64) + COUNT; "1": the last column an int64 key;
# "exact": exact sums. That covers the column counts of the `columns` family; a filter, the seven reducers of `rows` / `runs`, uint64 / bool /
# computed keys and columns without validity cannot be expressed and are compiled on the device only.
HASH_SHAPES = HASH_CASES  # (tests/jit_corpus.py)


def test_hash_kernels_of_the_cases_column_counts_compile_without_scratch(jit_dump):  # noqa: F811
    exe, out = jit_dump

    def one(shape):
        name, args = shape
        src = subprocess.run([exe] + args, check=True, capture_output=True, text=True).stdout
        assert "void fdb_hash_kernel(" in src, name
        path = str(out / (name + ".hip"))
        with open(path, "w") as f:
            f.write(src)
        r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-munsafe-fp-atomics", "-DFDB_DEVICE_ONLY=1", "-include", "hip/hip_runtime.h",
                            "-I", os.path.join(ROOT, "frostdb_amd", "csrc"), "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", path, "-o", path + ".o"],
                           capture_output=True, text=True)
        return name, r.returncode, r.stderr[-2000:] if r.returncode else "", [ln for ln in r.stderr.splitlines() if "ScratchSize" in ln]

    with ThreadPoolExecutor(max_workers=min(len(HASH_SHAPES), os.cpu_count() or 4)) as ex:
        results = list(ex.map(one, HASH_SHAPES))
    assert not [(n, err) for n, rc, err, _ in results if rc != 0]
    assert all(s for _, _, _, s in results)
    spilled = [(n, s) for n, _, _, s in results if not all("ScratchSize [bytes/lane]: 0" in ln for ln in s)]
    assert not spilled, spilled
