"""The cases of tests/hash_merge_cases.py cover what they claim: over the generated families every side of every branch of
hash_merge_wave_kernel<TABLE_SRC>, hash_partition_wave_kernel<PASS> and partition_bases_kernel is claimed by at least one case, the
oracle finds in every case the number of groups the case states, and fdb_merge.hip compiles for gfx950 without scratch. No GPU is touched.

The launch shapes are a Python RESTATEMENT of the host arithmetic and can drift from the C++ they restate:
  Plan::hash_layout (fdb_hash.cpp:36-61), Plan::hash_reserve (:71-96), Plan::hash_merge_args (:174-195), Plan::switch_to_hash (:210-244),
  push_hash's reservation (:381-450), Plan::hash_export (:1036-1125, `in_words` / `same_layout` / `same_ids`: :1104-1113), Plan::hash_import
  (:1127-1177), Plan::merge_hash_tables (:1182-1247), Plan::merge_hash (:1251-1319), the mode decision of Plan::push_batches
  (fdb_plan.cpp:1418-1427), Plan::merge_from (:2123-2143), and wave_lds_bytes / geometry / quads_ok / fdb_launch_hash_merge / part_plan of
  fdb_merge.hip. Four shapes worked out by hand below pin it; whoever changes how those functions shape a launch changes
  hash_merge_cases.py with them."""
import os
import re
import subprocess

import pytest

from tests import hash_merge_cases as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def shapes(families=H.FAMILIES):
    return [(c, s) for f in families for c in H.cases(f) for s in c.shapes]


# What the families together must reach: (name of the value, predicate over a claimed launch shape)
COVERED = [
    ("TABLE_SRC = 0", lambda s: s["kernel"] == "merge" and s["table_src"] == 0),
    ("TABLE_SRC = 1", lambda s: s["kernel"] == "merge" and s["table_src"] == 1),
    ("merge: alias = 0", lambda s: s["kernel"] == "merge" and s["alias"] == 0),
    ("merge: alias = 1", lambda s: s["kernel"] == "merge" and s["alias"] == 1),
    ("partition: alias = 0", lambda s: s["kernel"] == "partition" and s["alias"] == 0),
    ("partition: alias = 1", lambda s: s["kernel"] == "partition" and s["alias"] == 1),
    ("quads = 0", lambda s: s["quads"] == 0),
    ("quads = 1 from packed rows", lambda s: s["quads"] == 1 and s["table_src"] == 0 and s["why"] != "import"),
    ("quads = 1 from a table", lambda s: s["quads"] == 1 and s["table_src"] == 1),
    ("a LUT", lambda s: s["lut"] == 1 and s["table_src"] == 1),
    ("no LUT", lambda s: s["lut"] == 0 and s["table_src"] == 1),
    ("packed rows without a LUT", lambda s: s["lut"] == 0 and s["table_src"] == 0 and s["why"] == "migrate"),
    ("a column with src_word < 0 from a table", lambda s: s["absent"] == 1 and s["table_src"] == 1),
    ("a column with src_word < 0 from packed rows", lambda s: s["absent"] == 1 and s["table_src"] == 0),
    ("same_ids = 0", lambda s: s.get("same_ids") == 0),
    ("same_ids = 1", lambda s: s.get("same_ids") == 1),
    ("same_ids = 0 in place", lambda s: s.get("same_ids") == 0 and s["alias"] == 1),
    ("1 wave per workgroup", lambda s: s["waves"] == 1),
    ("2 waves per workgroup", lambda s: s["waves"] == 2),
    ("3 waves per workgroup", lambda s: s["waves"] == 3),
    ("4 waves per workgroup", lambda s: s["waves"] == 4),
    ("3 waves per workgroup in the partition passes", lambda s: s["kernel"] == "partition" and s["waves"] == 3),
    ("dynamic LDS <= 48 KiB", lambda s: s["lds"] <= 48 << 10),
    ("dynamic LDS > 48 KiB", lambda s: s["lds"] > 48 << 10),
    ("partitions <= 16", lambda s: s["kernel"] == "partition" and s["n_parts"] <= 16),
    ("partitions > 16", lambda s: s["kernel"] == "partition" and s["n_parts"] > 16),
    ("partitions = 16", lambda s: s["kernel"] == "partition" and s["n_parts"] == 16),
    ("partitions = 17", lambda s: s["kernel"] == "partition" and s["n_parts"] == 17),
    ("partitions = 1", lambda s: s["kernel"] == "partition" and s["n_parts"] == 1),
    ("partitions = 63", lambda s: s["kernel"] == "partition" and s["n_parts"] == 63),
    ("partitions = 64", lambda s: s["kernel"] == "partition" and s["n_parts"] == 64),
    ("launch waves <= 64", lambda s: s["launch_waves"] is not None and s["launch_waves"] <= 64),
    ("launch waves 65 ... 256", lambda s: s["launch_waves"] is not None and 65 <= s["launch_waves"] <= 256),
    ("merge: launch waves > 256", lambda s: s["kernel"] == "merge" and s["launch_waves"] is not None and s["launch_waves"] > 256),
    ("partition: launch waves 65 ... 256", lambda s: s["kernel"] == "partition" and 65 <= s["launch_waves"] <= 256),
    ("partition: launch waves > 256", lambda s: s["kernel"] == "partition" and s["launch_waves"] > 256),
    ("partition: launch waves > 256 with more than 16 partitions", lambda s: s["kernel"] == "partition" and s["launch_waves"] > 256 and s["n_parts"] > 16),
    ("merge: a table source at load >= 0.45", lambda s: s["kernel"] == "merge" and s["src_load"] is not None and s["src_load"] >= 0.45),
    ("partition: a table source at load >= 0.45", lambda s: s["kernel"] == "partition" and s["src_load"] is not None and s["src_load"] >= 0.45),
    ("63 incoming groups from a table", lambda s: s["incoming"] == 63 and s["table_src"] == 1),
    ("64 incoming groups from a table", lambda s: s["incoming"] == 64 and s["table_src"] == 1),
    ("65 incoming groups from a table", lambda s: s["incoming"] == 65 and s["table_src"] == 1),
    ("63 incoming packed rows", lambda s: s["incoming"] == 63 and s["table_src"] == 0),
    ("64 incoming packed rows", lambda s: s["incoming"] == 64 and s["table_src"] == 0),
    ("65 incoming packed rows", lambda s: s["incoming"] == 65 and s["table_src"] == 0),
    ("1 incoming packed row", lambda s: s["incoming"] == 1 and s["table_src"] == 0),
    ("entry words = 4", lambda s: s["entry_words"] == 4),
    ("entry words = 8", lambda s: s["entry_words"] == 8),
    ("entry words = 12", lambda s: s["entry_words"] == 12),
    ("a destination whose key words grow", lambda s: s.get("kw_before") is not None and s["kw_after"] > s["kw_before"]),
    ("a destination whose key words grow across a quad, 16 -> 20", lambda s: s.get("kw_before") == 16 and s.get("kw_after") == 20),
    ("a destination whose new column lands on its tuples' padding", lambda s: s.get("kw_before") is not None and s["kw_after"] == s["kw_before"] and s["used_after"] > s["used_before"]),
    ("a destination without a table", lambda s: s["why"] == "merge" and s.get("kw_before") is None),
]
# which families a value may come from: taking a family out of the generator must leave at least one of these uncovered
FAMILY_OWNS = {
    "widths": "2 waves per workgroup",
    "layouts": "dynamic LDS > 48 KiB",
    "counts": "merge: launch waves > 256",
    "packed": "63 incoming packed rows",
    "reducers": "entry words = 4",
    "exports": "partitions = 64",
}


def uncovered(families):
    found = shapes(families)
    return [name for name, hit in COVERED if not any(hit(s) for _, s in found)]


def test_every_branch_is_claimed_by_some_case():
    missing = uncovered(H.FAMILIES)
    assert not missing, "no case claims: " + "; ".join(missing)
    assert all(s["lds"] <= 150 << 10 for _, s in shapes()), "a case asks for more LDS than the launch accepts"


@pytest.mark.parametrize("family", H.FAMILIES)
def test_without_a_family_a_value_goes_uncovered_and_is_named(family):
    missing = uncovered([f for f in H.FAMILIES if f != family])
    assert FAMILY_OWNS[family] in missing, (family, missing)


def test_the_families_hold_the_cases_the_kernels_edges_ask_for():
    ids = {c.id for c in H.all_cases()}
    assert len(ids) == len(H.all_cases())
    for n in (1, 63, 64, 65, 127, 128, 129):
        assert "counts-%d_into_3000_half_shared" % n in ids
    for kind in ("empty", "identical", "disjoint", "half_shared"):
        assert "counts-65_into_%s" % kind in ids and "counts-32768_into_%s" % kind in ids
    for k in (1, 2, 3, 4, 8):
        for n in (1, 63, 64, 65, 4097):
            assert "packed-dense_%d_columns_%d_groups_into_hash" % (k, n) in ids and "packed-migrate_%d_columns_%d_groups" % (k, n) in ids
    for P in H.EXPORT_PARTS:
        assert "exports-3000_groups_%d_parts" % P in ids
    for n in (1, 65, 32768, 70000):
        assert {"exports-%d_groups_17_parts" % n, "exports-%d_groups_64_parts" % n} <= ids
    # word gathers for every packed tuple but the 4-word one; the tuples of a dense source are 2 + (1 | 2 per column) words
    for c in H.cases("packed"):
        if c.op == "dense_into_hash":
            k = int(c.id.split("_")[1])
            (s,) = c.shapes
            assert s["in_words"] == 2 + k and s["quads"] == int(k == 2), (c.id, s)
    # the sources without groups launch nothing
    assert [c.shapes for c in H.cases("counts")[:2]] == [[], []]


def test_restatement_on_four_shapes_worked_out_by_hand():
    # (a) 12 dictionary columns, COUNT + SUM, a 3 000-group source scanned from 9 000 rows, same order and dictionaries.
    #   key words 4 + 12 = 16 (no padding), entry words (3 + 2 + 3) / 4 * 4 = 8; the source's table: next_pow2(max(2 * 9 000, 65 536)) = 65 536
    #   slots. reach = 15 + 1 = 16 → in_words 16, same layout → one tile of 16 words: 256 * 16 + 1 792 = 5 888 bytes per wave, 40 960 / 5 888 = 6 → 4
    #   waves, 23 552 bytes; 1 024 batches / 16 + 1 = 65 → 17 workgroups (the cap is 128 * 4) → 68 waves.
    (s,) = next(c for c in H.cases("widths") if c.id == "widths-12_dict").shapes
    assert (s["table_src"], s["in_words"], s["out_words"], s["alias"], s["quads"], s["lut"], s["waves"], s["lds"], s["launch_waves"], s["entry_words"]) == \
        (1, 16, 16, 1, 1, 0, 4, 23552, 68, 8), s
    assert s["src_load"] == 3000 / 65536
    # (b) 64 int64 keys, the source's fields reversed: key words 4 + 128 = 132 on both sides, no column at its own word → two tiles:
    #   256 * 264 + 1 792 = 69 376 bytes per wave (67.75 KiB) → 1 wave; 159 744 / 69 440 = 2 workgroups per CU; 65 batches → 65 workgroups of one wave.
    (s,) = next(c for c in H.cases("layouts") if c.id == "layouts-64_int64_reversed_fields").shapes
    assert (s["in_words"], s["out_words"], s["alias"], s["quads"], s["waves"], s["lds"], s["launch_waves"]) == (132, 132, 0, 1, 1, 69376, 65), s
    # (c) a dense source of 3 dictionary columns and 65 groups into 12 columns: packed tuples of 2 + 3 = 5 words, reach 5 → min(8, 5) = 5 words
    #   gathered word by word, two tiles of 5 + 16 words: 256 * 21 + 1 792 = 7 168 → 4 waves, 28 672 bytes; 2 batches → 1 workgroup → 4 waves.
    (s,) = next(c for c in H.cases("packed") if c.id == "packed-dense_3_columns_65_groups_into_hash").shapes
    assert (s["table_src"], s["in_words"], s["out_words"], s["alias"], s["quads"], s["lut"], s["absent"], s["waves"], s["lds"], s["launch_waves"]) == \
        (0, 5, 16, 0, 0, 1, 1, 4, 28672, 4), s
    # (d) the export of 70 000 groups (105 000 rows: 2^18 slots) for 64 owners: rows of (16 + 2 * 3 + 3) & ~3 = 24 words, in place:
    #   256 * 24 + 1 792 + 512 = 8 448 → 4 waves, 33 792 bytes; 4 096 batches / 16 + 1 = 257 → 65 workgroups → 260 waves.
    s = next(c for c in H.cases("exports") if c.id == "exports-70000_groups_64_parts").shapes[0]
    assert (s["in_words"], s["out_words"], s["alias"], s["same_ids"], s["waves"], s["lds"], s["launch_waves"], s["n_parts"]) == (16, 24, 1, 1, 4, 33792, 260, 64), s
    assert H.geometry(H.wave_lds_bytes(32, 32, True), 65)[0] == 4 and H.geometry(H.wave_lds_bytes(36, 36, True), 65)[0] == 3  # 28 columns: the last 4-wave shape


@pytest.mark.parametrize("family", H.FAMILIES)
def test_the_oracle_finds_the_groups_every_case_states(family):
    for c in H.cases(family):
        want = H.oracle_rows(c)
        assert sum(want.values()) == len(want) == c.groups, (c.id, len(want), c.groups)
        counts = [row[len(c.names)] for row in want] if c.aggs[0].Name().startswith("count(") else None
        if counts is not None and not c.final_stage:
            assert sum(counts) == sum(int(H.selected(c, r).sum()) for r in c.oracle_recs()), c.id


def test_merge_kernels_compile_for_gfx950_without_scratch(tmp_path):
    """fdb_merge.hip compiled offline for gfx950: the compiler's resource report shows both merge instances, both partition passes and the
    bases kernel — no scratch, no vector register spilled (scalar registers that move into vector lanes touch no memory)."""
    src = os.path.join(ROOT, "frostdb_amd", "csrc", "fdb_merge.hip")
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-munsafe-fp-atomics", "-I", os.path.join(ROOT, "frostdb_amd", "csrc"),
                        "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", str(tmp_path / "fdb_merge.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    remarks = [ln.split("remark: ")[-1].replace(" [-Rpass-analysis=kernel-resource-usage]", "").strip() for ln in r.stderr.splitlines() if "remark:" in ln]
    names = [u for u in remarks if u.startswith("Function Name:")]
    print(" | ".join(remarks))
    assert sum("hash_merge_wave_kernel" in u for u in names) == 2, names
    assert sum("hash_partition_wave_kernel" in u for u in names) == 2, names
    assert sum("partition_bases_kernel" in u for u in names) == 1, names
    scratch = [u for u in remarks if "ScratchSize" in u]
    assert len(scratch) == len(names) and all("ScratchSize [bytes/lane]: 0" in u for u in scratch), remarks
    spills = [u for u in remarks if "VGPRs Spill" in u]
    assert len(spills) == len(names) and all(re.search(r"Spill: 0\b", u) for u in spills), remarks
