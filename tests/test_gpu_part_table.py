"""The dense quad scan takes its per-record fields from the packed part table (frostdb_amd/csrc/fdb_jit.h, JitShape::part_table): W words
per record, packed on the host from the records' argument blocks and read by the kernel when a workgroup's tile crosses into the next record.

Records of 2^20 … 2^20 + 4 101 rows are the smallest that take the quad path (a narrow-index cache needs 2^20 rows). Every result is
compared group by group with a numpy group-by over the records' host copies, keyed by VALUE (the records do not all share dictionaries):
counts exactly, float64 sums to 1e-9 relative (the values are positive: no cancellation; the order of the fold is not fixed).

What can go wrong here and nowhere else: a record boundary. So the launches differ in how many boundaries a workgroup crosses (grids of 1
and 2 workgroups cross every one; a grid above the tile count gives every workgroup one tile), in what changes at a boundary (row counts,
column pointers, a second dictionary and with it the LUT class and the LDS restage, a bitmap that one record has and its neighbour lacks),
and in whether the table is used at all ($FDB_PART_TABLE_CAP lowers the size cap: the launch then reads the argument blocks, as before)."""
import os
import re
import subprocess
import sys

import numpy as np
import pyarrow as pa
import pytest

from frostdb_amd import physicalplan as pp
from frostdb_amd.logicalplan import Col, Count, Sum

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = 1 << 20
ROWS = [T, T + 1, T + 1023, T + 4096 + 5]
# two dictionaries per column with different contents (and orders): ids are the numbers in the names
F_A, F_B = [0, 1, 2, 3, 4], [3, 9, 1]
G_A, G_B = list(range(300)), list(range(449, 99, -1))
G_256 = list(range(256))  # 256 entries: the 1-byte cache has no index left for NULL, the column keeps its bitmap


class Rec:
    """One resident record: dictionary columns f and g over the given value ids, v float64 in (0, 1]; host copies as value ids (−1 = NULL)."""

    def __init__(self, rows, f_vals, g_vals, nulls, seed):
        rng = np.random.default_rng(seed)
        self.rows = rows
        cols = []
        self.ids = {}
        for name, vals in (("f", f_vals), ("g", g_vals)):
            idx = rng.integers(0, len(vals), rows, dtype=np.uint32)
            mask = None
            if nulls and rows:
                mask = rng.random(rows) < 0.1
                mask[0] = True
            ids = np.asarray(vals, dtype=np.int64)[idx]
            self.ids[name] = np.where(mask, -1, ids) if mask is not None else ids
            cols.append(pa.DictionaryArray.from_arrays(pa.array(idx, mask=mask), pa.array([("%s%d" % (name, v)).encode() for v in vals], type=pa.binary())))
        self.v = 1.0 - rng.random(rows)
        self.rb = pp.ResidentBatch(pa.RecordBatch.from_arrays(cols + [pa.array(self.v)], names=["f", "g", "v"]))


@pytest.fixture(scope="module")
def recs():
    live0 = pp.live_allocations()
    r = {
        "a0": Rec(ROWS[0], F_A, G_A, False, 1),   # NULL-free
        "a1": Rec(ROWS[1], F_A, G_A, True, 2),    # null-folded caches
        "b2": Rec(ROWS[2], F_B, G_B, True, 3),    # other dictionaries: a second LUT class
        "a3": Rec(ROWS[3], F_A, G_A, False, 4),
        "b0": Rec(ROWS[0], F_B, G_B, False, 5),
        "zero": Rec(0, F_A, G_A, False, 6),
        "k0": Rec(ROWS[1], F_A, G_256, True, 7),  # g keeps its bitmap …
        "k1": Rec(ROWS[2], F_A, G_256, False, 8), # … beside a record whose g has none
    }
    yield r
    for x in r.values():
        x.rb.close()
    assert pp.live_allocations() == live0  # records, caches and every plan's tables are gone


def expected(rs):
    """SUM(v), COUNT over the rows with f == f3, by g's value id (NULL: −1): {id: (count, sum)}."""
    g = np.concatenate([r.ids["g"][r.ids["f"] == 3] for r in rs]) + 1
    v = np.concatenate([r.v[r.ids["f"] == 3] for r in rs])
    counts, sums = np.bincount(g), np.bincount(g, weights=v)
    return {int(k) - 1: (int(counts[k]), float(sums[k])) for k in np.flatnonzero(counts)}


def scan(rs, grid=0):
    plan = pp.HashAggregatePlan(Col("f") == "f3", [Sum(Col("v")), Count(Col("v"))], [Col("g")])
    try:
        plan.set_tuning(0, grid)
        plan.CallbackResident([r.rb for r in rs])
        assert plan.last_kernel() == "fdb_plan_kernel", plan.last_kernel()
        assert plan.stats()["launches"] == 1
        out = plan.Finish()
    finally:
        plan.Close()
    keys = [-1 if k is None else int(k.decode()[1:]) for k in out.column("g").dictionary_decode().to_pylist()]
    got = {k: (c, s) for k, c, s in zip(keys, out.column("count(v)").to_pylist(), out.column("sum(v)").to_pylist())}
    assert len(got) == out.num_rows
    return got


def check(rs, grid=0):
    got, want = scan(rs, grid), expected(rs)
    assert got.keys() == want.keys(), (sorted(set(got) ^ set(want))[:10])
    for k, (c, s) in want.items():
        assert got[k][0] == c, (k, got[k], c)
        assert abs(got[k][1] - s) <= 1e-9 * abs(s), (k, got[k][1], s)


LAUNCHES = {
    "1_record": ["a3"],
    "2_records": ["a0", "a1"],                       # NULL-free beside null-folded
    "3_records": ["a1", "a3", "a0"],
    "5_records_two_classes": ["a0", "a1", "b2", "a3", "b0"],
    "zero_rows_between": ["a1", "zero", "a3"],
    "bitmap_kept_in_one": ["k0", "k1"],
}


def launch_line(err):
    lines = [ln for ln in err.splitlines() if ln.startswith("[fdb] dense launch")]
    assert len(lines) == 1, err[-2000:]
    return lines[0]


# words per record the launch's shape needs (fdb_jit.h, jit_part_fields): 3 range words, 3 column pointers, truth bits, group LUT pointer,
# 5 32-bit fields in 3 words = 11; + 1 for the one bitmap pointer of the launch whose 256-entry column keeps it. 0: one record, no table.
WORDS = {"1_record": 0, "2_records": 11, "3_records": 11, "5_records_two_classes": 11, "zero_rows_between": 11, "bitmap_kept_in_one": 12}


# LUT classes of each launch: one per distinct group LUT — per dictionary, and per whether the record's null-folded cache adds the entry for NULL
# (a record without NULLs has none; the 256-entry column is never folded)
CLASSES = {"1_record": 1, "2_records": 2, "3_records": 2, "5_records_two_classes": 4, "zero_rows_between": 2, "bitmap_kept_in_one": 1}


@pytest.mark.parametrize("grid", [0, 1, 2, 1 << 20], ids=["grid_default", "grid_1", "grid_2", "grid_above_tiles"])
@pytest.mark.parametrize("launch", sorted(LAUNCHES))
def test_records_of_different_sizes_in_one_launch(recs, launch, grid, monkeypatch, capfd):
    """Results, and that the launch was the one meant: the quad shape, with the table (or, for one record, without), over the live records."""
    rs = [recs[n] for n in LAUNCHES[launch]]
    monkeypatch.setenv("FDB_PROFILE", "1")
    capfd.readouterr()
    check(rs, grid)
    line = launch_line(capfd.readouterr().err)
    live = sum(1 for r in rs if r.rows)
    assert " parts=%d " % live in line and " ptab=%d " % WORDS[launch] in line, line
    assert re.search(r"shape=\S*q%s\|" % ("p" if WORDS[launch] else ""), line), line
    classes = set(re.findall(r" (\d+):", line.split("class:w4/wl4=")[1]))
    assert len(classes) == CLASSES[launch], line


def test_cap_forces_the_fallback(recs, monkeypatch, capfd):
    """3 records of 11 words each are 264 bytes: above a cap of 200 the launch ships and reads the argument blocks; same results."""
    rs = [recs[n] for n in LAUNCHES["3_records"]]
    monkeypatch.setenv("FDB_PROFILE", "1")
    capfd.readouterr()
    check(rs)
    line = launch_line(capfd.readouterr().err)
    assert re.search(r" ptab=(\d+) ", line).group(1) == "11" and " parts=3 " in line, line
    assert re.search(r"shape=\S*qp\|", line), line
    monkeypatch.setenv("FDB_PART_TABLE_CAP", "200")
    check(rs, 2)
    line = launch_line(capfd.readouterr().err)
    assert " ptab=0 " in line and " parts=3 " in line and re.search(r"shape=\S*q\|", line), line


CHILD = r"""
import sys
sys.path.insert(0, %r)
import numpy as np, pyarrow as pa
from frostdb_amd import physicalplan as pp
from frostdb_amd.logicalplan import Col, Sum
rows = (1 << 20) + 5
rbs = []
for k in range(2):
    rng = np.random.default_rng(k)
    f = pa.DictionaryArray.from_arrays(pa.array(rng.integers(0, 5, rows, dtype=np.uint32)), pa.array([b"f%%d" %% i for i in range(5)], type=pa.binary()))
    g = pa.DictionaryArray.from_arrays(pa.array(rng.integers(0, 1024, rows, dtype=np.uint32)), pa.array([b"g%%d" %% i for i in range(1024)], type=pa.binary()))
    rbs.append(pp.ResidentBatch(pa.RecordBatch.from_arrays([f, g, pa.array(np.ones(rows))], names=["f", "g", "v"])))
plan = pp.HashAggregatePlan(Col("f") == "f3", [Sum(Col("v"))], [Col("g")])
plan.CallbackResident(rbs)
out = plan.Finish()
plan.Close()
print("groups", out.num_rows, "sum", float(np.sum(out.column("sum(v)").to_numpy())))
""" % ROOT


def test_default_path_reports_its_table():
    """The headline's shape (no NULLs, SUM alone) in a fresh process: the launch line names the table's words per record."""
    r = subprocess.run([sys.executable, "-c", CHILD], cwd=ROOT, env=dict(os.environ, FDB_PROFILE="1"), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    line = launch_line(r.stderr)
    assert " ptab=11 " in line and " parts=2 " in line, line
    m = re.search(r"groups (\d+) sum ([0-9.]+)", r.stdout)
    assert m and int(m.group(1)) == 1024, r.stdout
    want = 0
    for k in range(2):  # (the child's generator, restated: v is 1.0, so the sum counts the selected rows)
        want += int(np.sum(np.random.default_rng(k).integers(0, 5, (1 << 20) + 5, dtype=np.uint32) == 3))
    assert float(m.group(2)) == want, (m.group(2), want)
