"""The host-side decisions of a dense scan launch, without a GPU: the LDS plan, the records' tile ranges, the fold table of the partial
tables (frostdb_amd/csrc/fdb_launch_plan.h) and the LUT classes (LutClasses, fdb_plan_internal.h). tools/launch_plan_dump.cpp prints what
they give; every expectation below is worked out by hand from the rules stated next to it, never taken from the code under test.

The rules (Plan::DenseLaunch, fdb_dense.cpp):
  * dynamic LDS = [LUT copies: lut_lds_max][table: acc_bytes]. The table is in LDS while lut_lds_max + acc_bytes ≤ 150 KiB; above
    FDB_LDS_BUDGET (64 KiB, two workgroups per CU) only one workgroup fits a CU, so the sequential kernel's grid is halved, unless the
    caller fixed the grid. Above 150 KiB the table stays in global memory and the specialised kernel, if there can be one, gets a combining
    cache of the largest power-of-two entry count with entries × (8 + 8 × n_aggs) ≤ 48 KiB behind the LUT copies.
  * deterministic float sums (fixed_order): four per-wave tables; refused without the specialised kernel / slots / partial tables, and
    when lut_lds_max + 4 × acc_bytes > 150 KiB. No cache, no halving.
  * records own consecutive ranges of ceil(rows / tile_rows) tiles, in launch order.
  * records with byte-identical LUT sets share one device copy and one class; classes are numbered in first-seen order; every set starts
    16-byte aligned in the blob.
"""
import glob
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KIB = 1024
BUDGET = 64 * KIB       # FDB_LDS_BUDGET
LDS_MAX = 150 * KIB
LUT = 1024              # bytes of LUT copies in these cases (any 16-byte multiple)
GRID = 512


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    from frostdb_amd import build
    lib = build.build()
    exe = str(tmp_path_factory.mktemp("launch_plan") / "launch_plan_dump")
    # LutClasses works on Plan::Resolved, a library internal (the .so exports the C ABI only): the tool links the library's OBJECTS
    objs = sorted(glob.glob(os.path.join(os.path.dirname(lib), "csrc", "*.o")))
    assert objs, "frostdb_amd/csrc/*.o missing: build.build() keeps them next to the sources"
    subprocess.check_call(["g++", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROOT, "frostdb_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                           "-I", "/opt/rocm/include", os.path.join(ROOT, "tools", "launch_plan_dump.cpp")] + objs +
                          ["-L/opt/rocm/lib", "-lamdhip64", "-lhiprtc", "-ldl", "-lpthread", "-lz", "-Wl,-rpath,/opt/rocm/lib", "-o", exe])

    def run(*args):
        return subprocess.run([exe] + [str(a) for a in args], check=True, capture_output=True, text=True).stdout.splitlines()
    return run


def lds(dump, lut, acc, n_aggs=1, jit=True, slots=True, fixed=False, partials=True, override=0):
    line, = dump("lds", lut, acc, n_aggs, int(jit), int(slots), int(fixed), int(partials), override, override if override > 0 else GRID)
    head, refusal = line.split(" refusal=")
    got = {k: int(v) for k, v in (f.split("=") for f in head.split())}
    got["refusal"] = refusal
    return got


@pytest.mark.parametrize("override", [0, 100])
def test_plan_lds_at_the_budget(dump, override):
    grid = override or GRID
    at = lds(dump, LUT, BUDGET - LUT, override=override)
    assert at == {"lds_acc": 1, "lds_bytes": BUDGET, "cache_slots": 0, "base_grid": grid, "refusal": ""}
    past = lds(dump, LUT, BUDGET - LUT + 16, override=override)
    # the table is still in LDS; the grid is halved only without an override
    assert past == {"lds_acc": 1, "lds_bytes": BUDGET + 16, "cache_slots": 0, "base_grid": grid if override else GRID // 2, "refusal": ""}


@pytest.mark.parametrize("n_aggs,slots", [(1, 2048), (2, 2048), (8, 512)])  # 48 KiB / 16 = 3072, / 24 = 2048, / 72 = 682.7
@pytest.mark.parametrize("jit", [True, False])
def test_plan_lds_at_150_kib(dump, n_aggs, slots, jit):
    assert slots * (8 + 8 * n_aggs) <= 48 * KIB < 2 * slots * (8 + 8 * n_aggs)
    at = lds(dump, LUT, LDS_MAX - LUT, n_aggs=n_aggs, jit=jit)
    assert at == {"lds_acc": 1, "lds_bytes": LDS_MAX, "cache_slots": 0, "base_grid": GRID // 2, "refusal": ""}
    past = lds(dump, LUT, LDS_MAX - LUT + 16, n_aggs=n_aggs, jit=jit)
    want_slots = slots if jit else 0
    assert past == {"lds_acc": 0, "lds_bytes": LUT + want_slots * (8 + 8 * n_aggs), "cache_slots": want_slots, "base_grid": GRID, "refusal": ""}


def test_plan_lds_fixed_order(dump):
    acc = (LDS_MAX - LUT) // 4  # four tables fill the 150 KiB exactly
    assert LUT + 4 * acc == LDS_MAX
    fits = lds(dump, LUT, acc, fixed=True)
    assert fits == {"lds_acc": 1, "lds_bytes": LDS_MAX, "cache_slots": 0, "base_grid": GRID, "refusal": ""}  # (past the budget, and no halving)
    small = lds(dump, LUT, 4096, fixed=True)
    assert small == {"lds_acc": 1, "lds_bytes": LUT + 4 * 4096, "cache_slots": 0, "base_grid": GRID, "refusal": ""}
    # one byte more of LUT copies: the second refusal begins
    assert lds(dump, LUT + 1, acc, fixed=True)["refusal"] == f"deterministic float sums: four per-wave tables of {acc} bytes do not fit LDS"
    # the first refusal: no specialised kernel, a record that does not fit the slots, or atomics instead of partial tables — whatever the size
    for kw in ({"jit": False}, {"slots": False}, {"partials": False}):
        for a in (4096, acc + 4):
            assert lds(dump, LUT, a, fixed=True, **kw)["refusal"] == "deterministic float sums need the run-time specialised dense kernel"


@pytest.mark.parametrize("tile_rows", [1024, 16384])
def test_assign_tiles(dump, tile_rows):
    # (records without rows are not part of a launch: `live` leaves them out)
    rows = [1, tile_rows, tile_rows + 1, tile_rows - 1, 3 * tile_rows]
    tiles = [1, 1, 2, 1, 3]
    out = dump("tiles", tile_rows, *rows)
    ranges = [tuple(int(v) for v in ln.split()) for ln in out[:-1]]
    assert len(ranges) == len(rows)
    at = 0
    for (b, e), n in zip(ranges, tiles):
        assert b == at and e == b + n and e > b  # contiguous, non-empty, ceil(rows / tile_rows) long
        at = e
    assert out[-1] == f"total={sum(tiles)}"
    assert dump("tiles", tile_rows, 1) == ["0 1", "total=1"]


A = "0001000100"   # a 5-entry truth table
C = "0001000101"   # … one byte different


@pytest.mark.parametrize("order,classes", [("ABC", [0, 0, 1]), ("ACB", [0, 1, 0]), ("CAB", [0, 1, 1])])
def test_lut_classes(dump, order, classes):
    sets = {"A": A, "B": A, "C": C}
    out = dump("luts", *[sets[r] for r in order])
    got = [dict((k, int(v)) for k, v in (f.split("=") for f in ln.split())) for ln in out[:-1]]
    assert [g["class"] for g in got] == classes
    base = {r: g["blob_base"] for r, g in zip(order, got)}
    assert base["A"] == base["B"] != base["C"]
    # two sets of 5 bytes, each 16-byte aligned: the first at 0, the second at 16
    assert sorted({base["A"], base["C"]}) == [0, 16]
    assert base[order[0]] == 0
    assert out[-1] == "blob=21"


def test_lut_classes_without_luts(dump):
    assert dump("luts", "-", "-", "-") == ["class=0 blob_base=0"] * 3 + ["blob=0"]


def test_fold_funcs(dump):
    # fdb_agg_func SUM 1, MIN 2, MAX 3, COUNT 4; FdbAggType I64 1, F64 2. [0] the row counts: an integer sum; COUNT reads them: nothing
    # of its own to fold; SUM by accumulator type: 1 integer, 2 float64; MIN 3; MAX 4 (whatever the type)
    assert dump("funcs", "4:1", "1:1", "1:2", "2:2", "3:1") == ["1 0 1 2 3 4"]
    assert dump("funcs") == ["1"]
