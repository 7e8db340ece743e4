"""CPU-side checks of the device MergeRecords (fdb_batches_merge): the oracle (tests/merge_oracle.py) reproduces the reference's TestMerge
vectors; the merge-path code the kernels compile — diagonal search, tie rule, per-lane serial merge, walked tile by tile and lane by lane
on the host by fdb_selftest_merge_path with the kernels' own tile and items constants — gives the stable merge on the inputs where
partitions go wrong (ties across tile boundaries, empty and one-row runs, one run wholly before the other); fdb_mergepath.hip compiles
for gfx950 without scratch; header, version script and symbols agree. No GPU is touched."""
import os
import re
import subprocess

import numpy as np
import pyarrow as pa
import pytest

from tests import merge_oracle
from tests.golden.merge_cases import CASES, COLUMNS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

ENTRY_POINTS = ["fdb_batches_merge", "fdb_merge_tile_rows", "fdb_selftest_merge_path", "fdb_merge_bench"]
WORDS = [1, 2, 5]


# ---- the golden cases ------------------------------------------------------------------------------------------------------------------------
def golden_record(rows) -> pa.RecordBatch:
    types = {"int64": pa.int64(), "string": pa.string()}
    return pa.RecordBatch.from_arrays([pa.array([r[k] for r in rows], type=types[t]) for k, (_, t) in enumerate(COLUMNS)], names=[n for n, _ in COLUMNS])


def golden_columns(case):
    return [(ix, direction == 1, nulls_first) for ix, direction, nulls_first in case["columns"]]


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_oracle_reproduces_the_reference_vectors(case):
    records = [golden_record(rows) for rows in case["records"]]
    for r in records:
        assert merge_oracle.is_ordered(r, golden_columns(case)), case["cite"]
    got = merge_oracle.merge(records, golden_columns(case), case["limit"])
    want = merge_oracle.decoded_record(golden_record(case["expected"]))
    assert got.to_pydict() == want.to_pydict(), case["cite"]


# ---- the merge path --------------------------------------------------------------------------------------------------------------------------
def check_merge_path(a, b, words):
    """`a`, `b`: sorted lists of `words`-tuples. The walk's sources against sorted(…, key=(key words, source))."""
    from frostdb_amd import physicalplan as pp
    got = pp.selftest_merge_path(np.array(a, dtype=np.uint64).reshape(-1, words), np.array(b, dtype=np.uint64).reshape(-1, words), words).tolist()
    tagged = [(tuple(k), i) for i, k in enumerate(a)] + [(tuple(k), len(a) + j) for j, k in enumerate(b)]
    want = [src for _, src in sorted(tagged)]
    assert got == want, (words, len(a), len(b), next(o for o in range(len(want)) if got[o] != want[o]))


def key(words, v, last=None):
    """v in every word (so that the leading words tie whenever v does), `last` in the last one"""
    return (v,) * (words - 1) + (v if last is None else last,)


@pytest.mark.parametrize("words", WORDS)
def test_merge_path_tile_boundaries_and_ties(words):
    from frostdb_amd import physicalplan as pp
    T = pp.merge_tile_rows(words)
    assert T > 0 and T % 256 == 0
    big = 2**64 - 1
    # all keys equal, na + nb = 3 tiles + 1: pure source order, every boundary inside a tie
    for na in (0, 1, T - 1, T, T + 1, 3 * T):
        check_merge_path([key(words, 7)] * na, [key(words, 7)] * (3 * T + 1 - na), words)
    # every A key below every B key, and the reverse
    lo, hi = [key(words, v) for v in range(T + 3)], [key(words, v) for v in range(T + 3, 2 * T + 10)]
    check_merge_path(lo, hi, words)
    check_merge_path(hi, lo, words)
    # strict interleaving
    check_merge_path([key(words, 2 * v) for v in range(T + 5)], [key(words, 2 * v + 1) for v in range(T + 5)], words)
    # A or B empty
    check_merge_path([], [key(words, v // 3) for v in range(2 * T + 1)], words)
    check_merge_path([key(words, v // 3) for v in range(2 * T + 1)], [], words)
    check_merge_path([], [], words)
    # na = 1 against nb = 2 tiles: below, tied with a stretch that spans the tile boundary, above
    run = [key(words, 1)] * (T - 5) + [key(words, 2)] * 10 + [key(words, 3)] * (T - 5)
    for v in (0, 1, 2, 3, big):
        check_merge_path([key(words, v)], run, words)
        check_merge_path(run, [key(words, v)], words)
    # keys equal in the leading words, different only in the last
    check_merge_path([key(words, 5, 3 * v) for v in range(T + 1)], [key(words, 5, 2 * v) for v in range(T + 2)], words)
    check_merge_path([key(words, big, v // 4) for v in range(T + 1)], [key(words, big, v // 4) for v in range(T + 2)], words)


@pytest.mark.parametrize("words", WORDS)
def test_merge_path_random_runs_with_heavy_ties(words):
    from frostdb_amd import physicalplan as pp
    T = pp.merge_tile_rows(words)
    for seed in range(200):
        rng = np.random.default_rng(1000 * words + seed)
        n = int(rng.integers(0, 3 * T + 1))
        na = int(rng.integers(0, n + 1))
        distinct = int(rng.choice([1, 2, 3, 17, 1000]))
        def run(m):
            k = rng.integers(0, distinct, (m, words)).astype(np.uint64)
            k[:, : words - 1] //= np.uint64(max(1, distinct // 2))  # the leading words tie most of the time
            return sorted(tuple(int(x) for x in row) for row in k)
        check_merge_path(run(na), run(n - na), words)


def test_merge_path_selftest_refuses_bad_arguments():
    from frostdb_amd import physicalplan as pp
    out = np.zeros(8, dtype=np.uint32)
    one = np.array([1], dtype=np.uint64)
    L = pp.lib()
    assert L.fdb_selftest_merge_path(one.ctypes.data, 1, one.ctypes.data, 1, 0, out.ctypes.data) == pp.FDB_ERR_INVALID
    assert L.fdb_selftest_merge_path(None, 1, one.ctypes.data, 1, 1, out.ctypes.data) == pp.FDB_ERR_INVALID
    assert L.fdb_selftest_merge_path(one.ctypes.data, -1, one.ctypes.data, 1, 1, out.ctypes.data) == pp.FDB_ERR_INVALID
    assert L.fdb_selftest_merge_path(one.ctypes.data, 1, one.ctypes.data, 1, 1, None) == pp.FDB_ERR_INVALID
    assert pp.merge_tile_rows(-1) == 0
    # the tile shrinks as the key grows, and stays a whole number of 256-lane rows
    tiles = [pp.merge_tile_rows(w) for w in range(1, 12)]
    assert all(t % 256 == 0 and t >= 256 for t in tiles) and tiles == sorted(tiles, reverse=True)
    assert tiles[0] * (8 * 1 + 4) * 2 <= 160 * 1024  # two workgroups' LDS images on one CU at W = 1


# ---- the kernels and the interface -----------------------------------------------------------------------------------------------------------
def test_merge_kernels_compile_for_gfx950_without_scratch(tmp_path):
    """fdb_mergepath.hip compiled offline for gfx950: the compiler's resource report shows the order check, the partition, the LDS merge
    for 1 … 4 words, the run-time-W merge and the gather — no scratch, no spills, and LDS images that leave two workgroups per CU."""
    src = os.path.join(ROOT, "frostdb_amd", "csrc", "fdb_mergepath.hip")
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-munsafe-fp-atomics", "-I", os.path.join(ROOT, "frostdb_amd", "csrc"),
                        "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", str(tmp_path / "fdb_mergepath.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    remarks = [ln.split("remark: ")[-1].replace(" [-Rpass-analysis=kernel-resource-usage]", "").strip() for ln in r.stderr.splitlines() if "remark:" in ln]
    names = [u for u in remarks if u.startswith("Function Name:")]
    print(" | ".join(remarks))
    assert sum("merge_tile_kernelILi" in u for u in names) == 4, names
    for kernel in ("merge_order_kernel", "merge_partition_kernel", "merge_tile_kernel_any", "merge_gather_kernel"):
        assert sum(kernel in u for u in names) == 1, (kernel, names)
    scratch = [u for u in remarks if "ScratchSize" in u]
    assert len(scratch) == len(names) and all("ScratchSize [bytes/lane]: 0" in u for u in scratch), remarks
    spills = [u for u in remarks if "Spill" in u]
    assert spills and all(re.search(r"Spill: 0\b", u) for u in spills), remarks
    lds = [int(u.split(":")[-1]) for u in remarks if u.startswith("LDS Size")]
    assert len(lds) == len(names) and max(lds) * 2 <= 160 * 1024, lds


def test_entry_points_are_in_library_header_version_script_and_binding():
    from frostdb_amd import physicalplan as pp
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "frostdb_amd.h")).read(), flags=re.S)
    exports = open(os.path.join(ROOT, "frostdb_amd", "csrc", "exports.map")).read()
    L = pp.lib()
    for name in ENTRY_POINTS:
        assert hasattr(L, name), name
        assert re.search(r"^FDB_API (?:int|int32_t) %s\(" % name, header, flags=re.M), name
        assert getattr(L, name).argtypes is not None, name
        assert name in exports, name
    defined = subprocess.check_output(["nm", "-D", "--defined-only", pp.lib()._name], text=True)
    for name in ENTRY_POINTS:
        assert re.search(r" T %s$" % name, defined, flags=re.M), name
    for attr in ("merge", "merge_bench"):
        assert isinstance(pp.ResidentBatch.__dict__[attr], staticmethod), attr
    assert callable(pp.merge_tile_rows) and callable(pp.selftest_merge_path)
    build_py = open(os.path.join(ROOT, "frostdb_amd", "build.py")).read()
    for f in ("fdb_mergepath.hip", "fdb_mergerec.cpp", "fdb_mergepath.h", "fdb_mergerec.h", "fdb_sortplan.h"):
        assert '"%s"' % f in build_py, f
