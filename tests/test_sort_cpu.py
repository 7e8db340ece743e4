"""CPU-side checks of the device Sort (fdb_batch_sort_indices / fdb_batch_sort): the Python restatement of the reference's comparison
(tests/sort_oracle.py) reproduces the reference's own test vectors, the radix-key encoding of int64 / uint64 / float64 values — the
definition the key kernel compiles, run on the host through fdb_selftest_sort_key — orders every pair of a list of extreme values as
the restatement compares them, fdb_sortkeys.hip compiles for gfx950 without scratch, and the entry points and fdb_sort_col are what
the header says. No GPU is touched."""
import ctypes
import itertools
import os
import re
import struct
import subprocess

import pyarrow as pa
import pytest

from tests import sort_oracle
from tests.golden.sort_cases import CASES, COLUMNS, INDEX_OF, ZERO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

ENTRY_POINTS = ["fdb_batch_sort_indices", "fdb_batch_sort", "fdb_selftest_sort_key", "fdb_sort_bench"]


# ---- the golden cases as records -----------------------------------------------------------------------------------------------------------
def golden_record(samples) -> pa.RecordBatch:
    """Samples.Record() (sort_test.go:684-752) without its dictFixed column: unset fields take the struct's zero value, a timestamp of 0
    is NULL."""
    rows = [dict(ZERO, **s) for s in samples]
    arrays = []
    for name, typ in COLUMNS:
        vals = [r[name] for r in rows]
        if typ == "dict":
            entries = list(dict.fromkeys(v.encode() for v in vals))  # BinaryDictionaryBuilder: first seen first
            arrays.append(pa.DictionaryArray.from_arrays(pa.array([entries.index(v.encode()) for v in vals], type=pa.uint32()), pa.array(entries, type=pa.binary())))
        elif typ == "timestamp":
            arrays.append(pa.array([None if v == 0 else v for v in vals], type=pa.int64()))  # (see COLUMNS)
        else:
            arrays.append(pa.array(vals, type={"int64": pa.int64(), "float64": pa.float64(), "string": pa.string()}[typ]))
    return pa.RecordBatch.from_arrays(arrays, names=[n for n, _ in COLUMNS])


def golden_columns(case):
    return [(INDEX_OF[ix], direction, nulls_first) for ix, direction, nulls_first in case["columns"]]


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_oracle_reproduces_the_reference_vectors(case):
    rec = golden_record(case["samples"])
    assert rec.num_rows == len(case["samples"])
    if "error" in case:
        with pytest.raises(ValueError, match=case["error"]):
            sort_oracle.sort_indices(rec, golden_columns(case))
        return
    assert sort_oracle.sort_indices(rec, golden_columns(case)) == case["indices"], case["cite"]


def test_oracle_float_compare_is_gos_not_numpys():
    nan, neg_nan = float("nan"), struct.unpack("<d", struct.pack("<Q", 0xFFF8000000000000))[0]
    assert sort_oracle.go_cmp(nan, neg_nan) == 0 and sort_oracle.go_cmp(nan, float("-inf")) == -1 and sort_oracle.go_cmp(float("-inf"), nan) == 1
    assert sort_oracle.go_cmp(-0.0, 0.0) == 0 and sort_oracle.go_cmp(5e-324, 0.0) == 1
    rec = pa.RecordBatch.from_arrays([pa.array([1.0, nan, float("-inf"), None, neg_nan, -0.0, 0.0])], names=["f"])
    assert sort_oracle.sort_indices(rec, [0]) == [1, 4, 2, 5, 6, 0, 3]
    assert sort_oracle.sort_indices(rec, [(0, True, True)]) == [3, 0, 5, 6, 2, 1, 4]


# ---- the key encoding ----------------------------------------------------------------------------------------------------------------------
def f64_bits(x: float) -> int:
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def bits_f64(b: int) -> float:
    return struct.unpack("<d", struct.pack("<Q", b))[0]


I64_VALUES = [-2**63, -2**63 + 1, -1, 0, 1, 2**31, 2**63 - 1]
U64_VALUES = [0, 1, 2**31, 2**63 - 1, 2**63, 2**64 - 2, 2**64 - 1]
F64_BITS = [f64_bits(v) for v in (float("-inf"), float("inf"), -0.0, 0.0, 5e-324, -5e-324, -1e308, 1e308, 1.5, -1.5)] + [
    0x7FF8000000000000,  # the quiet NaN
    0xFFF8000000000000,  # a negative NaN
    0x7FF0000000000001,  # a signalling NaN with a payload
    0xFFFFFFFFFFFFFFFF,  # negative, every payload bit set
]


def sign(x):
    return (x > 0) - (x < 0)


@pytest.mark.parametrize("kind", ["int64", "uint64", "float64"])
def test_key_encoding_orders_every_pair_like_the_oracle(kind):
    """sign(key(a) - key(b)) == cmp.Compare(a, b) ascending and its negative descending, for every ordered pair (a with itself included)."""
    from frostdb_amd import physicalplan as pp
    if kind == "int64":
        values = [(v & 0xFFFFFFFFFFFFFFFF, v) for v in I64_VALUES]
        code = pp.SORT_KIND_INT64
    elif kind == "uint64":
        values = [(v, v) for v in U64_VALUES]
        code = pp.SORT_KIND_UINT64
    else:
        values = [(b, bits_f64(b)) for b in F64_BITS]
        code = pp.SORT_KIND_FLOAT64
    for descending in (False, True):
        keys = [pp.selftest_sort_key(code, descending, raw) for raw, _ in values]
        assert all(0 <= k < 2**64 for k in keys)
        for (ka, (_, a)), (kb, (_, b)) in itertools.product(zip(keys, values), repeat=2):
            assert sign(ka - kb) == sort_oracle.go_cmp(a, b) * (-1 if descending else 1), (kind, descending, a, b, hex(ka), hex(kb))


def test_key_encoding_of_nans_and_zeros():
    from frostdb_amd import physicalplan as pp
    key = lambda bits, desc=False: pp.selftest_sort_key(pp.SORT_KIND_FLOAT64, desc, bits)  # noqa: E731
    nans = [b for b in F64_BITS if bits_f64(b) != bits_f64(b)]
    assert len(nans) == 4
    assert len({key(b) for b in nans}) == 1 and key(nans[0]) == 0          # all NaNs share one key …
    assert key(nans[0]) < key(f64_bits(float("-inf")))                      # … below -Inf's, ascending
    assert key(nans[0], True) > key(f64_bits(float("-inf")), True)
    assert key(f64_bits(-0.0)) == key(f64_bits(0.0)) and key(f64_bits(-0.0), True) == key(f64_bits(0.0), True)
    assert key(f64_bits(-5e-324)) < key(f64_bits(0.0)) < key(f64_bits(5e-324))
    # int64: v ^ 1<<63; uint64: v
    assert pp.selftest_sort_key(pp.SORT_KIND_INT64, False, -2**63) == 0 and pp.selftest_sort_key(pp.SORT_KIND_INT64, False, 2**63 - 1) == 2**64 - 1
    assert pp.selftest_sort_key(pp.SORT_KIND_UINT64, False, 2**64 - 1) == 2**64 - 1 and pp.selftest_sort_key(pp.SORT_KIND_UINT64, True, 2**64 - 1) == 0


def test_key_selftest_refuses_bad_arguments():
    from frostdb_amd import physicalplan as pp
    for kind, direction in ((0, 0), (4, 0), (6, 0), (1, 2)):
        out = ctypes.c_uint64()
        assert pp.lib().fdb_selftest_sort_key(kind, direction, 0, ctypes.byref(out)) == pp.FDB_ERR_INVALID
    assert pp.lib().fdb_selftest_sort_key(1, 0, 0, None) == pp.FDB_ERR_INVALID


# ---- the kernel and the interface ----------------------------------------------------------------------------------------------------------
def test_sort_key_kernels_compile_for_gfx950_without_scratch(tmp_path):
    """fdb_sortkeys.hip compiled offline for gfx950: the compiler's resource report shows both instantiations of sort_keys_kernel (row
    order, through a permutation), no scratch and no spills."""
    src = os.path.join(ROOT, "frostdb_amd", "csrc", "fdb_sortkeys.hip")
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-munsafe-fp-atomics", "-I", os.path.join(ROOT, "frostdb_amd", "csrc"),
                        "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", str(tmp_path / "fdb_sortkeys.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    remarks = [ln.split("remark: ")[-1].replace(" [-Rpass-analysis=kernel-resource-usage]", "").strip() for ln in r.stderr.splitlines() if "remark:" in ln]
    names = [u for u in remarks if u.startswith("Function Name:")]
    print(" | ".join(remarks))
    assert sum("sort_keys_kernel" in u for u in names) == 2 and any("sort_iota_kernel" in u for u in names), names
    scratch = [u for u in remarks if "ScratchSize" in u]
    assert len(scratch) == len(names) and all("ScratchSize [bytes/lane]: 0" in u for u in scratch), remarks
    spills = [u for u in remarks if "Spill" in u]
    assert spills and all(re.search(r"Spill: 0\b", u) for u in spills), remarks


def test_entry_points_are_in_library_header_and_binding():
    from frostdb_amd import physicalplan as pp
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "frostdb_amd.h")).read(), flags=re.S)
    L = pp.lib()
    for name in ENTRY_POINTS:
        assert hasattr(L, name), name
        assert re.search(r"^FDB_API int %s\(" % name, header, flags=re.M), name
        assert getattr(L, name).argtypes is not None, name
    assert re.search(r"^FDB_API const char\* fdb_batch_column_name\(", header, flags=re.M)
    for method in ("sort", "sort_indices"):
        assert hasattr(pp.ResidentBatch, method)
    build_py = open(os.path.join(ROOT, "frostdb_amd", "build.py")).read()
    for f in ("fdb_sortkeys.hip", "fdb_sort.cpp", "fdb_sortkey.h"):
        assert '"%s"' % f in build_py, f


def test_sort_col_layout_matches_header(tmp_path):
    from frostdb_amd import physicalplan as pp
    src = tmp_path / "t.c"
    src.write_text(r'''
#include <stdio.h>
#include <stddef.h>
#include "frostdb_amd.h"
int main(void) {
  printf("%zu %zu %zu %zu\n", sizeof(fdb_sort_col), offsetof(fdb_sort_col, index), offsetof(fdb_sort_col, direction), offsetof(fdb_sort_col, nulls_first));
  return 0;
}
''')
    exe = tmp_path / "t"
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).decode().split()]
    assert got == [ctypes.sizeof(pp.SortCol)] + [getattr(pp.SortCol, f).offset for f in ("index", "direction", "nulls_first")]
    assert got == [12, 0, 4, 8]
