"""CPU-side checks of the merge of records with differing field lists (fdb_batches_merge_named) and the OrderedSynchronizer: the oracle
(tests/osync_oracle.py) reproduces the reference's TestEnsureSameSchema vector; the library's schema union and per-input column map
(fdb_selftest_merge_schema, host-only) equal the oracle's on that vector and on seeded random field lists, and refuse what the rules
refuse; fdb_order_col and its ctypes mirror agree; the entry points are in header, version script, library and binding. No GPU is touched."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pyarrow as pa
import pytest

from frostdb_amd.logicalplan import Col, DynCol
from tests import osync_oracle
from tests.golden.osync_cases import ENSURE_SAME_SCHEMA, ORDERED_SYNCHRONIZER

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ENTRY_POINTS = ["fdb_batches_merge_named", "fdb_selftest_merge_schema", "fdb_osync_create", "fdb_osync_push", "fdb_osync_finish"]
KIND_INT64, KIND_FLOAT64, KIND_DICT = 1, 3, 6  # fdb::ColKind, as in include/frostdb_amd.h's sort kinds


def vector_records():
    return [pa.RecordBatch.from_arrays([pa.array([row[k] for row in rec["rows"]], type=pa.int64()) for k in range(len(rec["fields"]))], names=rec["fields"])
            for rec in ENSURE_SAME_SCHEMA["records"]]


def test_oracle_reproduces_the_ensure_same_schema_vector():
    records = vector_records()
    schema, columns = osync_oracle.unify(records, ["Field1"])
    assert schema.names == ENSURE_SAME_SCHEMA["fields"] and columns == [(0, False, False)], ENSURE_SAME_SCHEMA["cite"]
    padded = [osync_oracle.pad(r, schema) for r in records]
    rows = [tuple(r.column(k)[i].as_py() for k in range(3)) for r in padded for i in range(r.num_rows)]
    assert rows == ENSURE_SAME_SCHEMA["expected"], ENSURE_SAME_SCHEMA["cite"]
    # the reference's reader shows the zero value under the virtual NULLs
    zero = ENSURE_SAME_SCHEMA["value_under_absent"]
    assert [tuple(zero if v is None else v for v in row) for row in rows] == [(1, 2, 0), (1, 3, 0), (1, 0, 2), (1, 0, 3), (1, 1, 1), (2, 2, 2)]
    # and the merge by Field1 alone keeps the five rows with Field1 == 1 in record order, then row order
    merged = osync_oracle.merge(records, ["Field1"])
    assert merged.to_pydict() == {"Field1": [1, 1, 1, 1, 1, 2], "Field2": [2, 3, None, None, 1, 2], "Field3": [None, None, 2, 3, 1, 2]}
    assert ORDERED_SYNCHRONIZER["inputs"] == 8 and ORDERED_SYNCHRONIZER["finish_without_pushing"] == [0, 4]


def check_against_oracle(field_lists, order_by):
    """field_lists: per record [(name, kind)]"""
    from frostdb_amd import physicalplan as pp
    columns, n_sort, col_map = pp.selftest_merge_schema(field_lists, order_by)
    names, want_sort, _ = osync_oracle.unify_fields(field_lists, order_by)
    got_names = [field_lists[r][f][0] for r, f in columns]
    assert got_names == names, (field_lists, order_by)
    assert n_sort == want_sort, (field_lists, order_by)
    for i, (r, f) in enumerate(columns):  # the first occurrence, in record order then field order
        assert all(names[i] not in [n for n, _ in field_lists[q]] for q in range(r)), (field_lists, names[i])
    for r, fields in enumerate(field_lists):
        own = [n for n, _ in fields]
        assert col_map[r] == [own.index(n) if n in own else -1 for n in names], (field_lists, order_by, r)


def test_schema_selftest_equals_the_oracle_on_the_vector():
    lists = [[(n, KIND_INT64) for n in rec["fields"]] for rec in ENSURE_SAME_SCHEMA["records"]]
    check_against_oracle(lists, ["Field1"])
    check_against_oracle(lists, ["Field1", "Field2", "Field3"])
    check_against_oracle(lists, ["Field3", ("Field1", True)])
    from frostdb_amd import physicalplan as pp
    columns, n_sort, col_map = pp.selftest_merge_schema(lists, ["Field1"])
    assert columns == [(0, 0), (0, 1), (1, 1)] and n_sort == 1 and col_map == [[0, 1, -1], [0, -1, 1], [0, 1, 2]]


def random_field_lists(rng):
    pool = [("labels.%s" % s, KIND_DICT) for s in "abcde"] + [("pprof.%s" % s, KIND_DICT) for s in ("x", "y", "z")] + \
           [("timestamp", KIND_INT64), ("value", KIND_INT64), ("duration", KIND_FLOAT64), ("labels", KIND_INT64), ("labels.", KIND_DICT), ("labelsx", KIND_INT64)]
    lists = []
    for _ in range(int(rng.integers(1, 7))):
        k = int(rng.integers(0, 9))
        lists.append([pool[i] for i in rng.permutation(len(pool))[:k]])
    exprs = [DynCol("labels"), DynCol("pprof"), Col("timestamp"), Col("labels"), Col("labels.a"), Col("missing"), DynCol("missing"), Col("value")]
    order = [(exprs[i], bool(rng.integers(0, 2)), bool(rng.integers(0, 2))) for i in rng.permutation(len(exprs))[: int(rng.integers(1, 3))]]
    return lists, order


def test_schema_selftest_equals_the_oracle_on_random_field_lists():
    for seed in range(300):
        lists, order = random_field_lists(np.random.default_rng(7000 + seed))
        check_against_oracle(lists, order)
    check_against_oracle([[], [], []], [DynCol("labels")])  # nothing at all
    check_against_oracle([[("labels.b", KIND_DICT), ("labels.a", KIND_DICT)]], [Col("labels.b"), DynCol("labels")])  # a field is matched once


def test_schema_selftest_refusals():
    from frostdb_amd import physicalplan as pp
    with pytest.raises(pp.FdbError) as e:
        pp.selftest_merge_schema([[("a", KIND_INT64)], [("b", KIND_INT64), ("a", KIND_INT64), ("b", KIND_INT64)]], ["a"])
    assert e.value.code == pp.FDB_ERR_INVALID and "found multiple fields" in str(e.value) and "for name b" in str(e.value) and "record 1" in str(e.value)
    with pytest.raises(pp.FdbError) as e:
        pp.selftest_merge_schema([[("a", KIND_INT64)], [], [("a", KIND_FLOAT64)]], ["a"])
    assert e.value.code == pp.FDB_ERR_INVALID and "record 0" in str(e.value) and "record 2" in str(e.value)
    with pytest.raises(ValueError):
        osync_oracle.unify_fields([[("b", 1), ("b", 1)]], ["a"])
    with pytest.raises(ValueError):
        osync_oracle.unify_fields([[("a", 1)], [("a", 3)]], ["a"])
    # bad arguments of the C entry point
    L = pp.lib()
    n_out, n_sort = ctypes.c_int32(), ctypes.c_int32()
    one = (pp.OrderCol * 1)(pp.OrderCol(b"a", 0, 0, 0))
    no_name = (pp.OrderCol * 1)(pp.OrderCol(None, 0, 0, 0))
    names, kinds, counts = (ctypes.c_char_p * 2)(b"a", b"b"), (ctypes.c_int32 * 2)(1, 1), (ctypes.c_int32 * 1)(2)
    out_fields, col_map = (ctypes.c_int32 * 2)(), (ctypes.c_int32 * 2)()
    assert L.fdb_selftest_merge_schema(names, kinds, counts, 1, None, 1, out_fields, col_map, 2, ctypes.byref(n_out), ctypes.byref(n_sort)) == pp.FDB_ERR_INVALID
    assert L.fdb_selftest_merge_schema(names, kinds, counts, 1, one, 0, out_fields, col_map, 2, ctypes.byref(n_out), ctypes.byref(n_sort)) == pp.FDB_ERR_INVALID
    assert L.fdb_selftest_merge_schema(names, kinds, counts, 1, no_name, 1, out_fields, col_map, 2, ctypes.byref(n_out), ctypes.byref(n_sort)) == pp.FDB_ERR_INVALID
    assert L.fdb_selftest_merge_schema(names, kinds, counts, 1, one, 1, out_fields, col_map, 1, ctypes.byref(n_out), ctypes.byref(n_sort)) == pp.FDB_ERR_INVALID
    assert (n_out.value, n_sort.value) == (2, 1)  # … too small a buffer still learns the size
    assert L.fdb_selftest_merge_schema(names, kinds, counts, 1, one, 1, out_fields, col_map, 2, ctypes.byref(n_out), ctypes.byref(n_sort)) == 0
    assert list(out_fields) == [0, 1] and list(col_map) == [0, 1]


def test_osync_state_machine_of_the_oracle():
    """The counting the GPU test compares the library with, on the shapes the reference's Callback / Finish go through."""
    r = osync_oracle.Rounds(3)
    assert r.push(0, "a") is None and r.push(2, "c") is None
    with pytest.raises(osync_oracle.Rounds.StateError):
        r.push(0, "again")
    assert r.push(1, "b") == [(0, "a"), (1, "b"), (2, "c")]
    assert r.push(1, "d") is None and r.finish(0) == (None, False)
    assert r.finish(2) == ([(1, "d")], False)  # running == waiting: the finish completes the round
    with pytest.raises(osync_oracle.Rounds.StateError):
        r.push(2, "late")
    assert r.finish(1) == (None, True)
    with pytest.raises(osync_oracle.Rounds.StateError):
        r.finish(1)


def test_order_col_layout_matches_header(tmp_path):
    from frostdb_amd import physicalplan as pp
    src = tmp_path / "t.c"
    src.write_text(r'''
#include <stdio.h>
#include <stddef.h>
#include "frostdb_amd.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu\n", sizeof(fdb_order_col), offsetof(fdb_order_col, name), offsetof(fdb_order_col, dynamic), offsetof(fdb_order_col, direction),
         offsetof(fdb_order_col, nulls_first));
  return 0;
}
''')
    exe = tmp_path / "t"
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).decode().split()]
    assert got == [ctypes.sizeof(pp.OrderCol)] + [getattr(pp.OrderCol, f).offset for f in ("name", "dynamic", "direction", "nulls_first")]
    assert got == [24, 0, 8, 12, 16]


def test_entry_points_are_in_library_header_version_script_and_binding():
    from frostdb_amd import physicalplan as pp
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "frostdb_amd.h")).read(), flags=re.S)
    exports = open(os.path.join(ROOT, "frostdb_amd", "csrc", "exports.map")).read()
    L = pp.lib()
    defined = subprocess.check_output(["nm", "-D", "--defined-only", L._name], text=True)
    for name in ENTRY_POINTS + ["fdb_osync_close"]:
        assert hasattr(L, name), name
        assert re.search(r"^FDB_API (?:int|void) %s\(" % name, header, flags=re.M), name
        assert getattr(L, name).argtypes is not None, name
        assert name in exports or "fdb_osync_*" in exports, name
        assert re.search(r" T %s$" % name, defined, flags=re.M), name
    assert isinstance(pp.ResidentBatch.__dict__["merge_named"], staticmethod)
    for attr in ("Callback", "Finish", "Close"):
        assert callable(getattr(pp.OrderedSynchronizer, attr))
    # the kernels carry the absent marker the host sets
    csrc = os.path.join(ROOT, "frostdb_amd", "csrc")
    assert "FDB_SORT_ABSENT" in open(os.path.join(csrc, "fdb_sortkeys.hip")).read() and "FDB_SORT_ABSENT" in open(os.path.join(csrc, "fdb_mergerec.cpp")).read()
    assert "s.values != nullptr" in open(os.path.join(csrc, "fdb_mergepath.hip")).read()
