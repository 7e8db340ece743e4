"""CPU-side checks of statistics, the page index and sorting_columns in the Parquet writer (fdb_batch_to_parquet_indexed):
fdb_selftest_parquet_write_indexed runs the writer over a host record, the min / max kernel replaced by the host walk of the keys it
compiles (fdb_pqstats.h) — byte for byte the file the device path writes (tests/test_gpu_parquet_index.py holds the two against each
other). Here: the test-side reader is first pinned on a page index that pyarrow wrote; then chunk statistics are held against those of
pyarrow's own writer for the same table, every ColumnIndex and OffsetIndex against a restatement of the rules
(tests/parquet_index_cases.py) and against the page headers found by walking the chunk, on every column kind, row count and NULL
pattern, on the values and strings where the order or the cut can go wrong, with DELTA and SNAPPY columns mixed in. Without the new
arguments the bytes are the older calls'. No GPU is touched."""
import ctypes
import io
import os
import re
import struct
import subprocess

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq
import pytest

from tests import parquet_index_cases as X
from tests import parquet_snappy_cases as S
from tests import parquet_write_cases as cases
from tests.parquet_util import row_group_chunks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
ENTRY_POINTS = ["fdb_batch_to_parquet_indexed", "fdb_selftest_parquet_write_indexed"]
PAGE = X.PAGE


@pytest.fixture(scope="module")
def pp():
    from frostdb_amd import physicalplan
    return physicalplan


def read_back(data: bytes) -> pa.RecordBatch:
    t = pq.read_table(io.BytesIO(data)).combine_chunks()
    return pa.RecordBatch.from_arrays([c.chunk(0) if c.num_chunks else pa.array([], type=c.type) for c in t.columns], names=t.schema.names)


def write_and_check(pp, record, page_rows=PAGE, statistics="page", limit=0, **kw) -> bytes:
    data = pp.selftest_parquet_write(record, page_rows=page_rows, statistics=statistics, index_size_limit=limit, **kw)
    X.assert_index(record, data, page_rows, statistics, limit)
    rg = pq.ParquetFile(io.BytesIO(data)).metadata.row_group(0)
    chunks = X.chunk_fields(data)
    for j in range(rg.num_columns):
        assert rg.column(j).has_offset_index == (statistics == "page")
        assert rg.column(j).has_column_index == (chunks[j]["column_index"] is not None)
    cases.assert_same_record(read_back(data), record)
    return data


# ---- 0. the yardstick: the reader reads a page index pyarrow wrote -----------------------------------------------------------------------------
def test_the_reader_reads_pyarrows_page_index():
    rng = np.random.default_rng(5)
    n = 5000
    valid = rng.random(n) < 0.8
    valid[1000:2500] = False
    table = pa.table({"i": pa.array(rng.integers(-2**62, 2**62, n), mask=~valid), "f": pa.array(rng.standard_normal(n)),
                      "s": pa.array(["s%05d" % v for v in rng.integers(0, 99999, n)], mask=~valid), "u": pa.array(rng.integers(0, 2**64, n, dtype=np.uint64))})
    buf = io.BytesIO()
    pq.write_table(table, buf, compression="NONE", write_page_index=True, data_page_size=2048, use_dictionary=False, write_batch_size=100, data_page_version="1.0")
    data = buf.getvalue()
    chunks = X.chunk_fields(data)
    assert X.row_group_fields(data)["column_orders"] == [{1: {}}] * 4
    for c, name, fmt in zip(chunks, ["i", "f", "s", "u"], ["<q", "<d", None, "<Q"]):
        locs = X.offset_index(data, c["offset_index"])
        ci = X.column_index(data, c["column_index"])
        pages = X.walk_pages(data, c)
        assert len(locs) > 3 and [(p[0], p[1]) for p in pages] == [(o, size) for o, size, _ in locs], name
        assert locs[0][2] == 0 and len(ci["null_pages"]) == len(locs)
        col = table.column(name).combine_chunks()
        for p, (_, _, first) in enumerate(locs):
            end = locs[p + 1][2] if p + 1 < len(locs) else n
            part = col.slice(first, end - first)
            assert ci["null_counts"][p] == part.null_count, (name, p)
            assert ci["null_pages"][p] == (part.null_count == len(part)), (name, p)
            if ci["null_pages"][p]:
                continue
            vals = [v for v in part.to_pylist() if v is not None]
            lo, hi = (min(vals), max(vals))
            if fmt is None:
                assert (ci["min_values"][p], ci["max_values"][p]) == (lo.encode(), hi.encode()), (name, p)
            else:
                assert (struct.unpack(fmt, ci["min_values"][p])[0], struct.unpack(fmt, ci["max_values"][p])[0]) == (lo, hi), (name, p)
        st = pq.ParquetFile(io.BytesIO(data)).metadata.row_group(0).column(["i", "f", "s", "u"].index(name)).statistics
        assert c["null_count"] == st.null_count
        if fmt is not None:
            assert (struct.unpack(fmt, c["min_value"])[0], struct.unpack(fmt, c["max_value"])[0]) == (st.min, st.max), name
    assert X.cut_max(b"ab\xff\xffzz", 4) == b"ac" and X.cut_max(b"\xff\xff\xff", 2) == b"\xff\xff\xff" and X.cut_max(b"abc", 3) == b"abc" and X.cut_min(b"abcd", 2) == b"ab"


# ---- 1. chunk statistics: what pyarrow reads of our file == what it reads of its own writer's ------------------------------------------------------
def assert_statistics_as_pyarrows(pp, record, statistics, page_rows=PAGE):
    data = pp.selftest_parquet_write(record, page_rows=page_rows, statistics=statistics)
    ours, theirs = X.pyarrow_statistics(data), X.pyarrow_statistics(X.pyarrow_writes(record))
    for name, a, b in zip(record.schema.names, ours, theirs):
        if isinstance(a[1], float):
            assert a[0] == b[0] and struct.pack("<dd", a[1], a[2]) == struct.pack("<dd", b[1], b[2]), (name, a, b)   # (the zeros' signs too)
        else:
            assert a == b, (name, a, b)
    return data


@pytest.mark.parametrize("statistics", ["chunk", "page"])
@pytest.mark.parametrize("family", sorted(X.FAMILIES))
def test_chunk_statistics_are_pyarrows(pp, family, statistics):
    record = X.FAMILIES[family]()
    assert_statistics_as_pyarrows(pp, record, statistics)


@pytest.mark.parametrize("pattern", cases.NULL_PATTERNS)
def test_chunk_statistics_of_every_kind_under_every_null_pattern(pp, pattern):
    for rows in X.INDEX_ROWS:
        data = assert_statistics_as_pyarrows(pp, cases.mixed_record(rows, pattern), "chunk")
        X.assert_index(cases.mixed_record(rows, pattern), data, PAGE, "chunk")


def test_uint64_bounds_past_2_63_read_back_unsigned(pp):
    u = np.array([2**63 + 5, 3, 2**64 - 1, 2**63 - 1], dtype=np.uint64)
    record = pa.RecordBatch.from_arrays([pa.array(u), pa.array(u[:4] >> np.uint64(1))], names=["u", "half"])
    data = assert_statistics_as_pyarrows(pp, record, "page")
    st = X.pyarrow_statistics(data)
    assert st[0] == (True, 3, 2**64 - 1) and st[1] == (True, 1, 2**63 - 1)
    ci = X.column_index(data, X.chunk_fields(data)[0]["column_index"])
    assert ci["min_values"] == [struct.pack("<Q", 3)] and ci["max_values"] == [struct.pack("<Q", 2**64 - 1)]


# ---- 2. the page index ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", cases.NULL_PATTERNS)
def test_page_index_of_every_kind_rows_and_null_pattern(pp, pattern):
    for rows in X.INDEX_ROWS:
        write_and_check(pp, cases.mixed_record(rows, pattern))


@pytest.mark.parametrize("family", sorted(X.FAMILIES))
def test_page_index_of_the_families(pp, family):
    record = X.FAMILIES[family]()
    write_and_check(pp, record)
    write_and_check(pp, record, statistics="chunk")


def test_values(pp):
    record = X.values_record()
    data = write_and_check(pp, record)
    chunks = {c["name"]: c for c in X.chunk_fields(data)}
    d = lambda b: struct.unpack("<d", b)[0]
    neg, pos = struct.pack("<d", -0.0), struct.pack("<d", 0.0)
    assert (chunks["i"]["min_value"], chunks["i"]["max_value"]) == (struct.pack("<q", -2**63), struct.pack("<q", 2**63 - 1))
    assert (chunks["u"]["min_value"], chunks["u"]["max_value"]) == (struct.pack("<Q", 0), struct.pack("<Q", 2**64 - 1))
    assert (d(chunks["f"]["min_value"]), d(chunks["f"]["max_value"])) == (-np.inf, np.inf)
    for name in ("zeros_a", "zeros_b"):   # a page of zeros only: −0.0 below, +0.0 above, whichever came first and whichever occurred
        ci = X.column_index(data, chunks[name]["column_index"])
        assert (ci["min_values"][1], ci["max_values"][1]) == (neg, pos) and (ci["min_values"][2], ci["max_values"][2]) == (neg, pos), name
    for name in ("nan_page", "nan_page_null"):   # a page of NaNs only: no ColumnIndex, the OffsetIndex is there, the chunk's bounds are the other pages'
        assert chunks[name]["column_index"] is None and chunks[name]["offset_index"] is not None
        assert (d(chunks[name]["min_value"]), d(chunks[name]["max_value"])) == ((-np.inf, np.inf) if name == "nan_page" else (np.inf, np.inf))   # (the even rows hold +inf and NaNs)
    assert chunks["only_nan"]["column_index"] is None and chunks["only_nan"]["min_value"] is None and chunks["only_nan"]["max_value"] is None
    assert chunks["only_nan"]["offset_index"] is not None and chunks["only_nan"]["null_count"] == 0
    assert X.column_index(data, chunks["flag"]["column_index"])["min_values"] == [b"\x00", b"\x00", b"\x01", b"\x00"]


def test_strings_and_the_cut(pp):
    record = X.strings_record()
    data = write_and_check(pp, record)
    chunks = {c["name"]: c for c in X.chunk_fields(data)}
    assert (chunks["unused"]["min_value"], chunks["unused"]["max_value"]) == (b"b", b"y")          # the unused entries never show
    assert (chunks["dup"]["min_value"], chunks["dup"]["max_value"]) == (b"", b"b")                  # the empty string is a minimum
    assert chunks["lengths"]["max_value"] == b"\xff" * 17                                            # never cut in the chunk's Statistics
    ci = X.column_index(data, chunks["ff"]["column_index"])
    assert ci["max_values"] == [b"\xff" * 17, b"a" * 14 + b"b", b"a" * 13 + b"b"]        # all 0xFF: whole; trailing 0xFF inside the limit: dropped, then + 1
    assert ci["min_values"] == [b"\xff" * 16, b"a" * 15 + b"\xff", b"a" * 14 + b"\xff\xff"]
    ci = X.column_index(data, chunks["lengths"]["column_index"])
    assert all(len(v) <= 16 for v in ci["min_values"])
    assert (chunks["raw"]["min_value"], chunks["raw"]["max_value"]) == (b"\x00", b"\xfe")
    for limit in (1, 15, 17, 65536):
        data = write_and_check(pp, record, limit=limit)
        ci = X.column_index(data, {c["name"]: c for c in X.chunk_fields(data)}["lengths"]["column_index"])
        if limit == 1:
            assert set(ci["min_values"]) == {b"a"} and set(ci["max_values"]) <= {b"b", b"\xff" * 17}
        ff = X.column_index(data, {c["name"]: c for c in X.chunk_fields(data)}["ff"]["column_index"])
        if limit >= 17:   # nothing is cut
            assert ff["max_values"] == ff["min_values"] == [b"\xff" * 17, b"a" * 15 + b"\xffz", b"a" * 14 + b"\xff\xff\xff"]
        if limit == 15:
            assert ff["max_values"] == [b"\xff" * 17, b"a" * 14 + b"b", b"a" * 13 + b"b"] and ff["min_values"] == [b"\xff" * 15, b"a" * 15, b"a" * 14 + b"\xff"]


def test_boundary_order(pp):
    record = X.order_record()
    data = write_and_check(pp, record)
    got = {c["name"]: X.column_index(data, c["column_index"])["boundary_order"] for c in X.chunk_fields(data)}
    assert got == {"up": X.ASCENDING, "down": X.DESCENDING, "same": X.ASCENDING, "mixed": X.UNORDERED, "up_gap": X.ASCENDING, "down_gap": X.DESCENDING, "nested": X.UNORDERED,
                   "up_str": X.ASCENDING, "down_str": X.DESCENDING, "up_u64": X.ASCENDING, "flag_up": X.ASCENDING}
    gap = X.column_index(data, X.chunk_fields(data)[4]["column_index"])
    assert gap["null_pages"] == [False, False, True, False, False] and gap["min_values"][2] == b"" and gap["null_counts"][2] == PAGE
    one = pa.RecordBatch.from_arrays([pa.array([3, 1, 2], type=pa.int64()), pa.array([None, None, None], type=pa.float64())], names=["one", "none"])
    data = write_and_check(pp, one)
    assert [X.column_index(data, c["column_index"])["boundary_order"] for c in X.chunk_fields(data)] == [X.ASCENDING, X.ASCENDING]


# ---- 3. the rest of the footer, and the other encodings ----------------------------------------------------------------------------------------------
def test_sorting_columns(pp):
    record = cases.mixed_record(200, "alternate")
    want = [("timestamp",), ("labels.utf8", True), (2, False, True), ("flag", True, True)]
    for statistics in (None, "chunk", "page"):
        data = pp.selftest_parquet_write(record, page_rows=PAGE, statistics=statistics, sorting_columns=want)
        got = pq.ParquetFile(io.BytesIO(data)).metadata.row_group(0).sorting_columns
        assert [(s.column_index, s.descending, s.nulls_first) for s in got] == [(0, False, False), (4, True, False), (2, False, True), (3, True, True)]
        assert X.row_group_fields(data)["sorting_columns"] == [(0, False, False), (4, True, False), (2, False, True), (3, True, True)]
        cases.assert_same_record(read_back(data), record)
        if statistics is None:   # nothing else changes: the same file but for RowGroup field 4
            plain = pp.selftest_parquet_write(record, page_rows=PAGE)
            assert X.row_group_fields(data)["column_orders"] is None and len(data) - len(plain) == 2 + 4 * 5 and X.chunk_fields(data) == X.chunk_fields(plain)


@pytest.mark.parametrize("rows", [65, 1000, 4097])
def test_with_delta_and_snappy_columns(pp, rows):
    record = cases.mixed_record(rows, "whole_page")
    n = record.num_columns
    enc = {"timestamp": "delta", "dense": "delta"}
    for compression in ("snappy", ["snappy", None] * 4 + ["snappy"], {"labels.utf8": "snappy", "timestamp": "snappy"}, None):
        data = write_and_check(pp, record, encodings=enc, compression=compression)
        chunks = X.chunk_fields(data)
        assert X.row_group_fields(data)["total_compressed_size"] == sum(c["total_compressed_size"] for c in chunks)
        if compression is not None:   # the pages still inflate to the bodies of the uncompressed file
            plain = pp.selftest_parquet_write(record, page_rows=PAGE, encodings=enc)
            without = pp.selftest_parquet_write(record, page_rows=PAGE, encodings=enc, compression=compression)
            S.assert_compressed_file(pp, record, without, plain, compression)
            assert [c["total_compressed_size"] for c in chunks] == [c["total_compressed_size"] for c in X.chunk_fields(without)]
    assert n == 9


def test_the_projects_own_parser_accepts_the_chunks(pp):
    """The project's own reader parses row group 0: on a machine without a GPU it gets as far as the device call (FDB_ERR_DEVICE, the
    convention of tests/test_capi_cpu.py), never FDB_ERR_INVALID; with one it simply succeeds. And the chunks are, byte for byte, those
    of the file without an index: the index touches no page."""
    record = cases.mixed_record(1000, "alternate")
    kw = dict(page_rows=PAGE, encodings={"timestamp": "delta"}, compression={"value": "snappy"})
    data = pp.selftest_parquet_write(record, statistics="page", sorting_columns=[("timestamp",)], **kw)
    chunks, rows = row_group_chunks(data, 0)
    assert rows == 1000
    try:
        pp.ResidentBatch.from_parquet(chunks, rows).close()
    except pp.FdbError as e:
        assert e.code == pp.FDB_ERR_DEVICE, (e.code, str(e))
    assert [c[4] for c in chunks] == [c[4] for c in row_group_chunks(pp.selftest_parquet_write(record, **kw), 0)[0]]


# ---- 4. the unchanged path, refusals, names -------------------------------------------------------------------------------------------------------
def call_indexed(pp, record, index, page_rows=PAGE, codecs=None):
    opts = pp.ParquetWriteOptions(page_rows, 0, None)
    out, nb = ctypes.c_void_p(), ctypes.c_int64()
    arr = (ctypes.c_int8 * len(codecs))(*codecs) if codecs else None
    with pp.ExportedBatch(record) as ex:
        rc = pp.lib().fdb_selftest_parquet_write_indexed(ctypes.addressof(ex.array), ctypes.addressof(ex.schema), ctypes.byref(opts), None, 0, ctypes.cast(arr, ctypes.c_void_p) if codecs else None,
                                                         len(codecs) if codecs else 0, ctypes.byref(index) if index is not None else None, ctypes.byref(out), ctypes.byref(nb))
    if rc != 0:
        assert not out.value
        return rc, pp.lib().fdb_last_error().decode()
    try:
        return 0, ctypes.string_at(out.value, nb.value)
    finally:
        pp.lib().fdb_bytes_free(out.value)


def test_without_an_index_the_bytes_are_the_older_calls(pp):
    record = cases.mixed_record(1000, "alternate")
    n = record.num_columns
    for codecs, compression in ((None, None), ([1] * n, "snappy"), ([1, 0] * 4 + [1], ["snappy", None] * 4 + ["snappy"])):
        old = pp.selftest_parquet_write(record, page_rows=PAGE, compression=compression if compression else [None] * n)
        assert call_indexed(pp, record, None, codecs=codecs) == (0, old)
        assert call_indexed(pp, record, pp.ParquetIndexOptions(0, 0, None, 0), codecs=codecs) == (0, old)
        assert call_indexed(pp, record, pp.ParquetIndexOptions(0, 16, None, 0), codecs=codecs) == (0, old)
    assert pp.selftest_parquet_write(record, page_rows=PAGE, statistics=None, index_size_limit=0, sorting_columns=None) == pp.selftest_parquet_write(record, page_rows=PAGE)
    assert pp.selftest_parquet_write(record, page_rows=PAGE, sorting_columns=[]) == pp.selftest_parquet_write(record, page_rows=PAGE)


def test_refusals(pp):
    record = cases.mixed_record(100, "alternate")
    n = record.num_columns
    sort = lambda *cols: (pp.ParquetSortingColumn * len(cols))(*[pp.ParquetSortingColumn(c, 0, 0) for c in cols])
    for statistics in (-1, 3, 100):
        rc, text = call_indexed(pp, record, pp.ParquetIndexOptions(statistics, 0, None, 0))
        assert rc == pp.FDB_ERR_INVALID and "statistics is %d" % statistics in text
    for limit in (-1, 65537, 2**31 - 1):
        for statistics in (0, 2):
            rc, text = call_indexed(pp, record, pp.ParquetIndexOptions(statistics, limit, None, 0))
            assert rc == pp.FDB_ERR_INVALID and "index_size_limit is %d" % limit in text
    for cols, text in (((n,), "outside the record's"), ((-1,), "outside the record's"), ((0, 1, 0), "named twice")):
        arr = sort(*cols)
        rc, got = call_indexed(pp, record, pp.ParquetIndexOptions(0, 0, ctypes.cast(arr, ctypes.c_void_p), len(cols)))
        assert rc == pp.FDB_ERR_INVALID and text in got, (cols, got)
    rc, got = call_indexed(pp, record, pp.ParquetIndexOptions(1, 0, None, 2))
    assert rc == pp.FDB_ERR_INVALID and "sorting_columns" in got
    rc, got = call_indexed(pp, record, pp.ParquetIndexOptions(1, 0, None, -1))
    assert rc == pp.FDB_ERR_INVALID and "sorting_columns" in got
    # everything the older calls refuse stays refused
    rc, got = call_indexed(pp, record, pp.ParquetIndexOptions(2, 0, None, 0), page_rows=100)
    assert rc == pp.FDB_ERR_INVALID and "page_rows" in got
    rc, got = call_indexed(pp, record, pp.ParquetIndexOptions(2, 0, None, 0), codecs=[2] + [0] * (n - 1))
    assert rc == pp.FDB_ERR_INVALID and "codecs[0] is 2" in got
    with pytest.raises(pp.FdbError) as e:
        pp.selftest_parquet_write(record, statistics="page", encodings={"value": "delta"})
    assert e.value.code == pp.FDB_ERR_UNSUPPORTED and "DELTA" in str(e.value)
    # the binding's own
    for kw, text in (({"statistics": "pages"}, "unknown statistics"), ({"statistics": 2}, "unknown statistics"), ({"statistics": "page", "index_size_limit": 70000}, "index_size_limit"),
                     ({"index_size_limit": -5}, "index_size_limit"), ({"sorting_columns": ["nobody"]}, "nobody"), ({"sorting_columns": [("timestamp",), ("timestamp", True)]}, "named twice"),
                     ({"sorting_columns": [(n,)]}, "outside the record's"), ({"sorting_columns": [()]}, "a sorting column is"), ({"sorting_columns": [(1.5,)]}, "a name or an index")):
        with pytest.raises(pp.FdbError) as e:
            pp.selftest_parquet_write(record, **kw)
        assert e.value.code == pp.FDB_ERR_INVALID and text in str(e.value), kw
    # a row that points past its dictionary is still the survey's to refuse, and the min / max pass does not follow it
    bad = pa.DictionaryArray.from_arrays(pa.array([0, 1, 0], type=pa.uint32()), pa.array([b"a", b"b"], type=pa.binary()))
    buffers = bad.indices.buffers()
    idx = np.frombuffer(buffers[1], dtype=np.uint32).copy()
    idx[1] = 7
    wrong = pa.DictionaryArray.from_arrays(pa.Array.from_buffers(pa.uint32(), 3, [None, pa.py_buffer(idx.tobytes())]), bad.dictionary, safe=False)
    with pytest.raises(pp.FdbError) as e:
        pp.selftest_parquet_write(pa.RecordBatch.from_arrays([wrong], names=["d"]), statistics="page")
    assert e.value.code == pp.FDB_ERR_INVALID and "out of range" in str(e.value)


def test_entry_points_are_in_library_header_exports_and_binding(pp):
    L = pp.lib()
    header = open(os.path.join(ROOT, "include", "frostdb_amd.h")).read()
    exports = open(os.path.join(ROOT, "frostdb_amd", "csrc", "exports.map")).read()
    for name in ENTRY_POINTS:
        assert re.search(r"^FDB_API int %s\(.*const fdb_parquet_index_options\* index /\* NULL: none \*/, uint8_t\*\* bytes, int64_t\* n_bytes\);" % name, header, flags=re.M), name
        assert name in exports and re.search(r"global:\s*fdb_\*;", exports)
        assert getattr(L, name).argtypes is not None
    assert [f[0] for f in pp.ParquetWriteOptions._fields_] == ["page_rows", "n_optional", "optional"] and ctypes.sizeof(pp.ParquetWriteOptions) == 16
    assert [f[0] for f in pp.ParquetIndexOptions._fields_] == ["statistics", "index_size_limit", "sorting_columns", "n_sorting_columns"] and ctypes.sizeof(pp.ParquetIndexOptions) == 24
    assert ctypes.sizeof(pp.ParquetSortingColumn) == 8
    assert "fdb_pqstats.hip" in open(os.path.join(ROOT, "frostdb_amd", "build.py")).read()


def test_minmax_kernel_compiles_for_gfx950_without_scratch(tmp_path):
    """fdb_pqstats.hip compiled offline for gfx950 with the flags of the writer's compile test: the resource report shows the kernel, no
    scratch and no spills."""
    src = os.path.join(ROOT, "frostdb_amd", "csrc", "fdb_pqstats.hip")
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-munsafe-fp-atomics", "-I", os.path.join(ROOT, "frostdb_amd", "csrc"),
                        "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", str(tmp_path / "fdb_pqstats.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    remarks = [ln.split("remark: ")[-1].replace(" [-Rpass-analysis=kernel-resource-usage]", "").strip() for ln in r.stderr.splitlines() if "remark:" in ln]
    names = [u for u in remarks if u.startswith("Function Name:")]
    print(" | ".join(remarks))
    assert len(names) == 1 and "pqx_minmax_kernel" in names[0], names
    scratch = [u for u in remarks if "ScratchSize" in u]
    assert len(scratch) == 1 and "ScratchSize [bytes/lane]: 0" in scratch[0], remarks
    spills = [u for u in remarks if "Spill" in u]
    assert spills and all(re.search(r"Spill: 0\b", u) for u in spills), remarks
