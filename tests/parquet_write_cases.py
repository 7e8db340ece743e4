"""Records and comparisons shared by tests/test_parquet_write_cpu.py (the host walk, fdb_selftest_parquet_write) and
tests/test_gpu_parquet_write.py (the device encoders, fdb_batch_to_parquet): the shapes both must get right, and what "pyarrow reads the
file back to the record" means — numeric columns by their bits under valid rows, NULL positions exactly, dictionary and string columns as
decoded values, names / order / logical types / null_count in the metadata."""
import io

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq

PAGE = 64  # page_rows of the small shapes: one page, exact pages, pages + 1

ROWS = [0, 1, 7, 8, 9, 63, 64, 65, 127, 128, 129, 1000]
NULL_PATTERNS = ["none", "all", "alternate", "first_of_page", "last_of_page", "whole_page"]
DICT_SIZES = [1, 2, 3, 4, 5, 255, 256, 257, 65536, 65537]  # widths 0, 1, 2, 2, 3, 8, 8, 9, 16, 17

# Calls on mixed_record() that are wrong in two ways at once: (options, the code's name, a piece of the text). The writer checks its
# options in the parameters' order — write options and columns, index, bloom, runs — so the refusal is that of the EARLIER parameter,
# from the host walk and from the device alike.
DOUBLY_WRONG = [
    ({"bloom_filters": ["flag"], "runs": {"timestamp": "values"}}, "FDB_ERR_UNSUPPORTED", "a bloom filter is not written for a boolean column (flag)"),
    ({"index_size_limit": 70000, "bloom_filters": ["timestamp"], "bloom_bits_per_value": 65}, "FDB_ERR_INVALID", "index_size_limit is 70000"),
]


def valid_mask(rows: int, pattern: str, page: int = PAGE) -> np.ndarray:
    """True = the row holds a value."""
    r = np.arange(rows)
    if pattern == "none":
        return np.ones(rows, dtype=bool)
    if pattern == "all":
        return np.zeros(rows, dtype=bool)
    if pattern == "alternate":
        return r % 2 == 0
    if pattern == "first_of_page":   # only the first row of every page is NULL
        return r % page != 0
    if pattern == "last_of_page":
        return r % page != page - 1
    if pattern == "whole_page":      # the second page NULL between two that are not
        return r // page != 1
    raise ValueError(pattern)


def _masked(values, valid, typ):
    return pa.array(values, type=typ, mask=~valid)


def dict_entries(n: int, utf8: bool):
    return [("entry-%d" % i) if utf8 else b"e%d" % i for i in range(n)]


def mixed_record(rows: int, pattern: str, seed: int = 0, dict_size: int = 5) -> pa.RecordBatch:
    """Every column kind the resident record holds, each with the NULL pattern (shifted per column where that keeps it a pattern)."""
    rng = np.random.default_rng(seed + rows)
    valid = valid_mask(rows, pattern)
    i64 = rng.integers(-2**62, 2**62, rows, dtype=np.int64)
    u64 = rng.integers(0, 2**64, rows, dtype=np.uint64)
    f64 = rng.standard_normal(rows)
    flag = rng.random(rows) < 0.5
    idx = rng.integers(0, dict_size, rows).astype(np.uint32)
    if rows:
        idx[-1] = dict_size - 1  # the widest index is there
    words = np.array(["w%d" % (v % 11) for v in rng.integers(0, 1000, rows)], dtype=object)
    blobs = np.array([b"\x00b%d" % (v % 7) for v in rng.integers(0, 1000, rows)], dtype=object)
    cols = [
        ("timestamp", _masked(i64, valid, pa.int64())),
        ("count", _masked(u64, valid, pa.uint64())),
        ("value", _masked(f64, valid, pa.float64())),
        ("flag", _masked(flag, valid, pa.bool_())),
        ("labels.utf8", pa.DictionaryArray.from_arrays(_masked(idx, valid, pa.uint32()), pa.array(dict_entries(dict_size, True), type=pa.string()))),
        ("labels.bin", pa.DictionaryArray.from_arrays(_masked(idx[::-1].copy(), valid, pa.uint32()), pa.array(dict_entries(dict_size, False), type=pa.binary()))),
        ("plain_str", _masked(words, valid, pa.string())),
        ("plain_bin", _masked(blobs, valid, pa.binary())),
        ("dense", pa.array(i64[::-1].copy(), type=pa.int64())),  # never NULL: a required column, copied as it is
    ]
    return pa.RecordBatch.from_arrays([c for _, c in cols], names=[n for n, _ in cols])


def dict_record(rows: int, entries: int, pattern: str = "alternate", seed: int = 0) -> pa.RecordBatch:
    """One dictionary column that uses its first and last entry, beside an int64."""
    rng = np.random.default_rng(seed + entries)
    valid = valid_mask(rows, pattern)
    idx = rng.integers(0, entries, rows).astype(np.uint32)
    hold = np.flatnonzero(valid)
    if len(hold) >= 2:
        idx[hold[0]], idx[hold[-1]] = 0, entries - 1
    d = pa.DictionaryArray.from_arrays(_masked(idx, valid, pa.uint32()), pa.array(dict_entries(entries, False), type=pa.binary()))
    return pa.RecordBatch.from_arrays([d, pa.array(np.arange(rows, dtype=np.int64))], names=["labels.d", "timestamp"])


def rle_record(rows: int = 6 * PAGE + 5) -> pa.RecordBatch:
    """Pages of one repeated index — with and without NULLs, the leading sorting column of an ordered record — beside mixed pages, and a
    page whose equal indices are all NULL but one."""
    r = np.arange(rows)
    page = r // PAGE
    idx = np.where(page % 2 == 0, page % 7, r % 7).astype(np.uint32)
    valid = np.ones(rows, dtype=bool)
    valid[(page == 2) & (r % 3 == 0)] = False
    valid[(page == 4)] = False
    valid[4 * PAGE + 9] = True
    d = pa.DictionaryArray.from_arrays(_masked(idx, valid, pa.uint32()), pa.array(dict_entries(7, True), type=pa.string()))
    ordered = pa.DictionaryArray.from_arrays(pa.array((page // 3).astype(np.uint32)), pa.array(dict_entries(300, True), type=pa.string()))
    return pa.RecordBatch.from_arrays([ordered, d], names=["labels.ordered", "labels.d"])


F64_BITS = [0x7FF8000000000000, 0xFFF8000000000000, 0x7FF0000000000001, 0x7FFFFFFFFFFFFFFF, 0xFFF00000DEADBEEF,  # NaNs, payloads kept
            0x0000000000000000, 0x8000000000000000, 0x7FF0000000000000, 0xFFF0000000000000, 0x0000000000000001, 0x7FEFFFFFFFFFFFFF]


def extremes_record() -> pa.RecordBatch:
    n = 3 * PAGE + 1
    i64 = np.resize(np.array([-2**63, 2**63 - 1, -1, 0, 1], dtype=np.int64), n)
    u64 = np.resize(np.array([0, 2**64 - 1, 2**63, 2**63 - 1, 1], dtype=np.uint64), n)
    f64 = np.resize(np.array(F64_BITS, dtype=np.uint64), n).view(np.float64)
    valid = np.arange(n) % 5 != 3
    return pa.RecordBatch.from_arrays([pa.array(i64), _masked(i64, valid, pa.int64()), pa.array(u64), _masked(u64, valid, pa.uint64()), pa.array(f64), _masked(f64, valid, pa.float64())],
                                      names=["i", "i_null", "u", "u_null", "f", "f_null"])


def duplicates_record() -> pa.RecordBatch:
    idx = np.resize(np.array([0, 1, 2, 3, 2, 0], dtype=np.uint32), 2 * PAGE + 3)
    d = pa.DictionaryArray.from_arrays(pa.array(idx), pa.array([b"a", b"b", b"a", b""], type=pa.binary()))
    return pa.RecordBatch.from_arrays([d], names=["labels.dup"])


def empty_dictionary_record(rows: int = PAGE + 3) -> pa.RecordBatch:
    e = pa.DictionaryArray.from_arrays(pa.array([None] * rows, type=pa.uint32()), pa.array([], type=pa.string()))
    return pa.RecordBatch.from_arrays([e, pa.array(np.arange(rows, dtype=np.int64))], names=["labels.none", "timestamp"])


def large_strings_record(rows: int = PAGE + 9) -> pa.RecordBatch:
    valid = valid_mask(rows, "alternate")
    s = np.array(["large-%d" % (i % 5) for i in range(rows)], dtype=object)
    return pa.RecordBatch.from_arrays([_masked(s, valid, pa.large_string()), pa.array([b"z%d" % (i % 3) for i in range(rows)], type=pa.large_binary())], names=["ls", "lb"])


# ---- comparison -------------------------------------------------------------------------------------------------------------------------------
def _bits(arr: pa.Array) -> np.ndarray:
    """The 8-byte values of an int64 / uint64 / float64 array as uint64, NULL slots as they lie."""
    arr = arr.combine_chunks() if isinstance(arr, pa.ChunkedArray) else arr
    buf = arr.buffers()[1]
    if buf is None or len(arr) == 0:
        return np.zeros(len(arr), dtype=np.uint64)
    return np.frombuffer(buf, dtype=np.uint64)[arr.offset:arr.offset + len(arr)]


def _validity(arr) -> np.ndarray:
    arr = arr.combine_chunks() if isinstance(arr, pa.ChunkedArray) else arr
    return np.asarray(arr.is_valid()).astype(bool) if len(arr) else np.zeros(0, dtype=bool)


def _decoded(arr) -> pa.Array:
    """Without its dictionary, string-like values as binary: they are compared by their bytes."""
    arr = arr.combine_chunks() if isinstance(arr, pa.ChunkedArray) else arr
    if pa.types.is_dictionary(arr.type):
        arr = arr.dictionary_decode()
    return arr.cast(pa.large_binary())


def logical_type_of(typ: pa.DataType) -> str:
    """What str(ColumnSchema.logical_type) starts with for a column of Arrow type `typ`."""
    if pa.types.is_dictionary(typ):
        typ = typ.value_type
    if pa.types.is_string(typ) or pa.types.is_large_string(typ):
        return "String"
    if pa.types.is_uint64(typ):
        return "Int(bitWidth=64, isSigned=false)"
    return "None"


PHYSICAL = {pa.int64(): "INT64", pa.uint64(): "INT64", pa.float64(): "DOUBLE", pa.bool_(): "BOOLEAN"}


def assert_reads_back(record: pa.RecordBatch, data: bytes, optional=None) -> pq.FileMetaData:
    """pyarrow reads `data` back to `record`. `optional`: {name: bool} where the test asked for it; else the automatic rule."""
    assert data[:4] == b"PAR1" and data[-4:] == b"PAR1"
    pf = pq.ParquetFile(io.BytesIO(data))
    md = pf.metadata
    assert md.num_rows == record.num_rows and md.num_row_groups == 1 and md.num_columns == record.num_columns
    rg = md.row_group(0)
    assert rg.num_rows == record.num_rows
    table = pf.read()
    assert table.num_rows == record.num_rows
    assert table.schema.names == record.schema.names
    for j, name in enumerate(record.schema.names):
        want, got = record.column(j), table.column(j)
        typ = want.type
        col, sc = rg.column(j), pf.schema.column(j)
        assert col.path_in_schema == name and sc.name == name
        assert col.compression == "UNCOMPRESSED" and col.num_values == record.num_rows
        assert str(sc.logical_type).replace(" ", "").startswith(logical_type_of(typ).replace(" ", "")), (name, str(sc.logical_type))
        stringish = pa.types.is_dictionary(typ) or typ in (pa.string(), pa.binary(), pa.large_string(), pa.large_binary())
        assert col.physical_type == ("BYTE_ARRAY" if stringish else PHYSICAL[typ]), name
        auto = want.null_count > 0 or stringish
        assert sc.max_definition_level == int(optional[name] if optional and optional.get(name) is not None else auto), name
        assert sc.max_repetition_level == 0
        assert col.statistics is not None and col.statistics.null_count == want.null_count, name
        assert not col.statistics.has_min_max
        np.testing.assert_array_equal(_validity(got), _validity(want), err_msg=name)
        if stringish:
            assert _decoded(got).equals(_decoded(want)), name
        elif typ == pa.bool_():
            assert got.to_pylist() == want.to_pylist(), name
        else:
            assert got.type == typ, (name, got.type)
            ok = _validity(want)
            np.testing.assert_array_equal(_bits(got)[ok], _bits(want)[ok], err_msg=name)
    return md


def assert_same_record(got: pa.RecordBatch, want: pa.RecordBatch, what="") -> None:
    """Two records hold the same: names and order, NULL positions exactly, dictionary / string columns as decoded bytes, bools as they
    are, 8-byte columns by their bits on the valid rows (and by type)."""
    assert got.schema.names == want.schema.names, what
    assert got.num_rows == want.num_rows, (what, got.num_rows, want.num_rows)
    for j, name in enumerate(want.schema.names):
        g, w = got.column(j), want.column(j)
        np.testing.assert_array_equal(_validity(g), _validity(w), err_msg="%s %s: NULL positions" % (what, name))
        if pa.types.is_dictionary(w.type) or w.type in (pa.string(), pa.binary(), pa.large_string(), pa.large_binary()):
            assert _decoded(g).equals(_decoded(w)), (what, name)
        elif w.type == pa.bool_():
            assert g.type == w.type and g.fill_null(False).equals(w.fill_null(False)), (what, name)
        else:
            assert g.type == w.type, (what, name, g.type, w.type)
            ok = _validity(w)
            np.testing.assert_array_equal(_bits(g)[ok], _bits(w)[ok], err_msg="%s %s" % (what, name))
