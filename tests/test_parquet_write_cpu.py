"""CPU-side checks of the Parquet writer (fdb_batch_to_parquet): fdb_selftest_parquet_write runs the writer's layout, thrift, dictionary
page and tail code over a host record, the two kernels replaced by a host walk of the arithmetic they compile (fdb_pqwrite.h) — the file
is byte for byte what the device path writes (tests/test_gpu_parquet_write.py holds the two against each other). Here pyarrow reads the
files back to the records, the project's own parser accepts them, every refusal returns its code, and fdb_pqwrite.hip compiles for
gfx950 without scratch. No GPU is touched."""
import io
import os
import re
import subprocess

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq
import pytest

from tests import parquet_write_cases as cases
from tests.parquet_util import row_group_chunks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

ENTRY_POINTS = ["fdb_batch_to_parquet", "fdb_selftest_parquet_write", "fdb_bytes_free"]


@pytest.fixture(scope="module")
def pp():
    from frostdb_amd import physicalplan
    return physicalplan


def parser_accepts(pp, data: bytes) -> None:
    """The project's own reader parses row group 0 of `data`: on a machine without a GPU it gets as far as the device call
    (FDB_ERR_DEVICE, the convention of tests/test_capi_cpu.py), never FDB_ERR_INVALID; with one it simply succeeds."""
    chunks, rows = row_group_chunks(data, 0)
    try:
        pp.ResidentBatch.from_parquet(chunks, rows).close()
    except pp.FdbError as e:
        assert e.code == pp.FDB_ERR_DEVICE, (e.code, str(e))


@pytest.mark.parametrize("pattern", cases.NULL_PATTERNS)
@pytest.mark.parametrize("rows", cases.ROWS)
def test_every_column_kind_round_trips_through_pyarrow(pp, rows, pattern):
    record = cases.mixed_record(rows, pattern)
    data = pp.selftest_parquet_write(record, page_rows=cases.PAGE)
    cases.assert_reads_back(record, data)
    if rows > 0:
        parser_accepts(pp, data)


def test_a_zero_row_record_is_a_valid_file_with_a_zero_row_row_group(pp):
    record = cases.mixed_record(0, "none")
    for page_rows in (0, 64):
        data = pp.selftest_parquet_write(record, page_rows=page_rows)
        md = cases.assert_reads_back(record, data)
        assert md.num_row_groups == 1 and md.row_group(0).num_rows == 0
    no_columns = pa.RecordBatch.from_arrays([], names=[])
    md = pq.ParquetFile(io.BytesIO(pp.selftest_parquet_write(no_columns))).metadata
    assert md.num_rows == 0 and md.num_columns == 0


@pytest.mark.parametrize("entries", cases.DICT_SIZES)
def test_dictionary_sizes_pack_at_the_width_of_their_last_index(pp, entries):
    rows = 1000
    record = cases.dict_record(rows, entries)
    data = pp.selftest_parquet_write(record, page_rows=cases.PAGE)
    md = cases.assert_reads_back(record, data)
    parser_accepts(pp, data)
    col = md.row_group(0).column(0)
    assert col.has_dictionary_page and set(col.encodings) == {"PLAIN", "RLE", "RLE_DICTIONARY"}
    width = (entries - 1).bit_length()
    pages = -(-rows // cases.PAGE)
    data_bytes = col.total_compressed_size - (col.data_page_offset - col.dictionary_page_offset)
    values = rows - record.column(0).null_count
    # the data pages hold the packed indices, per page a header (< 32 bytes), 4 + 2 + 8 level bytes, the width byte and a run header (≤ 2),
    # and up to 7 padding values: one bit more per index would not fit
    assert data_bytes <= values * width // 8 + pages * (32 + 14 + 3 + width), (entries, data_bytes)
    assert data_bytes >= values * width // 8
    # the dictionary page is the dictionary, entry by entry
    got = pq.read_table(io.BytesIO(data), read_dictionary=["labels.d"]).column(0).combine_chunks()
    assert got.dictionary.to_pylist() == record.column(0).dictionary.to_pylist()


def test_duplicate_dictionary_entries_stay_in_entry_order(pp):
    record = cases.duplicates_record()
    data = pp.selftest_parquet_write(record, page_rows=cases.PAGE)
    cases.assert_reads_back(record, data)
    parser_accepts(pp, data)
    # (pyarrow's dictionary reader merges equal entries, so the page is looked at as bytes: four PLAIN BYTE_ARRAY values behind its header)
    col = pq.ParquetFile(io.BytesIO(data)).metadata.row_group(0).column(0)
    page = data[col.dictionary_page_offset:col.data_page_offset]
    body = b"\x01\x00\x00\x00a" + b"\x01\x00\x00\x00b" + b"\x01\x00\x00\x00a" + b"\x00\x00\x00\x00"
    assert page.endswith(body) and len(page) - len(body) < 24


def test_pages_of_one_repeated_index_are_one_rle_run(pp):
    record = cases.rle_record()
    data = pp.selftest_parquet_write(record, page_rows=cases.PAGE)
    md = cases.assert_reads_back(record, data)
    parser_accepts(pp, data)
    # the ordered column: every page is one run — header, 6 level bytes, the width byte, a run header and two value bytes
    col = md.row_group(0).column(0)
    pages = -(-record.num_rows // cases.PAGE)
    assert col.total_compressed_size - (col.data_page_offset - col.dictionary_page_offset) <= pages * (32 + 6 + 1 + 2 + 2)
    # the same indices shuffled do not fit that
    rng = np.random.default_rng(5)
    perm = rng.permutation(record.num_rows)
    shuffled = pp.selftest_parquet_write(record.take(pa.array(perm)), page_rows=cases.PAGE)
    assert len(shuffled) > len(data)


def test_numeric_extremes_keep_every_bit(pp):
    record = cases.extremes_record()
    data = pp.selftest_parquet_write(record, page_rows=cases.PAGE)
    cases.assert_reads_back(record, data)
    parser_accepts(pp, data)
    got = pq.read_table(io.BytesIO(data))
    assert [hex(v) for v in cases._bits(got.column("f"))[:len(cases.F64_BITS)]] == [hex(v) for v in cases.F64_BITS]


def test_large_string_and_binary_columns_are_written_as_plain_ones(pp):
    record = cases.large_strings_record()
    data = pp.selftest_parquet_write(record, page_rows=cases.PAGE)
    cases.assert_reads_back(record, data)
    parser_accepts(pp, data)


def test_an_all_null_column_with_an_empty_dictionary_has_no_dictionary_page(pp):
    """The project's parser refuses bit width 0 into an empty dictionary (tests/test_capi_cpu.py), so such a column is written without a
    dictionary page, its data pages PLAIN with zero values: pyarrow and the parser both read it."""
    record = cases.empty_dictionary_record()
    data = pp.selftest_parquet_write(record, page_rows=cases.PAGE)
    md = cases.assert_reads_back(record, data)
    parser_accepts(pp, data)
    col = md.row_group(0).column(0)
    assert not col.has_dictionary_page and col.dictionary_page_offset is None
    assert set(col.encodings) == {"PLAIN", "RLE"} and col.physical_type == "BYTE_ARRAY"
    assert col.statistics.null_count == record.num_rows
    # per page: header, 4 length bytes, one RLE run of definition level 0 (2 bytes) — and nothing else
    pages = -(-record.num_rows // cases.PAGE)
    assert col.total_compressed_size <= pages * (32 + 6)


def test_default_page_rows_and_explicit_optional(pp):
    record = cases.mixed_record(1000, "none")
    assert pp.selftest_parquet_write(record) == pp.selftest_parquet_write(record, page_rows=65536)
    names = record.schema.names
    # no column holds a NULL: each may be required or optional, by position or by name
    data = pp.selftest_parquet_write(record, page_rows=cases.PAGE, optional=[False] * len(names))
    md = cases.assert_reads_back(record, data, optional={n: False for n in names})
    parser_accepts(pp, data)
    # a required column has no definition levels: its chunk names no RLE
    assert [set(md.row_group(0).column(j).encodings) for j in (0, 4)] == [{"PLAIN"}, {"PLAIN", "RLE_DICTIONARY"}]
    data = pp.selftest_parquet_write(record, page_rows=cases.PAGE, optional={"timestamp": True, "labels.utf8": False})
    cases.assert_reads_back(record, data, optional={"timestamp": True, "labels.utf8": False})
    parser_accepts(pp, data)
    assert pp.selftest_parquet_write(record, page_rows=cases.PAGE, optional=[None] * len(names)) == pp.selftest_parquet_write(record, page_rows=cases.PAGE)


def test_sliced_records_are_written_from_their_offset(pp):
    record = cases.mixed_record(1000, "alternate").slice(37, 333)
    data = pp.selftest_parquet_write(record, page_rows=cases.PAGE)
    cases.assert_reads_back(record, data)


@pytest.mark.parametrize("page_rows", [1, 63, 65, 100, 32, -64, (1 << 24) + 64, 1 << 25])
def test_page_rows_outside_the_rule_are_refused(pp, page_rows):
    with pytest.raises(pp.FdbError) as e:
        pp.selftest_parquet_write(cases.mixed_record(9, "none"), page_rows=page_rows)
    assert e.value.code == pp.FDB_ERR_INVALID and "page_rows" in str(e.value)


def test_page_rows_at_both_ends_of_the_rule_are_taken(pp):
    record = cases.mixed_record(129, "alternate")
    for page_rows in (64, 128, 1 << 24):
        cases.assert_reads_back(record, pp.selftest_parquet_write(record, page_rows=page_rows))


def test_refusals_return_their_codes(pp):
    record = cases.mixed_record(65, "alternate")
    n = record.num_columns
    for optional in ([], [False] * (n - 1), [False] * (n + 1), [2] * n, [-2] * n):   # another length; an entry outside -1 … 1
        with pytest.raises(pp.FdbError) as e:
            pp.selftest_parquet_write(record, optional=optional)
        assert e.value.code == pp.FDB_ERR_INVALID, optional
    with pytest.raises(pp.FdbError) as e:                                          # required asked of a column that holds NULLs
        pp.selftest_parquet_write(record, optional={"value": False})
    assert e.value.code == pp.FDB_ERR_INVALID and "value" in str(e.value) and "NULL" in str(e.value)
    with pytest.raises(pp.FdbError) as e:
        pp.selftest_parquet_write(record, optional={"no such column": True})
    assert e.value.code == pp.FDB_ERR_INVALID
    odd = pa.RecordBatch.from_arrays([pa.array([1, 2, 3], type=pa.int32()), pa.array([1, 2, 3], type=pa.int64())], names=["narrow", "wide"])
    with pytest.raises(pp.FdbError) as e:                                          # a column kind the resident record does not hold
        pp.selftest_parquet_write(odd)
    assert e.value.code == pp.FDB_ERR_UNSUPPORTED and "narrow" in str(e.value)
    bad = pa.DictionaryArray.from_arrays(pa.array([0, 5, 1], type=pa.uint32()), pa.array([b"a", b"b"], type=pa.binary()), safe=False)
    with pytest.raises(pp.FdbError) as e:                                          # an index beyond the dictionary
        pp.selftest_parquet_write(pa.RecordBatch.from_arrays([bad], names=["labels.bad"]))
    assert e.value.code == pp.FDB_ERR_INVALID and "out of range" in str(e.value)


@pytest.mark.parametrize("kw,code,text", cases.DOUBLY_WRONG)
def test_a_doubly_wrong_call_is_refused_for_the_earlier_parameter(pp, kw, code, text):
    with pytest.raises(pp.FdbError) as e:
        pp.selftest_parquet_write(cases.mixed_record(64, "alternate"), page_rows=cases.PAGE, **kw)
    assert e.value.code == getattr(pp, code) and text in str(e.value), str(e.value)


def test_entry_points_are_in_library_header_and_binding(pp):
    L = pp.lib()
    header = open(os.path.join(ROOT, "include", "frostdb_amd.h")).read()
    for name in ENTRY_POINTS:
        assert re.search(r"^FDB_API (?:int|void) %s\(" % name, header, flags=re.M), name
        assert getattr(L, name).argtypes is not None
    assert "typedef struct fdb_parquet_write_options" in header
    assert [f[0] for f in pp.ParquetWriteOptions._fields_] == ["page_rows", "n_optional", "optional"]
    L.fdb_bytes_free(None)  # NULL is a no-op


def test_write_kernels_compile_for_gfx950_without_scratch(tmp_path):
    """fdb_pqwrite.hip compiled offline for gfx950: the compiler's resource report shows the survey and the encode kernel, no scratch and
    no spills (resource usage only, as tests/test_sort_cpu.py checks its kernels)."""
    src = os.path.join(ROOT, "frostdb_amd", "csrc", "fdb_pqwrite.hip")
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-munsafe-fp-atomics", "-I", os.path.join(ROOT, "frostdb_amd", "csrc"),
                        "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", str(tmp_path / "fdb_pqwrite.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    remarks = [ln.split("remark: ")[-1].replace(" [-Rpass-analysis=kernel-resource-usage]", "").strip() for ln in r.stderr.splitlines() if "remark:" in ln]
    names = [u for u in remarks if u.startswith("Function Name:")]
    print(" | ".join(remarks))
    assert len(names) == 2 and any("pqw_survey_kernel" in u for u in names) and any("pqw_encode_kernel" in u for u in names), names
    scratch = [u for u in remarks if "ScratchSize" in u]
    assert len(scratch) == len(names) and all("ScratchSize [bytes/lane]: 0" in u for u in scratch), remarks
    spills = [u for u in remarks if "Spill" in u]
    assert spills and all(re.search(r"Spill: 0\b", u) for u in spills), remarks
