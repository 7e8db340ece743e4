"""CPU-side checks of DELTA_BINARY_PACKED in the Parquet writer (fdb_batch_to_parquet_encoded): fdb_selftest_parquet_write_encoded runs the
writer over a host record, the DELTA kernels replaced by a host walk of the arithmetic they compile (fdb_pqdelta.h) — byte for byte the
file the device path writes (tests/test_gpu_parquet_delta.py holds the two against each other). Here, for every value family, row count,
page size and NULL pattern: pyarrow reads the file back to the record, bits exact; the chunk names DELTA_BINARY_PACKED (+ RLE when
optional) and no PLAIN; every page's value bytes are tests/parquet_pages.py::delta_binary_packed of the page's non-NULL values — the
byte oracle, written from the format specification and sharing nothing with the library; and the project's own parser accepts the file.
No GPU is touched."""
import functools
import io
import os
import re
import subprocess

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq
import pytest

from tests import parquet_pages as P
from tests import parquet_write_cases as cases
from tests.parquet_util import row_group_chunks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

ROWS = [0, 1, 2, 32, 33, 34, 64, 65, 128, 129, 130, 257, 258, 1000, 4097]
PAGE_ROWS = [64, 128, 192, 4160, 0]   # 0: the default, 65 536
ENTRY_POINTS = ["fdb_batch_to_parquet_encoded", "fdb_selftest_parquet_write_encoded"]


@pytest.fixture(scope="module")
def pp():
    from frostdb_amd import physicalplan
    return physicalplan


def parser_accepts(pp, data: bytes) -> None:
    """As in tests/test_parquet_write_cpu.py: the project's reader parses row group 0 — without a GPU it gets as far as the device call
    (FDB_ERR_DEVICE), never FDB_ERR_INVALID; with one it succeeds."""
    chunks, rows = row_group_chunks(data, 0)
    try:
        pp.ResidentBatch.from_parquet(chunks, rows).close()
    except pp.FdbError as e:
        assert e.code == pp.FDB_ERR_DEVICE, (e.code, str(e))


# ---- value families ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def families(rows: int, seed: int = 0):
    """[(name, uint64 bit patterns)]: every value family at `rows` rows (computed once per row count; nobody writes to them)."""
    rng = np.random.default_rng(1000 * seed + rows)
    r = np.arange(rows, dtype=np.uint64)
    out = [("constant", np.full(rows, 0x0123456789ABCDEF, dtype=np.uint64)),
           ("stride_up", np.uint64(5) + r * np.uint64(1000)),
           ("stride_down", np.uint64(2**62) - r * np.uint64(37)),                                       # a negative stride
           ("stride_wraps", np.uint64(2**64 - 300) + r * np.uint64(7)),                                 # … through 2^64 / through 0
           ("steps", np.cumsum(rng.integers(0, 2000, rows, dtype=np.int64)).astype(np.int64).view(np.uint64)),
           ("steps_both_ways", np.cumsum(rng.integers(-50, 50, rows, dtype=np.int64)).view(np.uint64)),
           ("random", rng.integers(0, 2**64, rows, dtype=np.uint64)),
           ("alternating", np.where(r % 2 == 0, np.uint64(P.INT64_MAX), np.uint64(1 << 63))),          # INT64_MAX / INT64_MIN
           ("high", np.uint64(1 << 63) + rng.integers(0, 2**63, rows, dtype=np.uint64)),                # uint64 values at and above 2^63
           ("at_2_63", np.where(r % 3 == 0, np.uint64(1 << 63), np.uint64((1 << 63) - 1) + r))]
    for w in range(65):
        v = P.delta_values_of_width(rng, rows, w, 128, 4).view(np.uint64) if rows > 0 else np.zeros(0, dtype=np.uint64)
        out.append(("w%02d" % w, v))
    return [(n, np.ascontiguousarray(v, dtype=np.uint64)) for n, v in out]


def family_record(rows: int, pattern: str, page: int):
    """Every family as an int64 and as a uint64 column with the NULL pattern (pages of `page` rows), and the `encodings` that ask all of
    them to be DELTA."""
    valid = cases.valid_mask(rows, pattern, page)
    cols, names = [], []
    for name, bits in families(rows):
        cols.append(pa.array(bits.view(np.int64), type=pa.int64(), mask=~valid))
        names.append("i." + name)
        cols.append(pa.array(bits, type=pa.uint64(), mask=~valid))
        names.append("u." + name)
    return pa.RecordBatch.from_arrays(cols, names=names), ["delta"] * len(names)


# ---- a reader of page headers (thrift compact protocol), as far as the writer's data pages V1 need it ------------------------------------------
def _varint(data, at):
    v, shift = 0, 0
    while True:
        b = data[at]
        at += 1
        v |= (b & 0x7F) << shift
        shift += 7
        if b < 0x80:
            return v, at


def _struct(data, at):
    """{field id: int or nested dict}, end. Fields of the types a PageHeader holds."""
    out, last = {}, 0
    while True:
        b = data[at]
        at += 1
        if b == 0:
            return out, at
        ty, delta = b & 0x0F, b >> 4
        if delta == 0:
            z, at = _varint(data, at)
            fid = (z >> 1) ^ -(z & 1)
        else:
            fid = last + delta
        last = fid
        if ty in (P.T_I32, P.T_I64):
            z, at = _varint(data, at)
            out[fid] = (z >> 1) ^ -(z & 1)
        elif ty == P.T_STRUCT:
            out[fid], at = _struct(data, at)
        elif ty in (P.T_TRUE, P.T_FALSE):
            out[fid] = ty == P.T_TRUE
        else:
            raise AssertionError("a field type no page header of the writer holds: %d" % ty)


def data_pages(data: bytes, col):
    """[(rows, encoding, body bytes)] of the chunk's data pages."""
    at, end = col.data_page_offset, (col.dictionary_page_offset or col.data_page_offset) + col.total_compressed_size
    pages = []
    while at < end:
        h, at = _struct(data, at)
        assert h[1] == P.DATA_PAGE and h[2] == h[3]
        pages.append((h[5][1], h[5][2], data[at:at + h[2]]))
        at += h[2]
    assert at == end
    return pages


def assert_delta_pages(record: pa.RecordBatch, data: bytes, md, page: int, delta_names) -> None:
    """The chunk of every column of `delta_names` names DELTA_BINARY_PACKED (+ RLE when optional) and no PLAIN, and the value bytes of
    each of its pages — what follows the definition levels — are the oracle's for the page's non-NULL values."""
    rg = md.row_group(0)
    sch = pq.ParquetFile(io.BytesIO(data)).schema
    for j, name in enumerate(record.schema.names):
        if name not in delta_names:
            continue
        col = rg.column(j)
        optional = sch.column(j).max_definition_level == 1
        assert set(col.encodings) == ({"DELTA_BINARY_PACKED", "RLE"} if optional else {"DELTA_BINARY_PACKED"}), (name, col.encodings)
        assert not col.has_dictionary_page
        arr = record.column(j)
        bits, ok = cases._bits(arr), cases._validity(arr)
        pages = data_pages(data, col)
        assert len(pages) == -(-record.num_rows // page), name
        for k, (n, encoding, body) in enumerate(pages):
            lo = k * page
            assert n == min(page, record.num_rows - lo) and encoding == P.DELTA_BINARY_PACKED, (name, k)
            if optional:
                body = body[4 + int.from_bytes(body[:4], "little"):]
            want = P.delta_binary_packed(bits[lo:lo + n][ok[lo:lo + n]].view(np.int64))
            assert body == want, "%s page %d: %d value bytes, the oracle has %d" % (name, k, len(body), len(want))


# ---- every family × rows × page size × NULL pattern ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", cases.NULL_PATTERNS)
@pytest.mark.parametrize("page_rows", PAGE_ROWS)
def test_every_family_reads_back_and_matches_the_byte_oracle(pp, page_rows, pattern):
    page = page_rows or 65536
    for rows in ROWS:
        record, encodings = family_record(rows, pattern, page)
        data = pp.selftest_parquet_write(record, page_rows=page_rows, encodings=encodings)
        md = cases.assert_reads_back(record, data)
        assert_delta_pages(record, data, md, page, set(record.schema.names))
        if rows > 0:
            parser_accepts(pp, data)


def test_short_pages_are_their_headers(pp):
    """A page of one value is its header alone; a page without a value — inside an optional column — is 80 01 04 00 00."""
    rows = 3 * 64
    valid = np.zeros(rows, dtype=bool)
    valid[0] = valid[2 * 64 + 5] = True                     # page 0: one value, page 1: none, page 2: one value
    v = np.full(rows, -3, dtype=np.int64)
    record = pa.RecordBatch.from_arrays([pa.array(v, mask=~valid)], names=["timestamp"])
    data = pp.selftest_parquet_write(record, page_rows=64, encodings=["delta"])
    md = cases.assert_reads_back(record, data)
    parser_accepts(pp, data)
    bodies = [body[4 + int.from_bytes(body[:4], "little"):] for _, _, body in data_pages(data, md.row_group(0).column(0))]
    assert bodies == [b"\x80\x01\x04\x01\x05", b"\x80\x01\x04\x00\x00", b"\x80\x01\x04\x01\x05"]


def chunk_bytes(data: bytes, j: int) -> bytes:
    col = pq.ParquetFile(io.BytesIO(data)).metadata.row_group(0).column(j)
    start = col.dictionary_page_offset or col.data_page_offset
    return data[start:start + col.total_compressed_size]


@pytest.mark.parametrize("pattern", ["none", "alternate", "whole_page"])
def test_a_mixed_record_leaves_the_other_columns_chunks_as_they_were(pp, pattern):
    record = cases.mixed_record(1000, pattern)
    names = record.schema.names
    plain = pp.selftest_parquet_write(record, page_rows=cases.PAGE)
    mixed = pp.selftest_parquet_write(record, page_rows=cases.PAGE, encodings={"timestamp": "delta", "count": "delta", "value": "plain"})
    md = cases.assert_reads_back(record, mixed)
    parser_accepts(pp, mixed)
    assert_delta_pages(record, mixed, md, cases.PAGE, {"timestamp", "count"})
    for j, name in enumerate(names):
        if name in ("timestamp", "count"):
            assert chunk_bytes(mixed, j) != chunk_bytes(plain, j)
        else:
            assert chunk_bytes(mixed, j) == chunk_bytes(plain, j), name
            assert "DELTA_BINARY_PACKED" not in md.row_group(0).column(j).encodings
    # by position, the never-NULL column too
    by_position = pp.selftest_parquet_write(record, page_rows=cases.PAGE, encodings=["delta", "delta"] + [None] * (len(names) - 3) + ["delta"])
    md = cases.assert_reads_back(record, by_position)
    assert_delta_pages(record, by_position, md, cases.PAGE, {"timestamp", "count", "dense"})
    assert set(md.row_group(0).column(len(names) - 1).encodings) == {"DELTA_BINARY_PACKED"}   # required: no levels, no RLE


def test_sorted_timestamps_shrink(pp):
    rows = 20000
    ts = np.cumsum(np.random.default_rng(7).integers(0, 2000, rows, dtype=np.int64))
    record = pa.RecordBatch.from_arrays([pa.array(ts)], names=["timestamp"])
    plain, delta = pp.selftest_parquet_write(record), pp.selftest_parquet_write(record, encodings=["delta"])
    cases.assert_reads_back(record, delta)
    assert len(plain) > rows * 8 and len(delta) < rows * 11 // 8 + rows // 128 * 8 + 400   # 11-bit miniblocks, a block head of <= 7 bytes


def test_optional_asked_of_a_delta_column_without_nulls(pp):
    record = cases.mixed_record(300, "none")
    data = pp.selftest_parquet_write(record, page_rows=128, optional={"timestamp": True, "dense": False}, encodings={"timestamp": "delta", "dense": "delta"})
    md = cases.assert_reads_back(record, data, optional={"timestamp": True, "dense": False})
    assert_delta_pages(record, data, md, 128, {"timestamp", "dense"})
    parser_accepts(pp, data)


def test_without_encodings_the_file_is_the_old_one(pp):
    for rows, pattern in ((0, "none"), (65, "alternate"), (1000, "whole_page")):
        record = cases.mixed_record(rows, pattern)
        n = record.num_columns
        old = pp.selftest_parquet_write(record, page_rows=cases.PAGE)
        assert pp.selftest_parquet_write(record, page_rows=cases.PAGE, encodings=None) == old
        assert pp.selftest_parquet_write(record, page_rows=cases.PAGE, encodings=[None] * n) == old
        assert pp.selftest_parquet_write(record, page_rows=cases.PAGE, encodings=["plain"] * n) == old
        assert pp.selftest_parquet_write(record, page_rows=cases.PAGE, encodings={}) == old
        assert pp.selftest_parquet_write(record, page_rows=cases.PAGE, encodings={"value": None}) == old


def test_refusals_return_their_codes(pp):
    record = cases.mixed_record(65, "alternate")
    n = record.num_columns
    for name in ("value", "flag", "labels.utf8", "labels.bin", "plain_str", "plain_bin"):   # float64, bool, dictionary, string
        with pytest.raises(pp.FdbError) as e:
            pp.selftest_parquet_write(record, encodings={name: "delta"})
        assert e.value.code == pp.FDB_ERR_UNSUPPORTED and name in str(e.value) and "DELTA" in str(e.value), name
    for encodings in ([], ["delta"] * (n - 1), ["delta"] + [None] * n):                      # a wrong length
        with pytest.raises(pp.FdbError) as e:
            pp.selftest_parquet_write(record, encodings=encodings)
        assert e.value.code == pp.FDB_ERR_INVALID, encodings
    for bad in ("DELTA", "rle", 1, True, b"delta"):                                          # an unknown value
        with pytest.raises(pp.FdbError) as e:
            pp.selftest_parquet_write(record, encodings=[bad] + [None] * (n - 1))
        assert e.value.code == pp.FDB_ERR_INVALID, bad
    with pytest.raises(pp.FdbError) as e:                                                    # an unknown name
        pp.selftest_parquet_write(record, encodings={"no such column": "delta"})
    assert e.value.code == pp.FDB_ERR_INVALID and "no such column" in str(e.value)
    # the C entry point itself: an entry outside 0 … 1, a length that is neither 0 nor the column count
    import ctypes
    opts = pp.ParquetWriteOptions(0, 0, None)
    for enc in ([2] + [0] * (n - 1), [-1] + [0] * (n - 1), [0] * (n + 1)):
        arr = (ctypes.c_int8 * len(enc))(*enc)
        out, nb = ctypes.c_void_p(), ctypes.c_int64()
        with pp.ExportedBatch(record) as ex:
            rc = pp.lib().fdb_selftest_parquet_write_encoded(ctypes.addressof(ex.array), ctypes.addressof(ex.schema), ctypes.byref(opts), ctypes.cast(arr, ctypes.c_void_p), len(enc),
                                                             ctypes.byref(out), ctypes.byref(nb))
        assert rc == pp.FDB_ERR_INVALID and not out.value, enc


def test_entry_points_are_in_library_header_exports_and_binding(pp):
    L = pp.lib()
    header = open(os.path.join(ROOT, "include", "frostdb_amd.h")).read()
    exports = open(os.path.join(ROOT, "frostdb_amd", "csrc", "exports.map")).read()
    for name in ENTRY_POINTS:
        assert re.search(r"^FDB_API int %s\(" % name, header, flags=re.M), name
        assert re.search(r"const int8_t\* encodings, int32_t n_encodings, uint8_t\*\* bytes, int64_t\* n_bytes\);", header)
        assert name in exports and re.search(r"global:\s*fdb_\*;", exports)
        assert getattr(L, name).argtypes is not None
    # the options struct has not grown
    assert [f[0] for f in pp.ParquetWriteOptions._fields_] == ["page_rows", "n_optional", "optional"]


def test_delta_kernels_compile_for_gfx950_without_scratch(tmp_path):
    """fdb_pqdelta.hip compiled offline for gfx950 with the flags of the writer's compile test: the resource report shows the four DELTA
    kernels, no scratch and no spills."""
    src = os.path.join(ROOT, "frostdb_amd", "csrc", "fdb_pqdelta.hip")
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-munsafe-fp-atomics", "-I", os.path.join(ROOT, "frostdb_amd", "csrc"),
                        "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", str(tmp_path / "fdb_pqdelta.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    remarks = [ln.split("remark: ")[-1].replace(" [-Rpass-analysis=kernel-resource-usage]", "").strip() for ln in r.stderr.splitlines() if "remark:" in ln]
    names = [u for u in remarks if u.startswith("Function Name:")]
    print(" | ".join(remarks))
    kernels = ["pqd_compact_kernel", "pqd_block_survey_kernel", "pqd_page_walk_kernel", "pqd_encode_kernel"]
    assert len(names) == len(kernels) and all(any(k in u for u in names) for k in kernels), names
    scratch = [u for u in remarks if "ScratchSize" in u]
    assert len(scratch) == len(names) and all("ScratchSize [bytes/lane]: 0" in u for u in scratch), remarks
    spills = [u for u in remarks if "Spill" in u]
    assert spills and all(re.search(r"Spill: 0\b", u) for u in spills), remarks
