"""CPU-side checks of SNAPPY in the Parquet writer (fdb_batch_to_parquet_compressed): fdb_selftest_parquet_write_compressed runs the writer
over a host record, the compress kernel replaced by the host walk of the rule it compiles (fdb_pqsnappy.h) — byte for byte the file the
device path writes (tests/test_gpu_parquet_snappy.py holds the two against each other). Here: pyarrow reads every file back; every
compressed page, dictionary pages included, inflates under pyarrow's Snappy and under the library's host decoder to the page body of the
uncompressed file; a test-side element walker (tests/parquet_snappy_cases.py) finds no copy that leaves its fragment; the footer names
the codec and both sizes; the shapes where the rule can go wrong give the elements the rule says; and on nine corpora the page is at
most 1.25 × what Google's Snappy (pyarrow's codec) makes of the same body. No page the writer makes has an empty body (a page holds a
row, a dictionary page an entry), so the block `00` cannot be reached from here: the shortest bodies are those of 1 … 3 bytes. No GPU is
touched."""
import ctypes
import io
import os
import re
import subprocess

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq
import pytest

from tests import parquet_snappy_cases as S
from tests import parquet_write_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
ENTRY_POINTS = ["fdb_batch_to_parquet_compressed", "fdb_selftest_parquet_write_compressed"]
F = S.FRAGMENT


@pytest.fixture(scope="module")
def pp():
    from frostdb_amd import physicalplan
    return physicalplan


def write_both(pp, record, page_rows, compression, **kw):
    return pp.selftest_parquet_write(record, page_rows=page_rows, compression=compression, **kw), pp.selftest_parquet_write(record, page_rows=page_rows, **kw)


def one_page_block(pp, record, page_rows, **kw):
    """(the Snappy block of the record's only data page, its body) — checked against both decoders on the way."""
    data, plain = write_both(pp, record, page_rows, "snappy", **kw)
    blocks = S.assert_compressed_file(pp, record, data, plain, "snappy")
    assert len(blocks[0]) == 1
    pages, _ = S.chunk_pages(plain, pq.ParquetFile(io.BytesIO(plain)).metadata.row_group(0).column(0))
    return blocks[0][0], [p for p in pages if p[0] == S.DATA_PAGE][0][2]


def block_of(pp, payload: bytes):
    record, page_rows = S.bytes_record(payload)
    block, body = one_page_block(pp, record, page_rows)
    assert body == payload
    return block


# ---- every column kind × rows × NULL pattern ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", cases.NULL_PATTERNS)
def test_every_kind_reads_back_and_inflates(pp, pattern):
    for rows in cases.ROWS:
        record = cases.mixed_record(rows, pattern)
        data, plain = write_both(pp, record, cases.PAGE, "snappy")
        S.assert_compressed_file(pp, record, data, plain, "snappy")
        delta = {"timestamp": "delta", "count": "delta", "dense": "delta"}
        data, plain = write_both(pp, record, cases.PAGE, "snappy", encodings=delta)
        S.assert_compressed_file(pp, record, data, plain, "snappy")
        assert set(pq.ParquetFile(io.BytesIO(data)).metadata.row_group(0).column(0).encodings) >= {"DELTA_BINARY_PACKED"}


@pytest.mark.parametrize("record", [cases.rle_record(), cases.extremes_record(), cases.duplicates_record(), cases.empty_dictionary_record(), cases.large_strings_record(),
                                    cases.dict_record(1000, 257), cases.dict_record(300, 65537)], ids=["rle", "extremes", "duplicates", "empty_dictionary", "large_strings", "dict257", "dict65537"])
def test_the_writer_s_own_shapes(pp, record):
    data, plain = write_both(pp, record, cases.PAGE, "snappy")
    S.assert_compressed_file(pp, record, data, plain, "snappy")


def test_the_project_s_own_parser_accepts_the_files(pp):
    """As in tests/test_parquet_write_cpu.py: the project's reader parses row group 0 — without a GPU it gets as far as the device call
    (FDB_ERR_DEVICE), never FDB_ERR_INVALID; with one it succeeds."""
    from tests.parquet_util import row_group_chunks
    for record in (cases.mixed_record(1000, "alternate"), cases.rle_record(), cases.dict_record(300, 257)):
        chunks, rows = row_group_chunks(pp.selftest_parquet_write(record, page_rows=cases.PAGE, compression="snappy"), 0)
        assert all(c[5] == "SNAPPY" for c in chunks)
        try:
            pp.ResidentBatch.from_parquet(chunks, rows).close()
        except pp.FdbError as e:
            assert e.code == pp.FDB_ERR_DEVICE, (e.code, str(e))


def test_compressed_beside_uncompressed_columns(pp):
    record = cases.mixed_record(1000, "alternate")
    names = record.schema.names
    for compression in ({"timestamp": "snappy", "labels.utf8": "snappy", "flag": "uncompressed"}, ["snappy", None] * 4 + ["snappy"], [None] * 8 + ["snappy"], ["snappy"] + [None] * 8):
        data, plain = write_both(pp, record, cases.PAGE, compression, encodings={"timestamp": "delta"})
        S.assert_compressed_file(pp, record, data, plain, compression)
    by_name = pp.selftest_parquet_write(record, page_rows=cases.PAGE, compression={n: "snappy" for n in names})
    assert by_name == pp.selftest_parquet_write(record, page_rows=cases.PAGE, compression="snappy") == pp.selftest_parquet_write(record, page_rows=cases.PAGE, compression=["snappy"] * len(names))


def test_footer_sizes_and_codec(pp):
    record = cases.mixed_record(1000, "last_of_page")
    data, plain = write_both(pp, record, 128, {"timestamp": "snappy", "plain_str": "snappy"})
    rg, rg0 = pq.ParquetFile(io.BytesIO(data)).metadata.row_group(0), pq.ParquetFile(io.BytesIO(plain)).metadata.row_group(0)
    for j, name in enumerate(record.schema.names):
        col, col0 = rg.column(j), rg0.column(j)
        if name in ("timestamp", "plain_str"):
            assert col.compression == "SNAPPY" and col.total_compressed_size != col.total_uncompressed_size
            # the bodies are the uncompressed file's; only the page headers, which now hold two different sizes, may differ in length
            assert abs(col.total_uncompressed_size - col0.total_uncompressed_size) <= 2 * len(S.chunk_pages(data, col)[0])
        else:
            assert col.compression == "UNCOMPRESSED" and col.total_compressed_size == col.total_uncompressed_size == col0.total_compressed_size
    assert rg.total_byte_size == sum(rg.column(j).total_uncompressed_size for j in range(rg.num_columns))


def test_without_codecs_the_file_is_the_older_entry_points(pp):
    for rows in (0, 65, 1000):
        record = cases.mixed_record(rows, "whole_page")
        n = record.num_columns
        old = pp.selftest_parquet_write(record, page_rows=cases.PAGE)
        old_delta = pp.selftest_parquet_write(record, page_rows=cases.PAGE, encodings={"timestamp": "delta"})
        for compression in ([None] * n, ["uncompressed"] * n, {}, {"value": None}, {"value": "uncompressed"}):
            assert pp.selftest_parquet_write(record, page_rows=cases.PAGE, compression=compression) == old
            assert pp.selftest_parquet_write(record, page_rows=cases.PAGE, encodings={"timestamp": "delta"}, compression=compression) == old_delta
        assert pp.selftest_parquet_write(record, page_rows=cases.PAGE, compression=None) == old
        # the C entry point with n_codecs == 0
        opts = pp.ParquetWriteOptions(cases.PAGE, 0, None)
        out, nb = ctypes.c_void_p(), ctypes.c_int64()
        with pp.ExportedBatch(record) as ex:
            rc = pp.lib().fdb_selftest_parquet_write_compressed(ctypes.addressof(ex.array), ctypes.addressof(ex.schema), ctypes.byref(opts), None, 0, None, 0, ctypes.byref(out), ctypes.byref(nb))
        assert rc == 0
        try:
            assert ctypes.string_at(out.value, nb.value) == old
        finally:
            pp.lib().fdb_bytes_free(out.value)


def test_the_older_entry_points_still_write_uncompressed_files(pp):
    """Their bytes are the parent's: the header still holds one size twice and the footer UNCOMPRESSED with equal totals (the existing
    suites compare them with pyarrow and the DELTA oracle byte for byte; this is the part of them this change touched)."""
    record = cases.mixed_record(129, "alternate")
    for data in (pp.selftest_parquet_write(record, page_rows=cases.PAGE), pp.selftest_parquet_write(record, page_rows=cases.PAGE, encodings={"timestamp": "delta"})):
        rg = cases.assert_reads_back(record, data).row_group(0)
        for j in range(rg.num_columns):
            col = rg.column(j)
            assert col.total_compressed_size == col.total_uncompressed_size
            assert all(raw == len(stored) for _, raw, stored, _ in S.chunk_pages(data, col)[0])


# ---- shapes where the rule can go wrong ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_bytes", [1, 2, 3, 4, 5, F - 1, F, F + 1, 2 * F - 1, 2 * F, 2 * F + 1])
def test_bodies_around_the_fragment_size(pp, n_bytes):
    record, page_rows = S.bits_record(n_bytes)
    block, body = one_page_block(pp, record, page_rows)
    assert len(body) == n_bytes
    u, elems = S.walk_elements(block)
    assert u == n_bytes
    starts = {pos for _, pos, _, _ in elems}
    assert all(k * F in starts for k in range(-(-n_bytes // F))), "every fragment begins an element"
    if n_bytes < 4:
        assert elems == [(0, 0, n_bytes, 0)]


@pytest.mark.parametrize("rows", [F // 8 - 1, F // 8, F // 8 + 1, 2 * F // 8 - 1, 2 * F // 8 + 1])
@pytest.mark.parametrize("kind", ["int64", "float64", "optional"])
def test_eight_byte_columns_around_the_fragment_size(pp, rows, kind):
    rng = np.random.default_rng(rows)
    if kind == "int64":
        arr = pa.array(rng.integers(0, 1000, rows).astype(np.int64))
    elif kind == "float64":
        arr = pa.array(rng.standard_normal(rows))
    else:  # levels in front of the values: 4 + a run header + ⌈rows / 8⌉ bytes more, an odd body
        arr = pa.array(rng.integers(0, 1000, rows).astype(np.int64), mask=np.arange(rows) % 9 == 4)
    record = pa.RecordBatch.from_arrays([arr], names=["c"])
    one_page_block(pp, record, -(-rows // 64) * 64)


def copies(block):
    return [e for e in S.merged(S.assert_elements_stay_in_fragments(block)) if e[0]]


@pytest.mark.parametrize("length", [4, 11, 12, 64, 65, 68, 129])
@pytest.mark.parametrize("literal", [60, 61, 256, 257])
def test_match_and_literal_lengths(pp, length, literal):
    """`literal` bytes of noise, their last 8 bytes again and again for `length` bytes (8 back is within FDB_PQS_NEAR, wherever in its
    window the repeat starts; the copy runs over itself), then other noise: one literal of `literal` bytes, one copy of exactly
    `length` from 8 back, one literal."""
    a = S.noise(literal, literal)
    again = bytes(a[literal - 8 + i % 8] for i in range(length))
    tail = bytearray(S.noise(literal + 1000, 8 + (-(literal + length)) % 8))
    tail[0] = (a[literal - 8 + length % 8] + 1) & 0xFF  # the match ends where it is meant to
    elems = S.merged(S.assert_elements_stay_in_fragments(block_of(pp, a + again + bytes(tail))))
    assert elems == [(False, 0, literal, 0), (True, literal, length, 8), (False, literal + length, len(tail), 0)], elems
    kinds = [(k, n) for k, _, n, _ in S.walk_elements(block_of(pp, a + again + bytes(tail)))[1] if k != 0]
    want = [(2, 64)] * ((length - 4) // 64 if length >= 68 else 0)
    rest = length - 64 * len(want)
    if rest > 64:
        want, rest = want + [(2, 60)], rest - 60
    assert kinds == want + [(1 if rest <= 11 else 2, rest)]


@pytest.mark.parametrize("offset", [2047, 2048])
def test_copy_offsets_at_the_one_byte_form_s_edge(pp, offset):
    a = S.noise(offset, offset)
    tail = bytearray(S.noise(offset + 1, 8 + (-(offset + 8)) % 8))
    tail[0] = (a[8] + 1) & 0xFF
    _, elems = S.walk_elements(block_of(pp, a + a[:8] + bytes(tail)))
    assert [(k, n, off) for k, _, n, off in elems if k != 0] == [(1 if offset < 2048 else 2, 8, offset)]


def test_a_whole_fragment_literal(pp):
    _, elems = S.walk_elements(block_of(pp, S.noise(5, 2 * F)))
    assert elems == [(0, 0, F, 0), (0, F, F, 0)]


def test_matches_at_the_fragment_s_end(pp):
    """A match that ends exactly at the fragment's end; and one the end cuts: its first part is a copy up to the end, and what the next
    fragment holds of it cannot be copied from before that fragment's first byte."""
    a = S.noise(6, F - 40)
    whole = a + a[-200:-160] + S.noise(7, 64)  # (from 200 back: the table of 4 096 entries still knows a position that near)
    elems = S.merged(S.assert_elements_stay_in_fragments(block_of(pp, whole)))
    assert elems == [(False, 0, F - 40, 0), (True, F - 40, 40, 200), (False, F, 64, 0)], elems
    a = S.noise(8, F - 24)
    cut = a + a[-200:-120] + S.noise(9, 8)  # 24 bytes of the repeat in fragment 0, 56 in fragment 1
    elems = S.merged(S.assert_elements_stay_in_fragments(block_of(pp, cut)))
    assert elems == [(False, 0, F - 24, 0), (True, F - 24, 24, 200), (False, F, 64, 0)], elems


def test_a_hash_collision_is_not_a_match(pp):
    """Two different 4-byte values under one hash of the rule (fdb_pqs_hash: × 0x1e35a7bd, the top 12 bits): the second finds the first
    in the table, compares, and stays a literal."""
    h = lambda x: ((x * 0x1E35A7BD) & 0xFFFFFFFF) >> 20
    x = 0x11223344
    y = next(v for v in range(0x55667788, 0x55667788 + 1_000_000) if h(v) == h(x))
    payload = x.to_bytes(4, "little") + S.noise(10, 196) + y.to_bytes(4, "little") + S.noise(11, 60)
    _, elems = S.walk_elements(block_of(pp, payload))
    assert elems == [(0, 0, len(payload), 0)]


@pytest.mark.parametrize("period", [1, 2, 4, 8, 3, 5, 7, 13, 16])
def test_a_run_starting_mid_window(pp, period):
    """100 bytes of noise, 300 of a period-`period` run, noise: the run is found inside the window it starts in — the table does not
    know that window's positions yet — one unit after its start, and copied to its end. (A longer period than FDB_PQS_NEAR is found
    a window later, through the table: tests/test_gpu_parquet_snappy.py has 63, 64 and 65 among its shapes.)"""
    unit = bytes(range(200, 200 + period))
    run = (unit * 300)[:300]
    tail = S.noise(13, 8 + (-(100 + 300)) % 8)
    elems = S.merged(S.assert_elements_stay_in_fragments(block_of(pp, S.noise(12, 100) + run + tail)))
    assert elems == [(False, 0, 100 + period, 0), (True, 100 + period, 300 - period, period), (False, 400, len(tail), 0)], elems


# ---- ratio against the reference compressor -----------------------------------------------------------------------------------------------------------
N = 32768


def corpus(name):
    r = np.random.default_rng
    entries = pa.array(["label-%04d" % i for i in range(1000)])
    if name == "constant":
        return pa.array(np.full(N, 123_456_789, dtype=np.int64))
    if name == "cumsum":
        return pa.array(np.cumsum(r(1).integers(0, 2000, N)).astype(np.int64))
    if name == "timestamps":
        return pa.array((1.7e12 + 1000 * np.arange(N)).astype(np.int64))
    if name == "standard_normal":
        return pa.array(r(2).standard_normal(N))
    if name == "integers_0_100":
        return pa.array(r(3).integers(0, 100, N).astype(np.int64))
    if name == "integers_0_100_f64":
        return pa.array(r(8).integers(0, 100, N).astype(np.float64))
    if name == "fifty_floats":
        return pa.array(r(4).standard_normal(50)[r(5).integers(0, 50, N)])
    if name == "dictionary_random":
        return pa.DictionaryArray.from_arrays(pa.array(r(6).integers(0, 1000, N).astype(np.uint32)), entries)
    if name == "dictionary_runs_of_64":
        return pa.DictionaryArray.from_arrays(pa.array(np.repeat(r(7).integers(0, 1000, N // 64), 64).astype(np.uint32)), entries)
    raise ValueError(name)


CORPORA = ["constant", "cumsum", "timestamps", "standard_normal", "integers_0_100", "integers_0_100_f64", "fifty_floats", "dictionary_random", "dictionary_runs_of_64"]


@pytest.mark.parametrize("name", CORPORA)
def test_ratio_against_the_reference_compressor(pp, name):
    """One required column in one page of 32 768 rows: the compressed data page is at most 1.25 × what pyarrow's Snappy (Google's) makes
    of the same body."""
    record = pa.RecordBatch.from_arrays([corpus(name)], names=["c"])
    block, body = one_page_block(pp, record, N, optional=[False])
    reference = len(pa.compress(body, codec="snappy", asbytes=True))
    print("%s: body %d, ours %d, reference %d, %.3f x" % (name, len(body), len(block), reference, len(block) / reference))
    assert len(block) <= 1.25 * reference, (name, len(block), reference)
    assert len(block) <= S.bound(len(body))


# ---- refusals, symbols, the offline compile ---------------------------------------------------------------------------------------------------------------
def test_refusals_return_their_codes(pp):
    record = cases.mixed_record(65, "alternate")
    n = record.num_columns
    for compression in ([], ["snappy"] * (n - 1), ["snappy"] + [None] * n):                  # a wrong length
        with pytest.raises(pp.FdbError) as e:
            pp.selftest_parquet_write(record, compression=compression)
        assert e.value.code == pp.FDB_ERR_INVALID and "codecs" in str(e.value), compression
    for bad in ("SNAPPY", "lz4_raw", "zstd", 1, True, b"snappy"):                             # an unknown codec
        with pytest.raises(pp.FdbError) as e:
            pp.selftest_parquet_write(record, compression=[bad] + [None] * (n - 1))
        assert e.value.code == pp.FDB_ERR_INVALID and "unknown codec" in str(e.value), bad
    with pytest.raises(pp.FdbError) as e:
        pp.selftest_parquet_write(record, compression="gzip")
    assert e.value.code == pp.FDB_ERR_INVALID
    with pytest.raises(pp.FdbError) as e:                                                    # an unknown name
        pp.selftest_parquet_write(record, compression={"no such column": "snappy"})
    assert e.value.code == pp.FDB_ERR_INVALID and "no such column" in str(e.value)
    with pytest.raises(pp.FdbError) as e:                                                    # the older pairs' refusals, unchanged
        pp.selftest_parquet_write(record, encodings={"value": "delta"}, compression="snappy")
    assert e.value.code == pp.FDB_ERR_UNSUPPORTED and "DELTA" in str(e.value)
    with pytest.raises(pp.FdbError) as e:
        pp.selftest_parquet_write(record, page_rows=100, compression="snappy")
    assert e.value.code == pp.FDB_ERR_INVALID and "page_rows" in str(e.value)
    # the C entry point itself: an entry outside 0 … 1, a length that is neither 0 nor the column count
    opts = pp.ParquetWriteOptions(0, 0, None)
    for codecs, text in (([2] + [0] * (n - 1), "codecs[0] is 2"), ([0, -1] + [0] * (n - 2), "codecs[1] is -1"), ([1] * (n + 1), "`codecs` has"), ([1] * (n - 1), "`codecs` has")):
        arr = (ctypes.c_int8 * len(codecs))(*codecs)
        out, nb = ctypes.c_void_p(), ctypes.c_int64()
        with pp.ExportedBatch(record) as ex:
            rc = pp.lib().fdb_selftest_parquet_write_compressed(ctypes.addressof(ex.array), ctypes.addressof(ex.schema), ctypes.byref(opts), None, 0, ctypes.cast(arr, ctypes.c_void_p),
                                                                 len(codecs), ctypes.byref(out), ctypes.byref(nb))
        assert rc == pp.FDB_ERR_INVALID and not out.value and text in pp.lib().fdb_last_error().decode(), codecs


def test_entry_points_are_in_library_header_exports_and_binding(pp):
    L = pp.lib()
    header = open(os.path.join(ROOT, "include", "frostdb_amd.h")).read()
    exports = open(os.path.join(ROOT, "frostdb_amd", "csrc", "exports.map")).read()
    for name in ENTRY_POINTS:
        assert re.search(r"^FDB_API int %s\(.*const int8_t\* codecs, int32_t n_codecs, uint8_t\*\* bytes, int64_t\* n_bytes\);" % name, header, flags=re.M), name
        assert name in exports and re.search(r"global:\s*fdb_\*;", exports)
        assert getattr(L, name).argtypes is not None
    assert [f[0] for f in pp.ParquetWriteOptions._fields_] == ["page_rows", "n_optional", "optional"]
    assert S.FRAGMENT <= S.RING_REACH and S.FRAGMENT <= 65536


def test_snappy_kernels_compile_for_gfx950_without_scratch(tmp_path):
    """fdb_pqsnappy.hip compiled offline for gfx950 with the flags of the writer's compile test: the resource report shows the four
    kernels, no scratch and no spills."""
    src = os.path.join(ROOT, "frostdb_amd", "csrc", "fdb_pqsnappy.hip")
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-munsafe-fp-atomics", "-I", os.path.join(ROOT, "frostdb_amd", "csrc"),
                        "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", str(tmp_path / "fdb_pqsnappy.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    remarks = [ln.split("remark: ")[-1].replace(" [-Rpass-analysis=kernel-resource-usage]", "").strip() for ln in r.stderr.splitlines() if "remark:" in ln]
    names = [u for u in remarks if u.startswith("Function Name:")]
    print(" | ".join(remarks))
    kernels = ["pqs_place_kernel", "pqs_compress_kernel", "pqs_scan_kernel", "pqs_gather_kernel"]
    assert len(names) == len(kernels) and all(any(k in u for u in names) for k in kernels), names
    scratch = [u for u in remarks if "ScratchSize" in u]
    assert len(scratch) == len(names) and all("ScratchSize [bytes/lane]: 0" in u for u in scratch), remarks
    spills = [u for u in remarks if "Spill" in u]
    assert spills and all(re.search(r"Spill: 0\b", u) for u in spills), remarks
