"""CPU-side checks of LZ4_RAW in the Parquet writer (`compression="lz4"`, codec 7 at the C entry points): fdb_selftest_parquet_write_* runs
the writer over a host record, the three kernels of fdb_pqlz4.hip replaced by the host walk of the rule they compile (fdb_pqlz4.h) — byte
for byte the file the device path writes (tests/test_gpu_parquet_write_lz4.py holds the two against each other). Here: every LZ4 page,
dictionary pages included, inflates under liblz4 (pyarrow's `lz4_raw`) and under the library's host decoder to the page body of the
uncompressed file; a test-side sequence walker (tests/parquet_lz4_cases.py) holds every block to the rule — matches inside their
fragments, none starting behind U − 12 or ending behind U − 5, a closing sequence without a match, LZ4_compressBound; the footer says
codec 7 and the sizes; the shapes where the rule can go wrong give the sequences the rule says; on nine corpora the page is at most
1.25 × what liblz4 makes of the same body; SNAPPY, LZ4_RAW and uncompressed columns stand side by side with every other writer option.
No GPU is touched."""
import ctypes
import io
import os
import re
import subprocess

import pyarrow as pa
import pyarrow.parquet as pq
import pytest

from tests import parquet_lz4_cases as Z
from tests import parquet_write_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
F = Z.F
DELTA = {"timestamp": "delta", "count": "delta", "dense": "delta"}


@pytest.fixture(scope="module")
def pp():
    from frostdb_amd import physicalplan
    return physicalplan


@pytest.fixture(scope="module")
def shapes():
    return Z.rule_shapes()


def write_both(pp, record, page_rows, compression, **kw):
    return pp.selftest_parquet_write(record, page_rows=page_rows, compression=compression, **kw), pp.selftest_parquet_write(record, page_rows=page_rows, **kw)


def one_page_block(pp, record, page_rows, **kw):
    """(the LZ4 block of the record's only data page, its body) — checked against the decoders and the rule on the way."""
    data, plain = write_both(pp, record, page_rows, "lz4", **kw)
    blocks = Z.assert_compressed_file(pp, record, data, plain, "lz4")
    assert len(blocks[0]) == 1
    pages, _ = Z.chunk_pages(plain, Z.footer_chunks(plain)[0][0])
    return blocks[0][0], [p for p in pages if p[0] == Z.S.DATA_PAGE][0][2]


def block_of(pp, payload: bytes):
    record, page_rows = Z.bytes_record(payload)
    block, body = one_page_block(pp, record, page_rows)
    assert body == payload
    return block


# ---- every column kind × rows × NULL pattern, the writer's own shapes -----------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", cases.NULL_PATTERNS)
def test_every_kind_reads_back_and_inflates(pp, pattern):
    for rows in cases.ROWS:
        record = cases.mixed_record(rows, pattern)
        data, plain = write_both(pp, record, cases.PAGE, "lz4")
        Z.assert_compressed_file(pp, record, data, plain, "lz4")
        data, plain = write_both(pp, record, cases.PAGE, "lz4", encodings=DELTA)
        Z.assert_compressed_file(pp, record, data, plain, "lz4")
        assert set(pq.ParquetFile(io.BytesIO(data)).metadata.row_group(0).column(0).encodings) >= {"DELTA_BINARY_PACKED"}


@pytest.mark.parametrize("record", [cases.rle_record(), cases.extremes_record(), cases.duplicates_record(), cases.empty_dictionary_record(), cases.large_strings_record(),
                                    cases.dict_record(1000, 257), cases.dict_record(300, 65537)], ids=["rle", "extremes", "duplicates", "empty_dictionary", "large_strings", "dict257", "dict65537"])
def test_the_writer_s_own_shapes(pp, record):
    data, plain = write_both(pp, record, cases.PAGE, "lz4")
    Z.assert_compressed_file(pp, record, data, plain, "lz4")


def test_the_three_ways_to_name_the_codec_write_one_file(pp):
    record = cases.mixed_record(1000, "alternate")
    names = record.schema.names
    by_name = pp.selftest_parquet_write(record, page_rows=cases.PAGE, compression={n: "lz4" for n in names})
    assert by_name == pp.selftest_parquet_write(record, page_rows=cases.PAGE, compression="lz4") == pp.selftest_parquet_write(record, page_rows=cases.PAGE, compression=["lz4"] * len(names))
    assert pp.PARQUET_WRITE_CODECS["lz4"] == 7 and all(c["codec"] == 7 for c in Z.footer_chunks(by_name)[0])
    from tests.parquet_util import row_group_chunks
    chunks, rows = row_group_chunks(by_name, 0)   # the project's own parser: without a GPU it gets as far as the device call
    try:
        pp.ResidentBatch.from_parquet(chunks, rows).close()
    except pp.FdbError as e:
        assert e.code == pp.FDB_ERR_DEVICE, (e.code, str(e))


# ---- body lengths around the block's end conditions and the fragment size ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind", Z.BODY_KINDS)
@pytest.mark.parametrize("n_bytes", Z.BODY_LENGTHS)
def test_body_lengths(pp, n_bytes, kind):
    """A short last fragment is where the second-last fragment's match must be cut at U − 5 and barred behind U − 12: the walker inside
    one_page_block asserts both, liblz4 refuses a block that breaks either."""
    record, page_rows = Z.body_bits(n_bytes, kind)
    block, body = one_page_block(pp, record, page_rows)
    assert len(body) == n_bytes
    seqs = Z.walk_sequences(block, n_bytes)
    if n_bytes < 13 or kind == "noise":  # no position may win in a body of fewer than 13 bytes (position 0 has no candidate)
        assert seqs == [(0, n_bytes, None, 0, 0)] and len(block) == 1 + (0 if n_bytes < 15 else (n_bytes - 15) // 255 + 1) + n_bytes
    elif kind == "run":  # every fragment is one match from 1 back, the last one cut at U − 5
        got = [(p, n, off) for _, _, p, n, off in seqs if p is not None]
        want = [(k * F + 1, min(F, n_bytes - 5 - k * F) - 1, 1) for k in range(-(-n_bytes // F)) if k * F + 1 <= n_bytes - 12]
        assert got == want, (got, want)
    else:
        assert all(off == 5 for _, _, p, _, off in seqs if p is not None) and (len(seqs) >= 2) == (n_bytes >= 17)  # (its first candidate is position 5)


# ---- the shapes of the rule -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("literal", [14, 15, 16, 269, 270, 271])
def test_literal_run_lengths(pp, literal):
    payload, want = Z.repeat_shape(literal, 40)
    block = block_of(pp, payload)
    seqs = Z.walk_sequences(block, len(payload))
    assert [(p, n, off) for _, _, p, n, off in seqs if p is not None] == want and seqs[0][:2] == (0, literal)
    extension = [] if literal < 15 else [255] * ((literal - 15) // 255) + [(literal - 15) % 255]
    assert block[0] >> 4 == min(literal, 15) and list(block[1:1 + len(extension)]) == extension and block[1 + len(extension):][:literal] == payload[:literal]


@pytest.mark.parametrize("length", [18, 19, 20, 273, 274, 275])
def test_match_lengths(pp, length):
    payload, want = Z.repeat_shape(100, length)
    block = block_of(pp, payload)
    assert Z.matches(block, len(payload)) == want
    assert block[0] & 15 == min(length - 4, 15)
    extension = 0 if length - 4 < 15 else (length - 19) // 255 + 1
    assert block[1 + 1 + 100 + 2:][:extension] == bytes([255] * (extension - 1) + [(length - 19) % 255][:extension])


def test_literals_across_a_fragment_boundary(pp, shapes):
    payload = shapes["tail_and_head"]
    seqs = Z.walk_sequences(block_of(pp, payload), len(payload))
    assert (F - 48, 40, 200) in [(p, n, off) for _, _, p, n, off in seqs]
    crossing = [s for s in seqs if s[0] < F < s[0] + s[1]]
    assert crossing == [(F - 8, 8 + 25, F + 25, 47, 1)], seqs   # fragment 0's tail of 8 + fragment 1's head of 25; the zeros, from their second byte on


def test_a_joined_run_of_more_than_a_fragment(pp, shapes):
    payload = shapes["joined_run"]
    block = block_of(pp, payload)
    seqs = Z.walk_sequences(block, len(payload))
    assert seqs == [(0, 1, 1, F - 1, 1), (F, F + 1, 2 * F + 1, F - 1 - 5, 1), (3 * F - 5, 5, None, 0, 0)], seqs
    assert (F + 1 - 15) // 255 + 1 > 128  # the joined run's extension bytes


def test_matches_at_the_fragment_s_end(pp, shapes):
    payload = shapes["match_to_fragment_end"]
    assert Z.matches(block_of(pp, payload), len(payload)) == [(F - 40, 40, 200)]
    payload = shapes["match_cut_by_fragment_end"]   # 24 bytes of the repeat in fragment 0; what fragment 1 holds of it cannot be copied from before its first byte
    assert Z.matches(block_of(pp, payload), len(payload)) == [(F - 24, 24, 200)]


def test_the_furthest_offset(pp, shapes):
    """A match of 4 bytes lies inside its fragment, so the furthest a match reaches back is F − 4 = 32 764: the fragment's last 4 bytes
    held against its first 4. Below LZ4's 65 535 and the device decoder's reach."""
    payload = shapes["furthest_offset"]
    assert Z.matches(block_of(pp, payload), len(payload)) == [(5, F - 9, 1), (F - 4, 4, F - 4)]
    assert F - 4 < 32768 <= Z.S.RING_REACH


def test_a_hash_collision_is_not_a_match(pp, shapes):
    payload = shapes["hash_collision"]
    assert Z.walk_sequences(block_of(pp, payload), len(payload)) == [(0, len(payload), None, 0, 0)]


@pytest.mark.parametrize("period", range(1, 17))
def test_a_run_starting_mid_window(pp, shapes, period):
    payload = shapes["period_%d" % period]
    got = Z.matches(block_of(pp, payload), len(payload))
    assert len(got) == 1 and got[0][0] == 100 + period and got[0][2] == period and got[0][1] >= 300 - period, got


def test_a_page_without_a_match_is_one_closing_sequence(pp, shapes):
    payload = shapes["no_match_anywhere"]
    block = block_of(pp, payload)
    assert Z.walk_sequences(block, len(payload)) == [(0, len(payload), None, 0, 0)]
    assert len(block) == 1 + (len(payload) - 15) // 255 + 1 + len(payload)
    payload = shapes["one_run_over_eight_fragments"]
    assert len(Z.matches(block_of(pp, payload), len(payload))) == 8


# ---- ratio against liblz4 ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", Z.CORPORA)
def test_ratio_against_liblz4(pp, name):
    """One required column in one page of 32 768 rows: the LZ4 data page is at most 1.25 × what liblz4 (pyarrow's `lz4_raw`) makes of
    the same body — the figure the project holds this match finder to against a greedy reference compressor."""
    record = pa.RecordBatch.from_arrays([Z.corpus(name)], names=["c"])
    block, body = one_page_block(pp, record, Z.N, optional=[False])
    reference = len(pa.Codec("lz4_raw").compress(body, asbytes=True))
    print("%s: body %d, ours %d, liblz4 %d, %.3f x" % (name, len(body), len(block), reference, len(block) / reference))
    assert len(block) <= 1.25 * reference, (name, len(block), reference)


# ---- mixes ---------------------------------------------------------------------------------------------------------------------------------------------
MIX = ["snappy", "lz4", None, "lz4", "snappy", "lz4", None, "snappy", "lz4"]


@pytest.mark.parametrize("options", [{}, {"statistics": "page"}, {"statistics": "page", "bloom_filters": ["labels.bin", "timestamp"]}, {"runs": True}, {"dictionaries": "used"},
                                     {"row_group_rows": 64, "statistics": "page", "bloom_filters": ["labels.bin"], "runs": True, "dictionaries": "used"}],
                         ids=["plain", "page_index", "bloom", "runs", "used_dictionaries", "row_groups_and_everything"])
def test_mixes_in_one_file(pp, options):
    """SNAPPY + LZ4_RAW + uncompressed + DELTA in one file, with each of the writer's other options: the PageLocations are the page
    headers found by walking the chunks, the filters and index regions sit where the footer says (Z.assert_compressed_file)."""
    record = cases.mixed_record(1000, "alternate", dict_size=300)
    assert len(MIX) == record.num_columns
    page_rows = 64 if "row_group_rows" in options else cases.PAGE
    for compression in (MIX, {"timestamp": "lz4", "labels.utf8": "lz4", "flag": "snappy"}, "lz4"):
        data, plain = write_both(pp, record, page_rows, compression, encodings={"timestamp": "delta"}, **options)
        Z.assert_compressed_file(pp, record, data, plain, compression)


def test_the_older_files_keep_their_bytes(pp):
    """Without `compression` and with "snappy" the files are what they were (tests/golden/parquet_write_digests.json and the older suites
    guard the bytes themselves): no LZ4 column, no LZ4 byte — an entry of None or "uncompressed" beside nothing else changes nothing."""
    record = cases.mixed_record(1000, "whole_page")
    n = record.num_columns
    old, old_snappy = pp.selftest_parquet_write(record, page_rows=cases.PAGE), pp.selftest_parquet_write(record, page_rows=cases.PAGE, compression="snappy")
    assert pp.selftest_parquet_write(record, page_rows=cases.PAGE, compression=[None] * n) == old
    assert pp.selftest_parquet_write(record, page_rows=cases.PAGE, compression=["snappy"] * n) == old_snappy
    assert all(c["codec"] == 0 for c in Z.footer_chunks(old)[0]) and all(c["codec"] == 1 for c in Z.footer_chunks(old_snappy)[0])
    lz4 = pp.selftest_parquet_write(record, page_rows=cases.PAGE, compression="lz4")
    assert lz4 != old_snappy and lz4 != old and all(c["codec"] == 7 for c in Z.footer_chunks(lz4)[0])


# ---- refusals, the offline compile -----------------------------------------------------------------------------------------------------------------------
def test_refusals_return_their_codes(pp):
    record = cases.mixed_record(65, "alternate")
    n = record.num_columns
    before = pp.live_allocations()
    for compression in ([], ["lz4"] * (n - 1), ["lz4"] + [None] * n):                        # a wrong length
        with pytest.raises(pp.FdbError) as e:
            pp.selftest_parquet_write(record, compression=compression)
        assert e.value.code == pp.FDB_ERR_INVALID and "codecs" in str(e.value), compression
    for bad in ("LZ4", "lz4_raw", "lz4raw", 7):                                             # an unknown codec: the message lists the three names
        with pytest.raises(pp.FdbError) as e:
            pp.selftest_parquet_write(record, compression=[bad] + [None] * (n - 1))
        assert e.value.code == pp.FDB_ERR_INVALID and "unknown codec" in str(e.value) and all(w in str(e.value) for w in ("'uncompressed'", "'snappy'", "'lz4'")), bad
    with pytest.raises(pp.FdbError) as e:                                                    # DELTA on a column that is not int64, as ever
        pp.selftest_parquet_write(record, encodings={"value": "delta"}, compression="lz4")
    assert e.value.code == pp.FDB_ERR_UNSUPPORTED and "DELTA" in str(e.value)
    # the C entry point itself: every CompressionCodec number the writer does not write
    opts = pp.ParquetWriteOptions(0, 0, None)
    for k, bad in enumerate((2, 5, 6, 8, -1)):
        codecs = [7] * n
        codecs[k] = bad
        arr = (ctypes.c_int8 * n)(*codecs)
        out, nb = ctypes.c_void_p(), ctypes.c_int64()
        with pp.ExportedBatch(record) as ex:
            rc = pp.lib().fdb_selftest_parquet_write_compressed(ctypes.addressof(ex.array), ctypes.addressof(ex.schema), ctypes.byref(opts), None, 0, ctypes.cast(arr, ctypes.c_void_p), n,
                                                                 ctypes.byref(out), ctypes.byref(nb))
        message = pp.lib().fdb_last_error().decode()
        assert rc == pp.FDB_ERR_INVALID and not out.value and "codecs[%d] is %d" % (k, bad) in message and "(0 UNCOMPRESSED, 1 SNAPPY, 7 LZ4_RAW)" in message, (bad, message)
    arr = (ctypes.c_int8 * n)(*([7] * n))                                                    # … and 7 itself is taken
    out, nb = ctypes.c_void_p(), ctypes.c_int64()
    with pp.ExportedBatch(record) as ex:
        rc = pp.lib().fdb_selftest_parquet_write_compressed(ctypes.addressof(ex.array), ctypes.addressof(ex.schema), ctypes.byref(opts), None, 0, ctypes.cast(arr, ctypes.c_void_p), n,
                                                             ctypes.byref(out), ctypes.byref(nb))
    assert rc == 0
    try:
        assert ctypes.string_at(out.value, nb.value) == pp.selftest_parquet_write(record, compression="lz4")
    finally:
        pp.lib().fdb_bytes_free(out.value)
    assert pp.live_allocations() == before


def test_lz4_kernels_compile_for_gfx950_without_scratch(tmp_path):
    """fdb_pqlz4.hip compiled offline for gfx950 with the flags of the Snappy compile test: the resource report names the three kernels,
    no scratch and no spills."""
    src = os.path.join(ROOT, "frostdb_amd", "csrc", "fdb_pqlz4.hip")
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-munsafe-fp-atomics", "-I", os.path.join(ROOT, "frostdb_amd", "csrc"),
                        "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", str(tmp_path / "fdb_pqlz4.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    remarks = [ln.split("remark: ")[-1].replace(" [-Rpass-analysis=kernel-resource-usage]", "").strip() for ln in r.stderr.splitlines() if "remark:" in ln]
    names = [u for u in remarks if u.startswith("Function Name:")]
    print(" | ".join(remarks))
    kernels = ["pql_compress_kernel", "pql_scan_kernel", "pql_gather_kernel"]
    assert len(names) == len(kernels) and all(any(k in u for u in names) for k in kernels), names
    scratch = [u for u in remarks if "ScratchSize" in u]
    assert len(scratch) == len(names) and all("ScratchSize [bytes/lane]: 0" in u for u in scratch), remarks
    spills = [u for u in remarks if "Spill" in u]
    assert spills and all(re.search(r"Spill: 0\b", u) for u in spills), remarks
