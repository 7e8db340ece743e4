"""Several row groups and dictionaries of used entries only, the host side (fdb_selftest_parquet_write_grouped,
selftest_parquet_write(row_group_rows=…, dictionaries="used")): no GPU.

1. The host walk's files against the restatement (tests/parquet_group_cases.py): every chunk's dictionary page holds exactly the used
   entries in entry order and says their count, every data page's width byte is bits(U − 1), every decoded index stream is the re-keyed
   one, no page is longer than with the whole dictionary, bounds, ColumnIndex and bloom filters are over the same values, pyarrow and
   the project's chunk parser read the file — on dictionaries of 1 … 65 537 entries with 0, 1, 3 and all entries used, used entries
   only in the first or the last presence word and at bits 31, 32 and 63 of one, duplicate and empty entries, a column of NULLs, pages
   of one repeated index, a plain string column, the mixed record under every NULL pattern, and mixed with DELTA, SNAPPY, the page
   index, sorting columns, bloom filters and runs.
2. Several row groups: pyarrow reads ⌈rows / R⌉ groups of the right rows and the record bit for bit, at rows 0 … 4 097 around R and 2 R,
   R of 64, 128 and 1 024, pages of 64 and 128 rows, under every NULL pattern; every group's chunk region, filters, ColumnIndexes and
   OffsetIndexes are those of the file written for its row slice alone, with every option alone and mixed; the regions' order, the
   per-group ordinal, file_offset and sorting_columns; with dictionaries="used" every group's dictionaries are its own rows' used
   entries, an all-NULL group between others has no dictionary page.
3. NULL options, zero options and the older argument combinations give the older calls' bytes; every refusal has its code and names the
   field and the value; header, exports, binding and build list the entry points; fdb_pqdict.hip compiles for gfx950 without scratch or
   spills."""
import ctypes
import io
import os
import re
import subprocess

import numpy as np
import pyarrow as pa
import pytest

from tests import parquet_group_cases as G
from tests import parquet_runs_cases as R
from tests import parquet_write_cases as cases
from tests.parquet_util import row_group_chunks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
ENTRY_POINTS = ["fdb_batch_to_parquet_grouped", "fdb_selftest_parquet_write_grouped"]
PAGE = G.PAGE
MIXES = {
    "delta": dict(encodings={"timestamp": "delta"}),
    "snappy": dict(compression="snappy"),
    "page_index": dict(statistics="page", sorting_columns=[("labels.utf8",), ("timestamp", True)]),
    "bloom": dict(bloom_filters=["labels.utf8", "labels.bin", "plain_str", "timestamp"]),
    "runs": dict(runs=True),
    "all": dict(encodings={"timestamp": "delta"}, compression={"labels.utf8": "snappy", "timestamp": "snappy", "plain_bin": "snappy"}, statistics="page", sorting_columns=[("labels.bin",)],
                bloom_filters="sorting", bloom_bits_per_value=7, runs=True),
}


@pytest.fixture(scope="module")
def pp():
    from frostdb_amd import physicalplan
    return physicalplan


def write_and_check(pp, record, page_rows=PAGE, expect_pruned=None, **kw) -> bytes:
    """The host walk's file with dictionaries="used", held to the restatement and to the file with the whole dictionaries."""
    data = pp.selftest_parquet_write(record, page_rows=page_rows, dictionaries="used", **kw)
    whole = pp.selftest_parquet_write(record, page_rows=page_rows, **kw)
    flags = R.flags_of(record, kw["runs"]) if kw.get("runs") else None
    pruned = G.assert_used_file(record, data, whole, page_rows, flags, kw.get("bloom_filters"), kw.get("bloom_bits_per_value", 0), kw.get("sorting_columns"))
    if expect_pruned is not None:
        assert (pruned > 0) == expect_pruned, pruned
        assert not expect_pruned or len(data) < len(whole)   # an entry less is at least 5 bytes less; the ordinal costs 2
    cases.assert_same_record(R.read_back(data), record)
    if record.num_rows:
        chunks, rows = row_group_chunks(data, 0)
        assert rows == record.num_rows
        try:
            # the project's own reader: without a device it walks every chunk's page headers and then fails for want of one — a chunk it
            # cannot walk is refused with another code before that; the pages' decoding is tests/test_gpu_parquet_groups.py's to check
            pp.ResidentBatch.from_parquet(chunks, rows).close()
        except pp.FdbError as e:
            assert e.code == pp.FDB_ERR_DEVICE, (e.code, str(e))
    return data


# ---- 1. the files ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entries", G.DICT_SIZES)
@pytest.mark.parametrize("used", G.USED)
def test_dictionary_sizes_and_how_much_of_them_is_used(pp, entries, used):
    record = G.sized_record(entries, used)
    k = entries if used == "all" else min(used, entries)
    page_rows = 4096 if used == "all" and entries > 4096 else PAGE
    data = write_and_check(pp, record, page_rows=page_rows, expect_pruned=k < entries, statistics="chunk", bloom_filters=["labels.d"])
    nv = G.dictionary_pages(data)[0]
    assert (nv[0] if nv else 0) == k


def test_used_entries_at_the_edges_of_the_presence_words(pp):
    data = write_and_check(pp, G.word_edges_record(), expect_pruned=True)
    assert [d[0] for d in G.dictionary_pages(data)] == [3, 2, 6]


def test_duplicate_and_empty_entries(pp):
    record = G.duplicates_record()
    data = write_and_check(pp, record, expect_pruned=True, statistics="page")
    nv, body = G.dictionary_pages(data)[0]
    assert nv == 4 and body == b"".join(len(e).to_bytes(4, "little") + e for e in (b"a", b"a", b"", b"c"))   # entries 0, 2, 3, 5: both b"a" stay


def test_pages_of_one_repeated_index_hold_the_rank(pp):
    record = G.equal_pages_record()
    for kw in (dict(), dict(runs=True), dict(compression="snappy")):
        data = write_and_check(pp, record, expect_pruned=True, **kw)
    _pf, cols = R.data_pages(pp.selftest_parquet_write(record, page_rows=PAGE, dictionaries="used"))
    used = G.restate(record.column(0))[0].tolist()
    valid = np.asarray(record.column(0).is_valid())
    for p in (0, 2, 4):   # one RLE run of the rank of entry 90 + 3p
        _levels, width, rest = R.split_page(cols[0][2][p], True, True)
        got, runs = R.decode_hybrid(rest, width, int(valid[p * PAGE:(p + 1) * PAGE].sum()))
        assert [r[0] for r in runs] == ["rle"] and set(got) == {used.index(90 + 3 * p)} and used.index(90 + 3 * p) != 90 + 3 * p


@pytest.mark.parametrize("pattern", cases.NULL_PATTERNS)
@pytest.mark.parametrize("rows", [0, 1, 63, 64, 65, 1000, 4097])
def test_the_mixed_record_under_every_null_pattern(pp, rows, pattern):
    record = cases.mixed_record(rows, pattern, dict_size=300)
    write_and_check(pp, record, expect_pruned=rows < 4097 or pattern == "all")


@pytest.mark.parametrize("mix", sorted(MIXES))
def test_mixed_with_the_other_options(pp, mix):
    for pattern in ("alternate", "whole_page"):
        write_and_check(pp, cases.mixed_record(1000, pattern, dict_size=300), expect_pruned=True, **MIXES[mix])
    write_and_check(pp, G.filtered_record(2000), page_rows=128, expect_pruned=True, **{k: v for k, v in MIXES[mix].items() if k not in ("encodings", "compression", "sorting_columns", "bloom_filters")})


def test_a_filtered_label_column_shrinks(pp):
    record = G.filtered_record(5000)
    data = write_and_check(pp, record, page_rows=1024, expect_pruned=True, runs=True, bloom_filters=["labels.wide"])
    whole = pp.selftest_parquet_write(record, page_rows=1024, runs=True, bloom_filters=["labels.wide"])
    assert len(data) * 10 < len(whole)   # three entries of 65 537, two bits an index instead of seventeen


def test_nothing_used_zero_rows_and_an_empty_dictionary(pp):
    for record in (G.sized_record(65, 0), cases.mixed_record(0, "none"), cases.empty_dictionary_record(), cases.mixed_record(130, "all")):
        data = write_and_check(pp, record, statistics="page", bloom_filters=[n for n in record.schema.names if n.startswith("labels.")])
        for j, name in enumerate(record.schema.names):
            if pa.types.is_dictionary(record.column(j).type):
                assert G.dictionary_pages(data)[j] is None, name
        write_and_check(pp, record, runs=True, compression="snappy")


# ---- 2. several row groups --------------------------------------------------------------------------------------------------------------------
def write_groups(pp, record, rg_rows, page_rows, dictionaries=None, **kw) -> bytes:
    """The host walk's file with row_group_rows, read by pyarrow and held, group by group, to the files of the row slices alone. Every
    column is written optional: a slice without NULLs of a column that has some would otherwise be a required column on its own."""
    import pyarrow.parquet as pq
    kw = dict(kw, optional={n: True for n in record.schema.names})
    data = pp.selftest_parquet_write(record, page_rows=page_rows, row_group_rows=rg_rows, dictionaries=dictionaries, **kw)
    md = pq.ParquetFile(io.BytesIO(data)).metadata
    assert md.num_row_groups == max(1, -(-record.num_rows // rg_rows)) and md.num_rows == record.num_rows
    assert [md.row_group(g).num_rows for g in range(md.num_row_groups)] == [min(rg_rows, record.num_rows - g * rg_rows) for g in range(md.num_row_groups)]
    cases.assert_same_record(R.read_back(data), record)
    held = G.interned(record)
    assert pp.selftest_parquet_write(held, page_rows=page_rows, row_group_rows=rg_rows, dictionaries=dictionaries, **kw) == data
    G.assert_groups(held, data, rg_rows, lambda part: pp.selftest_parquet_write(part, page_rows=page_rows, dictionaries=dictionaries, **kw))
    return data


@pytest.mark.parametrize("pattern", cases.NULL_PATTERNS)
@pytest.mark.parametrize("rg_rows", [64, 128, 1024])
def test_row_groups_of_the_mixed_record(pp, rg_rows, pattern):
    for rows in sorted({0, 1, 63, 64, 65, rg_rows - 1, rg_rows, rg_rows + 1, 2 * rg_rows, 2 * rg_rows + 1, 4097}):
        for page_rows in (64, 128):
            write_groups(pp, cases.mixed_record(rows, pattern, dict_size=300), rg_rows, page_rows)


@pytest.mark.parametrize("mix", sorted(MIXES))
@pytest.mark.parametrize("dictionaries", [None, "used"])
def test_row_groups_mixed_with_the_other_options(pp, mix, dictionaries):
    for pattern, rows, rg_rows, page_rows in (("alternate", 1000, 192, 128), ("whole_page", 1000, 128, 64), ("first_of_page", 321, 64, 64), ("none", 2049, 1024, 128)):
        write_groups(pp, cases.mixed_record(rows, pattern, dict_size=300), rg_rows, page_rows, dictionaries=dictionaries, **MIXES[mix])


def test_every_group_has_the_dictionaries_of_its_own_rows(pp):
    rg_rows, page_rows = 256, 128
    record = G.grouped_record(5 * rg_rows + 70, rg_rows)
    for kw in (dict(), dict(runs=True, statistics="page", bloom_filters=["labels.g", "labels.gap"], compression={"labels.g": "snappy"})):
        data = write_groups(pp, record, rg_rows, page_rows, dictionaries="used", **kw)
        opt = {n: True for n in record.schema.names}
        for g, rg in enumerate(G.groups(data)):
            part = G.interned(record).slice(g * rg_rows, rg["rows"])
            alone = pp.selftest_parquet_write(part, page_rows=page_rows, dictionaries="used", optional=opt, **kw)
            whole = pp.selftest_parquet_write(part, page_rows=page_rows, optional=opt, **kw)
            G.assert_used_file(part, alone, whole, page_rows, R.flags_of(part, True) if kw.get("runs") else None, kw.get("bloom_filters"), 0, None)   # the slice's file IS the restatement's
            pages = G.group_dictionary_pages(data, rg)
            for j in range(3):
                used, body, _rekeyed, _valid = G.restate(part.column(j))
                if len(used) == 0:
                    assert pages[j] is None and g % 2 == 1 and j == 1 and rg["chunks"][j]["encodings"] == [0, 3]   # PLAIN, RLE: the all-NULL group between the others
                elif rg["chunks"][j]["codec"] == 0:
                    assert pages[j] == (len(used), body), (g, j)
                else:
                    assert pages[j][0] == len(used), (g, j)
            assert pages[3] is None and pages[4] is not None
        assert len({G.group_dictionary_pages(data, rg)[0][0] for rg in G.groups(data)}) >= 1
        # the whole dictionaries instead: every group carries all 4 097 entries of labels.g
        plain = write_groups(pp, record, rg_rows, page_rows, **kw)
        assert all(G.group_dictionary_pages(plain, rg)[0][0] == 4097 for rg in G.groups(plain)) and len(data) < len(plain)
        for rg in G.groups(data):   # the project's own chunk parser accepts every group's chunks
            chunks, rows = row_group_chunks(data, rg["ordinal"])
            assert rows == rg["rows"] and b"".join(c[4] for c in chunks) == G.chunk_region(data, rg)


# ---- 3. the unchanged path, refusals, the interface ------------------------------------------------------------------------------------------
def call_grouped(pp, record, groups, page_rows=PAGE, codecs=None, index=None, bloom=None, runs=None, encodings=None, entry="fdb_selftest_parquet_write_grouped"):
    opts = pp.ParquetWriteOptions(page_rows, 0, None)
    out, nb = ctypes.c_void_p(), ctypes.c_int64()
    arr = (ctypes.c_int8 * len(codecs))(*codecs) if codecs else None
    enc = (ctypes.c_int8 * len(encodings))(*encodings) if encodings else None
    with pp.ExportedBatch(record) as ex:
        rc = getattr(pp.lib(), entry)(ctypes.addressof(ex.array), ctypes.addressof(ex.schema), ctypes.byref(opts), ctypes.cast(enc, ctypes.c_void_p) if encodings else None,
                                      len(encodings) if encodings else 0, ctypes.cast(arr, ctypes.c_void_p) if codecs else None, len(codecs) if codecs else 0,
                                      ctypes.byref(index) if index is not None else None, ctypes.byref(bloom) if bloom is not None else None,
                                      ctypes.byref(runs) if runs is not None else None, *([ctypes.byref(groups) if groups is not None else None] if entry.endswith("_grouped") else []),
                                      ctypes.byref(out), ctypes.byref(nb))
    if rc != 0:
        assert not out.value
        return rc, pp.lib().fdb_last_error().decode()
    try:
        return 0, ctypes.string_at(out.value, nb.value)
    finally:
        pp.lib().fdb_bytes_free(out.value)


def test_without_group_options_the_bytes_are_the_older_calls(pp):
    record = cases.mixed_record(1000, "alternate", dict_size=300)
    n = record.num_columns
    run_arr = (ctypes.c_int8 * n)(*R.flags_of(record, True))
    all_runs = pp.ParquetRunOptions(ctypes.cast(run_arr, ctypes.c_void_p), n, 0)
    for codecs in (None, [1] * n):
        for index in (None, pp.ParquetIndexOptions(2, 0, None, 0)):
            for runs in (None, all_runs):
                rc, old = call_grouped(pp, record, None, codecs=codecs, index=index, runs=runs, entry="fdb_selftest_parquet_write_runs")
                assert rc == 0
                assert call_grouped(pp, record, None, codecs=codecs, index=index, runs=runs) == (0, old)
                assert call_grouped(pp, record, pp.ParquetGroupOptions(0, 0, 0), codecs=codecs, index=index, runs=runs) == (0, old)
    # the ten older argument combinations of the binding, with the keywords at their defaults and spelled out
    for kw in (dict(), dict(optional={"dense": True}), dict(encodings={"timestamp": "delta"}), dict(compression="snappy"), dict(statistics="chunk"), dict(statistics="page", index_size_limit=4),
               dict(sorting_columns=[("timestamp",)]), dict(bloom_filters=["timestamp"]), dict(bloom_filters=["labels.utf8"], bloom_bits_per_value=3), dict(runs=True)):
        old = pp.selftest_parquet_write(record, page_rows=PAGE, **kw)
        assert G.ordinal(old) is None
        assert pp.selftest_parquet_write(record, page_rows=PAGE, row_group_rows=0, dictionaries=None, **kw) == old
        assert pp.selftest_parquet_write(record, page_rows=PAGE, dictionaries="whole", **kw) == old
        assert pp.selftest_parquet_write(record, page_rows=PAGE, dictionaries="used", **kw) != old
    # a row_group_rows that leaves one row group is taken: the same pages, and the row group says its ordinal
    old = pp.selftest_parquet_write(record, page_rows=PAGE)
    one = pp.selftest_parquet_write(record, page_rows=PAGE, row_group_rows=1024)
    assert G.ordinal(one) == 0 and len(one) == len(old) + 2 and R.data_pages(one)[1][4][2] == R.data_pages(old)[1][4][2]
    cases.assert_same_record(R.read_back(one), record)
    # zero rows: one zero-row group
    empty = cases.mixed_record(0, "none")
    for kw in (dict(), dict(row_group_rows=64), dict(dictionaries="used")):
        cases.assert_same_record(R.read_back(pp.selftest_parquet_write(empty, **kw)), empty)


def test_refusals(pp):
    record = cases.mixed_record(100, "alternate")
    n = record.num_columns
    for rows in (-64, -1, 1, 63, 65, 100):
        rc, text = call_grouped(pp, record, pp.ParquetGroupOptions(rows, 0, 0))
        assert rc == pp.FDB_ERR_INVALID and "row_group_rows must be a multiple of 64 (0: one row group), got %d" % rows in text, text
    big = pa.RecordBatch.from_arrays([pa.array(np.zeros(64 * 32767 + 1, dtype=np.int64))], names=["dense"])
    rc, text = call_grouped(pp, big, pp.ParquetGroupOptions(64, 0, 0))
    assert rc == pp.FDB_ERR_INVALID and "row_group_rows 64 cuts 2097089 rows into 32768 row groups, more than 32767" in text, text
    for d in (-1, 2, 7):
        rc, text = call_grouped(pp, record, pp.ParquetGroupOptions(0, d, 0))
        assert rc == pp.FDB_ERR_INVALID and "dictionaries is %d" % d in text, text
    rc, text = call_grouped(pp, record, pp.ParquetGroupOptions(0, 1, 5))
    assert rc == pp.FDB_ERR_INVALID and "pad is 5" in text, text
    # in the fields' order
    rc, text = call_grouped(pp, record, pp.ParquetGroupOptions(65, 2, 5))
    assert rc == pp.FDB_ERR_INVALID and "row_group_rows" in text
    rc, text = call_grouped(pp, record, pp.ParquetGroupOptions(64, 2, 5))
    assert rc == pp.FDB_ERR_INVALID and "dictionaries is 2" in text
    # the largest values that are taken
    for rows, d in ((64, 0), (64, 1), (2 ** 62, 0), (128, 1)):
        assert call_grouped(pp, record, pp.ParquetGroupOptions(rows, d, 0))[0] == 0
    rc, most = call_grouped(pp, pa.RecordBatch.from_arrays([pa.array(np.zeros(64 * 32767, dtype=np.int64))], names=["dense"]), pp.ParquetGroupOptions(64, 0, 0))
    assert rc == 0 and [(g["rows"], g["ordinal"]) for g in G.groups(most)[-2:]] == [(64, 32765), (64, 32766)]
    # everything the older calls refuse stays refused, and comes first
    bad = pp.ParquetGroupOptions(65, 2, 5)
    rc, text = call_grouped(pp, record, bad, page_rows=100)
    assert rc == pp.FDB_ERR_INVALID and "page_rows" in text
    rc, text = call_grouped(pp, record, bad, codecs=[2] + [0] * (n - 1))
    assert rc == pp.FDB_ERR_INVALID and "codecs[0] is 2" in text
    rc, text = call_grouped(pp, record, bad, index=pp.ParquetIndexOptions(3, 0, None, 0))
    assert rc == pp.FDB_ERR_INVALID and "statistics is 3" in text
    rc, text = call_grouped(pp, record, bad, bloom=pp.ParquetBloomOptions(None, 0, 65))
    assert rc == pp.FDB_ERR_INVALID and "bits_per_value is 65" in text
    rc, text = call_grouped(pp, record, bad, runs=pp.ParquetRunOptions(None, n, 0))
    assert rc == pp.FDB_ERR_INVALID and "run options" in text
    # the binding's own
    for kw, text in (({"dictionaries": "some"}, "`dictionaries` is None, 'whole' or 'used'"), ({"dictionaries": True}, "`dictionaries` is"), ({"dictionaries": ["used"]}, "`dictionaries` is"),
                     ({"row_group_rows": "64"}, "row_group_rows must be"), ({"row_group_rows": True}, "row_group_rows must be"), ({"row_group_rows": 65}, "got 65")):
        with pytest.raises(pp.FdbError) as e:
            pp.selftest_parquet_write(record, **kw)
        assert e.value.code == pp.FDB_ERR_INVALID and text in str(e.value), (kw, str(e.value))
    # a row that points past its dictionary is refused as it is with the whole dictionary
    ok = pa.DictionaryArray.from_arrays(pa.array([0, 1, 0], type=pa.uint32()), pa.array([b"a", b"b"], type=pa.binary()))
    idx = np.frombuffer(ok.indices.buffers()[1], dtype=np.uint32).copy()
    idx[1] = 70
    wrong = pa.DictionaryArray.from_arrays(pa.Array.from_buffers(pa.uint32(), 3, [None, pa.py_buffer(idx.tobytes())]), ok.dictionary, safe=False)
    texts = []
    for kw in (dict(), dict(dictionaries="used")):
        with pytest.raises(pp.FdbError) as e:
            pp.selftest_parquet_write(pa.RecordBatch.from_arrays([wrong], names=["d"]), **kw)
        assert e.value.code == pp.FDB_ERR_INVALID and "out of range" in str(e.value)
        texts.append(str(e.value))
    assert texts[0] == texts[1]


def test_entry_points_are_in_library_header_exports_and_binding(pp):
    L = pp.lib()
    header = open(os.path.join(ROOT, "include", "frostdb_amd.h")).read()
    exports = open(os.path.join(ROOT, "frostdb_amd", "csrc", "exports.map")).read()
    for name in ENTRY_POINTS:
        assert re.search(r"^FDB_API int %s\(.*const fdb_parquet_run_options\* runs /\* NULL: none \*/, const fdb_parquet_group_options\* groups /\* NULL: none \*/, uint8_t\*\* bytes, int64_t\* n_bytes\);" % name,
                         header, flags=re.M), name
        assert re.search(r"global:\s*fdb_\*;", exports)
        assert getattr(L, name).argtypes is not None and len(getattr(L, name).argtypes) == len(getattr(L, name.replace("_grouped", "_runs")).argtypes) + 1
    assert ENTRY_POINTS[0] in exports
    assert re.search(r"typedef struct fdb_parquet_group_options \{\s*int64_t row_group_rows;[^}]*int32_t dictionaries;[^}]*int32_t pad;[^}]*\} fdb_parquet_group_options;", header)
    assert [f[0] for f in pp.ParquetGroupOptions._fields_] == ["row_group_rows", "dictionaries", "pad"] and ctypes.sizeof(pp.ParquetGroupOptions) == 16
    assert (pp.ParquetGroupOptions.row_group_rows.offset, pp.ParquetGroupOptions.dictionaries.offset, pp.ParquetGroupOptions.pad.offset) == (0, 8, 12)
    assert ctypes.sizeof(pp.ParquetRunOptions) == 16 and ctypes.sizeof(pp.ParquetBloomOptions) == 16 and ctypes.sizeof(pp.ParquetIndexOptions) == 24 and ctypes.sizeof(pp.ParquetWriteOptions) == 16
    assert pp.PARQUET_WRITE_ENTRIES[-1] == ("_grouped", 6)
    build = open(os.path.join(ROOT, "frostdb_amd", "build.py")).read()
    assert "fdb_pqdict.hip" in build and "fdb_pqdict.h" in build


def test_dictionary_kernels_compile_for_gfx950_without_scratch(tmp_path):
    """fdb_pqdict.hip compiled offline for gfx950 with the flags of the writer's compile test: the resource report shows the two kernels,
    no scratch, no spills, and the 1 KiB of LDS the present kernel stages a small bitmap in (FDB_PQG_LDS_WORDS words)."""
    src = os.path.join(ROOT, "frostdb_amd", "csrc", "fdb_pqdict.hip")
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-munsafe-fp-atomics", "-I", os.path.join(ROOT, "frostdb_amd", "csrc"),
                        "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", str(tmp_path / "fdb_pqdict.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    remarks = [ln.split("remark:", 1)[1].split("[-Rpass")[0].strip() for ln in r.stderr.splitlines() if "remark:" in ln]
    names = [u for u in remarks if u.startswith("Function Name:")]
    print(" | ".join(remarks))
    assert len(names) == 2 and all(any(k in u for u in names) for k in ("pqg_present_kernel", "pqg_remap_kernel")), names
    scratch = [u for u in remarks if "ScratchSize" in u]
    assert len(scratch) == 2 and all("ScratchSize [bytes/lane]: 0" in u for u in scratch), remarks
    spills = [u for u in remarks if "Spill" in u]
    assert spills and all(re.search(r"Spill: 0\b", u) for u in spills), remarks
    lds = [u for u in remarks if "LDS Size" in u]
    words = int(re.search(r"^#define FDB_PQG_LDS_WORDS (\d+)", open(os.path.join(ROOT, "frostdb_amd", "csrc", "fdb_pqdict.h")).read(), flags=re.M).group(1))
    assert sorted(lds) == sorted(["LDS Size [bytes/block]: %d" % (8 * words), "LDS Size [bytes/block]: 0"]) and 8 * words <= 160 * 1024, remarks
