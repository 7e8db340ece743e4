"""PLAIN and DELTA_LENGTH_BYTE_ARRAY value pages, the host side (fdb_selftest_parquet_write_strings, selftest_parquet_write(strings=…)):
no GPU.

0. The test-side page builder (tests/parquet_strings_cases.py: `value_bytes`, from parquet_pages.plain, delta_binary_packed and
   concatenation) is pinned first: pyarrow reads pages built from it, and one reader written from the format's description reads both
   the builder's pages and the pages pyarrow's own writer makes with use_dictionary=False, column_encoding="DELTA_LENGTH_BYTE_ARRAY" to
   the values that went in.
1. The host walk's files against it: every data page's value bytes, the footer's encodings lists, the missing dictionary offset, sizes
   that agree with a walk of the chunk, page header encodings; pyarrow reads the file back value for value; the project's own chunk
   parser accepts it — both forms × the four kinds, 0 … 1 000 and 4 095 / 4 096 / 4 097 rows, pages of 64 and 128 rows under the six
   NULL patterns, the entry lengths of LENGTHS and one of 70 001 bytes, empty strings only, duplicate and unused entries, 65 537 entries
   with three used, an all-NULL page between others, the all-NULL column over an empty dictionary, 0 rows.
2. Mixes, against the same call's file without `strings` for what must not move: SNAPPY and LZ4_RAW, DELTA int columns, the page
   index, bloom filters, runs on levels, row groups, dictionaries="used".
3. An all-distinct column is smaller as delta_length than as a dictionary; NULL / zero options give the older calls' bytes; every
   refusal's code and text; the page that would not fit its header is refused by the survey alone; entry points in library, header,
   exports, binding and build; fdb_pqbytes.hip compiles for gfx950 without scratch."""
import ctypes
import io
import os
import re
import resource
import subprocess

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq
import pytest

from tests import parquet_group_cases as G
from tests import parquet_index_cases as X
from tests import parquet_pages as PG
from tests import parquet_runs_cases as R
from tests import parquet_strings_cases as Y
from tests import parquet_write_cases as cases
from tests.parquet_util import row_group_chunks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
ENTRY_POINTS = ["fdb_batch_to_parquet_strings", "fdb_selftest_parquet_write_strings"]
PAGE = Y.PAGE


@pytest.fixture(scope="module")
def pp():
    from frostdb_amd import physicalplan
    return physicalplan


def write_and_check(pp, record, strings, page_rows=PAGE, **kw) -> bytes:
    """The host walk's file with `strings`, held to the rule, to pyarrow and to the project's chunk parser."""
    data = pp.selftest_parquet_write(record, page_rows=page_rows, strings=strings, **kw)
    Y.assert_strings_file(record, data, strings, page_rows, kw.get("row_group_rows", 0))
    Y.assert_reads_back(record, data)
    if record.num_rows and not kw.get("row_group_rows"):
        chunks, rows = row_group_chunks(data, 0)
        assert rows == record.num_rows
        try:
            # the project's own reader: without a device it walks every chunk's page headers and then fails for want of one — a chunk it
            # cannot walk is refused with another code before that; the pages' decoding is tests/test_gpu_parquet_strings.py's to check
            pp.ResidentBatch.from_parquet(chunks, rows).close()
        except pp.FdbError as e:
            assert e.code == pp.FDB_ERR_DEVICE, (e.code, str(e))
    return data


# ---- 0. the builder ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", Y.FORMS)
def test_pyarrow_reads_pages_built_by_the_builder(form):
    rng = np.random.default_rng(5)
    for n, nulls in ((0, False), (1, False), (129, False), (300, True), (64, "all")):
        values = [Y._entry(i, int(rng.integers(0, 40))) for i in range(n)]
        valid = np.ones(n, dtype=bool) if not nulls else np.zeros(n, dtype=bool) if nulls == "all" else rng.random(n) < 0.6
        held = [v for v, ok in zip(values, valid) if ok]
        page = PG.data_page(n, Y.ENCODING[form], Y.value_bytes(form, held), levels=valid.astype(np.uint8))
        got = pq.read_table(io.BytesIO(PG.file_of(PG.chunk_of("c", PG.BYTE_ARRAY, True, False, [page]), n))).column("c").to_pylist()
        assert got == [v if ok else None for v, ok in zip(values, valid)]
    assert Y.value_bytes("delta_length", []) == Y.ZERO_LENGTHS


def test_one_reader_reads_the_builders_pages_and_pyarrows_writers():
    """A reader written from the format's description (read_values / read_delta_lengths: any block geometry) takes the builder's value
    bytes back to the values they were built from — both forms, lengths that make the DELTA widths differ from miniblock to miniblock —
    and reads the pages pyarrow's own writer makes with use_dictionary=False, column_encoding="DELTA_LENGTH_BYTE_ARRAY" to the values
    that went in: held by values read back, not by bytes. The builder and pyarrow's writer therefore mean the same by a page."""
    rng = np.random.default_rng(9)
    for n in (0, 1, 2, 33, 128, 129, 300, 1000):
        values = [Y._entry(i, int(rng.integers(0, 1 << int(rng.integers(0, 9))))) for i in range(n)]
        for form in Y.FORMS:
            assert Y.read_values(form, Y.value_bytes(form, values), n) == values, (form, n)
    values = [Y._entry(i, (i * 7) % 50 + (300 if i % 97 == 0 else 0)) for i in range(3000)]
    sink = io.BytesIO()
    pq.write_table(pa.table({"c": pa.array(values, type=pa.binary())}), sink, use_dictionary=False, column_encoding="DELTA_LENGTH_BYTE_ARRAY", compression="NONE", data_page_version="1.0",
                   write_statistics=False, data_page_size=4096)
    data = sink.getvalue()
    optional = pq.ParquetFile(io.BytesIO(data)).schema.column(0).max_definition_level == 1
    pages = Y.chunk_data_pages(data, X.chunk_fields(data)[0])
    assert len(pages) >= 2
    got = []
    for _at, _size, nv, enc, body in pages:
        assert enc == Y.ENCODING["delta_length"]
        got += Y.read_values("delta_length", Y.split_levels(body, optional)[1], nv)   # (no NULLs: num_values values)
    assert got == values
    # the same values through the builder, in pyarrow's pages' sizes: the reader gives the same, and pyarrow reads the builder's pages
    at, built = 0, []
    for _at, _size, nv, _enc, _body in pages:
        built.append(PG.data_page(nv, Y.ENCODING["delta_length"], Y.value_bytes("delta_length", values[at:at + nv]), levels=np.ones(nv, dtype=np.uint8)))
        at += nv
    assert pq.read_table(io.BytesIO(PG.file_of(PG.chunk_of("c", PG.BYTE_ARRAY, True, False, built), len(values)))).column("c").to_pylist() == values


# ---- 1. the files -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", Y.FORMS)
@pytest.mark.parametrize("pattern", cases.NULL_PATTERNS)
def test_the_four_kinds_under_every_null_pattern(pp, form, pattern):
    for rows in (0, 1, 63, 64, 65, 127, 128, 129, 1000):
        for page_rows in (64, 128):
            write_and_check(pp, Y.kinds_record(rows, pattern, page=page_rows), form, page_rows=page_rows)


@pytest.mark.parametrize("form", Y.FORMS)
@pytest.mark.parametrize("rows", [4095, 4096, 4097])
def test_rows_around_a_tile(pp, form, rows):
    for pattern, page_rows in (("alternate", 4096), ("none", 8192), ("first_of_page", 64)):
        write_and_check(pp, Y.kinds_record(rows, pattern, page=page_rows), form, page_rows=page_rows)


@pytest.mark.parametrize("form", Y.FORMS)
def test_entry_lengths_and_a_long_entry(pp, form):
    record = Y.lengths_record()
    assert sorted({len(v) for v in Y.column_values(record.column(0))}) == sorted(Y.LENGTHS + [Y.LONG])
    write_and_check(pp, record, form)
    write_and_check(pp, Y.lengths_record(valid=np.arange(4 * PAGE + 3) % 3 != 0), form, page_rows=128)
    write_and_check(pp, Y.lengths_record(rows=PAGE, long_at=[0, PAGE - 1]), form)


@pytest.mark.parametrize("form", Y.FORMS)
def test_empty_duplicate_unused_and_wide(pp, form):
    write_and_check(pp, Y.empties_record(), form)
    data = write_and_check(pp, Y.duplicates_record(), form)
    assert b"unused" not in data   # an unused entry never shows
    data = write_and_check(pp, Y.wide_record(), form)
    assert len(data) < 4000 and b"e1\x00" not in data
    write_and_check(pp, Y.null_page_record(), form)
    write_and_check(pp, Y.offsets_record(), form)


@pytest.mark.parametrize("form", Y.FORMS)
def test_the_all_null_column_over_an_empty_dictionary_and_zero_rows(pp, form):
    record = cases.empty_dictionary_record()
    data = write_and_check(pp, record, form)
    if form == "plain":
        assert data == pp.selftest_parquet_write(record, page_rows=PAGE)   # its present form
    else:
        assert [b[-5:] for b in (body for _a, _s, _n, _e, body in Y.chunk_data_pages(data, G.groups(data)[0]["chunks"][0]))] == [Y.ZERO_LENGTHS] * 2
    for record in (Y.kinds_record(0, "none"), cases.mixed_record(130, "all")):
        write_and_check(pp, record, form)


def test_explicit_forms_per_column(pp):
    record = Y.kinds_record(300, "alternate")
    by_name = {"labels.utf8": "plain", "labels.bin": "dictionary", "plain_str": "delta_length", "plain_bin": None}
    data = write_and_check(pp, record, by_name)
    assert write_and_check(pp, record, ["plain", None, "delta_length", "dictionary", None]) == data
    plain = pp.selftest_parquet_write(record, page_rows=PAGE)
    a, b = G.groups(data)[0]["chunks"], G.groups(plain)[0]["chunks"]
    for j in (1, 3, 4):   # the columns without a form: their chunks byte for byte
        assert data[a[j]["file_offset"]:a[j]["file_offset"] + a[j]["total_compressed_size"]] == plain[b[j]["file_offset"]:b[j]["file_offset"] + b[j]["total_compressed_size"]]
        assert a[j]["encodings"] == b[j]["encodings"]


# ---- 2. mixes -----------------------------------------------------------------------------------------------------------------------------------
def inflated_pages(data):
    return [[body for _a, _s, _n, _e, body in Y.chunk_data_pages(data, ch)] if ch["dictionary_page_offset"] is None else None for ch in G.groups(data)[0]["chunks"]]


@pytest.mark.parametrize("form", Y.FORMS)
@pytest.mark.parametrize("codec", ["snappy", "lz4"])
def test_with_compression_every_page_inflates_to_the_uncompressed_body(pp, form, codec):
    record = Y.kinds_record(1000, "alternate")
    plain = pp.selftest_parquet_write(record, page_rows=PAGE, strings=form)
    data = write_and_check(pp, record, form, compression=codec)
    got, want = inflated_pages(data), inflated_pages(plain)
    assert got == want and all(p is not None for p in got[:4])
    assert [c["codec"] for c in G.groups(data)[0]["chunks"]] == [{"snappy": 1, "lz4": 7}[codec]] * record.num_columns
    mixed = write_and_check(pp, record, form, compression={"labels.utf8": "snappy", "plain_bin": "lz4"})
    assert inflated_pages(mixed) == want
    write_and_check(pp, Y.lengths_record(), form, compression=codec)   # a page of several fragments


@pytest.mark.parametrize("form", Y.FORMS)
def test_with_delta_int_columns(pp, form):
    record = cases.mixed_record(1000, "alternate", dict_size=300)
    enc = {"timestamp": "delta", "count": "delta", "dense": "delta"}
    data = write_and_check(pp, record, form, encodings=enc)
    without = pp.selftest_parquet_write(record, page_rows=PAGE, encodings=enc)
    a, b = G.groups(data)[0]["chunks"], G.groups(without)[0]["chunks"]
    for j, name in enumerate(record.schema.names):
        if not Y.is_byte_array(record.schema.field(name).type):
            assert data[a[j]["file_offset"]:a[j]["file_offset"] + a[j]["total_compressed_size"]] == without[b[j]["file_offset"]:b[j]["file_offset"] + b[j]["total_compressed_size"]], name


@pytest.mark.parametrize("form", Y.FORMS)
def test_with_statistics_and_bloom_filters_nothing_but_the_locations_moves(pp, form):
    record = cases.mixed_record(1000, "first_of_page", dict_size=300)
    kw = dict(statistics="page", sorting_columns=[("labels.utf8",), ("timestamp", True)], bloom_filters=["labels.utf8", "labels.bin", "plain_str", "timestamp"], bloom_bits_per_value=7)
    data = write_and_check(pp, record, form, **kw)
    without = pp.selftest_parquet_write(record, page_rows=PAGE, **kw)
    (rg,), (rg0,) = G.groups(data), G.groups(without)
    assert rg["sorting_columns"] == rg0["sorting_columns"]
    for ch, ch0 in zip(rg["chunks"], rg0["chunks"]):
        for key in ("null_count", "min_value", "max_value", "num_values"):
            assert ch[key] == ch0[key], (ch["name"], key)
        assert X.column_index(data, ch["column_index"]) == X.column_index(without, ch0["column_index"]), ch["name"]
        if ch0["bloom"] is not None:
            assert data[ch["bloom"][0]:sum(ch["bloom"])] == without[ch0["bloom"][0]:sum(ch0["bloom"])], ch["name"]
        else:
            assert ch["bloom"] is None
        oi = X.offset_index(data, ch["offset_index"])   # the PageLocations follow the new bodies: they agree with the walk
        assert [(pos, size) for pos, size, _t, _nv in X.walk_pages(data, ch) if _t == PG.DATA_PAGE] == [(o, s) for o, s, _r in oi], ch["name"]
        assert [r for _o, _s, r in oi] == [r for _o, _s, r in X.offset_index(without, ch0["offset_index"])]


@pytest.mark.parametrize("form", Y.FORMS)
def test_with_runs_on_levels(pp, form):
    record = R.sorted_record(1000)
    record = record.append_column("plain_str", pa.array(["s%d" % (i // 90) if (i // 40) % 3 else None for i in range(1000)], type=pa.string()))
    data = write_and_check(pp, record, form, page_rows=1024, runs=True)   # True leaves the indices of a column with a form alone
    levels_only = {n: "levels" for n in record.schema.names}
    assert pp.selftest_parquet_write(record, page_rows=1024, strings=form, runs=levels_only) == data
    plain_levels = pp.selftest_parquet_write(record, page_rows=1024, strings=form)
    assert len(data) < len(plain_levels)   # the stretches of NULL are runs
    j = record.schema.names.index("plain_str")
    with_runs = pp.selftest_parquet_write(record, page_rows=1024, runs=True)
    for p, (body, body0) in enumerate(zip(inflated_pages(data)[j], R.data_pages(with_runs)[1][j][2])):
        assert Y.split_levels(body, True)[0] == Y.split_levels(body0, True)[0], p   # the levels stream is the one the dictionary form has


@pytest.mark.parametrize("form", Y.FORMS)
def test_with_row_groups_every_region_is_its_slices_file(pp, form):
    for rows, rg_rows, page_rows, pattern in ((1000, 192, 128, "alternate"), (321, 64, 64, "first_of_page"), (2049, 1024, 128, "none"), (4097, 4096, 4096, "alternate")):
        record = G.interned(Y.kinds_record(rows, pattern, page=page_rows))
        opt = {n: True for n in record.schema.names}
        for kw in (dict(), dict(statistics="page", bloom_filters=["labels.bin"], compression={"plain_str": "snappy"})):
            data = write_and_check(pp, record, form, page_rows=page_rows, row_group_rows=rg_rows, optional=opt, **kw)
            G.assert_groups(record, data, rg_rows, lambda part: pp.selftest_parquet_write(part, page_rows=page_rows, strings=form, optional=opt, **kw))


@pytest.mark.parametrize("form", Y.FORMS)
def test_used_dictionaries_have_no_effect_on_a_column_with_a_form(pp, form):
    record = G.filtered_record(2000)   # labels.wide: three entries of 65 537 used; plain_str; timestamp
    data = write_and_check(pp, record, form, page_rows=128, dictionaries="used")
    assert data == write_and_check(pp, record, form, page_rows=128, dictionaries="whole", row_group_rows=4096)   # (the ordinal: group options either way)
    some = {"plain_str": form}
    used = write_and_check(pp, record, some, page_rows=128, dictionaries="used")
    whole = write_and_check(pp, record, some, page_rows=128)
    j = record.schema.names.index("plain_str")
    assert inflated_pages(used)[j] == inflated_pages(whole)[j] and len(used) < len(whole)   # the other columns are pruned as ever


# ---- 3. sizes, the unchanged path, refusals, the interface ----------------------------------------------------------------------------------
def test_an_all_distinct_column_is_smaller_without_its_dictionary(pp):
    record = Y.distinct_record(4096, 16)
    sizes = {s: len(pp.selftest_parquet_write(record, page_rows=1024, strings=s)) for s in (None, "plain", "delta_length")}
    assert sizes["delta_length"] < sizes["plain"] < sizes[None], sizes
    assert sizes[None] - sizes["delta_length"] > 4096 * 4   # the dictionary page's length words at least


def call_strings(pp, record, strings, page_rows=PAGE, runs=None, groups=None, codecs=None, entry="fdb_selftest_parquet_write_strings"):
    opts = pp.ParquetWriteOptions(page_rows, 0, None)
    out, nb = ctypes.c_void_p(), ctypes.c_int64()
    arr = (ctypes.c_int8 * len(codecs))(*codecs) if codecs else None
    tail = [ctypes.byref(groups) if groups is not None else None] if entry.endswith(("_grouped", "_strings")) else []
    tail += [ctypes.byref(strings) if strings is not None else None] if entry.endswith("_strings") else []
    with pp.ExportedBatch(record) as ex:
        rc = getattr(pp.lib(), entry)(ctypes.addressof(ex.array), ctypes.addressof(ex.schema), ctypes.byref(opts), None, 0, ctypes.cast(arr, ctypes.c_void_p) if codecs else None,
                                      len(codecs) if codecs else 0, None, None, ctypes.byref(runs) if runs is not None else None, *tail, ctypes.byref(out), ctypes.byref(nb))
    if rc != 0:
        assert not out.value
        return rc, pp.lib().fdb_last_error().decode()
    try:
        return 0, ctypes.string_at(out.value, nb.value)
    finally:
        pp.lib().fdb_bytes_free(out.value)


def forms_struct(pp, forms, n=None, pad=0):
    arr = (ctypes.c_int8 * max(1, len(forms)))(*forms)
    s = pp.ParquetStringOptions(ctypes.cast(arr, ctypes.c_void_p), len(forms) if n is None else n, pad)
    s._keep = arr
    return s


def test_without_string_options_the_bytes_are_the_older_calls(pp):
    record = cases.mixed_record(1000, "alternate", dict_size=300)
    n = record.num_columns
    run_arr = (ctypes.c_int8 * n)(*R.flags_of(record, True))
    all_runs = pp.ParquetRunOptions(ctypes.cast(run_arr, ctypes.c_void_p), n, 0)
    for codecs in (None, [1] * n):
        for runs in (None, all_runs):
            for groups in (None, pp.ParquetGroupOptions(128, 1, 0)):
                rc, old = call_strings(pp, record, None, codecs=codecs, runs=runs, groups=groups, entry="fdb_selftest_parquet_write_grouped")
                assert rc == 0
                for strings in (None, forms_struct(pp, [], 0), forms_struct(pp, [0] * n)):
                    assert call_strings(pp, record, strings, codecs=codecs, runs=runs, groups=groups) == (0, old)
    for kw in (dict(), dict(optional={"dense": True}), dict(encodings={"timestamp": "delta"}), dict(compression="snappy"), dict(statistics="page", index_size_limit=4),
               dict(bloom_filters=["labels.utf8"], bloom_bits_per_value=3), dict(runs=True), dict(row_group_rows=128), dict(dictionaries="used")):
        old = pp.selftest_parquet_write(record, page_rows=PAGE, **kw)
        for strings in (None, {}, {"labels.utf8": None}, {"labels.utf8": "dictionary", "plain_bin": None}, [None] * n):
            assert pp.selftest_parquet_write(record, page_rows=PAGE, strings=strings, **kw) == old
        assert pp.selftest_parquet_write(record, page_rows=PAGE, strings="plain", **kw) != old


def test_refusals(pp):
    record = cases.mixed_record(100, "alternate")
    names = record.schema.names
    n = record.num_columns
    for count in (1, n - 1, n + 1, -1):
        rc, text = call_strings(pp, record, forms_struct(pp, [0] * n, count))
        assert rc == pp.FDB_ERR_INVALID and "`forms` has %d entries, the record %d columns" % (count, n) in text, text
    rc, text = call_strings(pp, record, pp.ParquetStringOptions(None, n, 0))
    assert rc == pp.FDB_ERR_INVALID and "`forms` has" in text
    for e in (-1, 3, 7):
        forms = [0] * n
        forms[4] = e
        rc, text = call_strings(pp, record, forms_struct(pp, forms))
        assert rc == pp.FDB_ERR_INVALID and "forms[4] is %d" % e in text, text
    rc, text = call_strings(pp, record, forms_struct(pp, [0] * n, pad=5))
    assert rc == pp.FDB_ERR_INVALID and "pad is 5" in text, text
    for j, name in enumerate(names):
        if Y.is_byte_array(record.schema.field(name).type):
            continue
        for form, word in ((1, "PLAIN"), (2, "DELTA_LENGTH_BYTE_ARRAY")):
            forms = [0] * n
            forms[j] = form
            rc, text = call_strings(pp, record, forms_struct(pp, forms))
            assert rc == pp.FDB_ERR_UNSUPPORTED and word in text and "column %s is not one" % name in text, text
    # runs of indices on a column with a form: it has no index pages
    j = names.index("labels.utf8")
    flags, forms = [0] * n, [0] * n
    flags[j], forms[j] = 1, 2
    run_arr = (ctypes.c_int8 * n)(*flags)
    rc, text = call_strings(pp, record, forms_struct(pp, forms), runs=pp.ParquetRunOptions(ctypes.cast(run_arr, ctypes.c_void_p), n, 0))
    assert rc == pp.FDB_ERR_UNSUPPORTED and "labels.utf8" in text and "no index pages" in text, text
    flags[j] = 2
    run_arr = (ctypes.c_int8 * n)(*flags)
    assert call_strings(pp, record, forms_struct(pp, forms), runs=pp.ParquetRunOptions(ctypes.cast(run_arr, ctypes.c_void_p), n, 0))[0] == 0
    # after everything the older calls refuse, the group options' included
    bad = forms_struct(pp, [3] * n, pad=5)
    rc, text = call_strings(pp, record, bad, page_rows=100)
    assert rc == pp.FDB_ERR_INVALID and "page_rows" in text
    rc, text = call_strings(pp, record, bad, codecs=[2] + [0] * (n - 1))
    assert rc == pp.FDB_ERR_INVALID and "codecs[0] is 2" in text
    rc, text = call_strings(pp, record, bad, runs=pp.ParquetRunOptions(None, n, 0))
    assert rc == pp.FDB_ERR_INVALID and "run options" in text
    rc, text = call_strings(pp, record, bad, groups=pp.ParquetGroupOptions(65, 0, 0))
    assert rc == pp.FDB_ERR_INVALID and "row_group_rows" in text
    # the binding: a bare form skips what cannot take it, names and lists are explicit
    assert pp.selftest_parquet_write(record, strings="plain", runs={"labels.utf8": "values"}) == pp.selftest_parquet_write(
        record, strings={"labels.bin": "plain", "plain_str": "plain", "plain_bin": "plain"}, runs={"labels.utf8": "values"})
    for kw, code, text in (({"strings": "delta"}, pp.FDB_ERR_INVALID, "`strings` is None, 'plain', 'delta_length'"), ({"strings": {"nope": "plain"}}, pp.FDB_ERR_INVALID, "names no column of the record: nope"),
                           ({"strings": ["plain"]}, pp.FDB_ERR_INVALID, "`strings` has 1 entries"), ({"strings": {"plain_str": "rle"}}, pp.FDB_ERR_INVALID, "unknown string form 'rle'"),
                           ({"strings": {"plain_str": 1}}, pp.FDB_ERR_INVALID, "unknown string form 1"), ({"strings": {"timestamp": "plain"}}, pp.FDB_ERR_UNSUPPORTED, "column timestamp is not one"),
                           ({"strings": {"labels.utf8": "plain"}, "runs": {"labels.utf8": True}}, pp.FDB_ERR_UNSUPPORTED, "no index pages")):
        with pytest.raises(pp.FdbError) as e:
            pp.selftest_parquet_write(record, **kw)
        assert e.value.code == code and text in str(e.value), (kw, str(e.value))
    # a row that points past its dictionary is refused as it is in the dictionary form
    ok = pa.DictionaryArray.from_arrays(pa.array([0, 1, 0], type=pa.uint32()), pa.array([b"a", b"b"], type=pa.binary()))
    idx = np.frombuffer(ok.indices.buffers()[1], dtype=np.uint32).copy()
    idx[1] = 70
    wrong = pa.DictionaryArray.from_arrays(pa.Array.from_buffers(pa.uint32(), 3, [None, pa.py_buffer(idx.tobytes())]), ok.dictionary, safe=False)
    texts = []
    for kw in (dict(), dict(strings="plain"), dict(strings="delta_length")):
        with pytest.raises(pp.FdbError) as e:
            pp.selftest_parquet_write(pa.RecordBatch.from_arrays([wrong], names=["d"]), **kw)
        assert e.value.code == pp.FDB_ERR_INVALID and "out of range" in str(e.value)
        texts.append(str(e.value))
    assert texts[0] == texts[1] == texts[2]


@pytest.mark.parametrize("form", Y.FORMS)
def test_a_page_that_would_not_fit_its_header_is_refused_by_the_survey(pp, form):
    """A one-entry dictionary of 1 MiB referred to by 2 049 rows of one page: 2 GiB and more of values. The byte survey's sums alone
    answer — the refusal comes before any image is allocated, so the process's peak memory stays far below the page."""
    rows = 2049
    record = pa.RecordBatch.from_arrays([Y._dict(np.zeros(rows, np.uint32), [b"\x5a" * (1 << 20)])], names=["labels.big"])
    before = resource.getrusage(resource.RUSAGE_SELF).ru_maxrss
    with pytest.raises(pp.FdbError) as e:
        pp.selftest_parquet_write(record, page_rows=4096, strings=form)
    assert e.value.code == pp.FDB_ERR_INVALID and "page 0 of column labels.big" in str(e.value) and "2^31 - 1" in str(e.value), str(e.value)
    assert resource.getrusage(resource.RUSAGE_SELF).ru_maxrss - before < 512 * 1024   # KiB: no 2 GiB was allocated
    assert len(pp.selftest_parquet_write(record.slice(0, 3), page_rows=4096, strings=form)) > 3 << 20   # three rows of it are written


def test_entry_points_are_in_library_header_exports_binding_and_build(pp):
    L = pp.lib()
    header = open(os.path.join(ROOT, "include", "frostdb_amd.h")).read()
    exports = open(os.path.join(ROOT, "frostdb_amd", "csrc", "exports.map")).read()
    for name in ENTRY_POINTS:
        assert re.search(r"^FDB_API int %s\(.*const fdb_parquet_group_options\* groups /\* NULL: none \*/, const fdb_parquet_string_options\* strings /\* NULL: none \*/, uint8_t\*\* bytes, int64_t\* n_bytes\);" % name,
                         header, flags=re.M), name
        assert getattr(L, name).argtypes is not None and len(getattr(L, name).argtypes) == len(getattr(L, name.replace("_strings", "_grouped")).argtypes) + 1
    assert re.search(r"global:\s*fdb_\*;", exports) and ENTRY_POINTS[0] in exports
    assert re.search(r"typedef struct fdb_parquet_string_options \{\s*const int8_t\* forms;[^}]*int32_t n_columns;[^}]*int32_t pad;[^}]*\} fdb_parquet_string_options;", header)
    assert [f[0] for f in pp.ParquetStringOptions._fields_] == ["forms", "n_columns", "pad"] and ctypes.sizeof(pp.ParquetStringOptions) == 16
    assert (pp.ParquetStringOptions.forms.offset, pp.ParquetStringOptions.n_columns.offset, pp.ParquetStringOptions.pad.offset) == (0, 8, 12)
    assert ctypes.sizeof(pp.ParquetGroupOptions) == 16 and ctypes.sizeof(pp.ParquetWriteOptions) == 16   # the older structs keep their layouts
    assert pp.PARQUET_WRITE_STRINGS == ("_strings", 7) and pp.PARQUET_STRING_FORMS == {None: 0, "dictionary": 0, "plain": 1, "delta_length": 2}
    build = open(os.path.join(ROOT, "frostdb_amd", "build.py")).read()
    assert "fdb_pqbytes.hip" in build and "fdb_pqbytes.h" in build


def test_byte_kernels_compile_for_gfx950_without_scratch(tmp_path):
    """fdb_pqbytes.hip compiled offline for gfx950 with the flags of the writer's compile test: the resource report shows the two
    kernels, no scratch, no spills, and the LDS of the staged tile."""
    src = os.path.join(ROOT, "frostdb_amd", "csrc", "fdb_pqbytes.hip")
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-munsafe-fp-atomics", "-I", os.path.join(ROOT, "frostdb_amd", "csrc"),
                        "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", str(tmp_path / "fdb_pqbytes.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    remarks = [ln.split("remark:", 1)[1].split("[-Rpass")[0].strip() for ln in r.stderr.splitlines() if "remark:" in ln]
    names = [u for u in remarks if u.startswith("Function Name:")]
    print(" | ".join(remarks))
    assert len(names) == 2 and all(any(k in u for u in names) for k in ("pqy_survey_kernel", "pqy_encode_kernel")), names
    scratch = [u for u in remarks if "ScratchSize" in u]
    assert len(scratch) == 2 and all("ScratchSize [bytes/lane]: 0" in u for u in scratch), remarks
    spills = [u for u in remarks if "VGPRs Spill" in u]   # (what would go to scratch; SGPRs of the encode kernel's 64-bit item arithmetic may sit in spare VGPR lanes)
    assert len(spills) == 2 and all(re.search(r"Spill: 0\b", u) for u in spills), remarks
    lds = sorted(int(u.rsplit(":", 1)[1]) for u in remarks if "LDS Size" in u)
    assert len(lds) == 2 and lds[1] >= 2 * 4096 * 4 and lds[1] <= 64 * 1024, remarks   # entries and offsets of a tile's 4 096 values, and little more
