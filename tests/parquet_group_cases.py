"""Used-entry dictionaries of the Parquet writer (fdb_batch_to_parquet_grouped, dictionaries = 1), restated for
tests/test_parquet_groups_cpu.py (the host walk) and tests/test_gpu_parquet_groups.py (the device passes).

The rule, from include/frostdb_amd.h: a chunk's dictionary page holds the entries at least one non-NULL row refers to — `numpy.unique` of
the non-NULL indices of the chunk's rows, per row group — in entry order, duplicates of equal bytes both kept when both are used; num_values is their count U; an index
becomes its rank among them; the pages are packed at bits(U − 1); U = 0 is the form of an empty dictionary (no dictionary page, PLAIN
pages of zero values). Bounds and bloom filters are over the same byte values, a filter's size capped by U. Everything else of the file
is what the same call writes with the whole dictionary, which the files are compared with page by page.

Several row groups (row_group_rows = R): rows [g·R, min(rows, (g + 1)·R)) are group g, and the region of its chunks is byte for byte the
chunk region of the file the same call writes for that row slice alone — so are its filters, its ColumnIndexes and, shifted by where
the group starts, its OffsetIndexes (`assert_groups`, over `groups`, which cuts a file into its groups and chunks from the footer)."""
import io
import struct

import numpy as np
import pyarrow as pa

from tests import parquet_bloom_cases as B
from tests import parquet_index_cases as X
from tests import parquet_runs_cases as R
from tests import parquet_snappy_cases as S
from tests import parquet_write_cases as cases

PAGE = cases.PAGE
DICTIONARY_PAGE = 2


def bits(n: int) -> int:
    """bits(U − 1): the width of the indices of a dictionary of `n` entries."""
    return (n - 1).bit_length() if n > 0 else 0


def restate(col: pa.Array):
    """(the used entries' numbers, the page body of the pruned dictionary, the re-keyed index per row, validity) of a dictionary column."""
    valid, idx = R.column_symbols(col)
    entries = col.dictionary.cast(pa.large_binary()).to_pylist()
    used = np.unique(idx[valid].astype(np.int64))
    body = b"".join(struct.pack("<I", len(entries[i])) + entries[i] for i in used.tolist())
    rekeyed = np.searchsorted(used, idx.astype(np.int64))   # (NULL rows: whatever; they are not looked at)
    return used, body, rekeyed, valid


def dictionary_pages(data: bytes):
    """Per column chunk of row group 0 (num_values, the body inflated) of its dictionary page, or None where it has none."""
    import pyarrow.parquet as pq
    rg = pq.ParquetFile(io.BytesIO(data)).metadata.row_group(0)
    out = []
    for j, ch in enumerate(X.chunk_fields(data)):
        col = rg.column(j)
        pages, _start = S.chunk_pages(data, col)
        walked = X.walk_pages(data, ch)
        assert len(pages) == len(walked)
        found = None
        for k, ((ptype, usize, stored, _hl), (_pos, _size, wtype, nv)) in enumerate(zip(pages, walked)):
            assert ptype == wtype
            if ptype != DICTIONARY_PAGE:
                continue
            assert k == 0 and found is None, "one dictionary page, the chunk's first"
            body = stored if col.compression == "UNCOMPRESSED" else pa.decompress(stored, decompressed_size=usize, codec=col.compression.lower(), asbytes=True)
            found = (nv, body)
        assert (found is not None) == col.has_dictionary_page
        out.append(found)
    return out


def ordinal(data: bytes):
    """RowGroup.ordinal of row group 0, None where it is not written."""
    return X.file_metadata(data)[4][0].get(7)


def assert_used_file(record: pa.RecordBatch, data: bytes, whole: bytes, page_rows: int, flags=None, bloom_filters=None, bits_per_value: int = 0, sorting_columns=None):
    """`data` (dictionaries = "used") against the restatement and against `whole` (the same call with the whole dictionary): every
    dictionary page, width byte and decoded index stream; no page longer; bounds unchanged; filters over the same values, sized by U;
    footer sizes agree with a walk of the chunks. `flags`: the run bits per column, as parquet_runs_cases.flags_of makes them."""
    flags = flags or [0] * record.num_columns
    _pf, cols = R.data_pages(data)
    _pf0, cols0 = R.data_pages(whole)
    dicts, dicts0 = dictionary_pages(data), dictionary_pages(whole)
    fields, fields0 = X.chunk_fields(data), X.chunk_fields(whole)
    assert ordinal(data) == 0 and ordinal(whole) is None
    n_pages = -(-record.num_rows // page_rows)
    pruned = 0
    for j, ((col, sc, pages), (col0, _s0, pages0)) in enumerate(zip(cols, cols0)):
        name = record.schema.names[j]
        optional = sc.max_definition_level == 1
        assert (fields[j]["min_value"], fields[j]["max_value"], fields[j]["null_count"]) == (fields0[j]["min_value"], fields0[j]["max_value"], fields0[j]["null_count"]), name
        assert len(pages) == len(pages0) == n_pages, name
        if not pa.types.is_dictionary(record.column(j).type):   # other columns — a plain string column's interned entries are all used — stay as they are
            assert pages == pages0 and dicts[j] == dicts0[j], name
            continue
        used, body, rekeyed, valid = restate(record.column(j))
        U = len(used)
        pruned += U < len(record.column(j).dictionary)
        if U == 0:
            assert dicts[j] is None and col.encodings == ("PLAIN", "RLE") and not col.has_dictionary_page, name
        else:
            assert dicts[j] == (U, body), (name, dicts[j][0], U)
            assert col.encodings == col0.encodings
        for p, (page, page0) in enumerate(zip(pages, pages0)):
            lo, hi = p * page_rows, min((p + 1) * page_rows, record.num_rows)
            assert len(page) <= len(page0), (name, p, len(page), len(page0))
            levels, width, rest = R.split_page(page, optional, U > 0)
            levels0, _w0, _r0 = R.split_page(page0, optional, True)
            assert levels == levels0, (name, p)
            v = valid[lo:hi]
            count = int(v.sum())
            if U == 0:
                assert count == 0 and rest == b"", (name, p)
                continue
            assert width == bits(U), (name, p, width, U)
            got, _runs = R.decode_hybrid(rest, width, count)
            assert got == [int(i) for i in rekeyed[lo:hi][v]], (name, p)
            assert rest == (R.stream_bytes(got, width) if flags[j] & 1 else R.plain_bytes(got, width)), (name, p)
    at = 4
    for ch in fields:   # the chunks follow each other and their pages fill total_compressed_size exactly (walk_pages asserts it)
        assert (ch["dictionary_page_offset"] if ch["dictionary_page_offset"] is not None else ch["data_page_offset"]) == at, ch["name"]
        walked = X.walk_pages(data, ch)
        if ch["offset_index"] is not None:
            assert [(pos, size) for pos, size, ptype, _nv in walked if ptype == S.DATA_PAGE] == [(o, s) for o, s, _r in X.offset_index(data, ch["offset_index"])], ch["name"]
        at += ch["total_compressed_size"]
    assert X.row_group_fields(data)["total_compressed_size"] == at - 4
    for j in range(record.num_columns):   # the ColumnIndex says what it said
        ci, ci0 = fields[j]["column_index"], fields0[j]["column_index"]
        assert (ci is None) == (ci0 is None)
        if ci is not None:
            assert X.column_index(data, ci) == X.column_index(whole, ci0), record.schema.names[j]
    chosen = B.chosen_columns(record, bloom_filters, sorting_columns)
    for j, where in enumerate(B.filter_fields(data)):
        assert (where is not None) == (j in chosen)
        if where is None:
            continue
        off, length = where
        hashes, n = B.column_hashes(record.column(j))
        if pa.types.is_dictionary(record.column(j).type):
            n = min(n, len(restate(record.column(j))[0]))
        num_bytes, header_len = B.read_header(data, off)
        assert num_bytes == B.filter_bytes(n, bits_per_value) and length == header_len + num_bytes, (record.schema.names[j], num_bytes, n)
        assert data[off + header_len:off + length] == B.build(hashes, num_bytes), record.schema.names[j]
    return pruned


# ---- several row groups -----------------------------------------------------------------------------------------------------------------------
def groups(data: bytes):
    """Per row group of the footer its fields and, as X.chunk_fields names them, its chunks' (with num_values and the filter's place)."""
    out = []
    for rg in X.file_metadata(data)[4]:
        chunks = []
        for cc in rg[1]:
            m = cc[3]
            st = m.get(12, {})
            chunks.append({"name": b".".join(m[3]).decode(), "codec": m[4], "num_values": m[5], "total_uncompressed_size": m[6], "total_compressed_size": m[7], "data_page_offset": m[9],
                           "dictionary_page_offset": m.get(11), "encodings": m[2], "null_count": st.get(3), "max_value": st.get(5), "min_value": st.get(6), "file_offset": cc[2],
                           "bloom": (m[14], m[15]) if 14 in m else None, "offset_index": (cc[4], cc[5]) if 4 in cc else None, "column_index": (cc[6], cc[7]) if 6 in cc else None})
        out.append({"rows": rg[3], "total_byte_size": rg[2], "file_offset": rg.get(5), "total_compressed_size": rg.get(6), "ordinal": rg.get(7),
                    "sorting_columns": [(s[1], s[2], s[3]) for s in rg[4]] if 4 in rg else None, "chunks": chunks})
    return out


def chunk_region(data: bytes, rg: dict) -> bytes:
    """The bytes of a row group's chunks: its pages, dictionary pages included."""
    return data[rg["file_offset"]:rg["file_offset"] + rg["total_compressed_size"]]


def group_dictionary_pages(data: bytes, rg: dict):
    """Per chunk of a row group (num_values, the stored body) of its dictionary page, or None where it has none."""
    out = []
    for ch in rg["chunks"]:
        first = X.walk_pages(data, ch)[0] if ch["total_compressed_size"] else None
        if first is None or first[2] != DICTIONARY_PAGE:
            assert ch["dictionary_page_offset"] is None
            out.append(None)
            continue
        t = X.Thrift(data, first[0])
        t.struct()
        out.append((first[3], data[t.pos:first[0] + first[1]]))
    return out


def interned(record: pa.RecordBatch) -> pa.RecordBatch:
    """The record as the writer holds it: a plain string / binary column is a dictionary column of its values in order of first
    appearance. A slice of THIS record keeps the column's whole dictionary, as a group of the record does; a slice of the plain column
    would be interned anew. (The callers check that both forms give the same file.)"""
    cols = []
    for col in record.columns:
        if pa.types.is_string(col.type) or pa.types.is_binary(col.type) or pa.types.is_large_string(col.type) or pa.types.is_large_binary(col.type):
            enc = col.dictionary_encode()
            col = pa.DictionaryArray.from_arrays(enc.indices.cast(pa.uint32()), enc.dictionary)
        cols.append(col)
    return pa.RecordBatch.from_arrays(cols, names=record.schema.names)


def assert_groups(record: pa.RecordBatch, data: bytes, R: int, alone_of):
    """`data`, written with row_group_rows = R, against the files `alone_of(slice)` — the same call without row_group_rows — writes
    for every group's row slice alone: chunk regions, chunk metadata, filters, ColumnIndexes and OffsetIndexes; the footer's sizes and
    PageLocations agree with a walk of the chunks; the regions are pages | filters | ColumnIndexes | OffsetIndexes | footer, each in
    (group, column) order; ordinal, file_offset and sorting_columns are per group. Returns the groups."""
    gs = groups(data)
    rows = record.num_rows
    assert len(gs) == max(1, -(-rows // R)), (len(gs), rows, R)
    assert X.file_metadata(data)[3] == rows
    at = 4
    for g, rg in enumerate(gs):
        n = min(R, rows - g * R)
        assert (rg["rows"], rg["ordinal"], rg["file_offset"]) == (n, g, at), (g, rg["rows"], rg["ordinal"], rg["file_offset"], at)
        alone = alone_of(record.slice(g * R, n))
        a = groups(alone)
        assert len(a) == 1
        a = a[0]
        assert chunk_region(data, rg) == chunk_region(alone, a), "group %d's chunks are not those of its rows alone" % g
        assert (rg["sorting_columns"], rg["total_byte_size"], rg["total_compressed_size"]) == (a["sorting_columns"], a["total_byte_size"], a["total_compressed_size"]), g
        shift = at - 4
        assert len(rg["chunks"]) == len(a["chunks"]) == record.num_columns
        for ch, ch0 in zip(rg["chunks"], a["chunks"]):
            where = (g, ch["name"])
            for key in ("name", "codec", "num_values", "encodings", "total_uncompressed_size", "total_compressed_size", "null_count", "min_value", "max_value"):
                assert ch[key] == ch0[key], (where, key, ch[key], ch0[key])
            assert ch["num_values"] == n
            for key in ("data_page_offset", "dictionary_page_offset", "file_offset"):
                assert ch[key] == (ch0[key] + shift if ch0[key] is not None else None), (where, key)
            walked = X.walk_pages(data, ch)   # (asserts that the pages fill total_compressed_size exactly)
            assert (ch["bloom"] is None) == (ch0["bloom"] is None), where
            if ch["bloom"] is not None:
                assert data[ch["bloom"][0]:sum(ch["bloom"])] == alone[ch0["bloom"][0]:sum(ch0["bloom"])], where
            assert (ch["column_index"] is None) == (ch0["column_index"] is None) and (ch["offset_index"] is None) == (ch0["offset_index"] is None), where
            if ch["column_index"] is not None:
                assert X.column_index(data, ch["column_index"]) == X.column_index(alone, ch0["column_index"]), where
            if ch["offset_index"] is not None:
                oi = X.offset_index(data, ch["offset_index"])
                assert [(o - shift, s, r) for o, s, r in oi] == X.offset_index(alone, ch0["offset_index"]), where
                assert [(pos, size) for pos, size, ptype, _nv in walked if ptype == S.DATA_PAGE] == [(o, s) for o, s, _r in oi], where
        at += rg["total_compressed_size"]
    chunks = [ch for rg in gs for ch in rg["chunks"]]
    for key in ("bloom", "column_index", "offset_index"):   # each region in (group, column) order, one piece after the other, the regions in this order
        for ch in chunks:
            if ch[key] is not None:
                assert ch[key][0] == at, (key, ch["name"], ch[key][0], at)
                at += ch[key][1]
    assert at == len(data) - 8 - struct.unpack_from("<I", data, len(data) - 8)[0], "the footer follows the last OffsetIndex"
    return gs


def grouped_record(rows: int, R: int, seed: int = 0) -> pa.RecordBatch:
    """Dictionary columns whose groups differ: `labels.g` names other entries in every group (and one entry in a group's first page),
    `labels.gap` is all NULL in every second group, `labels.dup` names duplicate and empty entries; an int64 and a plain string column."""
    rng = np.random.default_rng(seed + rows + R)
    r = np.arange(rows)
    g = r // R
    idx = (g * 37 + rng.integers(0, 5, rows) * 3) % 4097
    idx[(r % R) < 64] = (g[(r % R) < 64] * 37 + 64) % 4097
    gap_valid = (g % 2 == 0) & (r % 3 != 1)
    dup = np.resize(np.array([0, 3, 2, 5, 2, 0], dtype=np.uint32), rows)
    words = np.array(["w%d" % (v % 11) for v in rng.integers(0, 1000, rows)], dtype=object)
    return pa.RecordBatch.from_arrays([_dict(idx, cases.dict_entries(4097, True), r % 5 != 2, typ=pa.string()), _dict((r * 7) % 65, cases.dict_entries(65, False), gap_valid),
                                       _dict(dup, [b"a", b"b", b"a", b"", b"a", b"c"]), pa.array(r.astype(np.int64) * 3 - 7), pa.array(words, type=pa.string(), mask=(r % 4 == 3))],
                                      names=["labels.g", "labels.gap", "labels.dup", "timestamp", "plain_str"])


# ---- records ---------------------------------------------------------------------------------------------------------------------------------
def _dict(idx, entries, valid=None, typ=pa.binary()) -> pa.DictionaryArray:
    idx = np.asarray(idx, dtype=np.uint32)
    return pa.DictionaryArray.from_arrays(pa.array(idx, type=pa.uint32(), mask=None if valid is None else ~np.asarray(valid, dtype=bool)), pa.array(entries, type=typ))


DICT_SIZES = [1, 2, 63, 64, 65, 4097, 65537]
USED = [0, 1, 3, "all"]


def sized_record(entries: int, used, rows: int = 3 * PAGE + 5, seed: int = 0) -> pa.RecordBatch:
    """A dictionary of `entries` entries of which `used` (a count, or "all") are referred to — the last entry among them, so the whole
    dictionary's width is needed — beside an int64. 0 used: every row NULL."""
    rng = np.random.default_rng(seed + entries)
    values = cases.dict_entries(entries, False)
    if used == "all":
        rows = max(rows, entries + entries // 6 + 3)
        idx = np.resize(rng.permutation(entries), rows)
        valid = np.ones(rows, dtype=bool)
        valid[::7] = False
        idx[np.flatnonzero(valid)[:entries]] = np.arange(entries)   # every entry is named by a row that holds a value
    else:
        k = min(used, entries)
        pick = np.sort(np.concatenate([[entries - 1], rng.choice(entries - 1, k - 1, replace=False)]))[:k] if k > 0 else np.zeros(1, dtype=np.int64)
        idx = pick[rng.integers(0, len(pick), rows)]
        valid = np.arange(rows) % 5 != 2 if k > 0 else np.zeros(rows, dtype=bool)
        if k > 0:
            idx[np.flatnonzero(valid)[:k]] = pick
    return pa.RecordBatch.from_arrays([_dict(idx, values, valid), pa.array(np.arange(rows, dtype=np.int64))], names=["labels.d", "timestamp"])


def word_edges_record(rows: int = 2 * PAGE + 9) -> pa.RecordBatch:
    """Dictionaries of 200 entries: used entries only in the first presence word, only in the last, and entries 31, 32 and 63 of a word."""
    r = np.arange(rows)
    values = cases.dict_entries(200, True)
    first = _dict(np.array([0, 5, 63])[r % 3], values, typ=pa.string())
    last = _dict(np.array([192, 199])[r % 2], values, r % 4 != 1, typ=pa.string())
    bits_ = _dict(np.array([64 + 31, 64 + 32, 64 + 63, 31, 32, 128])[r % 6], values, typ=pa.string())
    return pa.RecordBatch.from_arrays([first, last, bits_], names=["labels.first", "labels.last", "labels.bits"])


def duplicates_record(rows: int = 2 * PAGE + 3) -> pa.RecordBatch:
    """Entries of equal bytes and an empty entry: 0 and 2 are both b"a" and both used; 4 (b"a" again) and 1 are not."""
    idx = np.resize(np.array([0, 3, 2, 5, 2, 0], dtype=np.uint32), rows)
    return pa.RecordBatch.from_arrays([_dict(idx, [b"a", b"b", b"a", b"", b"a", b"c"])], names=["labels.dup"])


def equal_pages_record(rows: int = 4 * PAGE + 7) -> pa.RecordBatch:
    """Pages whose used indices are all equal — the RLE value is the rank, not the old index — beside mixed pages and a page of NULLs."""
    r = np.arange(rows)
    page = r // PAGE
    idx = np.where(page % 2 == 0, 90 + 3 * page, 17 + (r % 5) * 11).astype(np.uint32)
    valid = np.ones(rows, dtype=bool)
    valid[page == 3] = False
    valid[(page == 2) & (r % 3 == 0)] = False
    return pa.RecordBatch.from_arrays([_dict(idx, cases.dict_entries(300, True), valid, typ=pa.string())], names=["labels.ordered"])


def filtered_record(rows: int, entries: int = 65537, keep: int = 3, seed: int = 9) -> pa.RecordBatch:
    """What filter() leaves of a label column: a wide dictionary of which `keep` entries are referred to, in stretches, with NULLs; a
    plain string column and an int64 beside it."""
    rng = np.random.default_rng(seed)
    pick = np.sort(rng.choice(entries, keep, replace=False))
    idx = pick[np.minimum((np.arange(rows) // 37) % keep, keep - 1)]
    valid = rng.random(rows) < 0.9
    words = np.array(["w%d" % (v % 11) for v in rng.integers(0, 1000, rows)], dtype=object)
    return pa.RecordBatch.from_arrays([_dict(idx, cases.dict_entries(entries, True), valid, typ=pa.string()), pa.array(words, type=pa.string(), mask=~valid),
                                       pa.array(np.arange(rows, dtype=np.int64))], names=["labels.wide", "plain_str", "timestamp"])
