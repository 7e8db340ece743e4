"""What tests/test_parquet_index_cpu.py (the host walk, fdb_selftest_parquet_write_indexed) and tests/test_gpu_parquet_index.py (the device
pass, fdb_batch_to_parquet_indexed) share:

1. a thrift-compact reader, written from parquet.thrift, of what pyarrow does not show: the footer's index fields (ColumnChunk 4 … 7,
   Statistics 5 / 6, RowGroup.sorting_columns, FileMetaData.column_orders), ColumnIndex and OffsetIndex, and the page headers of a chunk;
2. a numpy / bytes restatement of the rules the writer's header states: per page and per chunk the bounds of the non-NULL (non-NaN)
   values in the column's order, the zero rule, the cut of BYTE_ARRAY bounds, null pages, null counts and the boundary order;
3. the record families of both test files."""
import io
import struct

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq

from tests import parquet_write_cases as cases

PAGE = cases.PAGE
UNORDERED, ASCENDING, DESCENDING = 0, 1, 2


# ---- 1. thrift compact ----------------------------------------------------------------------------------------------------------------------
class Thrift:
    """Structs as {field id: value}: bools, integers (zigzag), doubles, binaries as bytes, lists as lists, structs as dicts."""

    def __init__(self, buf: bytes, pos: int = 0):
        self.buf, self.pos = buf, pos

    def byte(self) -> int:
        b = self.buf[self.pos]
        self.pos += 1
        return b

    def varint(self) -> int:
        v, shift = 0, 0
        while True:
            b = self.byte()
            v |= (b & 0x7F) << shift
            shift += 7
            if not b & 0x80:
                return v

    def zigzag(self) -> int:
        v = self.varint()
        return (v >> 1) ^ -(v & 1)

    def value(self, t: int):
        if t in (1, 2):           # a bool outside a field header (a list element): one byte
            return self.byte() == 1
        if t == 3:
            v = self.byte()
            return v - 256 if v >= 128 else v
        if t in (4, 5, 6):
            return self.zigzag()
        if t == 7:
            v = struct.unpack_from("<d", self.buf, self.pos)[0]
            self.pos += 8
            return v
        if t == 8:
            n = self.varint()
            v = bytes(self.buf[self.pos:self.pos + n])
            assert len(v) == n, "binary past the end"
            self.pos += n
            return v
        if t in (9, 10):
            head = self.byte()
            n, et = head >> 4, head & 15
            if n == 15:
                n = self.varint()
            return [self.value(et) for _ in range(n)]
        if t == 12:
            return self.struct()
        raise AssertionError("thrift type %d" % t)

    def struct(self) -> dict:
        out, last = {}, 0
        while True:
            head = self.byte()
            if head == 0:
                return out
            t, delta = head & 15, head >> 4
            fid = last + delta if delta else self.zigzag()
            last = fid
            out[fid] = (t == 1) if t in (1, 2) else self.value(t)


def file_metadata(data: bytes) -> dict:
    assert data[:4] == b"PAR1" and data[-4:] == b"PAR1"
    n = struct.unpack_from("<I", data, len(data) - 8)[0]
    t = Thrift(data, len(data) - 8 - n)
    md = t.struct()
    assert t.pos == len(data) - 8, "the footer's length"
    return md


def chunk_fields(data: bytes):
    """Per column chunk of row group 0 what the index tests look at, by name."""
    md = file_metadata(data)
    out = []
    for cc in md[4][0][1]:
        m = cc[3]
        st = m.get(12, {})
        out.append({"name": b".".join(m[3]).decode(), "codec": m[4], "total_compressed_size": m[7], "data_page_offset": m[9], "dictionary_page_offset": m.get(11),
                    "null_count": st.get(3), "max_value": st.get(5), "min_value": st.get(6), "deprecated": (st.get(1), st.get(2)),
                    "offset_index": (cc[4], cc[5]) if 4 in cc else None, "column_index": (cc[6], cc[7]) if 6 in cc else None})
    return out


def row_group_fields(data: bytes) -> dict:
    md = file_metadata(data)
    rg = md[4][0]
    return {"total_byte_size": rg[2], "total_compressed_size": rg.get(6), "file_offset": rg.get(5),
            "sorting_columns": [(s[1], s[2], s[3]) for s in rg[4]] if 4 in rg else None, "column_orders": md.get(7)}


def column_index(data: bytes, where) -> dict:
    off, n = where
    t = Thrift(data, off)
    s = t.struct()
    assert t.pos == off + n, "the ColumnIndex's length"
    return {"null_pages": s[1], "min_values": s[2], "max_values": s[3], "boundary_order": s[4], "null_counts": s.get(5)}


def offset_index(data: bytes, where):
    """[(offset, compressed_page_size, first_row_index)]"""
    off, n = where
    t = Thrift(data, off)
    s = t.struct()
    assert t.pos == off + n, "the OffsetIndex's length"
    return [(p[1], p[2], p[3]) for p in s[1]]


def walk_pages(data: bytes, chunk: dict):
    """The pages of a chunk, found by reading header after header: [(header offset, header + stored body, page type, num_values)]."""
    start = chunk["dictionary_page_offset"] if chunk["dictionary_page_offset"] is not None else chunk["data_page_offset"]
    end = start + chunk["total_compressed_size"]
    pos, pages = start, []
    while pos < end:
        t = Thrift(data, pos)
        h = t.struct()
        size = t.pos - pos + h[3]
        pages.append((pos, size, h[1], (h.get(5) or h.get(7))[1]))
        pos += size
    assert pos == end
    return pages


# ---- 2. the rules, restated ------------------------------------------------------------------------------------------------------------------
def cut_min(b: bytes, limit: int) -> bytes:
    return b[:limit]


def cut_max(b: bytes, limit: int) -> bytes:
    if len(b) <= limit:
        return b
    p = b[:limit].rstrip(b"\xff")
    if not p:
        return b
    return p[:-1] + bytes([p[-1] + 1])


def _column_values(col: pa.Array):
    """(kind, python values with None for NULL) — numbers as python ints / floats, strings as bytes."""
    col = col.combine_chunks() if isinstance(col, pa.ChunkedArray) else col
    typ = col.type
    if pa.types.is_dictionary(typ):
        return "bytes", col.dictionary_decode().cast(pa.large_binary()).to_pylist()
    if typ in (pa.string(), pa.binary(), pa.large_string(), pa.large_binary()):
        return "bytes", col.cast(pa.large_binary()).to_pylist()
    if typ == pa.bool_():
        return "bool", col.to_pylist()
    if typ == pa.float64():
        valid = np.asarray(col.is_valid()).astype(bool) if len(col) else np.zeros(0, dtype=bool)
        bits = cases._bits(col)
        return "f64", [float(np.uint64(b).view(np.float64)) if v else None for b, v in zip(bits.tolist(), valid.tolist())]
    if typ == pa.int64():
        return "i64", col.to_pylist()
    if typ == pa.uint64():
        return "u64", col.to_pylist()
    raise AssertionError(typ)


def _bound_bytes(kind: str, v, is_max: bool) -> bytes:
    if kind == "bytes":
        return v
    if kind == "bool":
        return bytes([int(v)])
    if kind == "f64":
        if v == 0.0:
            v = 0.0 if is_max else -0.0
        return struct.pack("<d", v)
    return struct.pack("<q" if kind == "i64" else "<Q", v)


def _bounds(kind: str, values):
    """(min, max) of the values that count, as python values; None when there is none."""
    vs = [v for v in values if v is not None and not (kind == "f64" and v != v)]
    return (min(vs), max(vs)) if vs else None


def expected_index(record: pa.RecordBatch, page_rows: int, limit: int = 16):
    """Per column: {"min_value", "max_value" (None: not written), "column_index" (None: the column gets none)}."""
    limit = limit or 16
    out = []
    for j in range(record.num_columns):
        kind, values = _column_values(record.column(j))
        whole = _bounds(kind, values)
        e = {"min_value": _bound_bytes(kind, whole[0], False) if whole else None, "max_value": _bound_bytes(kind, whole[1], True) if whole else None}
        null_pages, mins, maxs, nulls, keys, sayable = [], [], [], [], [], True
        for first in range(0, len(values), page_rows):
            page = values[first:first + page_rows]
            count = sum(v is not None for v in page)
            b = _bounds(kind, page)
            nulls.append(len(page) - count)
            null_pages.append(count == 0)
            if b is None:
                sayable = sayable and count == 0
                mins.append(b"")
                maxs.append(b"")
                continue
            lo, hi = _bound_bytes(kind, b[0], False), _bound_bytes(kind, b[1], True)
            if kind == "bytes":
                lo, hi = cut_min(lo, limit), cut_max(hi, limit)
                keys.append((lo, hi))
            else:
                keys.append(b)  # (numbers compare as numbers; −0.0 == +0.0)
            mins.append(lo)
            maxs.append(hi)
        up = all(a[0] <= b[0] and a[1] <= b[1] for a, b in zip(keys, keys[1:]))
        down = all(a[0] >= b[0] and a[1] >= b[1] for a, b in zip(keys, keys[1:]))
        e["column_index"] = {"null_pages": null_pages, "min_values": mins, "max_values": maxs, "null_counts": nulls,
                             "boundary_order": ASCENDING if up else DESCENDING if down else UNORDERED} if sayable else None
        out.append(e)
    return out


def assert_index(record: pa.RecordBatch, data: bytes, page_rows: int, statistics: str, limit: int = 16):
    """The footer's fields, every ColumnIndex and every OffsetIndex of `data` are what the rules say for `record`."""
    want = expected_index(record, page_rows, limit)
    chunks = chunk_fields(data)
    rg = row_group_fields(data)
    assert rg["column_orders"] == [{1: {}}] * record.num_columns
    assert rg["total_compressed_size"] == sum(c["total_compressed_size"] for c in chunks)
    n_pages = -(-record.num_rows // page_rows)
    at = 4 + sum(c["total_compressed_size"] for c in chunks)  # where the pages end: the index starts here
    seen = []
    for c, w, name in zip(chunks, want, record.schema.names):
        assert c["name"] == name and c["deprecated"] == (None, None)
        assert c["null_count"] == record.column(name).null_count, name
        assert (c["min_value"], c["max_value"]) == (w["min_value"], w["max_value"]), (name, c["min_value"], c["max_value"], w["min_value"], w["max_value"])
        if statistics != "page":
            assert c["column_index"] is None and c["offset_index"] is None, name
            continue
        pages = [p for p in walk_pages(data, c) if p[2] == 0]
        assert len(pages) == n_pages, name
        assert c["offset_index"] is not None, name
        locs = offset_index(data, c["offset_index"])
        assert locs == [(p[0], p[1], i * page_rows) for i, p in enumerate(pages)], (name, locs[:3], pages[:3])
        seen.append(("o",) + c["offset_index"])
        if w["column_index"] is None:
            assert c["column_index"] is None, name
            continue
        assert c["column_index"] is not None, name
        assert column_index(data, c["column_index"]) == w["column_index"], (name, column_index(data, c["column_index"]), w["column_index"])
        seen.append(("c",) + c["column_index"])
    if statistics == "page":  # every ColumnIndex, then every OffsetIndex, back to back between the pages and the footer
        order = [s for s in seen if s[0] == "c"] + [s for s in seen if s[0] == "o"]
        for _, off, n in order:
            assert off == at, (off, at)
            at += n
        assert at == len(data) - 8 - struct.unpack_from("<I", data, len(data) - 8)[0]


def pyarrow_statistics(data: bytes):
    """[(has_min_max, min, max)] per column as pyarrow reads the file."""
    rg = pq.ParquetFile(io.BytesIO(data)).metadata.row_group(0)
    out = []
    for j in range(rg.num_columns):
        s = rg.column(j).statistics
        out.append((s.has_min_max, s.min, s.max) if s is not None and s.has_min_max else (False, None, None))
    return out


def pyarrow_writes(record: pa.RecordBatch) -> bytes:
    buf = io.BytesIO()
    pq.write_table(pa.Table.from_batches([record]), buf, compression="NONE", write_statistics=True)
    return buf.getvalue()


# ---- 3. records ------------------------------------------------------------------------------------------------------------------------------
INDEX_ROWS = [0, 1, 63, 64, 65, 1000, 4097]


def f64(bits) -> np.ndarray:
    return np.array(bits, dtype=np.uint64).view(np.float64)


QNAN, SNAN, NEG_QNAN = 0x7FF8000000000000, 0x7FF0000000000001, 0xFFF80000DEADBEEF
NEG_ZERO, POS_ZERO = 0x8000000000000000, 0x0000000000000000


def values_record() -> pa.RecordBatch:
    """Four pages of 64: extremes; ±inf beside NaNs of every kind; a page of ±0.0 only, in either sign order; a page of NaNs only."""
    n = 4 * PAGE
    r = np.arange(n)
    i64 = np.resize(np.array([-2**63, 2**63 - 1, -1, 0, 1], dtype=np.int64), n)
    u64 = np.resize(np.array([0, 2**64 - 1, 2**63, 2**63 - 1, 1], dtype=np.uint64), n)
    f = np.resize(np.array([0x7FF0000000000000, 0xFFF0000000000000, QNAN, SNAN, NEG_QNAN, 0x3FF0000000000000], dtype=np.uint64), n)
    zeros_a, zeros_b, nan_page = f.copy(), f.copy(), f.copy()
    zeros_a[PAGE:2 * PAGE] = np.resize(np.array([NEG_ZERO, POS_ZERO], dtype=np.uint64), PAGE)
    zeros_b[PAGE:2 * PAGE] = np.resize(np.array([POS_ZERO, NEG_ZERO], dtype=np.uint64), PAGE)
    zeros_b[2 * PAGE:3 * PAGE] = POS_ZERO   # only +0.0: the minimum is still written −0.0
    zeros_a[2 * PAGE:3 * PAGE] = NEG_ZERO   # only −0.0: the maximum is still written +0.0
    nan_page[2 * PAGE:3 * PAGE] = np.resize(np.array([QNAN, SNAN, NEG_QNAN], dtype=np.uint64), PAGE)
    only_nan = np.resize(np.array([QNAN, SNAN, NEG_QNAN], dtype=np.uint64), n)
    valid = r % 5 != 3
    cols = [("i", pa.array(i64)), ("i_null", pa.array(i64, mask=~valid)), ("u", pa.array(u64)), ("u_null", pa.array(u64, mask=~valid)),
            ("f", pa.array(f.view(np.float64))), ("f_null", pa.array(f.view(np.float64), mask=~valid)),
            ("zeros_a", pa.array(zeros_a.view(np.float64))), ("zeros_b", pa.array(zeros_b.view(np.float64), mask=~valid)),
            ("nan_page", pa.array(nan_page.view(np.float64))), ("nan_page_null", pa.array(nan_page.view(np.float64), mask=r % 2 == 1)),
            ("only_nan", pa.array(only_nan.view(np.float64))), ("flag", pa.array(r // PAGE == 2)), ("flag_null", pa.array(r % 3 == 0, mask=~valid))]
    return pa.RecordBatch.from_arrays([c for _, c in cols], names=[n for n, _ in cols])


def _dict(idx, entries, typ=pa.binary(), valid=None) -> pa.DictionaryArray:
    idx = np.asarray(idx, dtype=np.uint32)
    return pa.DictionaryArray.from_arrays(pa.array(idx, mask=None if valid is None else ~valid), pa.array(entries, type=typ))


def strings_record() -> pa.RecordBatch:
    """Three pages of 64 over dictionaries that try the byte order and the cut."""
    n = 3 * PAGE
    r = np.arange(n)
    unused = [b"\x00lowest", b"m", b"b", b"y", b"\xff\xffhighest"]         # the smallest and the largest entry have no row
    dup = [b"b", b"a", b"b", b"", b"a"]                                        # duplicates; the empty string is the minimum
    a15, a16, a17 = b"a" * 15, b"a" * 16, b"a" * 17
    lengths = [a15, a16, a17, b"a" * 16 + b"b", b"a" * 15 + b"\xffz", b"\xff" * 17, b"a" * 14 + b"\xff\xff\xff"]
    raw = [b"\x80\x81", b"\xfe", b"\x00", b"\x7f\xff", b"\xc3\x28", b"ab", b"a", b"abc"]   # not UTF-8; unsigned order; a prefix sorts first
    valid = r % 7 != 2
    cols = [("unused", _dict(1 + r % 3, unused)), ("dup", _dict(r % 5, dup)), ("dup_null", _dict(r % 5, dup, valid=valid)),
            ("lengths", _dict((r // 9) % len(lengths), lengths)), ("ff", _dict(np.where(r < PAGE, 5, np.where(r < 2 * PAGE, 4, 6)), lengths)),
            ("raw", _dict(r % len(raw), raw, valid=valid)), ("utf8", _dict(r % 4, ["zürich", "a", "", "añ" * 12], typ=pa.string())),
            ("plain", pa.array([("p%03d" % (v % 37)) * (1 + v % 7) for v in r], type=pa.string(), mask=~valid)),
            ("plain_bin", pa.array([bytes([255 - v % 3]) * (14 + v % 5) for v in r], type=pa.binary()))]
    return pa.RecordBatch.from_arrays([c for _, c in cols], names=[n for n, _ in cols])


def order_record() -> pa.RecordBatch:
    """Five pages of 64: ascending, descending, constant, unordered, ordered but for a page of NULLs in the middle, mins up and maxes down."""
    n = 5 * PAGE
    r = np.arange(n, dtype=np.int64)
    page = r // PAGE
    middle = page != 2
    names = ["k%02d" % i for i in range(8)]
    nest = np.where(r % PAGE == 0, page, np.where(r % PAGE == 1, 100 - page, 50))    # mins ascend, maxes descend
    cols = [("up", pa.array(r)), ("down", pa.array(-r)), ("same", pa.array(np.full(n, 7, dtype=np.int64))), ("mixed", pa.array((r * 37) % 101)),
            ("up_gap", pa.array(r, mask=~middle)), ("down_gap", pa.array((-r).astype(np.float64), mask=~middle)), ("nested", pa.array(nest)),
            ("up_str", _dict(page, names, typ=pa.string())), ("down_str", _dict(7 - page, names, typ=pa.string(), valid=middle)),
            ("up_u64", pa.array((r.astype(np.uint64) << np.uint64(58)))), ("flag_up", pa.array(page >= 3))]
    return pa.RecordBatch.from_arrays([c for _, c in cols], names=[n for n, _ in cols])


FAMILIES = {"values": values_record, "strings": strings_record, "order": order_record, "empty_dictionary": cases.empty_dictionary_record,
            "rle": cases.rle_record, "duplicates": cases.duplicates_record, "extremes": cases.extremes_record, "large_strings": cases.large_strings_record}
