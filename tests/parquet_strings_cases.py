"""PLAIN and DELTA_LENGTH_BYTE_ARRAY value pages of the Parquet writer (fdb_batch_to_parquet_strings), restated for
tests/test_parquet_strings_cpu.py (the host walk) and tests/test_gpu_parquet_strings.py (the device passes).

The rule, from include/frostdb_amd.h: a dictionary / string / binary column with a form has no dictionary page; a data page's body is its
definition levels as ever and then `value_bytes(form, the page's non-NULL values in row order)` — built here from
tests/parquet_pages.py's `plain` and `delta_binary_packed` and concatenation, sharing nothing with the library. The footer says
[PLAIN] or [DELTA_LENGTH_BYTE_ARRAY] (+ RLE of an optional column), no dictionary_page_offset, and sizes that agree with a walk of the
chunk; every page header says encoding 0 or 6. No test lives here."""
import io

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq

from tests import parquet_group_cases as G
from tests import parquet_pages as PG
from tests import parquet_snappy_cases as S
from tests import parquet_write_cases as cases

PAGE = cases.PAGE
FORMS = ("plain", "delta_length")
ENCODING = {"plain": 0, "delta_length": 6}   # parquet.thrift Encoding: PLAIN, DELTA_LENGTH_BYTE_ARRAY
RLE = 3
ZERO_LENGTHS = bytes([0x80, 0x01, 0x04, 0x00, 0x00])   # DELTA_BINARY_PACKED of no value: block 128, 4 miniblocks, count 0, first value 0
CODEC_NAMES = {1: "snappy", 7: "lz4_raw"}
LENGTHS = [0, 1, 3, 4, 5, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1023, 4097]
LONG = 70001


def value_bytes(form: str, values) -> bytes:
    """What follows the definition levels of a page that holds `values` (bytes objects, the non-NULL ones in row order)."""
    if form == "plain":
        return PG.plain(PG.BYTE_ARRAY, values)
    return PG.delta_binary_packed(np.array([len(v) for v in values], dtype=np.int64)) + b"".join(values)


def _varint(data: bytes, at: int):
    v, shift = 0, 0
    while True:
        b = data[at]
        at += 1
        v |= (b & 0x7F) << shift
        shift += 7
        if b < 0x80:
            return v, at


def read_delta_lengths(data: bytes):
    """A reader of DELTA_BINARY_PACKED from the format's description, for whatever block geometry the header names: (the values, the
    offset behind the last miniblock that holds one)."""
    block, at = _varint(data, 0)
    minis, at = _varint(data, at)
    count, at = _varint(data, at)
    z, at = _varint(data, at)
    out = [(z >> 1) ^ -(z & 1)] if count else []
    per = block // minis
    while len(out) < count:
        z, at = _varint(data, at)
        mn = (z >> 1) ^ -(z & 1)
        widths = data[at:at + minis]
        at += minis
        for w in widths:
            if len(out) >= count:
                break   # (a miniblock without a value has no body)
            bits = int.from_bytes(data[at:at + per * w // 8], "little")
            at += per * w // 8
            for j in range(per):
                if len(out) < count:
                    out.append(out[-1] + mn + ((bits >> (j * w)) & ((1 << w) - 1)))
    return out, at


def read_values(form: str, data: bytes, count: int):
    """The `count` values of a page's value bytes, by a reader that shares nothing with `value_bytes`; every byte is accounted for."""
    values, at = [], 0
    if form == "plain":
        for _ in range(count):
            n = int.from_bytes(data[at:at + 4], "little")
            values.append(data[at + 4:at + 4 + n])
            at += 4 + n
    else:
        lens, at = read_delta_lengths(data)
        assert len(lens) == count and all(n >= 0 for n in lens)
        for n in lens:
            values.append(data[at:at + n])
            at += n
    assert at == len(data), (at, len(data))
    return values


def is_byte_array(t: pa.DataType) -> bool:
    t = t.value_type if pa.types.is_dictionary(t) else t
    return pa.types.is_string(t) or pa.types.is_large_string(t) or pa.types.is_binary(t) or pa.types.is_large_binary(t)


def column_values(col: pa.Array):
    """Per row the value's bytes, None where the row is NULL."""
    if pa.types.is_dictionary(col.type):
        col = col.cast(col.type.value_type)
    return col.cast(pa.large_binary()).to_pylist()


def forms_of(record: pa.RecordBatch, strings) -> dict:
    """name → "plain" / "delta_length" for the columns `strings` (a bare form, a dict by name or a list per column) gives a form."""
    names = record.schema.names
    if isinstance(strings, str):
        return {n: strings for n, f in zip(names, record.schema) if is_byte_array(f.type)}
    if isinstance(strings, dict):
        return {n: f for n, f in strings.items() if f in FORMS}
    return {n: f for n, f in zip(names, strings or ()) if f in FORMS}


def chunk_data_pages(data: bytes, ch: dict):
    """[(header offset, header + stored bytes, num_values, encoding, the body inflated)] of a chunk's data pages; a dictionary page asserts."""
    at = ch["dictionary_page_offset"] if ch["dictionary_page_offset"] is not None else ch["data_page_offset"]
    end, out = at + ch["total_compressed_size"], []
    while at < end:
        h, body_at = S._struct(data, at)
        stored = data[body_at:body_at + h[3]]
        assert h[1] == PG.DATA_PAGE, "a page of type %d in a chunk without a dictionary" % h[1]
        body = stored if ch["codec"] == 0 else pa.decompress(stored, decompressed_size=h[2], codec=CODEC_NAMES[ch["codec"]], asbytes=True)
        assert len(body) == h[2]
        out.append((at, body_at - at + h[3], h[5][1], h[5][2], body))
        at = body_at + h[3]
    assert at == end
    return out


def split_levels(body: bytes, optional: bool):
    """(the definition levels with their 4-byte length, the rest) of a data page V1's body."""
    if not optional:
        return b"", body
    n = int.from_bytes(body[:4], "little")
    return body[:4 + n], body[4 + n:]


def assert_strings_file(record: pa.RecordBatch, data: bytes, strings, page_rows: int, rg_rows: int = 0):
    """Every chunk of a column with a form held to the rule: footer fields, page headers, and every page's value bytes against
    `value_bytes` of the page's non-NULL values. Returns the number of pages looked at."""
    forms = forms_of(record, strings)
    pf = pq.ParquetFile(io.BytesIO(data))
    gs = G.groups(data)
    rows, looked = record.num_rows, 0
    R = rg_rows if rg_rows and rows > rg_rows else max(rows, 1)
    assert len(gs) == max(1, -(-rows // R))
    for g, rg in enumerate(gs):
        first, n = g * R, min(R, rows - g * R)
        assert rg["rows"] == n
        for j, ch in enumerate(rg["chunks"]):
            form = forms.get(ch["name"])
            if form is None:
                continue
            col = record.column(j)
            optional = pf.schema.column(j).max_definition_level == 1
            no_values = pa.types.is_dictionary(col.type) and len(col.dictionary) == 0
            if no_values and form == "plain":
                form_enc = 0   # all NULL over an empty dictionary: its present form, PLAIN pages of zero values
            else:
                form_enc = ENCODING[form]
            assert ch["dictionary_page_offset"] is None, ch["name"]
            assert ch["encodings"] == [form_enc] + ([RLE] if optional else []), (ch["name"], ch["encodings"])
            pages = chunk_data_pages(data, ch)
            assert len(pages) == -(-n // page_rows), (ch["name"], len(pages))
            assert not pages or ch["data_page_offset"] == pages[0][0] == ch["file_offset"]
            assert ch["total_uncompressed_size"] == sum((S._struct(data, at)[1] - at) + len(body) for at, size, _nv, _enc, body in pages), ch["name"]
            values = column_values(col)[first:first + n]
            assert ch["null_count"] == sum(v is None for v in values)
            for p, (_at, _size, nv, enc, body) in enumerate(pages):
                page = values[p * page_rows:(p + 1) * page_rows]
                assert (nv, enc) == (len(page), form_enc), (ch["name"], p, nv, enc)
                _levels, rest = split_levels(body, optional)
                held = [v for v in page if v is not None]
                want = value_bytes(form, held) if not (no_values and form == "plain") else b""
                assert rest == want, "column %s, group %d, page %d: %d value bytes, the rule gives %d" % (ch["name"], g, p, len(rest), len(want))
                if form == "delta_length" and not held:
                    assert rest == ZERO_LENGTHS
                looked += 1
    return looked


def assert_reads_back(record: pa.RecordBatch, data: bytes):
    """pyarrow reads `data` back value for value and NULL for NULL."""
    from tests import parquet_runs_cases as R
    assert pq.ParquetFile(io.BytesIO(data)).metadata.num_rows == record.num_rows
    cases.assert_same_record(R.read_back(data), record)


# ---- records ---------------------------------------------------------------------------------------------------------------------------------
def _entry(i: int, n: int) -> bytes:
    """`n` bytes that differ from entry to entry and from byte to byte."""
    return bytes((i * 31 + k * 7 + (k >> 8)) & 0xFF for k in range(n)) if n < 5000 else (np.arange(n, dtype=np.uint32) * 7 + i * 31).astype(np.uint8).tobytes()


def _dict(idx, entries, valid=None, typ=pa.binary()) -> pa.DictionaryArray:
    idx = np.asarray(idx, dtype=np.uint32)
    return pa.DictionaryArray.from_arrays(pa.array(idx, type=pa.uint32(), mask=None if valid is None else ~np.asarray(valid, dtype=bool)), pa.array(entries, type=typ))


def kinds_record(rows: int, pattern: str, seed: int = 0, page: int = PAGE) -> pa.RecordBatch:
    """The four kinds that take a form — dictionary-utf8, dictionary-binary, plain string, plain binary — beside an int64, each under
    the NULL pattern; values of differing lengths, the empty one among them."""
    rng = np.random.default_rng(seed + rows)
    valid = cases.valid_mask(rows, pattern, page)
    idx = rng.integers(0, 37, rows).astype(np.uint32)
    utf8 = ["é" * (i % 5) + "entry-%d" % i for i in range(37)]
    binary = [_entry(i, (i * 3) % 23) for i in range(37)]
    words = np.array(["w" * (int(v) % 9) + str(int(v) % 13) for v in rng.integers(0, 1000, rows)], dtype=object)
    blobs = np.array([_entry(int(v), int(v) % 19) for v in rng.integers(0, 1000, rows)], dtype=object)
    return pa.RecordBatch.from_arrays([_dict(idx, utf8, valid, pa.string()), _dict(idx[::-1].copy(), binary, valid), pa.array(words, type=pa.string(), mask=~valid),
                                       pa.array(blobs, type=pa.binary(), mask=~valid), pa.array(np.arange(rows, dtype=np.int64) * 5 - 3)],
                                      names=["labels.utf8", "labels.bin", "plain_str", "plain_bin", "timestamp"])


def lengths_record(rows: int = 4 * PAGE + 3, long_at=None, valid=None) -> pa.RecordBatch:
    """One dictionary column over entries of every length of LENGTHS and one of LONG bytes (the last entry); `long_at`: the rows that
    hold the long one (default: one row in the middle), every other row walks the other lengths."""
    entries = [_entry(i, n) for i, n in enumerate(LENGTHS)] + [_entry(99, LONG)]
    idx = (np.arange(rows) * 5) % len(LENGTHS)
    for r in ([rows // 2] if long_at is None else long_at):
        idx[r] = len(LENGTHS)
    return pa.RecordBatch.from_arrays([_dict(idx, entries, valid), pa.array(np.arange(rows, dtype=np.int64))], names=["labels.len", "timestamp"])


def empties_record(rows: int = 2 * PAGE + 5) -> pa.RecordBatch:
    """A column of empty strings only (one entry, and an unused longer one), with NULLs."""
    return pa.RecordBatch.from_arrays([_dict(np.zeros(rows, np.uint32), ["", "never"], np.arange(rows) % 3 != 1, pa.string())], names=["labels.empty"])


def duplicates_record(rows: int = 2 * PAGE + 3) -> pa.RecordBatch:
    """Entries of equal bytes under different indices (0, 2, 4), an empty one and unused ones (1, 6)."""
    idx = np.resize(np.array([0, 3, 2, 5, 4, 0], dtype=np.uint32), rows)
    return pa.RecordBatch.from_arrays([_dict(idx, [b"a", b"unused", b"a", b"", b"a", b"c", b"unused too"])], names=["labels.dup"])


def wide_record(rows: int = 3 * PAGE + 5, entries: int = 65537) -> pa.RecordBatch:
    """A dictionary of 65 537 entries with three of them used: the first, one in the middle, the last."""
    used = np.array([0, entries // 2, entries - 1], dtype=np.uint32)
    return pa.RecordBatch.from_arrays([_dict(used[np.arange(rows) % 3], cases.dict_entries(entries, False), np.arange(rows) % 7 != 3)], names=["labels.wide"])


def null_page_record(page: int = PAGE) -> pa.RecordBatch:
    """An all-NULL page between pages of values."""
    rows = 3 * page + 7
    valid = np.ones(rows, dtype=bool)
    valid[page:2 * page] = False
    return kinds_record(rows, "none").set_column(0, "labels.utf8", _dict(np.arange(rows) % 37, ["é" * (i % 5) + "entry-%d" % i for i in range(37)], valid, pa.string()))


def distinct_record(rows: int = 4096, width: int = 16) -> pa.RecordBatch:
    """An all-distinct column of `width`-byte values — ids — beside an int64."""
    ids = [(b"%0*x" % (width, i * 2654435761 % (1 << 60)))[:width] for i in range(rows)]
    return pa.RecordBatch.from_arrays([pa.array(ids, type=pa.binary()), pa.array(np.arange(rows, dtype=np.int64))], names=["id", "timestamp"])


def offsets_record(rows: int = 2 * PAGE) -> pa.RecordBatch:
    """Values whose bytes start at every file offset mod 4: lengths 1, 2, 3, 5, 6, 7 in turn, so that the running sum walks the residues."""
    lens = [1, 2, 3, 5, 6, 7, 0, 9]
    entries = [_entry(i, n) for i, n in enumerate(lens)]
    return pa.RecordBatch.from_arrays([_dict(np.arange(rows) % len(lens), entries, np.arange(rows) % 11 != 4), _dict((np.arange(rows) * 3) % len(lens), entries)], names=["labels.a", "labels.b"])
