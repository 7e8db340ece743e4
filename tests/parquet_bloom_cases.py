"""What tests/test_parquet_bloom_cpu.py (the host walk, fdb_selftest_parquet_write_filtered) and tests/test_gpu_parquet_bloom.py (the device
pass, fdb_batch_to_parquet_filtered) share:

1. XXH64 in pure Python, written from the algorithm's description and pinned on its published vectors, and the same function for 8-byte
   values over numpy arrays;
2. a restatement of parquet-format's split-block rule (block, salts, bits) and of the writer's size rule;
3. a BloomFilterHeader reader (the thrift reader of tests/parquet_index_cases.py) and what the header must be, byte for byte;
4. from a record, a column and bits_per_value the expected bitset — and the check of a whole file: footer fields, headers, bitsets, the
   order of the filter and index regions, every PageLocation;
5. the record families of both test files."""
import io
import struct

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq

from tests import parquet_index_cases as X
from tests import parquet_write_cases as cases

PAGE = cases.PAGE
M64 = (1 << 64) - 1
P1, P2, P3, P4, P5 = 0x9E3779B185EBCA87, 0xC2B2AE3D27D4EB4F, 0x165667B19E3779F9, 0x85EBCA77C2B2AE63, 0x27D4EB2F165667C5
SALT = [0x47b6137b, 0x44974d91, 0x8824ad5b, 0xa2b7289d, 0x705495c7, 0x2df1424b, 0x9efc4947, 0x5c6bfb31]
MAX_BYTES = 128 << 20
XXH64_VECTORS = {b"": 0xef46db3751d8e999, b"a": 0xd24ec4f1a98c6e5b, b"abc": 0x44bc2cf5ad770999}


# ---- 1. XXH64, seed 0 ------------------------------------------------------------------------------------------------------------------------
def _rotl(x: int, r: int) -> int:
    return ((x << r) | (x >> (64 - r))) & M64


def _round(acc: int, lane: int) -> int:
    return (_rotl((acc + lane * P2) & M64, 31) * P1) & M64


def _merge(h: int, v: int) -> int:
    return (((h ^ _round(0, v)) * P1) + P4) & M64


def xxh64(data: bytes, seed: int = 0) -> int:
    n, p = len(data), 0
    if n >= 32:
        v1, v2, v3, v4 = (seed + P1 + P2) & M64, (seed + P2) & M64, seed, (seed - P1) & M64
        while p + 32 <= n:
            a, b, c, d = struct.unpack_from("<4Q", data, p)
            v1, v2, v3, v4 = _round(v1, a), _round(v2, b), _round(v3, c), _round(v4, d)
            p += 32
        h = (_rotl(v1, 1) + _rotl(v2, 7) + _rotl(v3, 12) + _rotl(v4, 18)) & M64
        for v in (v1, v2, v3, v4):
            h = _merge(h, v)
    else:
        h = (seed + P5) & M64
    h = (h + n) & M64
    while p + 8 <= n:
        h ^= _round(0, struct.unpack_from("<Q", data, p)[0])
        h = (_rotl(h, 27) * P1 + P4) & M64
        p += 8
    if p + 4 <= n:
        h ^= (struct.unpack_from("<I", data, p)[0] * P1) & M64
        h = (_rotl(h, 23) * P2 + P3) & M64
        p += 4
    while p < n:
        h ^= (data[p] * P5) & M64
        h = (_rotl(h, 11) * P1) & M64
        p += 1
    h ^= h >> 33
    h = (h * P2) & M64
    h ^= h >> 29
    h = (h * P3) & M64
    return h ^ (h >> 32)


def xxh64_of_8_bytes(bits: np.ndarray) -> np.ndarray:
    """xxh64 of the 8 little-endian bytes of every element of a uint64 array (the arithmetic wraps, as numpy's does on arrays)."""
    u = np.uint64
    rotl = lambda x, r: (x << u(r)) | (x >> u(64 - r))
    with np.errstate(over="ignore"):
        v = np.ascontiguousarray(bits, dtype=np.uint64)
        k = rotl(v * u(P2), 31) * u(P1)
        h = np.full(v.shape, (P5 + 8) & M64, dtype=np.uint64) ^ k
        h = rotl(h, 27) * u(P1) + u(P4)
        h ^= h >> u(33)
        h *= u(P2)
        h ^= h >> u(29)
        h *= u(P3)
        return h ^ (h >> u(32))


# ---- 2. the rule, restated ---------------------------------------------------------------------------------------------------------------------
def filter_bytes(n: int, bits_per_value: int = 0) -> int:
    """32 × max(1, ⌈⌈n × b / 8⌉ / 32⌉), at most 128 MiB; b = 0 means 10."""
    b = bits_per_value or 10
    whole_bytes = -(-n * b // 8)
    return min(32 * max(1, -(-whole_bytes // 32)), MAX_BYTES)


def block_of(h: int, n_blocks: int) -> int:
    return ((h >> 32) * n_blocks) >> 32


def bits_of(h: int):
    """The bit set in each of the block's eight words."""
    return [(((h & 0xFFFFFFFF) * s) & 0xFFFFFFFF) >> 27 for s in SALT]


def build(hashes, num_bytes: int) -> bytes:
    """The bitset of `num_bytes` bytes with every hash of the uint64 array `hashes` in it."""
    assert num_bytes % 32 == 0 and num_bytes >= 32
    h = np.unique(np.asarray(hashes, dtype=np.uint64))
    words = np.zeros(num_bytes // 4, dtype="<u4")
    if len(h):
        block = ((h >> np.uint64(32)) * np.uint64(num_bytes // 32)) >> np.uint64(32)
        key = h & np.uint64(0xFFFFFFFF)
        for i, s in enumerate(SALT):
            bit = ((key * np.uint64(s)) & np.uint64(0xFFFFFFFF)) >> np.uint64(27)
            np.bitwise_or.at(words, (block * np.uint64(8) + np.uint64(i)).astype(np.int64), (np.uint64(1) << bit).astype("<u4"))
    return words.tobytes()


def maybe(bitset: bytes, h: int) -> bool:
    """What a reader answers for a value of hash `h`: False = certainly absent."""
    at = block_of(h, len(bitset) // 32) * 32
    words = struct.unpack_from("<8I", bitset, at)
    return all((w >> b) & 1 for w, b in zip(words, bits_of(h)))


# ---- 3. the header ------------------------------------------------------------------------------------------------------------------------------
def header_bytes(num_bytes: int) -> bytes:
    """15 zigzag-varint(numBytes) 1c 1c 00 00 1c 1c 00 00 1c 1c 00 00 00 — BLOCK, XXHASH, UNCOMPRESSED."""
    z, out = num_bytes << 1, bytearray([0x15])
    while z >= 0x80:
        out.append((z & 0x7F) | 0x80)
        z >>= 7
    out.append(z)
    return bytes(out) + bytes.fromhex("1c1c00001c1c00001c1c000000")


def read_header(data: bytes, off: int):
    """(numBytes, the header's length) of the BloomFilterHeader at `off`; algorithm, hash and compression must be the only ones there are."""
    t = X.Thrift(data, off)
    s = t.struct()
    assert s[2] == {1: {}} and s[3] == {1: {}} and s[4] == {1: {}}, s
    return s[1], t.pos - off


def filter_fields(data: bytes):
    """Per column chunk (bloom_filter_offset, bloom_filter_length), or None where the chunk names none."""
    md = X.file_metadata(data)
    return [((cc[3][14], cc[3][15]) if 14 in cc[3] else None) for cc in md[4][0][1]]


# ---- 4. what a column's filter must be ---------------------------------------------------------------------------------------------------------
def column_hashes(col: pa.Array):
    """(the hashes of the non-NULL rows' values, n of the size rule)."""
    col = col.combine_chunks() if isinstance(col, pa.ChunkedArray) else col
    typ = col.type
    valid = cases._validity(col)
    count = int(valid.sum())
    if typ in (pa.int64(), pa.uint64(), pa.float64()):
        return xxh64_of_8_bytes(cases._bits(col)[valid]), count
    if pa.types.is_dictionary(typ):
        entries = col.dictionary.cast(pa.large_binary()).to_pylist()
        used = np.unique(np.asarray(col.indices.fill_null(0)).astype(np.int64)[valid])  # only the entries a non-NULL row refers to
        return np.array([xxh64(entries[i]) for i in used.tolist()], dtype=np.uint64), min(count, len(entries))
    if typ in (pa.string(), pa.binary(), pa.large_string(), pa.large_binary()):
        distinct = set(v for v in col.cast(pa.large_binary()).to_pylist() if v is not None)   # (the writer interns them: its dictionary's length)
        return np.array([xxh64(v) for v in distinct], dtype=np.uint64), min(count, len(distinct))
    raise AssertionError(typ)


def expected_bitset(record: pa.RecordBatch, column, bits_per_value: int = 0) -> bytes:
    col = record.column(column)
    hashes, n = column_hashes(col)
    return build(hashes, filter_bytes(n, bits_per_value))


def chosen_columns(record: pa.RecordBatch, bloom_filters, sorting_columns=None):
    names = record.schema.names
    if bloom_filters == "sorting":
        picked = []
        for e in sorting_columns or ():
            c = e[0] if isinstance(e, (tuple, list)) else e
            c = names.index(c) if isinstance(c, str) else c
            if record.column(c).type != pa.bool_():
                picked.append(c)
        return sorted(set(picked))
    if isinstance(bloom_filters, dict):
        return sorted(names.index(n) for n, on in bloom_filters.items() if on)
    return sorted(names.index(n) for n in (bloom_filters or ()))


def assert_filters(record: pa.RecordBatch, data: bytes, page_rows: int, bloom_filters, bits_per_value: int = 0, statistics=None, sorting_columns=None, limit: int = 0):
    """Footer fields, headers and bitsets of `data` are what the rule says for `record`; the filter regions and the index regions lie in
    the stated order without gap or overlap; with statistics the bounds and every PageLocation are still right."""
    chosen = chosen_columns(record, bloom_filters, sorting_columns)
    fields, chunks, rg = filter_fields(data), X.chunk_fields(data), X.row_group_fields(data)
    meta = pq.ParquetFile(io.BytesIO(data)).metadata.row_group(0)
    assert rg["total_compressed_size"] == sum(c["total_compressed_size"] for c in chunks)   # (pages only)
    at = 4 + sum(c["total_compressed_size"] for c in chunks)
    for j, name in enumerate(record.schema.names):
        seen = meta.column(j).to_dict()
        if j not in chosen:
            assert fields[j] is None and seen.get("bloom_filter_offset") is None and seen.get("bloom_filter_length") is None, name
            continue
        assert fields[j] is not None, name
        off, length = fields[j]
        assert (seen.get("bloom_filter_offset"), seen.get("bloom_filter_length")) == (off, length), name
        assert off == at, (name, off, at)
        hashes, n = column_hashes(record.column(j))
        num_bytes, header_len = read_header(data, off)
        assert num_bytes == filter_bytes(n, bits_per_value), (name, num_bytes, n)
        assert data[off:off + header_len] == header_bytes(num_bytes), name
        assert length == header_len + num_bytes, name
        bitset = data[off + header_len:off + length]
        want = expected_bitset(record, j, bits_per_value)
        if bitset != want:
            a, b = np.frombuffer(bitset, dtype=np.uint8), np.frombuffer(want, dtype=np.uint8)
            raise AssertionError("%s: the bitset differs from the restatement's at %d of %d bytes" % (name, int((a != b).sum()), num_bytes))
        at += length
    footer_at = len(data) - 8 - struct.unpack_from("<I", data, len(data) - 8)[0]
    if statistics is None:
        assert all(c["column_index"] is None and c["offset_index"] is None for c in chunks)
        assert at == footer_at, (at, footer_at)
        return
    want = X.expected_index(record, page_rows, limit)
    n_pages = -(-record.num_rows // page_rows)
    cis, ois = [], []
    for c, w, name in zip(chunks, want, record.schema.names):
        assert (c["min_value"], c["max_value"]) == (w["min_value"], w["max_value"]), name
        if statistics != "page":
            assert c["column_index"] is None and c["offset_index"] is None, name
            continue
        pages = [p for p in X.walk_pages(data, c) if p[2] == 0]
        assert len(pages) == n_pages and X.offset_index(data, c["offset_index"]) == [(p[0], p[1], i * page_rows) for i, p in enumerate(pages)], name
        ois.append(c["offset_index"])
        if w["column_index"] is None:
            assert c["column_index"] is None, name
            continue
        assert X.column_index(data, c["column_index"]) == w["column_index"], name
        cis.append(c["column_index"])
    for off, n in cis + ois:   # every ColumnIndex, then every OffsetIndex, after the filters and up to the footer
        assert off == at, (off, at)
        at += n
    assert at == footer_at, (at, footer_at)


# ---- 5. records ----------------------------------------------------------------------------------------------------------------------------------
BLOOM_ROWS = [0, 1, 63, 64, 65, 1000, 4097]
EIGHT_BYTE_AND_STRINGS = ["timestamp", "count", "value", "labels.utf8", "labels.bin", "plain_str", "plain_bin", "dense"]  # of cases.mixed_record: all but `flag`


def numeric_record() -> pa.RecordBatch:
    """I64 / U64 extremes and values ≥ 2^63; F64 with NaN payloads, ±inf and both zeros — with and without NULLs."""
    n = 3 * PAGE + 1
    r = np.arange(n)
    i64 = np.resize(np.array([-2**63, 2**63 - 1, -1, 0, 1, 2**62], dtype=np.int64), n)
    u64 = np.resize(np.array([0, 2**64 - 1, 2**63, 2**63 - 1, 2**63 + 12345, 1], dtype=np.uint64), n)
    f = np.resize(np.array(cases.F64_BITS + [X.NEG_QNAN, 0x3FF0000000000000], dtype=np.uint64), n).view(np.float64)
    valid = r % 5 != 3
    cols = [("i", pa.array(i64)), ("i_null", pa.array(i64, mask=~valid)), ("u", pa.array(u64)), ("u_null", pa.array(u64, mask=~valid)),
            ("f", pa.array(f)), ("f_null", pa.array(f, mask=~valid))]
    return pa.RecordBatch.from_arrays([c for _, c in cols], names=[n for n, _ in cols])


STRIPE_LENGTHS = list(range(0, 41)) + [63, 64, 65]   # XXH64's 32-byte stripe loop and its 8-, 4- and 1-byte tails; 31 / 32 / 33 are in the range


def dictionary_record() -> pa.RecordBatch:
    """Unused, duplicate and empty entries; entries of every length around XXH64's stripes and tails; plain strings."""
    n = 3 * PAGE + 7
    r = np.arange(n)
    rng = np.random.default_rng(11)
    lengths = [bytes(rng.integers(0, 256, k, dtype=np.uint8)) for k in STRIPE_LENGTHS]
    unused = [b"never", b"m", b"b", b"y", b"nor this"]
    dup = [b"b", b"a", b"b", b"", b"a"]
    valid = r % 7 != 2
    cols = [("lengths", X._dict(r % len(lengths), lengths)), ("lengths_null", X._dict((r * 5) % len(lengths), lengths, valid=valid)),
            ("unused", X._dict(1 + r % 3, unused)), ("dup", X._dict(r % 5, dup, valid=valid)), ("utf8", X._dict(r % 4, ["zürich", "a", "", "añ" * 12], typ=pa.string())),
            ("plain", pa.array([("p%03d" % (v % 37)) * (1 + v % 9) for v in r], type=pa.string(), mask=~valid)),
            ("plain_bin", pa.array([bytes([255 - v % 3]) * (14 + v % 23) for v in r], type=pa.binary())),
            ("large", pa.array(["large-%d" % (v % 5) for v in r], type=pa.large_string()))]
    return pa.RecordBatch.from_arrays([c for _, c in cols], names=[n for n, _ in cols])


def wide_dictionary_record(rows: int = 24) -> pa.RecordBatch:
    """A 65 537-entry dictionary of which 3 entries are used: what a filtered record keeps. 24 rows at 10 bits each: one block."""
    entries = cases.dict_entries(65537, False)
    idx = np.resize(np.array([5, 65536, 40000], dtype=np.uint32), rows)
    return pa.RecordBatch.from_arrays([X._dict(idx, entries), pa.array(np.arange(rows, dtype=np.int64))], names=["labels.wide", "timestamp"])


def sized_record(values: int) -> pa.RecordBatch:
    """`values` distinct int64 beside a NULL each: at 10 bits per value 25 of them fill one block, 26 need two, 52 three."""
    v = np.repeat(np.arange(values, dtype=np.int64) * 7919 - 3, 2)
    valid = np.arange(2 * values) % 2 == 0
    return pa.RecordBatch.from_arrays([pa.array(v, mask=~valid), X._dict(np.arange(2 * values) // 2, [b"k%d" % i for i in range(values)])], names=["v", "labels.k"])


FAMILIES = {"numeric": numeric_record, "dictionary": dictionary_record, "wide_dictionary": wide_dictionary_record, "empty_dictionary": cases.empty_dictionary_record,
            "rle": cases.rle_record, "duplicates": cases.duplicates_record, "extremes": cases.extremes_record, "large_strings": cases.large_strings_record,
            "values": lambda: X.values_record().drop_columns(["flag", "flag_null"]), "strings": X.strings_record, "order": lambda: X.order_record().drop_columns(["flag_up"])}
