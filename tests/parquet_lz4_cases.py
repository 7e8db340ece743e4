"""What tests/test_parquet_lz4_cpu.py (the host walk of fdb_pqlz4.h, fdb_selftest_parquet_write_*) and tests/test_gpu_parquet_write_lz4.py (the
kernels of fdb_pqlz4.hip, fdb_batch_to_parquet_*) share: a walker of LZ4 sequences written from the block format's description (it shares
nothing with the library) that holds a block to the writer's rule — every match inside one fragment, none starting behind U − 12 or ending
behind U − 5, the last sequence without a match, the block within LZ4_compressBound — and what "the LZ4_RAW file is right" means: every
page inflates under liblz4 (pyarrow's `lz4_raw`, the strict judge: the project's own decoder also takes a block that ends in a match) and
under the project's decoder to the page body of the uncompressed file; the footer says codec 7, read by the tests' own thrift reader;
sizes and offsets follow the compressed sizes; pyarrow reads the record back. The nine ratio corpora of tests/test_parquet_snappy_cpu.py
are restated here, and the byte strings of the rule's shapes are made here for both suites."""
import io

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq

from tests import parquet_index_cases as X
from tests import parquet_snappy_cases as S
from tests import parquet_write_cases as cases

FRAGMENT = S.FRAGMENT
F = FRAGMENT
CODEC = {None: 0, "uncompressed": 0, "snappy": 1, "lz4": 7}
LZ4_RAW = 7
noise, bytes_record, bits_record = S.noise, S.bytes_record, S.bits_record


def bound(u: int) -> int:
    return u + u // 255 + 16


# ---- LZ4 sequences, from the block format's description ------------------------------------------------------------------------------------------
def _length(block, at, nibble):
    n = nibble
    if nibble == 15:
        while True:
            b = block[at]
            at += 1
            n += b
            if b != 255:
                break
    return n, at


def walk_sequences(block: bytes, u: int):
    """[(literal start, literal length, match position, match length, offset)] of the block of a body of `u` bytes, the last with match
    position None; asserts what the writer's rule promises of it."""
    assert len(block) <= bound(u), (len(block), u)
    at, out, seqs = 0, 0, []
    while True:
        assert at < len(block), "the block ends inside a sequence, or in a match"
        token = block[at]
        lit, at = _length(block, at + 1, token >> 4)
        assert at + lit <= len(block)
        start = out
        at, out = at + lit, out + lit
        if at == len(block):
            assert token & 15 == 0, "the last sequence has no match"
            seqs.append((start, lit, None, 0, 0))
            break
        off = block[at] | (block[at + 1] << 8)
        n, at = _length(block, at + 2, token & 15)
        n += 4
        assert off >= 1 and n >= 4
        assert out // F == (out + n - 1) // F, "a match crosses a multiple of FDB_PQS_FRAGMENT: at %d, %d bytes" % (out, n)
        assert off <= out - out // F * F, "a match at %d reaches %d back, before its fragment's first byte" % (out, off)
        assert out <= u - 12, "a match starts at %d, behind U - 12 of %d" % (out, u)
        assert out + n <= u - 5, "a match ends at %d, behind U - 5 of %d" % (out + n, u)
        seqs.append((start, lit, out, n, off))
        out += n
    assert out == u, (out, u)
    return seqs


def matches(block: bytes, u: int):
    """[(position, length, offset)]"""
    return [(p, n, off) for _, _, p, n, off in walk_sequences(block, u) if p is not None]


def inflate(block: bytes, u: int) -> bytes:
    return pa.Codec("lz4_raw").decompress(block, decompressed_size=u, asbytes=True) if u else (b"" if block == b"\0" else None)


# ---- the file ------------------------------------------------------------------------------------------------------------------------------------
def codecs_of(record, compression):
    names = record.schema.names
    if compression is None or isinstance(compression, str):
        return [CODEC[compression]] * len(names)
    if isinstance(compression, dict):
        return [CODEC[compression.get(n)] for n in names]
    return [CODEC[c] for c in compression]


def footer_chunks(data: bytes):
    """Per row group, per column chunk: what the tests' own thrift reader finds of ColumnMetaData and the chunk's index fields."""
    out = []
    for rg in X.file_metadata(data)[4]:
        group = []
        for cc in rg[1]:
            m = cc[3]
            group.append({"name": b".".join(m[3]).decode(), "codec": m[4], "num_values": m[5], "total_uncompressed_size": m[6], "total_compressed_size": m[7], "data_page_offset": m[9],
                          "dictionary_page_offset": m.get(11), "bloom_filter_offset": m.get(14), "bloom_filter_length": m.get(15),
                          "offset_index": (cc[4], cc[5]) if 4 in cc else None, "column_index": (cc[6], cc[7]) if 6 in cc else None})
        out.append(group)
    return out


def chunk_pages(data: bytes, chunk: dict):
    """[(page type, uncompressed size, stored bytes, header bytes, header offset)] of every page of the chunk."""
    start = chunk["dictionary_page_offset"] if chunk["dictionary_page_offset"] is not None else chunk["data_page_offset"]
    at, end, pages = start, start + chunk["total_compressed_size"], []
    while at < end:
        h, body_at = S._struct(data, at)
        pages.append((h[1], h[2], data[body_at:body_at + h[3]], body_at - at, at))
        at = body_at + h[3]
    assert at == end
    return pages, start


def assert_compressed_file(pp, record: pa.RecordBatch, data: bytes, plain: bytes, compression, device: int = -1, read_back: bool = True):
    """`data` (written with `compression`: None / "uncompressed", "snappy" and "lz4" in any mix) against `plain` (the same record and
    options without): chunk for chunk, page for page the same bodies under liblz4 and the project's decoder (on `device`; −1: its host
    decoder), LZ4 blocks held to the rule by walk_sequences, Snappy blocks by the Snappy suite's walker, the footer's codec numbers, sizes
    and offsets, the page index's locations and the filters where the footer says; pyarrow reads the record back. Returns the LZ4
    blocks of the data pages, per column (of the first row group)."""
    assert data[:4] == b"PAR1" and data[-4:] == b"PAR1"
    groups, groups0 = footer_chunks(data), footer_chunks(plain)
    assert len(groups) == len(groups0)
    want = codecs_of(record, compression)
    md, md0 = pq.ParquetFile(io.BytesIO(data)).metadata, pq.ParquetFile(io.BytesIO(plain)).metadata
    assert md.num_rows == record.num_rows == md0.num_rows
    lz, lz_sizes, lz_bodies, sn, sn_sizes, sn_bodies, per_column, at = [], [], [], [], [], [], [], 4
    for gi, (group, group0) in enumerate(zip(groups, groups0)):
        assert [c["name"] for c in group] == [c["name"] for c in group0] == record.schema.names
        for j, (c, c0) in enumerate(zip(group, group0)):
            name = c["name"]
            assert c["codec"] == want[j] and c0["codec"] == 0, (name, c["codec"])
            pages, start = chunk_pages(data, c)
            pages0, _ = chunk_pages(plain, c0)
            assert start == at, (name, "chunks follow each other by their compressed sizes")
            at += c["total_compressed_size"]
            assert len(pages) == len(pages0) and [p[0] for p in pages] == [p[0] for p in pages0], name
            assert c["total_compressed_size"] == sum(p[3] + len(p[2]) for p in pages), name
            assert c["total_uncompressed_size"] == sum(p[3] + p[1] for p in pages), name
            assert (c["dictionary_page_offset"] is None) == (c0["dictionary_page_offset"] is None) and c["num_values"] == c0["num_values"], name
            assert c["data_page_offset"] == start + (pages[0][3] + len(pages[0][2]) if c["dictionary_page_offset"] is not None else 0), name
            col, col0 = md.row_group(gi).column(j), md0.row_group(gi).column(j)
            assert set(col.encodings) == set(col0.encodings) and col.physical_type == col0.physical_type, name
            assert col.statistics.null_count == col0.statistics.null_count and col.statistics.has_min_max == col0.statistics.has_min_max, name
            assert not col.statistics.has_min_max or (col.statistics.min, col.statistics.max) == (col0.statistics.min, col0.statistics.max), name
            mine = []
            for (kind, raw, stored, _, _), (kind0, raw0, body0, _, _) in zip(pages, pages0):
                assert raw == raw0 == len(body0), name
                if want[j] == 0:
                    assert stored == body0, name
                elif want[j] == LZ4_RAW:
                    walk_sequences(stored, raw)
                    lz.append(stored); lz_sizes.append(raw); lz_bodies.append(body0)
                    if kind == S.DATA_PAGE:
                        mine.append(stored)
                else:
                    S.assert_elements_stay_in_fragments(stored)
                    sn.append(stored); sn_sizes.append(raw); sn_bodies.append(body0)
            if gi == 0:
                per_column.append(mine)
            if c["offset_index"] is not None:  # the PageLocations are the page headers found by walking the chunk
                locations = X.offset_index(data, c["offset_index"])
                walked = [(p[4], p[3] + len(p[2])) for p in pages if p[0] == S.DATA_PAGE]
                assert [(off, size) for off, size, _ in locations] == walked, name
                assert [first for _, _, first in locations] == [first for _, _, first in X.offset_index(plain, c0["offset_index"])], name
            if c["column_index"] is not None:
                assert data[c["column_index"][0]:c["column_index"][0] + c["column_index"][1]] == plain[c0["column_index"][0]:c0["column_index"][0] + c0["column_index"][1]], name
            assert (c["bloom_filter_offset"] is None) == (c0["bloom_filter_offset"] is None), name
            if c["bloom_filter_offset"] is not None:  # filters are never compressed: the same bytes, where this footer says
                assert c["bloom_filter_length"] == c0["bloom_filter_length"] and c["bloom_filter_offset"] >= at, name
                assert data[c["bloom_filter_offset"]:c["bloom_filter_offset"] + c["bloom_filter_length"]] == plain[c0["bloom_filter_offset"]:c0["bloom_filter_offset"] + c0["bloom_filter_length"]], name
    regions = sorted((c[k][0], c[k][1]) for g in groups for c in g for k in ("offset_index", "column_index") if c[k] is not None)
    regions = sorted(regions + [(c["bloom_filter_offset"], c["bloom_filter_length"]) for g in groups for c in g if c["bloom_filter_offset"] is not None])
    for off, n in regions:  # the body, then filters and index regions one after the other, then the footer
        assert off == at, "a filter or index region does not follow what is in front of it"
        at += n
    assert at == len(data) - 8 - int.from_bytes(data[-8:-4], "little"), "the footer follows"
    for block, raw, body in zip(lz, lz_sizes, lz_bodies):
        assert inflate(block, raw) == body
    for block, raw, body in zip(sn, sn_sizes, sn_bodies):
        assert (pa.decompress(block, decompressed_size=raw, codec="snappy").to_pybytes() if raw else b"") == body
    for blocks, sizes, bodies, decode in ((lz, lz_sizes, lz_bodies, pp.lz4_decode_pages), (sn, sn_sizes, sn_bodies, pp.snappy_decode_pages)):
        if blocks:
            got, status, _ = decode(blocks, sizes, device=device)
            assert list(status) == [0] * len(blocks), status
            assert [bytes(g) for g in got] == bodies
    if read_back:
        table = pq.ParquetFile(io.BytesIO(data)).read()
        cases.assert_same_record(pa.RecordBatch.from_arrays([c.combine_chunks() for c in table.columns], names=table.schema.names), record)
    return per_column


# ---- bodies of chosen lengths and the rule's shapes ---------------------------------------------------------------------------------------------------
BODY_LENGTHS = list(range(1, 14)) + [F - 1, F, F + 1, F + 4, F + 5, F + 11, F + 12, F + 13, 2 * F - 1, 2 * F, 2 * F + 1]
BODY_KINDS = ["noise", "run", "period5"]


def body_bits(n_bytes: int, kind: str) -> "tuple[pa.RecordBatch, int]":
    """bits_record's shape — a required bool column whose one data page has a body of exactly n_bytes bytes — holding noise, one run,
    or data of period 5."""
    if kind == "noise":
        return bits_record(n_bytes)
    body = bytes(n_bytes) if kind == "run" else (b"\x11\x5a\xc3\x07\xee" * (n_bytes // 5 + 1))[:n_bytes]
    bits = np.unpackbits(np.frombuffer(body, dtype=np.uint8), bitorder="little").astype(bool)
    return pa.RecordBatch.from_arrays([pa.array(bits)], names=["bits"]), -(-len(bits) // 64) * 64


def pad8(payload: bytes, seed: int) -> bytes:
    """… to a multiple of 8 bytes and at least 16 more of noise, so that what stands in front is far from the block's end conditions."""
    return payload + noise(seed, 16 + (-len(payload)) % 8)


def repeat_shape(literal: int, length: int) -> "tuple[bytes, list]":
    """`literal` bytes of noise, their last 8 again and again for `length` bytes, then other noise: a literal run of `literal`, a match
    of exactly `length` from 8 back. Returns the payload and its matches."""
    a = noise(literal, literal)
    again = bytes(a[literal - 8 + i % 8] for i in range(length))
    tail = bytearray(pad8(a + again, literal + 1000)[literal + length:])
    tail[0] = (a[literal - 8 + length % 8] + 1) & 0xFF  # the match ends where it is meant to
    return a + again + bytes(tail), [(literal, length, 8)]


def joined_run_shape() -> bytes:
    """A fragment of zeros, a fragment of noise, a fragment of zeros: the noise fragment has no match, so its bytes join the tail of the
    first fragment and the head of the third into one run of more than 32 768 literals, its extension more than 128 bytes long."""
    return bytes(F) + noise(21, F) + bytes(F)


FAR = b"\x91\x5e\x37\xc2"


def _colliding():
    """Two different 4-byte values under one hash of the rule (fdb_pqs_hash: × 0x1e35a7bd, the top 12 bits)."""
    h = lambda x: ((x * 0x1E35A7BD) & 0xFFFFFFFF) >> 20
    x = 0x11223344
    y = next(v for v in range(0x55667788, 0x55667788 + 1_000_000) if h(v) == h(x))
    return x.to_bytes(4, "little"), y.to_bytes(4, "little")


COLLIDING = _colliding()


def rule_shapes() -> "dict[str, bytes]":
    """name → page body (a multiple of 8 bytes), the shapes of the rule both suites write."""
    out = {}
    for literal in (14, 15, 16, 269, 270, 271):
        out["literals_%d" % literal] = repeat_shape(literal, 40)[0]
    for length in (18, 19, 20, 273, 274, 275):
        out["match_%d" % length] = repeat_shape(100, length)[0]
    a = noise(6, F - 48)
    out["tail_and_head"] = a + a[-200:-160] + noise(7, 32) + bytes(48) + noise(8, 16)   # 8 literals behind fragment 0's match + 25 in front of fragment 1's
    out["joined_run"] = joined_run_shape()
    a = noise(6, F - 40)
    out["match_to_fragment_end"] = a + a[-200:-160] + noise(7, 64)
    a = noise(8, F - 24)
    out["match_cut_by_fragment_end"] = a + a[-200:-120] + noise(9, 24)
    out["furthest_offset"] = FAR + bytes(F - 8) + FAR + noise(10, 24)                 # the fragment's last 4 bytes are its first 4: F − 4 back
    out["hash_collision"] = COLLIDING[0] + noise(10, 196) + COLLIDING[1] + noise(11, 60)
    out["no_match_anywhere"] = noise(5, 2 * F + 8)
    out["one_run_over_eight_fragments"] = bytes(8 * F)
    for period in range(1, 17):
        unit = bytes(range(200, 200 + period))
        out["period_%d" % period] = pad8(noise(12, 100) + (unit * 300)[:300], 13)
    return out


# ---- the nine ratio corpora of tests/test_parquet_snappy_cpu.py, restated ------------------------------------------------------------------------------
N = 32768
CORPORA = ["constant", "cumsum", "timestamps", "standard_normal", "integers_0_100", "integers_0_100_f64", "fifty_floats", "dictionary_random", "dictionary_runs_of_64"]


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
