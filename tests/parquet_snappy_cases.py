"""What tests/test_parquet_snappy_cpu.py (the host walk, fdb_selftest_parquet_write_compressed) and tests/test_gpu_parquet_snappy.py (the
compress kernel, fdb_batch_to_parquet_compressed) share: a reader of the writer's pages, a walker of Snappy elements written from the
format's description (it shares nothing with the library), bodies that put a chosen byte string into one page, and what "the compressed
file is right" means — every page inflates, by pyarrow's codec and by the library's own decoder, to the page body of the uncompressed file
of the same record; no copy leaves its fragment; the footer says what the pages are; pyarrow reads the record back."""
import io
import os
import re

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq

from tests import parquet_write_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRAGMENT = int(re.search(r"^#define FDB_PQS_FRAGMENT (\d+)", open(os.path.join(ROOT, "frostdb_amd", "csrc", "fdb_pqsnappy.h")).read(), flags=re.M).group(1))
RING_REACH = 65_472  # the furthest back a copy may reach in the project's device decoder (fdb_kernels.h: FDB_PAGE_RING_REACH)
T_TRUE, T_FALSE, T_I32, T_I64, T_STRUCT = 1, 2, 5, 6, 12
DATA_PAGE, DICTIONARY_PAGE = 0, 2


def bound(u: int) -> int:
    return 32 + u + u // 6


# ---- page headers (thrift compact protocol), as far as the writer's pages need it -------------------------------------------------------------
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
        if ty in (T_I32, T_I64):
            z, at = _varint(data, at)
            out[fid] = (z >> 1) ^ -(z & 1)
        elif ty == T_STRUCT:
            out[fid], at = _struct(data, at)
        elif ty in (T_TRUE, T_FALSE):
            out[fid] = ty == T_TRUE
        else:
            raise AssertionError("a field type no page header of the writer holds: %d" % ty)


def chunk_pages(data: bytes, col):
    """[(page type, uncompressed size, stored bytes, header bytes)] of every page of the chunk, the dictionary page first, and the chunk's
    first byte."""
    start = col.dictionary_page_offset if col.has_dictionary_page else col.data_page_offset
    at, end = start, start + col.total_compressed_size
    pages = []
    while at < end:
        h, body_at = _struct(data, at)
        pages.append((h[1], h[2], data[body_at:body_at + h[3]], body_at - at))
        at = body_at + h[3]
    assert at == end
    return pages, start


# ---- Snappy elements, from the format's description -----------------------------------------------------------------------------------------
def walk_elements(block: bytes):
    """(announced length, [(kind, output position, length, offset)]) of a Snappy block; kind 0 literal, 1 / 2 a copy with a 1- / 2-byte offset."""
    u, at = _varint(block, 0)
    out, elems = 0, []
    while at < len(block):
        tag = block[at]
        kind = tag & 3
        if kind == 0:
            n = tag >> 2
            if n < 60:
                n, at = n + 1, at + 1
            elif n == 60:
                n, at = block[at + 1] + 1, at + 2
            elif n == 61:
                n, at = int.from_bytes(block[at + 1:at + 3], "little") + 1, at + 3
            else:
                raise AssertionError("a literal longer than 65 536 bytes")
            assert at + n <= len(block)
            elems.append((0, out, n, 0))
            at += n
        elif kind == 1:
            n, off = 4 + ((tag >> 2) & 7), ((tag >> 5) << 8) | block[at + 1]
            elems.append((1, out, n, off))
            at += 2
        elif kind == 2:
            n, off = (tag >> 2) + 1, int.from_bytes(block[at + 1:at + 3], "little")
            elems.append((2, out, n, off))
            at += 3
        else:
            raise AssertionError("a copy with a 4-byte offset")
        out += n
    assert at == len(block) and out == u, (at, len(block), out, u)
    return u, elems


def assert_elements_stay_in_fragments(block: bytes):
    u, elems = walk_elements(block)
    for kind, pos, n, off in elems:
        assert pos // FRAGMENT == (pos + n - 1) // FRAGMENT, "an element crosses a multiple of FDB_PQS_FRAGMENT: at %d, %d bytes" % (pos, n)
        if kind != 0:
            assert 1 <= off <= pos - pos // FRAGMENT * FRAGMENT, "a copy at %d reaches %d back, before its fragment's first byte" % (pos, off)
            assert off <= RING_REACH and n >= 4
            assert kind == (1 if n <= 11 and off < 2048 else 2), (kind, n, off)
    assert len(block) <= bound(u), (len(block), u)
    return elems


def merged(elems):
    """Neighbouring copy elements of one offset put together again: [(is copy, position, length, offset)]."""
    out = []
    for kind, pos, n, off in elems:
        if kind != 0 and out and out[-1][0] and out[-1][3] == off and out[-1][1] + out[-1][2] == pos:
            out[-1] = (True, out[-1][1], out[-1][2] + n, off)
        else:
            out.append((kind != 0, pos, n, off))
    return out


# ---- the file --------------------------------------------------------------------------------------------------------------------------------
def codecs_of(record, compression):
    names = record.schema.names
    if compression is None:
        return [False] * len(names)
    if isinstance(compression, str):
        return [compression == "snappy"] * len(names)
    if isinstance(compression, dict):
        return [compression.get(n) == "snappy" for n in names]
    return [c == "snappy" for c in compression]


def assert_compressed_file(pp, record: pa.RecordBatch, data: bytes, plain: bytes, compression, device: int = -1):
    """`data` (written with `compression`) against `plain` (the same record and options without): page for page the same bodies under
    both decoders, elements inside their fragments, the footer's codec and sizes, everything else in the footer as in `plain`; pyarrow
    reads the record back. Returns the compressed blocks of the data pages, per column."""
    assert data[:4] == b"PAR1" and data[-4:] == b"PAR1"
    pf, pf0 = pq.ParquetFile(io.BytesIO(data)), pq.ParquetFile(io.BytesIO(plain))
    md, md0 = pf.metadata, pf0.metadata
    assert md.num_rows == record.num_rows and md.num_row_groups == 1 and md.num_columns == record.num_columns
    rg, rg0 = md.row_group(0), md0.row_group(0)
    want = codecs_of(record, compression)
    blocks, sizes, bodies, per_column, at = [], [], [], [], 4
    for j, name in enumerate(record.schema.names):
        col, col0 = rg.column(j), rg0.column(j)
        pages, start = chunk_pages(data, col)
        pages0, _ = chunk_pages(plain, col0)
        assert start == at, (name, "chunks follow each other by their compressed sizes")
        at += col.total_compressed_size
        assert col.compression == ("SNAPPY" if want[j] else "UNCOMPRESSED"), name
        assert len(pages) == len(pages0) and [p[0] for p in pages] == [p[0] for p in pages0], name
        assert col.total_compressed_size == sum(p[3] + len(p[2]) for p in pages), name
        assert col.total_uncompressed_size == sum(p[3] + p[1] for p in pages), name
        assert col.has_dictionary_page == col0.has_dictionary_page and (not col.has_dictionary_page or col.dictionary_page_offset == start), name
        assert col.data_page_offset == start + (pages[0][3] + len(pages[0][2]) if col.has_dictionary_page else 0), name
        assert set(col.encodings) == set(col0.encodings) and col.physical_type == col0.physical_type and col.num_values == col0.num_values, name
        assert col.statistics.null_count == col0.statistics.null_count == record.column(j).null_count and not col.statistics.has_min_max, name
        assert str(pf.schema.column(j).logical_type) == str(pf0.schema.column(j).logical_type), name
        assert pf.schema.column(j).max_definition_level == pf0.schema.column(j).max_definition_level, name
        mine = []
        for (kind, raw, stored, _), (kind0, raw0, body0, _) in zip(pages, pages0):
            assert raw == raw0 == len(body0), name
            if not want[j]:
                assert stored == body0, name
                continue
            assert_elements_stay_in_fragments(stored)
            blocks.append(stored); sizes.append(raw); bodies.append(body0)
            if kind == DATA_PAGE:
                mine.append(stored)
        per_column.append(mine)
    assert at == len(data) - 8 - int.from_bytes(data[-8:-4], "little"), "the footer follows the last chunk"
    for block, raw, body in zip(blocks, sizes, bodies):
        assert (pa.decompress(block, decompressed_size=raw, codec="snappy").to_pybytes() if raw else b"") == body
    if blocks:
        got, status, _ = pp.snappy_decode_pages(blocks, sizes, device=device)
        assert list(status) == [0] * len(blocks), status
        assert [bytes(g) for g in got] == bodies
    table = pf.read()
    cases.assert_same_record(pa.RecordBatch.from_arrays([c.combine_chunks() for c in table.columns], names=table.schema.names), record)
    return per_column


def bytes_record(payload: bytes) -> "tuple[pa.RecordBatch, int]":
    """A record whose one required int64 column's single data page has exactly `payload` (a multiple of 8 bytes) as its body, and its page_rows."""
    assert len(payload) % 8 == 0 and payload
    rows = len(payload) // 8
    return pa.RecordBatch.from_arrays([pa.array(np.frombuffer(payload, dtype=np.int64))], names=["bytes"]), -(-rows // 64) * 64


def bits_record(n_bytes: int, seed: int = 0) -> "tuple[pa.RecordBatch, int]":
    """A required bool column of 8 × n_bytes random rows: one data page with a body of exactly n_bytes bytes."""
    rows = 8 * n_bytes
    return pa.RecordBatch.from_arrays([pa.array(np.random.default_rng(seed + n_bytes).random(rows) < 0.5)], names=["bits"]), -(-rows // 64) * 64


def noise(seed: int, n: int) -> bytes:
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()
