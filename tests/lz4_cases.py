"""LZ4 blocks for the decoders' tests (tests/test_lz4_cpu.py: the built-in host decoder; tests/test_gpu_lz4.py: lz4_decode_kernel):
payloads that pyarrow's lz4_raw codec compresses, hand-made streams that no compressor emits but the format allows, damaged pages —
and what the Parquet tests need to know about a file: the codec its footer names, the pages of a column chunk."""
import io

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq

RING_REACH = 65_472  # the furthest back a match may reach on the device (fdb_kernels.h: FDB_PAGE_RING_REACH); LZ4 allows 65 535


def payloads():
    """The families of tests/snappy_cases.py payloads, with a match 60 000 bytes back (inside LZ4's 64 KiB window)."""
    rng = np.random.default_rng(11)
    out = [b"", b"x", b"ab" * 3, bytes(range(60)), bytes(range(61)), bytes(rng.integers(0, 256, 59, dtype=np.uint8)), bytes(rng.integers(0, 256, 300, dtype=np.uint8)),
           bytes(rng.integers(0, 256, 70_000, dtype=np.uint8)),             # incompressible: one sequence, 274 extension bytes
           bytes(rng.integers(0, 256, 1 << 20, dtype=np.uint8)),            # 1 MiB of noise (a DOUBLE page of random values looks like this)
           b"\x00" * 100_000, b"\x07" * 17, b"abc" * 50_000, b"0123456" * 9_999, bytes(range(256)) * 300,  # patterns of period 1, 3, 7, 256
           np.arange(200_000, dtype=np.int64).tobytes(),                     # a timestamp-like column: int64 ramps
           (1_700_000_000_000 + 15_000 * (np.arange(131_072) // 7)).astype(np.int64).tobytes(),
           rng.integers(0, 6, 500_000).astype(np.uint32).tobytes(),         # dictionary indices: short matches, short literals
           b" ".join(b"/api/v1/p%04d" % rng.integers(0, 1000) for _ in range(40_000))]
    big = bytearray(rng.integers(0, 256, 300_000, dtype=np.uint8).tobytes())
    big[200_000:203_000] = big[140_000:143_000]  # a match 60 000 bytes back
    out.append(bytes(big))
    return out


def _ext(v: int) -> bytes:
    """a length's extension: bytes that add up to v, up to and including the first one != 255 (v = 255 k: k bytes of 0xFF and a 0)"""
    return b"\xff" * (v // 255) + bytes([v % 255])


def seq(lits: bytes, match_len=None, off=None) -> bytes:
    """One sequence: token, literal length extension, literals[, offset, match length extension]."""
    ll, ml = len(lits), 0 if match_len is None else match_len - 4
    assert match_len is None or (match_len >= 4 and 0 <= off <= 0xFFFF)
    out = bytes([(min(ll, 15) << 4) | min(ml, 15)]) + (_ext(ll - 15) if ll >= 15 else b"") + lits
    if match_len is not None:
        out += off.to_bytes(2, "little") + (_ext(ml - 15) if ml >= 15 else b"")
    return out


def apply(parts) -> bytes:
    """What a list of (literals, match_len or None, offset) decodes to, byte by byte (the format's definition)."""
    out = bytearray()
    for lits, ml, off in parts:
        out += lits
        if ml is not None:
            assert 0 < off <= len(out)
            for _ in range(ml):
                out.append(out[-off])
    return bytes(out)


def hand_made():
    """[(name, stream, plain, far)] — `far`: some match reaches further back than the device's ring keeps (the host decodes it, the
    device answers 6). Every stream ends in ≥ 12 literals, so that LZ4_decompress_safe (which wants the last match to begin ≥ 12 bytes
    before the end, and 5 literals behind it) takes it too: `check_hand_made` says so."""
    rng = np.random.default_rng(3)
    noise = lambda n: bytes(rng.integers(0, 256, n, dtype=np.uint8))  # noqa: E731
    tail = bytes(range(100, 116))
    cases = []

    def add(name, parts, far=False):
        cases.append((name, b"".join(seq(*p) for p in parts), apply(parts), far))
    # literal and match lengths that end exactly on a 255 boundary (the last extension byte is 0), and the neighbours of the first boundary
    for ll in (14, 15, 16, 15 + 255, 15 + 510, 15 + 254, 15 + 256):
        add(f"literal_{ll}", [(noise(ll), 8, 3), (tail, None, None)])
    for ml in (4, 18, 19, 20, 19 + 255, 19 + 510, 19 + 254, 19 + 256, 19 + 255 * 64, 19 + 255 * 65):
        add(f"match_{ml}", [(noise(40), ml, 33), (tail, None, None)])
    add("both_on_a_boundary", [(noise(15 + 255), 19 + 255, 15 + 255), (noise(15), 19, 15), (tail, None, None)])
    # offset 1 … 9 with matches longer than 64 (a pattern shorter than the 64 bytes a wave copies at a time)
    for off in range(1, 10):
        add(f"pattern_{off}", [(bytes(range(1, 10)), 64, off), (b"", 65, off), (b"", 200, off), (b"z", 11, off), (b"", 4, off), (tail, None, None)])
    for off in (31, 32, 33, 63, 64, 65, 127):
        add(f"pattern_{off}", [(noise(130), 64 * 5 + 7, off), (tail, None, None)])
    # a match whose source ends exactly where its destination starts
    for n in (4, 64, 100, 1000, 20_000):
        add(f"adjacent_{n}", [(noise(n), n, n), (tail, None, None)])
    # an empty literal in the last sequence's place is not a thing, but empty literals between matches are
    add("matches_back_to_back", [(noise(70), 5, 70), (b"", 70, 5), (b"", 4, 1), (tail, None, None)])
    # the furthest the device's ring reaches, multi-chunk, after more than a ring's worth of output …
    add("offset_ring_reach", [(noise(70_000), 200, RING_REACH), (noise(3_000), 300, RING_REACH), (tail, None, None)])
    # … and what LZ4 allows beyond it
    add("offset_65535", [(noise(65_535), 100, 65_535), (tail, None, None)], far=True)
    add("offset_ring_reach_plus_1", [(noise(70_000), 100, RING_REACH + 1), (tail, None, None)], far=True)
    return cases


def max_offset(stream: bytes) -> int:
    """The largest match offset of a well-formed block (the token walk of the format's definition): a page with one above RING_REACH
    is the host's, and the device's decoder says 6 to it."""
    ip, far, n = 0, 0, len(stream)
    while ip < n:
        token = stream[ip]; ip += 1
        ll, ml = token >> 4, token & 15
        if ll == 15:
            while True:
                b = stream[ip]; ip += 1; ll += b
                if b != 255:
                    break
        ip += ll
        if ip >= n:
            break
        far = max(far, int.from_bytes(stream[ip:ip + 2], "little")); ip += 2
        if ml == 15:
            while stream[ip] == 255:
                ip += 1
            ip += 1
    return far


def check_hand_made(cases):
    """The hand-made streams are LZ4: pyarrow's codec (liblz4) inflates them to the same bytes."""
    codec = pa.Codec("lz4_raw")
    for name, stream, plain, _ in cases:
        assert codec.decompress(stream, decompressed_size=len(plain), asbytes=True) == plain, name


def damaged():
    """[(name, stream, announced size, device status codes that name the damage)] — every one refused; the good page they sit between is
    `good()`."""
    rng = np.random.default_rng(5)
    lits = bytes(rng.integers(0, 256, 1000, dtype=np.uint8))
    tail = bytes(range(16))
    c, plain = good()
    ok = seq(lits, 40, 1000) + seq(tail)  # 1056 bytes
    return [("truncated_compressor_output", c[: len(c) // 2], len(plain), (2, 5)),
            ("truncated_in_literals", seq(lits)[:500], 1000, (2,)),
            ("truncated_in_length", bytes([0xF0]) + b"\xff" * 3, 1000, (2,)),
            ("truncated_in_offset", seq(lits, 8, 5)[:-1], 1008, (2,)),
            ("truncated_in_match_length", seq(lits, 19 + 255, 5)[:-1], 1000 + 274, (2,)),
            ("offset_0", seq(lits, 40, 0) + seq(tail), 1056, (4,)),
            ("offset_before_the_first_byte", seq(lits, 40, 1001) + seq(tail), 1056, (4,)),
            ("offset_before_the_first_byte_at_once", seq(b"", 8, 1) + seq(tail), 24, (4,)),
            ("literals_longer_than_announced", ok, 900, (3,)),
            ("match_longer_than_announced", ok, 1020, (3,)),
            ("output_shorter_than_announced", ok, 1100, (5,)),
            ("nothing_for_something", b"", 10, (5,))]


def good():
    plain = np.arange(50_000, dtype=np.int64).tobytes()
    return pa.Codec("lz4_raw").compress(plain, asbytes=True), plain


# ---- Parquet files ---------------------------------------------------------------------------------------------------------------
class _Thrift:
    """Thrift's compact protocol, as much as it takes to find a field in a Parquet footer or page header."""
    def __init__(self, b, p=0):
        self.b, self.p = b, p

    def varint(self):
        v = s = 0
        while True:
            c = self.b[self.p]; self.p += 1
            v |= (c & 0x7F) << s; s += 7
            if not c & 0x80:
                return v

    def zigzag(self):
        v = self.varint()
        return (v >> 1) ^ -(v & 1)

    def fields(self):
        """(field id, type) of the struct at p, one after the other; the caller reads or skips each value"""
        fid = 0
        while True:
            h = self.b[self.p]; self.p += 1
            if h == 0:
                return
            fid = fid + (h >> 4) if h >> 4 else self.zigzag()
            yield fid, h & 15

    def list_header(self):
        h = self.b[self.p]; self.p += 1
        return (h >> 4) if h >> 4 != 15 else self.varint(), h & 15

    def skip(self, t, in_list=False):
        if t in (1, 2):
            self.p += 1 if in_list else 0
        elif t == 3:
            self.p += 1
        elif t in (4, 5, 6):
            self.varint()
        elif t == 7:
            self.p += 8
        elif t == 8:
            n = self.varint()
            self.p += n
        elif t in (9, 10):
            n, et = self.list_header()
            for _ in range(n):
                self.skip(et, True)
        elif t == 12:
            for _, ft in self.fields():
                self.skip(ft)
        else:
            raise ValueError(f"thrift type {t}")


def footer_codecs(data: bytes):
    """CompressionCodec of every column chunk, as the file's footer has it (FileMetaData.row_groups[].columns[].meta_data.codec): pyarrow's
    metadata API says "LZ4" for both LZ4 (5, Hadoop-framed, deprecated) and LZ4_RAW (7)."""
    assert data[-4:] == b"PAR1"
    n = int.from_bytes(data[-8:-4], "little")
    t = _Thrift(data[len(data) - 8 - n: len(data) - 8])
    out = []
    for fid, ft in t.fields():                      # FileMetaData
        if fid != 4:
            t.skip(ft); continue
        n_rg, _ = t.list_header()
        for _ in range(n_rg):
            for fid2, ft2 in t.fields():            # RowGroup
                if fid2 != 1:
                    t.skip(ft2); continue
                n_col, _ = t.list_header()
                for _ in range(n_col):
                    for fid3, ft3 in t.fields():    # ColumnChunk
                        if fid3 != 3:
                            t.skip(ft3); continue
                        for fid4, ft4 in t.fields():  # ColumnMetaData
                            if fid4 == 4:
                                out.append(t.zigzag())
                            else:
                                t.skip(ft4)
    return out


def chunk_pages(chunk: bytes):
    """[{type, uncompressed, compressed, encoding, prefix, v2_compressed, num_values}] of a column chunk's pages (PageHeader: 1 type,
    2 uncompressed_page_size, 3 compressed_page_size, 5 DataPageHeader{1 num_values, 2 encoding}, 8 DataPageHeaderV2{1 num_values, 4 encoding,
    5 definition_levels_byte_length, 6 repetition_levels_byte_length, 7 is_compressed})."""
    t = _Thrift(chunk)
    pages = []
    while t.p < len(chunk):
        pg = dict(type=None, uncompressed=0, compressed=0, encoding=None, prefix=0, v2_compressed=True, num_values=0)
        for fid, ft in t.fields():
            if fid == 1:
                pg["type"] = t.zigzag()
            elif fid == 2:
                pg["uncompressed"] = t.zigzag()
            elif fid == 3:
                pg["compressed"] = t.zigzag()
            elif fid == 5:
                for f2, t2 in t.fields():
                    if f2 == 1:
                        pg["num_values"] = t.zigzag()
                    elif f2 == 2:
                        pg["encoding"] = t.zigzag()
                    else:
                        t.skip(t2)
            elif fid == 8:
                for f2, t2 in t.fields():
                    if f2 == 1:
                        pg["num_values"] = t.zigzag()
                    elif f2 == 4:
                        pg["encoding"] = t.zigzag()
                    elif f2 in (5, 6):
                        pg["prefix"] += t.zigzag()
                    elif f2 == 7:
                        pg["v2_compressed"] = t2 == 1
                    else:
                        t.skip(t2)
            else:
                t.skip(ft)
        pg["at"] = t.p
        t.p += pg["compressed"]
        pages.append(pg)
    return pages


def pages_for_the_device(chunk: bytes, physical_type: int) -> list:
    """The uncompressed body sizes of those of a chunk's pages that meet fdb_parquet.cpp's gate for the device's inflate, counted from the page headers: data pages (V1 = 0,
    V2 = 3) of PLAIN (0) INT64 (2) / DOUBLE (5) values, compressed, body ≥ 32 KiB, compressed body ≥ 0.9 × plain body."""
    n = []
    for pg in chunk_pages(chunk):
        comp, plain = pg["compressed"] - pg["prefix"], pg["uncompressed"] - pg["prefix"]
        if pg["type"] in (0, 3) and pg["v2_compressed"] and pg["encoding"] == 0 and physical_type in (2, 5) and plain >= 32 << 10 and comp * 10 >= plain * 9 and plain < 1 << 31:
            n.append(plain)
    return n


def page_header_v1(n_values: int, uncompressed: int, compressed: int) -> bytes:
    """PageHeader{1: DATA_PAGE, 2: uncompressed_page_size, 3: compressed_page_size, 5: DataPageHeader{1: num_values, 2: PLAIN, 3: RLE, 4: RLE}}"""
    def zz(v):
        v = (v << 1) ^ (v >> 31)
        out = bytearray()
        while v >= 0x80:
            out.append((v & 0x7F) | 0x80); v >>= 7
        out.append(v)
        return bytes(out)
    inner = b"\x15" + zz(n_values) + b"\x15" + zz(0) + b"\x15" + zz(3) + b"\x15" + zz(3) + b"\x00"
    return b"\x15" + zz(0) + b"\x15" + zz(uncompressed) + b"\x15" + zz(compressed) + b"\x2c" + inner + b"\x00"


def read_row_group(data: bytes, rg: int):
    return pq.ParquetFile(io.BytesIO(data)).read_row_group(rg)
