"""A test-side Parquet page writer, written from the parquet-format specification (Encodings.md, parquet.thrift) and sharing nothing
with the library: column chunks laid out page by page, run by run and miniblock by miniblock, in the geometries a stock writer never
chooses (pyarrow writes DELTA blocks of 128 / 4, bit-packed runs of at most 64 groups, index widths that follow the dictionary's
size). Every chunk also comes wrapped into a complete one-column file, so that pyarrow's READER — an implementation this builder
knows nothing about — is the judge of what the bytes mean: tests/test_parquet_pages_cpu.py holds the builder to it, and
tests/test_gpu_parquet_pages.py holds the device decoders to the same bytes.

No test lives here. `cases(family)` is the one generator both test modules run; it is seeded and deterministic."""
import functools
from collections import namedtuple

import numpy as np
import pyarrow as pa

BOOLEAN, INT64, DOUBLE, BYTE_ARRAY = 0, 2, 5, 6                                   # parquet.thrift Type
PLAIN, RLE, DELTA_BINARY_PACKED, RLE_DICTIONARY = 0, 3, 5, 8                      # parquet.thrift Encoding
DATA_PAGE, DICTIONARY_PAGE, DATA_PAGE_V2 = 0, 2, 3                                # parquet.thrift PageType
CODECS = {"UNCOMPRESSED": 0, "SNAPPY": 1}                                         # parquet.thrift CompressionCodec
UTF8, UINT_64 = 0, 14                                                             # parquet.thrift ConvertedType
INT64_MIN, INT64_MAX = -2**63, 2**63 - 1
M64 = 2**64 - 1

# ---- thrift compact protocol (thrift/doc/specs/thrift-compact-protocol.md) -------------------------------------------------------
T_TRUE, T_FALSE, T_I32, T_I64, T_BINARY, T_LIST, T_STRUCT = 1, 2, 5, 6, 8, 9, 12


def varint(v: int) -> bytes:
    assert v >= 0
    out = bytearray()
    while v >= 0x80:
        out.append((v & 0x7F) | 0x80)
        v >>= 7
    out.append(v)
    return bytes(out)


def zigzag(v: int) -> bytes:
    assert INT64_MIN <= v <= INT64_MAX
    return varint(((v << 1) ^ (v >> 63)) & M64)


class Struct:
    """One thrift struct in the compact protocol: fields in ascending id order, `end()` gives its bytes with the stop field."""

    def __init__(self):
        self.out, self.last = bytearray(), 0

    def _field(self, fid, ty):
        delta = fid - self.last
        if 0 < delta <= 15:
            self.out.append((delta << 4) | ty)
        else:
            self.out.append(ty)
            self.out += zigzag(fid)
        self.last = fid

    def i32(self, fid, v):
        self._field(fid, T_I32)
        self.out += zigzag(v)
        return self

    def i64(self, fid, v):
        self._field(fid, T_I64)
        self.out += zigzag(v)
        return self

    def boolean(self, fid, v):
        self._field(fid, T_TRUE if v else T_FALSE)
        return self

    def binary(self, fid, b):
        self._field(fid, T_BINARY)
        self.out += varint(len(b)) + b
        return self

    def struct(self, fid, body: bytes):
        self._field(fid, T_STRUCT)
        self.out += body
        return self

    def list_of(self, fid, elem_type, items):
        self._field(fid, T_LIST)
        self.out += bytes([(len(items) << 4) | elem_type]) if len(items) < 15 else bytes([0xF0 | elem_type]) + varint(len(items))
        for it in items:
            self.out += it
        return self

    def end(self) -> bytes:
        return bytes(self.out) + b"\x00"


def page_header(page_type, uncompressed, compressed, n_values, encoding, *, n_nulls=0, def_bytes=0, is_compressed=None) -> bytes:
    """parquet.thrift PageHeader for a DICTIONARY_PAGE, DATA_PAGE or DATA_PAGE_V2 (`is_compressed`: V2 only; None leaves the field out)."""
    h = Struct().i32(1, page_type).i32(2, uncompressed).i32(3, compressed)
    if page_type == DATA_PAGE:
        h.struct(5, Struct().i32(1, n_values).i32(2, encoding).i32(3, RLE).i32(4, RLE).end())
    elif page_type == DICTIONARY_PAGE:
        h.struct(7, Struct().i32(1, n_values).i32(2, encoding).end())
    else:
        assert page_type == DATA_PAGE_V2
        v2 = Struct().i32(1, n_values).i32(2, n_nulls).i32(3, n_values).i32(4, encoding).i32(5, def_bytes).i32(6, 0)
        if is_compressed is not None:
            v2.boolean(7, is_compressed)
        h.struct(8, v2.end())
    return h.end()


# ---- bit packing, the RLE / bit-packed hybrid, DELTA_BINARY_PACKED, PLAIN -------------------------------------------------------
def pack_bits(values, width: int) -> bytes:
    """`values` (a multiple of 8 of them) at `width` bits each, LSB first, back to back."""
    v = np.asarray(values, dtype=np.uint64)
    assert len(v) % 8 == 0 and 0 <= width <= 64
    if width == 0 or len(v) == 0:
        return b""
    shifts = np.arange(width, dtype=np.uint64)[None, :]
    step = 1 << 18  # (slices keep the values × width matrix of single bits small)
    return b"".join(np.packbits(((v[a:a + step, None] >> shifts) & np.uint64(1)).astype(np.uint8).ravel(), bitorder="little").tobytes() for a in range(0, len(v), step))


def hybrid(values, width: int, plan, pad=0) -> bytes:
    """The RLE / bit-packed hybrid of `values` at `width` bits, run by run as `plan` says: ("rle", count) writes the next `count`
    values (all equal) as one repeated run, its value in ⌈width / 8⌉ bytes; ("bp", groups) writes the next groups × 8 values
    bit-packed. Only the LAST run may hold fewer values than it declares (padded with `pad`). `width` is the caller's choice."""
    v = np.asarray(values, dtype=np.uint64)
    assert width == 64 or len(v) == 0 or int(v.max()) < (1 << width), "a value does not fit the declared width"
    out, at = bytearray(), 0
    for k, (kind, count) in enumerate(plan):
        last = k == len(plan) - 1
        if kind == "rle":
            assert count > 0 and at + count <= len(v) and (v[at:at + count] == v[at]).all(), "an RLE run of unequal values"
            out += varint(count << 1) + int(v[at]).to_bytes((width + 7) // 8, "little")
            at += count
        else:
            assert kind == "bp" and count > 0
            take = v[at:at + count * 8]
            assert len(take) == count * 8 or (last and len(take) > (count - 1) * 8), "only the last bit-packed run may be padded"
            out += varint((count << 1) | 1) + pack_bits(np.concatenate([take, np.full(count * 8 - len(take), pad, np.uint64)]), width)
            at += len(take)
    assert at == len(v), "the plan does not cover the values"
    return bytes(out)


def bp_plan(n: int):
    return [("bp", (n + 7) // 8)] if n else []


def fill_plan(rng, plan, n: int, hi: int, rle_value=None):
    """`n` values below `hi` that `plan` can carry: constant inside every RLE run, random inside bit-packed ones."""
    v = rng.integers(0, hi, n).astype(np.uint64)
    at = 0
    for kind, count in plan:
        if kind == "rle":
            v[at:at + count] = v[at] if rle_value is None else rle_value
            at += count
        else:
            at += count * 8
    assert at >= n
    return v


def delta_binary_packed(values, block=128, n_mini=4, min_width=0, junk_tail=False, widths_out=None) -> bytes:
    """DELTA_BINARY_PACKED of int64 `values`: <block size> <miniblocks per block> <count> <first value>, then per block <min delta>
    <one width byte per miniblock> <the miniblocks that hold a value, the last padded to full length>. `min_width` forces every
    written miniblock to at least that width; `junk_tail` leaves nonzero widths in the miniblocks of the last block that hold no
    value (they have no body; a reader must not look at them). Sums and differences wrap."""
    v = np.ascontiguousarray(values, dtype=np.int64)
    assert block % 128 == 0 and block % n_mini == 0 and (block // n_mini) % 32 == 0
    vpm = block // n_mini
    out = bytearray(varint(block) + varint(n_mini) + varint(len(v)) + zigzag(int(v[0]) if len(v) else 0))
    u = v.view(np.uint64)
    deltas = u[1:] - u[:-1]
    for b0 in range(0, len(deltas), block):
        blk = deltas[b0:b0 + block]
        m = int(blk.view(np.int64).min())
        rel = blk - np.uint64(m & M64)
        need = (len(blk) + vpm - 1) // vpm
        widths, bodies = [], []
        for k in range(n_mini):
            if k < need:
                mb = rel[k * vpm:(k + 1) * vpm]
                w = max(int(mb.max()).bit_length(), min_width)
                bodies.append(pack_bits(np.concatenate([mb, np.zeros(vpm - len(mb), np.uint64)]), w))
                widths.append(w)
            else:
                widths.append(5 + 7 * k if junk_tail else 0)
        if widths_out is not None:
            widths_out.extend(widths[:need])
        out += zigzag(m) + bytes(widths) + b"".join(bodies)
    return bytes(out)


def plain(ptype, values) -> bytes:
    if ptype in (INT64, DOUBLE):
        return np.ascontiguousarray(values).view(np.uint64).astype("<u8").tobytes()
    if ptype == BOOLEAN:
        return np.packbits(np.asarray(values, dtype=bool), bitorder="little").tobytes()
    assert ptype == BYTE_ARRAY
    return b"".join(len(s).to_bytes(4, "little") + s for s in values)


# ---- pages, chunks, files -------------------------------------------------------------------------------------------------------
def _squeeze(codec, body: bytes) -> bytes:
    return body if codec == "UNCOMPRESSED" else pa.compress(body, codec=codec.lower(), asbytes=True)


def dictionary_page(ptype, values, codec="UNCOMPRESSED") -> bytes:
    body = plain(ptype, values)
    packed = _squeeze(codec, body)
    return page_header(DICTIONARY_PAGE, len(body), len(packed), len(values), PLAIN) + packed


def data_page(n_rows, encoding, values: bytes, levels=None, level_plan=None, version=1, codec="UNCOMPRESSED", is_compressed=None) -> bytes:
    """One data page of `n_rows` rows whose encoded values are `values`. `levels` (0 / 1 per row) for an optional column, laid out as
    `level_plan` says (default: one bit-packed run); V1 keeps them inside the body behind a 4-byte length, V2 in front of it,
    uncompressed. `is_compressed` is the V2 header's flag: False leaves this page's values uncompressed inside a compressed chunk."""
    lv = b""
    n_nulls = 0
    if levels is not None:
        assert len(levels) == n_rows
        lv = hybrid(levels, 1, level_plan if level_plan is not None else bp_plan(n_rows), pad=1)  # (padding of ones: a reader that counts it is caught)
        n_nulls = int(n_rows - np.count_nonzero(levels))
    if version == 1:
        body = (len(lv).to_bytes(4, "little") + lv if levels is not None else b"") + values
        packed = _squeeze(codec, body)
        return page_header(DATA_PAGE, len(body), len(packed), n_rows, encoding) + packed
    packed = values if is_compressed is False else _squeeze(codec, values)
    return page_header(DATA_PAGE_V2, len(lv) + len(values), len(lv) + len(packed), n_rows, encoding, n_nulls=n_nulls, def_bytes=len(lv),
                       is_compressed=is_compressed) + lv + packed


def chunk_of(name, ptype, optional, flag, pages, codec="UNCOMPRESSED"):
    """The tuple ResidentBatch.from_parquet takes: (name, physical type, max definition level, utf8 / unsigned flag, bytes, codec)."""
    return (name, ptype, 1 if optional else 0, bool(flag), b"".join(pages), codec)


def file_of(chunk, n_rows, dictionary_bytes=0) -> bytes:
    """A complete Parquet file of one row group and one leaf column around `chunk`'s bytes (`dictionary_bytes`: the length of its
    dictionary page, header included, when it starts with one)."""
    name, ptype, optional, flag, body, codec = chunk
    leaf = Struct().i32(1, ptype).i32(3, 1 if optional else 0).binary(4, name.encode())
    if flag:
        leaf.i32(6, UTF8 if ptype == BYTE_ARRAY else UINT_64)
    schema = [Struct().binary(4, b"schema").i32(5, 1).end(), leaf.end()]
    meta = Struct().i32(1, ptype).list_of(2, T_I32, [zigzag(e) for e in (PLAIN, RLE, DELTA_BINARY_PACKED, RLE_DICTIONARY)])
    meta.list_of(3, T_BINARY, [varint(len(name.encode())) + name.encode()]).i32(4, CODECS[codec]).i64(5, n_rows)
    meta.i64(6, len(body)).i64(7, len(body)).i64(9, 4 + dictionary_bytes)
    if dictionary_bytes:
        meta.i64(11, 4)
    column = Struct().i64(2, 4).struct(3, meta.end()).end()
    group = Struct().list_of(1, T_STRUCT, [column]).i64(2, len(body)).i64(3, n_rows).end()
    footer = Struct().i32(1, 1).list_of(2, T_STRUCT, schema).i64(3, n_rows).list_of(4, T_STRUCT, [group]).binary(6, b"tests/parquet_pages.py").end()
    return b"PAR1" + body + footer + len(footer).to_bytes(4, "little") + b"PAR1"


Case = namedtuple("Case", "id chunk file rows expect")  # expect: the pyarrow Array the bytes were built from (values and NULLs)


def _case(cid, name, ptype, optional, flag, pages, expect, dictionary=None, codec="UNCOMPRESSED"):
    chunk = chunk_of(name, ptype, optional, flag, ([dictionary] if dictionary else []) + list(pages), codec)
    return Case(cid, chunk, file_of(chunk, len(expect), len(dictionary) if dictionary else 0), len(expect), expect)


def expect8(ptype, flag, bits, valid=None):
    """The Arrow array of 8-byte values whose uint64 view is `bits` (rows where `valid` is False are NULL)."""
    bits = np.ascontiguousarray(bits, dtype=np.uint64)
    vals = bits.view(np.float64) if ptype == DOUBLE else bits if flag else bits.view(np.int64)
    return pa.array(vals, mask=None if valid is None else ~np.asarray(valid, bool))


def spread(dense, valid):
    """Non-NULL values in rank order → one per row (0 where NULL)."""
    out = np.zeros(len(valid), dtype=np.asarray(dense).dtype)
    out[np.asarray(valid, bool)] = dense
    return out


# doubles that a float compare would let through: NaNs with payloads, −0.0, subnormals (as bit patterns)
SPECIAL_BITS = np.array([0x0000000000000000, 0x8000000000000000, 0x7FF8000000000000, 0x7FF8000000000001, 0xFFF8DEADBEEF0001, 0x7FF0000000000000,
                         0xFFF0000000000000, 0x0000000000000001, 0x800FFFFFFFFFFFFF, 0x3FF8000000000000, 0xC0091EB851EB851F], dtype=np.uint64)


def _rng(*key):
    return np.random.default_rng([20240607, *key])


def _random_u64(rng, n):
    return np.frombuffer(rng.bytes(8 * n), dtype=np.uint64).copy() if n else np.zeros(0, np.uint64)


def _dictionary_bits(rng, ptype, n):
    """`n` distinct 8-byte dictionary entries: the special doubles first for DOUBLE, full-range integers for INT64."""
    bits = np.unique(_random_u64(rng, n + 64))
    rng.shuffle(bits)
    bits = bits[:n].copy()
    if ptype == DOUBLE:
        bits[:min(n, len(SPECIAL_BITS))] = SPECIAL_BITS[:n]
    return bits


# ---- DELTA_BINARY_PACKED families ------------------------------------------------------------------------------------------------
def delta_values_of_width(rng, n, w, block, n_mini):
    """`n` int64 values whose every full miniblock is exactly `w` bits wide: each holds the all-zeros and the all-ones delta, eight
    deltas with the top bit set (one per bit offset modulo 8, for odd `w`) and eight with it clear. Sums wrap."""
    vpm = block // n_mini
    k = n - 1
    rel = _random_u64(rng, k) >> np.uint64(64 - w) if w else np.zeros(k, np.uint64)
    pos = np.arange(k) % vpm
    rel[pos == 0] = 0
    rel[pos == 1] = (1 << w) - 1
    if w:
        top = np.uint64(1 << (w - 1))
        rel[(pos >= 8) & (pos < 16)] |= top
        rel[(pos >= 16) & (pos < 24)] &= ~top
    mins = np.array([int(rng.integers(INT64_MIN, INT64_MAX - ((1 << w) - 1), endpoint=True)) & M64 for _ in range(0, max(k, 1), block)], dtype=np.uint64)
    deltas = mins[np.arange(k) // block] + rel
    first = _random_u64(rng, 1)
    return np.concatenate([first, first + np.cumsum(deltas, dtype=np.uint64)]).view(np.int64)


def _delta_case(cid, values, *, unsigned=False, block=128, n_mini=4, want_width=None, **kw):
    values = np.asarray(values, dtype=np.int64)
    widths = []
    body = delta_binary_packed(values, block, n_mini, widths_out=widths, **kw)
    if want_width is not None:
        assert widths and set(widths) == {want_width}, (cid, widths)
    return _case(cid, "d", INT64, False, unsigned, [data_page(len(values), DELTA_BINARY_PACKED, body)], expect8(INT64, unsigned, values.view(np.uint64)))


GEOMETRIES = ((128, 1), (256, 4), (256, 2), (512, 4), (1024, 32))


def _delta_widths():
    for w in range(65):
        rng = _rng(1, w)
        yield _delta_case(f"delta_widths/w{w}_128x4", delta_values_of_width(rng, 1 + 2 * 128 + 37, w, 128, 4), want_width=w, min_width=w)
    for block, n_mini in GEOMETRIES:
        for w in range(57, 65):
            rng = _rng(2, block, n_mini, w)
            n = 1 + block + (block // n_mini) + 5  # a full block, then one full and one partial miniblock
            yield _delta_case(f"delta_widths/w{w}_{block}x{n_mini}", delta_values_of_width(rng, n, w, block, n_mini), block=block, n_mini=n_mini, want_width=w, min_width=w)
    rng = _rng(3)
    yield _delta_case("delta_widths/w61_unsigned", delta_values_of_width(rng, 300, 61, 128, 4), unsigned=True, want_width=61, min_width=61)
    yield _delta_case("delta_widths/w61_signed", delta_values_of_width(rng, 300, 61, 128, 4), unsigned=False, want_width=61, min_width=61)
    yield _delta_case("delta_widths/forced_w5_over_constant_deltas", np.arange(200, dtype=np.int64) * 3 - 77, want_width=5, min_width=5)


def _mixed_walk(rng, n):
    """Steps of every size: small ones, a few that need 40 or 60 bits, so a page's miniblocks differ in width."""
    steps = rng.integers(-50, 50, n)
    big = rng.random(n) < 0.03
    steps[big] = rng.integers(-2**59, 2**59, int(big.sum()))
    mid = rng.random(n) < 0.05
    steps[mid] = rng.integers(0, 2**40, int(mid.sum()))
    return np.cumsum(steps.astype(np.int64)) + 1_700_000_000_000


def _delta_shapes():
    for n in (1, 2, 33, 129, 1024, 1025, 1026, 2049, 4100):
        yield _delta_case(f"delta_shapes/n{n}", _mixed_walk(_rng(4, n), n))
        yield _delta_case(f"delta_shapes/n{n}_256x2", _mixed_walk(_rng(5, n), n), block=256, n_mini=2)
    rng = _rng(6)
    wrap = _random_u64(rng, 700).view(np.int64)  # full-range values: the differences, and the sums that undo them, wrap
    wrap[0] = INT64_MIN
    yield _delta_case("delta_shapes/first_is_int64_min_and_sums_wrap", wrap)
    v = np.cumsum(rng.integers(0, 1000, 400).astype(np.int64))
    v[200:] += np.int64(INT64_MIN)  # one delta of INT64_MIN (+ a small step, wrapping) …
    v[130] += 5_000_000             # … in a block (deltas 128…255) that also has large positive ones
    widths = []
    delta_binary_packed(v, widths_out=widths)
    u = v.view(np.uint64)
    assert int((u[1:] - u[:-1]).view(np.int64)[128:256].min()) < INT64_MIN + 1000 and 64 in widths
    yield _delta_case("delta_shapes/min_delta_near_int64_min", v)
    exact = np.zeros(300, np.int64)
    exact[150:] = INT64_MIN  # the delta at 149 is exactly INT64_MIN, the others 0: min_delta = INT64_MIN, widths 64
    yield _delta_case("delta_shapes/min_delta_is_int64_min", exact)
    yield _delta_case("delta_shapes/junk_widths_behind_the_last_miniblock", _mixed_walk(rng, 1 + 128 + 40), junk_tail=True)
    yield _delta_case("delta_shapes/junk_widths_512x4", _mixed_walk(rng, 1 + 130), block=512, n_mini=4, junk_tail=True)
    # three pages of 1, 1 500 and 33 values
    parts = [_mixed_walk(rng, n) for n in (1, 1500, 33)]
    pages = [data_page(len(p), DELTA_BINARY_PACKED, delta_binary_packed(p)) for p in parts]
    yield _case("delta_shapes/pages_1_1500_33", "d", INT64, False, False, pages, expect8(INT64, False, np.concatenate(parts).view(np.uint64)))
    # optional, 30 % NULLs, the middle page entirely NULL
    pages, dense, valid = [], [], []
    for k, rows in enumerate((700, 333, 1201)):
        ok = rng.random(rows) >= 0.3 if k != 1 else np.zeros(rows, bool)
        p = _mixed_walk(rng, int(ok.sum()))
        pages.append(data_page(rows, DELTA_BINARY_PACKED, delta_binary_packed(p, block=256, n_mini=4), levels=ok))
        dense.append(p)
        valid.append(ok)
    valid = np.concatenate(valid)
    yield _case("delta_shapes/optional_with_an_all_null_page", "d", INT64, True, False, pages, expect8(INT64, False, spread(np.concatenate(dense), valid).view(np.uint64), valid))
    # more pages than the launch has workgroups (8 192): 8 200 pages of two values each
    two = _random_u64(rng, 2 * 8200).view(np.int64) >> np.int64(3)
    pages = [data_page(2, DELTA_BINARY_PACKED, delta_binary_packed(two[2 * i:2 * i + 2])) for i in range(8200)]
    yield _case("delta_shapes/8200_pages_of_two", "d", INT64, False, False, pages, expect8(INT64, False, two.view(np.uint64)))


# ---- dictionary-encoded families -------------------------------------------------------------------------------------------------
INDEX_PLAN = [("bp", 100), ("rle", 200), ("bp", 3)]  # a 2-byte run header, an RLE run, a padded bit-packed tail
INDEX_PLAN_VALUES = 100 * 8 + 200 + 21


def _index_page(rng, ptype, dictionary, width, optional, version=1, plan=None, n_values=None, null_frac=0.2, codec="UNCOMPRESSED", is_compressed=None):
    """One page of dictionary indices at a DECLARED `width`: (page bytes, values per row, validity or None)."""
    plan = INDEX_PLAN if plan is None else plan
    n_values = INDEX_PLAN_VALUES if n_values is None else n_values
    idx = fill_plan(rng, plan, n_values, len(dictionary), rle_value=len(dictionary) - 1)
    if plan and plan[0][0] == "bp" and n_values >= 2:
        idx[:2] = (0, len(dictionary) - 1)  # the first and the last entry always occur
    body = bytes([width]) + (hybrid(idx, width, plan) if width else varint(n_values << 1))
    valid = None
    if optional:
        valid = np.ones(n_values + int(n_values * null_frac), bool)
        valid[rng.choice(len(valid), len(valid) - n_values, replace=False)] = False
    rows = n_values if valid is None else len(valid)
    page = data_page(rows, RLE_DICTIONARY, body, levels=valid, version=version, codec=codec, is_compressed=is_compressed)
    vals = [dictionary[int(i)] for i in idx] if ptype == BYTE_ARRAY else np.asarray(dictionary)[idx.astype(np.int64)]
    return page, vals, valid


def _dict8_case(cid, rng, ptype, n_dict, width, optional, flag=False, version=1):
    d = _dictionary_bits(rng, ptype, n_dict)
    page, vals, valid = _index_page(rng, ptype, d, width, optional, version)
    bits = vals if valid is None else spread(vals, valid)
    return _case(cid, "x", ptype, optional, flag, [page], expect8(ptype, flag, bits, valid), dictionary=dictionary_page(ptype, d))


def _dict8_widths():
    for w in range(33):
        n_dict = min(1 << w, 37)
        for k, (ptype, optional) in enumerate(((INT64, False), (DOUBLE, True), (INT64, True), (DOUBLE, False))):
            tag = ("i64", "f64")[ptype == DOUBLE] + ("_opt" if optional else "_req")
            yield _dict8_case(f"dict8_widths/w{w}_{tag}", _rng(10, w, k), ptype, n_dict, w, optional, flag=(ptype == INT64 and w % 2 == 1), version=1 + (w + k) % 2)
    for w in (13, 24, 32):  # above FDB_PQ_DICT_LDS_ENTRIES = 4 096 entries the kernel reads the dictionary from global memory
        for k, (ptype, optional) in enumerate(((INT64, False), (DOUBLE, True))):
            yield _dict8_case(f"dict8_widths/w{w}_4097_entries_{'f64_opt' if optional else 'i64_req'}", _rng(11, w, k), ptype, 4097, w, optional)


def _random_plan(rng, n):
    """Short runs of both kinds with cuts at odd places: RLE runs of 1…9 values between bit-packed runs of 1…3 groups."""
    plan, left = [], n
    while left > 0:
        if rng.random() < 0.5 or left < 8:
            c = int(min(left, rng.integers(1, 10)))
            plan.append(("rle", c))
            left -= c
        else:
            g = int(min(left // 8, rng.integers(1, 4)))
            plan.append(("bp", g))
            left -= g * 8
    return plan


def _dict8_shapes():
    rng = _rng(12)
    for ptype in (INT64, DOUBLE):
        # rows cross page and run boundaries inside one lane's four rows: pages of 1 001 / 1 003 / 1 001 values, optional, odd run cuts
        d = _dictionary_bits(rng, ptype, 23)
        pages, dense, valid = [], [], []
        for n_values in (1001, 1003, 1001):
            page, vals, ok = _index_page(rng, ptype, d, 5, True, plan=_random_plan(rng, n_values), n_values=n_values, null_frac=0.3)
            pages.append(page), dense.append(vals), valid.append(ok)
        valid = np.concatenate(valid)
        tag = "i64" if ptype == INT64 else "f64"
        yield _case(f"dict8_shapes/odd_pages_and_run_cuts_{tag}", "x", ptype, True, False, pages, expect8(ptype, False, spread(np.concatenate(dense), valid), valid),
                    dictionary=dictionary_page(ptype, d))
        # an indexed page, then a PLAIN page (a writer's fallback): the switch falls inside a quad of rows (1 002 = 4 × 250 + 2)
        for optional in (False, True):
            page, vals, ok = _index_page(rng, ptype, d, 7, optional, plan=bp_plan(1002), n_values=1002)
            ok2 = rng.random(1300) < 0.75 if optional else None
            k2 = int(ok2.sum()) if optional else 999
            more = _random_u64(rng, k2) if ptype == INT64 else np.concatenate([SPECIAL_BITS, _random_u64(rng, k2 - len(SPECIAL_BITS))])
            fallback = data_page(1300 if optional else 999, PLAIN, plain(ptype, more), levels=ok2)
            bits = np.concatenate([vals if ok is None else spread(vals, ok), more if ok2 is None else spread(more, ok2)])
            yield _case(f"dict8_shapes/indexed_then_plain_{tag}_{'opt' if optional else 'req'}", "x", ptype, optional, False, [page, fallback],
                        expect8(ptype, False, bits, None if ok is None else np.concatenate([ok, ok2])), dictionary=dictionary_page(ptype, d))
    # the persistent grid (1 024 workgroups × 1 024-row tiles) takes a second tile: one hand-laid page of 2²⁰ + 1 027 rows
    n = 1024 * 1024 + 1027
    d = _dictionary_bits(rng, DOUBLE, 300)
    plan = [("bp", 70_000), ("rle", 400_000), ("bp", (n - 960_000 + 7) // 8)]
    idx = fill_plan(rng, plan, n, 300, rle_value=299)
    page = data_page(n, RLE_DICTIONARY, bytes([9]) + hybrid(idx, 9, plan))
    yield _case("dict8_shapes/second_tile_of_the_persistent_grid", "x", DOUBLE, False, False, [page], expect8(DOUBLE, False, d[idx.astype(np.int64)]), dictionary=dictionary_page(DOUBLE, d))


# ---- BYTE_ARRAY and BOOLEAN --------------------------------------------------------------------------------------------------------
def _strings(n):
    return [(b"v%03d-" % i) + b"\xc3\xa9" * (i % 5) for i in range(n)]


def _bytes_array(values, valid, utf8):
    out = pa.array([v if ok else None for v, ok in zip(values, valid)] if valid is not None else list(values), type=pa.binary())
    return out.cast(pa.string()) if utf8 else out


def _string_widths():
    for w in range(1, 33):
        d = _strings(min(1 << w, 37))
        for optional in (False, True):
            rng = _rng(20, w, int(optional))
            utf8 = w % 2 == 0
            page, vals, valid = _index_page(rng, BYTE_ARRAY, d, w, optional, version=1 + w % 2)
            rows = vals if valid is None else list(spread(np.array(vals, dtype=object), valid))
            yield _case(f"string_widths/w{w}_{'opt' if optional else 'req'}", "s", BYTE_ARRAY, optional, utf8, [page], _bytes_array(rows, valid, utf8),
                        dictionary=dictionary_page(BYTE_ARRAY, d))


# the definition-level plans: (name, [(levels' plan, rows) per page], how the levels are drawn)
def _level_pages(rng, name):
    """[(levels, plan)] per page for the named plan of definition levels."""
    def drawn(plan, n):
        return fill_plan(rng, plan, n, 2).astype(bool), plan
    if name == "bp_125_groups":            # one bit-packed run with a 2-byte header; 997 rows, so its last group is padded
        return [drawn([("bp", 125)], 997)]
    if name == "rle_20000":                # a 3-byte RLE header between two 8-group bit-packed runs
        lv, plan = drawn([("bp", 8), ("rle", 20000), ("bp", 8)], 20128)
        lv[64:20064] = True
        return [(lv, plan)]
    if name == "rle_cuts_31_1_32_33_1":    # runs that end one before, at and one after a 32-row word
        return [(np.repeat([True, False, True, False, True], [31, 1, 32, 33, 1]), [("rle", c) for c in (31, 1, 32, 33, 1)])]
    if name == "alternating_rle":          # 70 one-row runs across three words
        return [(np.arange(70) % 2 == 0, [("rle", 1)] * 70)]
    if name == "one_row_pages":            # pages of one row: a value, a NULL, a value
        return [(np.array([ok]), [("rle", 1)]) for ok in (True, False, True)]
    if name == "all_null_page_between":    # the pages around it share their neighbours' ranks
        return [drawn(_random_plan(rng, 45), 45), (np.zeros(50, bool), [("rle", 50)]), drawn(_random_plan(rng, 77), 77)]
    assert name == "all_valid_one_rle"
    return [(np.ones(100, bool), [("rle", 100)])]


LEVEL_PLANS = ("bp_125_groups", "rle_20000", "rle_cuts_31_1_32_33_1", "alternating_rle", "one_row_pages", "all_null_page_between", "all_valid_one_rle")


def _levels():
    for name in LEVEL_PLANS:
        for version in (1, 2):
            for kind in ("plain_i64", "dict_f64", "delta_i64"):
                rng = _rng(30, LEVEL_PLANS.index(name), version, len(kind))
                ptype = DOUBLE if kind == "dict_f64" else INT64
                d = _dictionary_bits(rng, DOUBLE, 11)
                pages, dense, valid = [], [], []
                for lv, plan in _level_pages(rng, name):
                    k = int(lv.sum())
                    if kind == "plain_i64":
                        vals = _random_u64(rng, k)
                        enc, body = PLAIN, plain(INT64, vals)
                    elif kind == "dict_f64":
                        idx = rng.integers(0, len(d), k).astype(np.uint64)
                        vals = d[idx.astype(np.int64)]
                        enc, body = RLE_DICTIONARY, bytes([4]) + hybrid(idx, 4, bp_plan(k))
                    else:
                        vals = _mixed_walk(rng, k).view(np.uint64)
                        enc, body = DELTA_BINARY_PACKED, delta_binary_packed(vals.view(np.int64))
                    pages.append(data_page(len(lv), enc, body, levels=lv, level_plan=plan, version=version))
                    dense.append(vals), valid.append(lv)
                valid = np.concatenate(valid)
                yield _case(f"levels/{name}_v{version}_{kind}", "x", ptype, True, False, pages, expect8(ptype, False, spread(np.concatenate(dense), valid), valid),
                            dictionary=dictionary_page(DOUBLE, d) if kind == "dict_f64" else None)


def _booleans():
    for name in LEVEL_PLANS:  # optional: BOOLEAN PLAIN in V1 pages, BOOLEAN RLE in V2 pages, under every plan of definition levels
        for version in (1, 2):
            rng = _rng(40, LEVEL_PLANS.index(name), version)
            pages, dense, valid = [], [], []
            for lv, plan in _level_pages(rng, name):
                k = int(lv.sum())
                vplan = _random_plan(rng, k)
                vals = fill_plan(rng, vplan, k, 2).astype(bool)
                if version == 1:
                    enc, body = PLAIN, plain(BOOLEAN, vals)
                else:
                    runs = hybrid(vals, 1, vplan)
                    enc, body = RLE, len(runs).to_bytes(4, "little") + runs
                pages.append(data_page(len(lv), enc, body, levels=lv, level_plan=plan, version=version))
                dense.append(vals), valid.append(lv)
            valid = np.concatenate(valid)
            yield _case(f"booleans/{name}_v{version}", "b", BOOLEAN, True, False, pages, pa.array(spread(np.concatenate(dense), valid), mask=~valid))
    for name in LEVEL_PLANS:  # required: the same plans drive the VALUES' runs (RLE) or just the page sizes (PLAIN)
        for version in (1, 2):
            rng = _rng(41, LEVEL_PLANS.index(name), version)
            pages, vals = [], []
            for lv, plan in _level_pages(rng, name):
                if version == 1:
                    enc, body = PLAIN, plain(BOOLEAN, lv)
                else:
                    runs = hybrid(lv, 1, plan)
                    enc, body = RLE, len(runs).to_bytes(4, "little") + runs
                pages.append(data_page(len(lv), enc, body, version=version))
                vals.append(lv)
            yield _case(f"booleans/required_{name}_v{version}", "b", BOOLEAN, False, False, pages, pa.array(np.concatenate(vals)))


# ---- V2 pages flagged uncompressed inside a SNAPPY chunk ---------------------------------------------------------------------------
def _v2_uncompressed():
    for optional in (False, True):
        tag = "opt" if optional else "req"
        rng = _rng(50, int(optional))
        pages, dense, valid = [], [], []
        for k, flag in enumerate((True, False, True)):  # PLAIN DOUBLE: the middle page's values are stored as they are
            ok = rng.random(900 + k) >= 0.25 if optional else np.ones(900 + k, bool)
            vals = np.concatenate([SPECIAL_BITS, np.repeat(_random_u64(rng, 40), 30)])[:int(ok.sum())]
            pages.append(data_page(len(ok), PLAIN, plain(DOUBLE, vals), levels=ok if optional else None, version=2, codec="SNAPPY", is_compressed=flag))
            dense.append(vals), valid.append(ok)
        valid = np.concatenate(valid)
        yield _case(f"v2_uncompressed/plain_f64_{tag}", "x", DOUBLE, optional, False, pages, expect8(DOUBLE, False, spread(np.concatenate(dense), valid), valid if optional else None),
                    codec="SNAPPY")
        d = _dictionary_bits(rng, INT64, 29)
        pages, dense, valid = [], [], []
        for k, flag in enumerate((True, False, True)):  # dictionary indices
            page, vals, ok = _index_page(rng, INT64, d, 6, optional, version=2, codec="SNAPPY", is_compressed=flag)
            pages.append(page), dense.append(vals), valid.append(ok if optional else np.ones(len(vals), bool))
        valid = np.concatenate(valid)
        yield _case(f"v2_uncompressed/dict_i64_{tag}", "x", INT64, optional, False, pages, expect8(INT64, False, spread(np.concatenate(dense), valid), valid if optional else None),
                    dictionary=dictionary_page(INT64, d, codec="SNAPPY"), codec="SNAPPY")


# ---- chunks larger than one launch's grid (pq_decode_kernel: 16 384 workgroups × 256 rows) -----------------------------------------
def _grid_stride():
    n = 16384 * 256 + 33
    rng = _rng(60)
    vals = _random_u64(rng, n)
    step = 1 << 17  # PLAIN INT64 in pages of 2¹⁷ values
    pages = [data_page(len(vals[a:a + step]), PLAIN, plain(INT64, vals[a:a + step])) for a in range(0, n, step)]
    yield _case("grid_stride/plain_i64", "x", INT64, False, True, pages, expect8(INT64, True, vals))
    d = _strings(200)
    plan = [("bp", 200_000), ("rle", 1_000_000), ("bp", (n - 2_600_000 + 7) // 8)]
    idx = fill_plan(rng, plan, n, len(d), rle_value=len(d) - 1)
    page = data_page(n, RLE_DICTIONARY, bytes([8]) + hybrid(idx, 8, plan))
    expect = pa.DictionaryArray.from_arrays(pa.array(idx.astype(np.int32)), pa.array(d, type=pa.binary())).dictionary_decode()
    yield _case("grid_stride/dictionary_strings", "s", BYTE_ARRAY, False, False, [page], expect, dictionary=dictionary_page(BYTE_ARRAY, d))


FAMILIES = {"delta_widths": _delta_widths, "delta_shapes": _delta_shapes, "dict8_widths": _dict8_widths, "dict8_shapes": _dict8_shapes,
            "string_widths": _string_widths, "levels": _levels, "booleans": _booleans, "v2_uncompressed": _v2_uncompressed, "grid_stride": _grid_stride}
MANY_FAMILIES = ("delta_widths", "delta_shapes", "dict8_widths", "dict8_shapes", "string_widths")  # decoded once more, three row groups to a call


@functools.lru_cache(maxsize=None)
def cases(family=None):
    """Every case of one family (or of all of them) as (id, chunk tuple, file bytes, row count, expected Arrow array); the CPU and the GPU
    tests run the same bytes. Generated once per process."""
    if family is None:
        return tuple(c for f in FAMILIES for c in cases(f))
    return tuple(FAMILIES[family]())


def refusals():
    """(id, chunk tuple, row count, length of the dictionary page) of chunks a reader must refuse: pyarrow does, and so must the library, with FDB_ERR_INVALID."""
    rng = _rng(70)
    v = delta_values_of_width(rng, 1 + 128 + 40, 9, 128, 4)
    body = delta_binary_packed(v, min_width=9)
    cut = body[:-(32 - 8) * 9 // 8]  # the last miniblock holds 8 of its 32 deltas: written without its padding
    yield "refusals/delta_last_miniblock_not_padded", chunk_of("d", INT64, False, False, [data_page(len(v), DELTA_BINARY_PACKED, cut)]), len(v), 0
    d = _dictionary_bits(rng, INT64, 8)
    idx = rng.integers(0, 8, 64).astype(np.uint64)
    runs = varint((20 << 1) | 1) + pack_bits(idx[:40], 3) + varint(3 << 1) + b"\x01"  # 20 groups = 160 values declared, then an RLE run
    page = data_page(43, RLE_DICTIONARY, bytes([3]) + runs)
    yield "refusals/bit_packed_run_longer_than_its_page", chunk_of("x", INT64, False, False, [dictionary_page(INT64, d), page]), 43, len(dictionary_page(INT64, d))
