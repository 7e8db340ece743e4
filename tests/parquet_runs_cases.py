"""What tests/test_parquet_runs_cpu.py (the host walk, fdb_selftest_parquet_write_runs) and tests/test_gpu_parquet_runs.py (the device
passes, fdb_batch_to_parquet_runs) share: a restatement of the rule by which a page's dictionary indices and definition levels are cut
into RLE and bit-packed runs, a decoder of the RLE / bit-packed hybrid written from the format's description, a walk of a written file
that takes every data page apart, the comparison of a file with the restatement, and the records whose pages have the shapes the rule
can go wrong on. No test lives here."""
import io

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq

from tests import parquet_index_cases as X, parquet_pages as P, parquet_snappy_cases as S, parquet_write_cases as cases

PAGE = cases.PAGE
WIDTHS = [1, 2, 3, 7, 8, 9, 15, 16, 17]
THRESHOLDS = [16, 8, 6, 3, 2, 2, 2, 1, 1]


def threshold(w: int) -> int:
    return -(-16 // w)


# ---- 1. the rule, restated -----------------------------------------------------------------------------------------------------------------
def plan_of(sym, w: int):
    """The runs of the stream `sym` at width w >= 1 by the rule: [("rle", symbols) | ("bp", groups)]."""
    sym = [int(s) for s in sym]
    n, full, tail = len(sym), len(sym) // 8, len(sym) % 8
    T = threshold(w)
    value = [sym[8 * g] if len(set(sym[8 * g:8 * g + 8])) == 1 else None for g in range(full)]   # a uniform group's value
    rle = [False] * full
    g = 0
    while g < full:                                                                                # stretches
        e = g + 1
        if value[g] is not None:
            while e < full and value[e] == value[g]:
                e += 1
            if e - g >= T:
                rle[g:e] = [True] * (e - g)
        g = e
    plan, g = [], 0
    while g < full:
        e = g + 1
        if rle[g]:
            while e < full and rle[e] and value[e] == value[g]:
                e += 1
            plan.append(["rle", 8 * (e - g)])
        else:
            while e < full and not rle[e]:
                e += 1
            plan.append(["bp", e - g])
        g = e
    if tail:
        if plan and plan[-1][0] == "rle" and all(s == value[full - 1] for s in sym[8 * full:]):
            plan[-1][1] += tail
        elif plan and plan[-1][0] == "bp":
            plan[-1][1] += 1
        else:
            plan.append(["bp", 1])
    return [tuple(r) for r in plan]


def restate(sym, w: int) -> bytes:
    """The stream's bytes by the rule, laid out by the page builder of tests/parquet_pages.py (padding zero)."""
    return P.hybrid(np.asarray(sym, dtype=np.uint64), w, plan_of(sym, w), pad=0)


def stream_bytes(sym, w: int) -> bytes:
    """What the writer puts for a stream with `runs`: nothing for no symbol, the one RLE run of today for equal symbols (and width 0),
    else the rule."""
    sym = [int(s) for s in sym]
    if not sym:
        return b""
    if len(set(sym)) == 1:
        return P.varint(len(sym) << 1) + sym[0].to_bytes((w + 7) // 8, "little")
    return restate(sym, w)


def plain_bytes(sym, w: int) -> bytes:
    """… and without: one RLE run or ONE bit-packed run."""
    sym = [int(s) for s in sym]
    if not sym or len(set(sym)) == 1:
        return stream_bytes(sym, w)
    return P.hybrid(np.asarray(sym, dtype=np.uint64), w, P.bp_plan(len(sym)), pad=0)


# ---- 2. the hybrid, decoded from the format's description (Encodings.md, "Run Length Encoding / Bit-Packing Hybrid") ----------------------------
def decode_hybrid(data: bytes, w: int, n: int):
    """(the n symbols, the runs as [("rle", count) | ("bp", groups)]) of a stream that fills `data` exactly."""
    out, runs, at = [], [], 0
    while at < len(data):
        head, shift = 0, 0
        while True:
            b = data[at]
            at += 1
            head |= (b & 0x7F) << shift
            shift += 7
            if b < 0x80:
                break
        if head & 1:
            groups = head >> 1
            assert groups > 0
            bits = int.from_bytes(data[at:at + groups * w], "little")
            assert at + groups * w <= len(data), "a bit-packed run past the stream's end"
            at += groups * w
            vals = [(bits >> (k * w)) & ((1 << w) - 1) for k in range(groups * 8)]
            assert len(out) + len(vals) < n + 8, "a bit-packed run that is not the last holds padding"
            if len(out) + len(vals) > n:
                assert not any(vals[n - len(out):]), "padding that is not zero"
                vals = vals[:n - len(out)]
            out += vals
            runs.append(("bp", groups))
        else:
            count = head >> 1
            assert count > 0
            nb = (w + 7) // 8
            v = int.from_bytes(data[at:at + nb], "little")
            assert at + nb <= len(data) and v < (1 << w) if w else v == 0
            at += nb
            out += [v] * count
            runs.append(("rle", count))
    assert at == len(data) and len(out) == n, (at, len(data), len(out), n)
    return out, runs


# ---- 3. a written file taken apart ---------------------------------------------------------------------------------------------------------
def data_pages(data: bytes):
    """(the file's metadata reader, per column (its chunk's metadata, its schema entry, the bodies of its data pages V1, inflated))."""
    pf = pq.ParquetFile(io.BytesIO(data))
    rg = pf.metadata.row_group(0)
    out = []
    for j in range(rg.num_columns):
        col, sc = rg.column(j), pf.schema.column(j)
        pages, _start = S.chunk_pages(data, col)
        mine = []
        for ptype, usize, stored, _hl in pages:
            if ptype != S.DATA_PAGE:
                continue
            body = stored if col.compression == "UNCOMPRESSED" else pa.decompress(stored, decompressed_size=usize, codec=col.compression.lower(), asbytes=True)
            assert len(body) == usize
            mine.append(body)
        out.append((col, sc, mine))
    return pf, out


def page_headers(data: bytes):
    """Per column the data pages' (num_values, encoding) in order, from the page headers."""
    out = []
    for ch in X.chunk_fields(data):
        pages = []
        for pos, _size, ptype, _nv in X.walk_pages(data, ch):
            if ptype == S.DATA_PAGE:
                h, _ = S._struct(data, pos)
                pages.append((h[5][1], h[5][2]))
        out.append(pages)
    return out


def split_page(body: bytes, optional: bool, indexed: bool):
    """(level bytes or None, index width or None, the rest) of a data page V1's body."""
    at, levels, width = 0, None, None
    if optional:
        n = int.from_bytes(body[:4], "little")
        levels, at = body[4:4 + n], 4 + n
    if indexed and at < len(body):
        width, at = body[at], at + 1
    return levels, width, body[at:]


def column_symbols(col: pa.Array):
    """(validity per row, the index per row or None) of a record's column; indices only of a dictionary-typed column, whose entries the
    writer keeps in order."""
    valid = np.asarray(col.is_valid()).astype(bool) if len(col) else np.zeros(0, bool)
    if not pa.types.is_dictionary(col.type):
        return valid, None
    idx = np.asarray(col.indices.fill_null(0).to_numpy(zero_copy_only=False)).astype(np.uint64)
    return valid, idx


def width_of(entries: int) -> int:
    return (entries - 1).bit_length() if entries > 0 else 0


def streams_of(flags: int):
    return bool(flags & 1), bool(flags & 2)


def assert_runs_file(record: pa.RecordBatch, data: bytes, plain: bytes, page_rows: int, flags):
    """`data` (written with runs: `flags`[column] bit 0 = indices, bit 1 = levels) against the restatement, page by page and stream by
    stream; no page longer than in `plain` (the same call without runs); sizes in the footer and the page index follow the pages.
    Returns how many streams were cut into more than one run."""
    pf, cols = data_pages(data)
    _pf0, cols0 = data_pages(plain)
    headers = page_headers(data)
    cut = 0
    for j, ((col, sc, pages), (_c0, _s0, pages0)) in enumerate(zip(cols, cols0)):
        name = record.schema.names[j]
        optional = sc.max_definition_level == 1
        indexed = col.physical_type == "BYTE_ARRAY"
        valid, idx = column_symbols(record.column(j))
        run_values, run_levels = streams_of(flags[j])
        n_pages = -(-record.num_rows // page_rows)
        assert len(pages) == len(pages0) == n_pages == len(headers[j]), name
        for p, (body, body0) in enumerate(zip(pages, pages0)):
            lo, hi = p * page_rows, min((p + 1) * page_rows, record.num_rows)
            assert headers[j][p][0] == hi - lo
            assert len(body) <= len(body0), (name, p, len(body), len(body0))
            levels, width, rest = split_page(body, optional, indexed)
            levels0, width0, rest0 = split_page(body0, optional, indexed)
            v = valid[lo:hi]
            if optional:
                got, runs = decode_hybrid(levels, 1, hi - lo)
                assert got == [int(b) for b in v], (name, p)
                assert levels == (stream_bytes(got, 1) if run_levels else plain_bytes(got, 1)), (name, p, runs)
                assert levels0 == plain_bytes(got, 1)
                cut += run_levels and len(runs) > 1
            else:
                assert v.all()
            if not indexed:
                assert rest == rest0, (name, p)
                continue
            count = int(v.sum())
            if width is None:   # PLAIN pages of zero values: an empty dictionary
                assert count == 0 and rest == b""
                continue
            got, runs = decode_hybrid(rest, width, count)
            if idx is not None:
                assert width == width_of(len(record.column(j).dictionary)), name
                assert got == [int(i) for i in idx[lo:hi][v]], (name, p)
            assert rest == (stream_bytes(got, width) if run_values else plain_bytes(got, width)), (name, p, runs)
            assert rest0 == plain_bytes(got, width) and width0 == width
            cut += run_values and len(runs) > 1
    # the footer's sizes and the page index agree with a walk of the chunks
    fields = X.chunk_fields(data)
    rg = X.row_group_fields(data)
    at = 4
    for ch in fields:
        start = ch["dictionary_page_offset"] if ch["dictionary_page_offset"] is not None else ch["data_page_offset"]
        assert start == at, ch["name"]
        walked = X.walk_pages(data, ch)   # (asserts that the pages fill total_compressed_size exactly)
        if ch["offset_index"] is not None:
            locs = X.offset_index(data, ch["offset_index"])
            assert [(pos, size) for pos, size, ptype, _nv in walked if ptype == S.DATA_PAGE] == [(o, s) for o, s, _r in locs], ch["name"]
            assert [r for _o, _s, r in locs] == [p * page_rows for p in range(len(locs))]
        at += ch["total_compressed_size"]
    if rg["total_compressed_size"] is not None:
        assert rg["total_compressed_size"] == at - 4
    md = pf.metadata.row_group(0)
    assert sum(md.column(j).total_uncompressed_size for j in range(md.num_columns)) == md.total_byte_size
    for j in range(md.num_columns):   # the encodings lists do not change
        assert md.column(j).encodings == pq.ParquetFile(io.BytesIO(plain)).metadata.row_group(0).column(j).encodings
    return cut


def read_back(data: bytes) -> pa.RecordBatch:
    t = pq.read_table(io.BytesIO(data)).combine_chunks()
    return pa.RecordBatch.from_arrays([c.chunk(0) if c.num_chunks else pa.array([], type=c.type) for c in t.columns], names=t.schema.names)


def flags_of(record: pa.RecordBatch, runs):
    """The per-column bits the binding makes of `runs` (True, names, or a dict)."""
    def indexed(t):
        t = t.value_type if pa.types.is_dictionary(t) else t
        return t in (pa.string(), pa.binary(), pa.large_string(), pa.large_binary())
    names = record.schema.names
    if runs is True:
        return [2 | int(indexed(f.type)) for f in record.schema]
    if isinstance(runs, dict):
        return [{None: 0, True: 3, "values": 1, "levels": 2}[runs.get(n)] for n in names]
    return [3 if n in runs else 0 for n in names]


# ---- 4. records ----------------------------------------------------------------------------------------------------------------------------
def _dict(idx, entries: int, valid=None, utf8=False) -> pa.DictionaryArray:
    idx = np.asarray(idx, dtype=np.uint32)
    return pa.DictionaryArray.from_arrays(pa.array(idx, mask=None if valid is None else ~np.asarray(valid, bool)), pa.array(cases.dict_entries(entries, utf8), type=pa.string() if utf8 else pa.binary()))


def entries_for(w: int) -> int:
    """A dictionary size whose indices are w bits wide."""
    return (1 << (w - 1)) + 1 if w > 1 else 2


def noise(rng, n: int, hi: int) -> np.ndarray:
    """n indices below hi of which no 8 in a row are equal (no uniform group anywhere they go)."""
    v = rng.integers(0, hi, n)
    v[1::2] = (v[0::2][:len(v[1::2])] + 1) % hi   # neighbours differ
    return v


def page_for(w: int) -> int:
    """The smallest page_rows that holds three stretches of T groups and two mixed groups: 448, 256, 192, 128, then 64."""
    return 64 * -(-8 * (3 * threshold(w) + 2) // 64)


def stretch_symbols(rng, w: int, pages: int = 0):
    """One page per shape at width w: stretches of T − 1, T and T + 1 groups at the page's start, middle and end, two RLE runs back to
    back, a stretch cut by one odd symbol. Pages are `pages` symbols; a stretch that does not fit is cut to the page."""
    T, hi = threshold(w), entries_for(w)
    out = []
    pages = pages or page_for(w)
    groups = pages // 8
    for length in (T - 1, T, T + 1):
        for where in ("start", "middle", "end"):
            page = noise(rng, pages, hi)
            length_ = min(max(length, 0), groups)
            g0 = 0 if where == "start" else groups - length_ if where == "end" else (groups - length_) // 2
            page[8 * g0:8 * (g0 + length_)] = hi - 1
            out.append(page)
    page = noise(rng, pages, hi)                    # back to back: two RLE runs of different values, then a third after one mixed group
    a = min(T, groups // 3)
    page[0:8 * a] = 0
    page[8 * a:16 * a] = hi - 1
    page[16 * a + 8:16 * a + 8 + 8 * a] = 1
    out.append(page)
    page = np.full(pages, hi - 1)                   # one long stretch but for one symbol in the middle
    page[pages // 2 + 3] = 0
    out.append(page)
    return np.concatenate(out)


def width_record(w: int, valid_pattern=None, seed: int = 0) -> pa.RecordBatch:
    """A dictionary column of width w whose pages (of page_for(w) non-NULL rows when there is no NULL) are stretch_symbols, beside a
    timestamp."""
    rng = np.random.default_rng(1000 * w + seed)
    idx = stretch_symbols(rng, w)
    valid = None if valid_pattern is None else cases.valid_mask(len(idx), valid_pattern)
    return pa.RecordBatch.from_arrays([_dict(idx, entries_for(w), valid), pa.array(np.arange(len(idx), dtype=np.int64))], names=["labels.w%d" % w, "timestamp"])


def tail_pieces(w: int):
    """[(indices, what)] — streams of 8 × k + t symbols whose tail (t = 1 … 7) joins the last RLE run, follows it without joining, or
    follows a bit-packed run; and n < 8."""
    T, hi = threshold(w), entries_for(w)
    rng = np.random.default_rng(77 + w)
    out = []
    for t in range(1, 8):
        head = noise(rng, 16, hi)
        out.append((np.concatenate([head, np.full(8 * T + t, hi - 1)]), "joins"))
        odd = np.full(t, hi - 1)
        odd[-1] = 0
        out.append((np.concatenate([head, np.full(8 * T, hi - 1), odd]), "after_rle"))
        out.append((np.concatenate([np.full(8 * T, 1), noise(rng, 8 + t, hi)]), "after_bp"))
        out.append((noise(rng, t, hi) if t > 1 else np.array([hi - 1]), "short"))
    return out


def levels_record(valid: np.ndarray, seed: int = 5) -> pa.RecordBatch:
    """An int64, a float64, a bool and a dictionary column that all have the NULLs of `valid`."""
    n = len(valid)
    rng = np.random.default_rng(seed)
    return pa.RecordBatch.from_arrays([pa.array(rng.integers(-9, 9, n), mask=~valid), pa.array(rng.standard_normal(n), mask=~valid), pa.array(rng.random(n) < 0.5, mask=~valid),
                                       _dict(noise(rng, n, 5), 5, valid, utf8=True)], names=["i", "f", "b", "labels.d"])


def clustered_valid(rows: int, stretch: int) -> np.ndarray:
    """NULLs and values in alternating stretches of `stretch` rows, the first at row 3."""
    r = np.arange(rows)
    return ((np.maximum(r - 3, 0) // stretch) % 2 == 0) | (r < 3)


def sorted_record(rows: int, seed: int = 3, labels: int = 3) -> pa.RecordBatch:
    """What FrostDB writes: label columns in long stretches (sorted), a dynamic column that is NULL in stretches, a timestamp."""
    rng = np.random.default_rng(seed)
    a = np.sort(rng.integers(0, 5, rows))
    b = np.sort(rng.integers(0, 300, rows))
    cols = [_dict(a, 5, utf8=True), _dict(b, 300, valid=a != 2, utf8=True), _dict(rng.integers(0, 70000, rows), 70000, valid=rng.random(rows) < 0.9),
            pa.array(np.sort(rng.integers(0, 10**12, rows))), pa.array(rng.standard_normal(rows), mask=a == 1)]
    return pa.RecordBatch.from_arrays(cols[:labels] + cols[3:], names=["labels.a", "labels.b", "labels.wide"][:labels] + ["timestamp", "value"])
