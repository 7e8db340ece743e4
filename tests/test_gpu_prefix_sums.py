"""The three device prefix sums, pinned directly: fdb_selftest_prefix_sums runs each launch sequence as the library runs it over a
caller's uint32 array, and the results are compared with numpy.cumsum over uint64, made exclusive — the uint32 outputs modulo 2^32,
the totals and rec_base in full. Nothing is approximate.

Sizes come from the code (frostdb_amd/csrc/fdb_kernels.hip):
  exclusive scan (fdb_launch_exclusive_scan): one workgroup of 1 024 threads up to n = 4 096 (one entry per thread up to 1 024, then two
    with idle tail threads), three launches beyond — 4 097 is the first — whose middle launch takes two block sums per thread from
    n = 1 024 x 1 024 + 1; without the block-sum scratch one workgroup at any n (4 097, 70 001).
  filter scan (fdb_launch_sel_block_sums + fdb_launch_sel_scan): one workgroup per 1 024 tiles; filter() goes two-level beyond 64
    workgroups — 65 536 tiles is the last one-level launch, 65 537 the first two-level one, both run in both forced levels here —, and
    from 1 024 x 1 024 + 1 025 tiles (1 026 workgroups) a thread of the two-level arm adds more than one block sum.
  strided scan (fdb_launch_scan_u32): its middle launch walks the block sums 1 024 at a time — n = 1 024 x 1 024 is exactly one trip,
    one more entry two trips and the carry between them. Stride 2 is how the run directory is read; the skipped words hold 0xFFFFFFFF.

Contents: all zero; all 2 048 (what a tile can hold); random in [0, 2 048]; ONE non-zero entry — at the first position, at the last and
at either side of a 1 024 boundary: every boundary up to 70 001 entries, and beyond that the boundaries where the code changes (the first,
the one at 1 024 x 1 024, the last) one array each plus one array with a distinct non-zero entry at either side of EVERY boundary and
zeros between (an entry dropped, doubled or moved at any boundary changes every later prefix); totals past 2^32."""
import numpy as np
import pytest

from frostdb_amd import physicalplan as pp

pytestmark = pytest.mark.gpu

TILE = 2048
M = 1024 * 1024
U32 = np.uint64(0xFFFFFFFF)
EVERY_BOUNDARY_UP_TO = 70_001


def exclusive(a: np.ndarray):
    """(exclusive prefix sums of `a` in uint64, their total)."""
    ex = np.zeros(len(a), dtype=np.uint64)
    if len(a) == 0:
        return ex, 0
    c = np.cumsum(a, dtype=np.uint64)
    ex[1:] = c[:-1]
    return ex, int(c[-1])


def low32(x: np.ndarray) -> np.ndarray:
    return (x & U32).astype(np.uint32)


def boundary_positions(n: int):
    """Where a single non-zero entry goes: first, last, either side of the 1 024 boundaries (see the module's docstring)."""
    bounds = list(range(1024, n, 1024))
    if n > EVERY_BOUNDARY_UP_TO:
        bounds = sorted({b for b in (1024, M, bounds[-1]) if b < n})
    at = {0, n - 1}
    for b in bounds:
        at.update((b - 1, b))
    return sorted(p for p in at if 0 <= p < n)


def contents(n: int):
    """(name, uint32 array) for every content class at n entries."""
    rng = np.random.default_rng(20261021 + n)
    yield "zeros", np.zeros(n, dtype=np.uint32)
    if n == 0:
        return
    yield "full", np.full(n, TILE, dtype=np.uint32)
    yield "random", rng.integers(0, TILE + 1, n).astype(np.uint32)
    for p in boundary_positions(n):
        a = np.zeros(n, dtype=np.uint32)
        a[p] = 1 + p % TILE
        yield f"single@{p}", a
    if n > 1024:
        a = np.zeros(n, dtype=np.uint32)
        b = np.arange(1024, n, 1024)
        a[b - 1] = 1 + (2 * b // 1024) % TILE
        a[b] = 1 + (2 * b // 1024 + 1) % TILE
        yield "either side of every boundary", a


def wide_contents(n: int):
    """Small counts with a few entries of 0xFFFFFFFF among them — next to each other, in one block of 1 024, blocks apart, at the end:
    the prefix wraps more than once and the total needs more than 32 bits."""
    rng = np.random.default_rng(77 + n)
    a = rng.integers(0, 8, n).astype(np.uint32)
    at = sorted({p for p in (0, 1, n // 2, n // 2 + 900, n - 1) if 0 <= p < n})
    a[at] = 0xFFFFFFFF
    yield f"0xFFFFFFFF at {at}", a
    b = rng.integers(0, 8, n).astype(np.uint32)
    b[[0, n - 1]] = 0xFFFFFFFF
    yield "0xFFFFFFFF first and last", b


# ---- kind 0: fdb_launch_exclusive_scan ------------------------------------------------------------------------------------------------

def check_exclusive_scan(a, no_block_sums, what):
    got, totals = pp.selftest_prefix_sums(pp.PREFIX_EXCLUSIVE_SCAN, a, 1 if no_block_sums else 0)
    ex, total = exclusive(a)
    bad = np.flatnonzero(got != low32(ex))
    assert len(bad) == 0, (what, len(a), bad[:4], got[bad[:4]], low32(ex)[bad[:4]])
    assert int(totals[0]) == total, (what, len(a), int(totals[0]), total)


@pytest.mark.parametrize("n", [0, 1, 1023, 1024, 1025, 4096, 4097, 5 * 1024 + 1, M + 1])
def test_exclusive_scan(n):
    for what, a in contents(n):
        check_exclusive_scan(a, False, what)


@pytest.mark.parametrize("n", [4097, 70_001])
def test_exclusive_scan_without_block_sums(n):
    for what, a in contents(n):
        check_exclusive_scan(a, True, what)


@pytest.mark.parametrize("n,no_block_sums", [(1025, False), (4097, False), (M + 1, False), (70_001, True)])
def test_exclusive_scan_total_past_32_bits(n, no_block_sums):
    for what, a in wide_contents(n):
        assert exclusive(a)[1] > 2**32
        check_exclusive_scan(a, no_block_sums, what)


# ---- kind 2: fdb_launch_scan_u32 -------------------------------------------------------------------------------------------------------

def check_strided_scan(a, stride, what):
    buf = np.full(len(a) * stride, 0xFFFFFFFF, dtype=np.uint32)
    buf[::stride] = a
    got, totals = pp.selftest_prefix_sums(pp.PREFIX_STRIDED_SCAN, buf, stride)
    assert len(got) == len(a)
    ex, total = exclusive(a)
    bad = np.flatnonzero(got != low32(ex))
    assert len(bad) == 0, (what, len(a), stride, bad[:4], got[bad[:4]], low32(ex)[bad[:4]])
    assert int(totals[0]) == total, (what, len(a), stride, int(totals[0]), total)


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("n", [0, 1, 1023, 1024, 1025, M, M + 1, 2 * M + 1025])
def test_strided_scan(n, stride):
    for what, a in contents(n):
        check_strided_scan(a, stride, what)


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("n", [1025, M + 1])
def test_strided_scan_total_past_32_bits(n, stride):
    for what, a in wide_contents(n):
        assert exclusive(a)[1] > 2**32
        check_strided_scan(a, stride, what)


# ---- kind 1: fdb_launch_sel_block_sums + fdb_launch_sel_scan --------------------------------------------------------------------------

AS_FILTER, ONE_LEVEL, TWO_LEVEL = 0, 1, 2


def table(begins, total_tiles):
    """The record table of records whose first tiles are `begins` (ascending, from 0): (first tile, rows); a record's last tile is
    partly filled, differently from record to record."""
    begins = np.asarray(begins, dtype=np.int64)
    ends = np.append(begins[1:], total_tiles)
    rows = (ends - begins) * TILE - (np.arange(len(begins)) * 37) % TILE
    return np.stack([begins, rows], axis=1)


def record_tables(total_tiles: int):
    yield "one record", table([0], total_tiles)
    if total_tiles == 1:
        return
    yield "first tile is the last tile", table([0, total_tiles - 1], total_tiles)
    if total_tiles > 1000:
        yield "1 000 one-tile records", table([0] + list(range(total_tiles - 1000, total_tiles)), total_tiles)
    b = np.arange(1024, total_tiles + 1, 1024)
    around = np.unique(np.concatenate([[0], b - 1, b, b + 1]))
    around = around[around < total_tiles]
    if len(around) > 1:
        yield "first tiles around every 1 024", table(around, total_tiles)


def check_filter_scan(counts, recs, level, what):
    offsets, rec_base = pp.selftest_prefix_sums(pp.PREFIX_FILTER_SCAN, counts, level, recs)
    ex, total = exclusive(counts)
    bad = np.flatnonzero(offsets != low32(ex))
    assert len(bad) == 0, (what, len(counts), level, bad[:4], offsets[bad[:4]], low32(ex)[bad[:4]])
    begins = recs[:, 0]
    want_base = np.append(ex[begins], np.uint64(total))
    bad = np.flatnonzero(rec_base != want_base)
    assert len(bad) == 0, (what, len(counts), level, bad[:4], rec_base[bad[:4]], want_base[bad[:4]])
    # what compact_stream computes: a tile's place inside its record's output, in 32-bit arithmetic
    r = np.searchsorted(begins, np.arange(len(counts)), side="right") - 1
    place = offsets - low32(rec_base[r])  # (uint32: wraps)
    want_place = ex - ex[begins][r]
    assert int(want_place.max()) < 2**32
    bad = np.flatnonzero(place != want_place.astype(np.uint32))
    assert len(bad) == 0, (what, len(counts), level, bad[:4], place[bad[:4]], want_place[bad[:4]])


FILTER_SCAN_CASES = [(1, AS_FILTER), (1023, AS_FILTER), (1024, AS_FILTER), (1025, AS_FILTER), (1025, TWO_LEVEL),
                     (65536, AS_FILTER), (65536, ONE_LEVEL), (65536, TWO_LEVEL), (65537, AS_FILTER), (65537, ONE_LEVEL), (65537, TWO_LEVEL),
                     (M + 1025, AS_FILTER)]


@pytest.mark.parametrize("total_tiles,level", FILTER_SCAN_CASES)
def test_filter_scan(total_tiles, level):
    tables = list(record_tables(total_tiles))
    for i, (what, counts) in enumerate(contents(total_tiles)):
        # every table with the random counts, the tables in turn with the other contents
        for name, recs in (tables if what == "random" else [tables[i % len(tables)]]):
            check_filter_scan(counts, recs, level, what + ", " + name)


def test_filter_scan_total_past_32_bits():
    """2 097 153 full tiles are 2^32 + 2 048 rows: the offsets wrap at the last tile, rec_base does not. A record boundary lies on
    each side of the wrap."""
    wrap = 2**32 // TILE
    counts = np.full(wrap + 1, TILE, dtype=np.uint32)
    begins = list(range(0, wrap - 65536 + 1, 65536)) + [wrap - 1, wrap]
    _, rec_base = pp.selftest_prefix_sums(pp.PREFIX_FILTER_SCAN, counts, AS_FILTER, table(begins, len(counts)))
    assert [int(x) for x in rec_base[-3:]] == [2**32 - TILE, 2**32, 2**32 + TILE]
    check_filter_scan(counts, table(begins, len(counts)), AS_FILTER, "2^32 + 2 048 rows")


def test_filter_scan_record_across_the_32_bit_wrap():
    """… and a record that begins 500 tiles before the wrap and ends 1 000 tiles behind it: for its later tiles offsets[t] is small
    and (uint32)rec_base[r] large, and their 32-bit difference is still the tile's place inside the record."""
    wrap = 2**32 // TILE
    counts = np.full(wrap + 3000, TILE, dtype=np.uint32)
    counts[wrap - 700:wrap + 1500:3] = 1999  # (so that the wrap does not fall on a tile boundary)
    begins = list(range(0, wrap - 65536 + 1, 65536)) + [wrap - 500, wrap + 1000]
    assert exclusive(counts)[0][wrap - 500] < 2**32 < exclusive(counts)[0][wrap + 1000]
    check_filter_scan(counts, table(begins, len(counts)), AS_FILTER, "record across the wrap")


# ---- arguments ---------------------------------------------------------------------------------------------------------------------------

def test_bad_arguments_are_refused():
    counts = np.zeros(4096, dtype=np.uint32)

    def refused(*args, **kw):
        with pytest.raises(pp.FdbError) as e:
            pp.selftest_prefix_sums(*args, **kw)
        return e.value.code == pp.FDB_ERR_INVALID

    assert refused(3, counts)
    assert refused(-1, counts)
    assert refused(pp.PREFIX_EXCLUSIVE_SCAN, counts, 2)
    assert refused(pp.PREFIX_EXCLUSIVE_SCAN, counts, 0, [(0, 1)])                      # a record table without the filter scan
    assert refused(pp.PREFIX_STRIDED_SCAN, counts, 0)                                  # stride 0
    assert refused(pp.PREFIX_STRIDED_SCAN, counts, 17)
    assert refused(pp.PREFIX_FILTER_SCAN, counts, 3, [(0, 4096 * TILE)])               # no such level
    assert refused(pp.PREFIX_FILTER_SCAN, counts, 0)                                   # no records
    assert refused(pp.PREFIX_FILTER_SCAN, counts, 0, [(1, 4095 * TILE)])               # the first record does not begin at tile 0
    assert refused(pp.PREFIX_FILTER_SCAN, counts, 0, [(0, 4095 * TILE)])               # the last record ends before the last tile
    assert refused(pp.PREFIX_FILTER_SCAN, counts, 0, [(0, 4096 * TILE + 1)])           # … behind it
    assert refused(pp.PREFIX_FILTER_SCAN, counts, 0, [(0, TILE), (2, 4094 * TILE)])    # a gap between two records
    assert refused(pp.PREFIX_FILTER_SCAN, counts, 0, [(0, 2 * TILE), (1, 4095 * TILE)])  # an overlap
    assert refused(pp.PREFIX_FILTER_SCAN, counts, 0, [(0, 4096 * TILE), (4096, 0)])    # a record without rows
    assert refused(pp.PREFIX_FILTER_SCAN, counts[:0], 0, [(0, 1)])                     # no tiles
    L = pp.lib()
    totals = np.zeros(1, dtype=np.uint64)
    assert L.fdb_selftest_prefix_sums(0, 0, None, 16, 0, None, 0, counts.ctypes.data, totals.ctypes.data) == pp.FDB_ERR_INVALID
    assert L.fdb_selftest_prefix_sums(0, 0, counts.ctypes.data, 16, 0, None, 0, None, totals.ctypes.data) == pp.FDB_ERR_INVALID
    assert L.fdb_selftest_prefix_sums(0, 0, counts.ctypes.data, 16, 0, None, 0, counts.ctypes.data, None) == pp.FDB_ERR_INVALID
    assert L.fdb_selftest_prefix_sums(0, 0, counts.ctypes.data, 2**28 + 1, 0, None, 0, counts.ctypes.data, totals.ctypes.data) == pp.FDB_ERR_INVALID
