"""The dense generated scan reads dictionary indices at 1 or 2 bytes from a per-record cache (frostdb_amd/csrc/fdb_record.h, ScanCache).

Every result is compared group by group with a numpy restatement of the query: counts and int64 MIN / MAX exactly, float64 sums to 1e-9
relative (the values are positive, so a sum has no cancellation). `algorithmic_bytes` is compared with the formula restated here at the
widths a launch must scan: 1 byte for dictionaries of ≤ 256 entries, 2 for ≤ 65 536, else the column's own 4 — and 4 for every part of a
launch unless all its parts can hold a cache of one width.

T is the row threshold (kScanCacheMinRows), restated. Rows T + {0, 1, 2, 3, 5, 1023, 1024, 1025}: the tail lanes of the narrow loads
(a lane holds 4 rows), a full 256-thread tile and its neighbours.

A cache buffer is sized like a values slot, align_up(rows * width + 256, 256), which is what `scan_cache_bytes` reports; it comes from
the device pool, whose blocks are whole multiples of 2 MiB, so `live_allocations()["device_bytes"]` grows by the slots rounded up to
that granularity (and `device_blocks` by one per referenced dictionary column)."""
import threading

import numpy as np
import pyarrow as pa
import pytest

from frostdb_amd import physicalplan as pp
from frostdb_amd.logicalplan import Col, Count, Max, Min, Sum

pytestmark = pytest.mark.gpu

T = 1 << 20
ROWS = [T + d for d in (0, 1, 2, 3, 5, 1023, 1024, 1025)]
DICTS = [1, 255, 256, 257, 65535, 65536, 65537]
POOL_GRAIN = 2 << 20


def width_of(entries: int) -> int:
    return 1 if entries <= 256 else 2 if entries <= 65536 else 4


def values_slot(rows: int, width: int) -> int:
    return (rows * width + 256 + 255) // 256 * 256


def pool_block(nbytes: int) -> int:
    return (nbytes + POOL_GRAIN - 1) // POOL_GRAIN * POOL_GRAIN


def words(n: int, tag: str):
    return pa.array([("%s%d" % (tag, i)).encode() for i in range(n)], type=pa.binary())


_WORDS = {}


def dictionary(n: int, tag: str):
    if (n, tag) not in _WORDS:
        _WORDS[(n, tag)] = words(n, tag)
    return _WORDS[(n, tag)]


def dict_column(rng, rows: int, entries: int, tag: str, nulls: bool, sort: bool = False):
    """Indices (uint32) over `entries` entries; a quarter of the rows and the last row hold the LAST entry. With `nulls`: ≈ 10 % NULL rows
    (row 1 among them) whose index slots hold 70 000 + something — above both narrow ranges and, but for the largest dictionary, above
    the dictionary, which the import allows under a NULL."""
    idx = rng.integers(0, entries, rows, dtype=np.uint32)
    idx[rng.random(rows) < 0.25] = entries - 1
    idx[-1] = entries - 1
    if sort:
        idx.sort()
    mask = None
    if nulls:
        mask = rng.random(rows) < 0.1
        mask[1] = True
        mask[-1] = False
        idx = np.where(mask, np.uint32(70000) + (idx & np.uint32(0xFFF)), idx).astype(np.uint32)
    arr = pa.DictionaryArray.from_arrays(pa.array(idx, mask=mask), dictionary(entries, tag))
    return arr, np.where(mask, -1, idx.astype(np.int64)) if nulls else idx.astype(np.int64)


class Table:
    """One record: dictionary columns by name → (entries, nulls), `v` float64 in (0, 1], `i` int64; the host copies of the indices (−1 = NULL)."""

    def __init__(self, rows: int, dicts: dict, seed: int, sort_by=None):
        rng = np.random.default_rng(seed)
        self.rows, self.dicts, self.idx = rows, dicts, {}
        arrays, names = [], []
        for name, (entries, nulls) in dicts.items():
            arr, host = dict_column(rng, rows, entries, name, nulls, sort=(name == sort_by))
            self.idx[name] = host
            arrays.append(arr); names.append(name)
        self.v = 1.0 - rng.random(rows)
        self.i = rng.integers(-2**40, 2**40, rows, dtype=np.int64)
        arrays += [pa.array(self.v), pa.array(self.i)]
        names += ["v", "i"]
        self.record = pa.RecordBatch.from_arrays(arrays, names=names)
        self.rb = pp.ResidentBatch(self.record)

    def close(self):
        self.rb.close()


def expected(tables, filt, groups, with_i):
    """The groups of the rows whose `filt` column holds its LAST entry, as arrays ordered by the flat key Σ (entry index + 1, 0 = NULL) in
    mixed radix (entries + 1 per group column): (flat keys, Σ v, counts, min i, max i); the last two only `with_i`."""
    flats, vs, is_ = [], [], []
    for t in tables:
        sel = np.ones(t.rows, dtype=bool) if filt is None else t.idx[filt] == t.dicts[filt][0] - 1
        flat = np.zeros(int(sel.sum()), dtype=np.int64)
        for g in groups:
            flat = flat * (tables[0].dicts[g][0] + 1) + (t.idx[g][sel] + 1)
        flats.append(flat); vs.append(t.v[sel]); is_.append(t.i[sel])
    flat, v, i = np.concatenate(flats), np.concatenate(vs), np.concatenate(is_)
    counts = np.bincount(flat)
    keys = np.flatnonzero(counts)
    sums = np.bincount(flat, weights=v)[keys]
    mins = maxs = None
    if with_i and len(keys) == 1:
        mins, maxs = np.array([i.min()]), np.array([i.max()])
    elif with_i:
        order = np.argsort(flat, kind="stable")
        starts = np.flatnonzero(np.concatenate([[True], np.diff(flat[order]) != 0]))
        mins, maxs = np.minimum.reduceat(i[order], starts), np.maximum.reduceat(i[order], starts)
    return keys, sums, counts[keys], mins, maxs


def scanned_bytes(tables, filt, groups, widths, with_i):
    """Restated: each referenced buffer once per row — dictionary columns at widths[name], a bitmap where the column holds NULLs, v (and i) at 8."""
    total = 0
    for t in tables:
        for name in dict.fromkeys(([filt] if filt else []) + list(groups)):
            total += t.rows * widths[name] + ((t.rows + 7) // 8 if t.dicts[name][1] else 0)
        total += t.rows * 8 * (2 if with_i else 1)
    return total


def run(tables, filt, groups, widths, with_i=False, ordered=False, kernel="fdb_plan_kernel"):
    """Scans `tables` in one launch and checks result, kernel name and algorithmic bytes; returns the result record."""
    t0 = tables[0]
    aggs = [Sum(Col("v"))] + ([] if ordered else [Count(Col("v"))]) + ([Min(Col("i")), Max(Col("i"))] if with_i else [])  # (an OrderedAggregate takes one aggregation)
    fexpr = None if filt is None else Col(filt) == "%s%d" % (filt, t0.dicts[filt][0] - 1)
    plan = pp.HashAggregatePlan(fexpr, aggs, [Col(g) for g in groups], ordered=ordered)
    try:
        plan.CallbackResident([t.rb for t in tables])
        assert plan.last_kernel() == kernel, plan.last_kernel()
        assert plan.stats()["algorithmic_bytes"] == scanned_bytes(tables, filt, groups, widths, with_i), (filt, groups, widths)
        out = plan.Finish()
    finally:
        plan.Close()
    keys, sums, counts, mins, maxs = expected(tables, filt, groups, with_i)
    assert out.num_rows == len(keys), (out.num_rows, len(keys))
    flat = np.zeros(out.num_rows, dtype=np.int64)
    for g in groups:
        c = out.column(g)
        entry = np.array([int(x.decode()[len(g):]) for x in c.dictionary.to_pylist()] + [-1], dtype=np.int64)  # (… of each value of the result's dictionary)
        ind = c.indices.fill_null(len(entry) - 1).to_numpy(zero_copy_only=False).astype(np.int64)
        flat = flat * (t0.dicts[g][0] + 1) + (entry[ind] + 1)
    order = np.argsort(flat, kind="stable")
    assert np.array_equal(flat[order], keys)  # the same groups, each once
    assert ordered or np.array_equal(out.column("count(v)").to_numpy()[order], counts)
    got_sums = out.column("v" if ordered else "sum(v)").to_numpy()[order]  # (an OrderedAggregate names its partial result after the column)
    assert np.all(np.abs(got_sums - sums) <= 1e-9 * np.abs(sums)), float(np.max(np.abs(got_sums - sums) / np.abs(sums)))
    if with_i:
        assert np.array_equal(out.column("min(i)").to_numpy()[order], mins) and np.array_equal(out.column("max(i)").to_numpy()[order], maxs)
    return out


def as_dict(out):
    return {k: (c, s) for k, c, s in zip(out.column("g").dictionary_decode().to_pylist(), out.column("count(v)").to_pylist(), out.column("sum(v)").to_pylist())}


@pytest.mark.parametrize("rows", ROWS, ids=["T+%d" % (r - T) for r in ROWS])
def test_rows_and_widths(rows):
    """Every dictionary size, with and without NULLs, as filter leaf only (two-phase: v and i are both aggregated), as group column only and
    as both (single-phase), and with a second group column of another width (two-phase)."""
    for entries in DICTS:
        w = width_of(entries)
        other = 300 if w == 1 else 50  # the second group column: 2 bytes beside a 1-byte column, else 1 byte (the key space stays dense)
        for nulls in (False, True):
            t = Table(rows, {"f": (entries, nulls), "g": (entries, nulls), "h": (other, nulls)}, seed=rows + entries + nulls)
            widths = {"f": w, "g": w, "h": width_of(other)}
            try:
                run([t], "f", [], widths, with_i=True)
                run([t], None, ["g"], widths)
                run([t], "f", ["g"], widths)
                run([t], "f", ["g", "h"], widths, with_i=True)
                want_cache = sum(values_slot(rows, widths[c]) for c in "fgh" if widths[c] < 4)
                assert t.rb.scan_cache_bytes == want_cache, (entries, nulls)
            finally:
                t.close()


@pytest.fixture(scope="module")
def fresh():
    """Tables the cache-life tests share: cfg 2's shape (5 codes, 1 024 paths, a third dictionary column nobody scans)."""
    made = []

    def make(rows=T, seed=7, **kw):
        t = Table(rows, {"f": (5, True), "g": (1024, False), "h": (9, False)}, seed=seed, **kw)
        made.append(t)
        return t

    yield make
    for t in made:
        t.close()


def test_cache_life(fresh):
    nothing = pp.live_allocations()
    t = fresh()
    widths = {"f": 1, "g": 2}
    device_bytes, before_arrow = t.rb.device_bytes, t.rb.to_arrow()
    some = np.arange(0, t.rows, 1000)
    taken = t.rb.take(some)
    taken_before = (taken.to_arrow(), taken.device_bytes)
    taken.close()
    live0 = pp.live_allocations()
    assert t.rb.scan_cache_bytes == 0
    first = run([t], "f", ["g"], widths)
    slots = [values_slot(t.rows, 1), values_slot(t.rows, 2)]  # f and g; h is not referenced
    assert t.rb.scan_cache_bytes == sum(slots)
    live1 = pp.live_allocations()  # (the plan is closed: what is left is the cache)
    assert live1["device_blocks"] - live0["device_blocks"] == len(slots)
    assert live1["device_bytes"] - live0["device_bytes"] == sum(pool_block(s) for s in slots)
    second = run([t], "f", ["g"], widths)
    assert pp.live_allocations() == live1 and t.rb.scan_cache_bytes == sum(slots)
    a, b = as_dict(first), as_dict(second)
    assert a.keys() == b.keys() and all(a[k][0] == b[k][0] and abs(a[k][1] - b[k][1]) <= 1e-9 * abs(a[k][1]) for k in a)
    # the record itself is what it was
    assert t.rb.device_bytes == device_bytes
    assert t.rb.to_arrow().equals(before_arrow)
    taken = t.rb.take(some)
    assert taken.to_arrow().equals(taken_before[0]) and taken.device_bytes == taken_before[1] and taken.scan_cache_bytes == 0
    taken.close()
    t.rb.close()
    assert pp.live_allocations() == nothing  # the cache goes with the record


def test_below_the_threshold_nothing_is_cached(fresh):
    t = fresh(rows=T - 1, seed=8)
    live0 = pp.live_allocations()
    run([t], "f", ["g"], {"f": 4, "g": 4})
    assert t.rb.scan_cache_bytes == 0 and pp.live_allocations() == live0


def test_the_interpreting_kernel_reads_the_record(fresh, monkeypatch):
    monkeypatch.setenv("FDB_NO_JIT", "1")
    t = fresh(seed=9)
    live0 = pp.live_allocations()
    run([t], "f", ["g"], {"f": 4, "g": 4}, kernel="scan_slots_kernel")
    assert t.rb.scan_cache_bytes == 0 and pp.live_allocations() == live0


def test_one_launch_over_records_of_mixed_widths():
    """g has 200 entries in one record and 300 in another: no common narrow width, so every part reads g at 4 bytes; f could be read at
    1 byte in both of them, but the third record is below T and has no cache: 4 bytes as well. Nothing is built."""
    a = Table(T, {"f": (5, False), "g": (200, True)}, seed=21)
    b = Table(T + 3, {"f": (5, False), "g": (300, True)}, seed=22)
    c = Table(T - 1, {"f": (5, False), "g": (200, True)}, seed=23)
    try:
        run([a, b, c], "f", ["g"], {"f": 4, "g": 4})
        assert a.rb.scan_cache_bytes == b.rb.scan_cache_bytes == c.rb.scan_cache_bytes == 0
        run([a, b], "f", ["g"], {"f": 1, "g": 4})  # without the small record f is narrow, g still is not
        assert a.rb.scan_cache_bytes == values_slot(T, 1) and b.rb.scan_cache_bytes == values_slot(T + 3, 1)
        run([a, b, c], "f", ["g"], {"f": 4, "g": 4})  # … and a cache that exists is not used when a part lacks one
    finally:
        for t in (a, b, c):
            t.close()


def test_two_threads_meet_a_fresh_record(fresh):
    t = fresh(seed=10)
    live0 = pp.live_allocations()
    start, errors = threading.Barrier(2), []

    def scan():
        try:
            start.wait()
            run([t], "f", ["g"], {"f": 1, "g": 2})
        except BaseException as e:  # noqa: BLE001 (reported by the main thread)
            errors.append(e)

    threads = [threading.Thread(target=scan) for _ in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    assert t.rb.scan_cache_bytes == values_slot(T, 1) + values_slot(T, 2)
    live1 = pp.live_allocations()
    assert live1["device_blocks"] - live0["device_blocks"] == 2
    assert live1["device_bytes"] - live0["device_bytes"] == pool_block(values_slot(T, 1)) + pool_block(values_slot(T, 2))


def test_ordered_plan_over_a_sorted_record(fresh):
    """Sorted by the group column: the rows a wave selects fall into one slot (the uniform-fold branch of the kernel)."""
    t = fresh(rows=T + 1025, seed=11, sort_by="g")
    assert np.all(np.diff(t.idx["g"]) >= 0)
    out = run([t], "f", ["g"], {"f": 1, "g": 2}, ordered=True)
    got = [int(x.decode()[1:]) for x in out.column("g").dictionary_decode().to_pylist()]
    assert got == sorted(got, key=lambda k: ("g%d" % k).encode())  # (an ordered plan emits its groups in key order: bytewise)
