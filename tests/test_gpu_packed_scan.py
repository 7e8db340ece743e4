"""The dense generated scan reads dictionary indices at 4 bits (form H) or 12 bits (form T) from a per-record cache of whole frames
(frostdb_amd/csrc/fdb_record.h, scan_cache_packed_position), for records of at least 4 Mi rows.

Every result is compared group by group with numpy, as tests/test_gpu_narrow_scan.py does (its Table, expected and comparison are used):
counts and int64 MIN / MAX exactly, float64 sums to 1e-9 relative over positive values. The rule, restated (form_of): H where entries +
(nulls > 0) <= 16, else 1 byte where entries <= 256, else T where entries + (nulls > 0) <= 4 096, else 2 bytes where entries <= 65 536.
`algorithmic_bytes` of an index slot is (rows x bits + 7) / 8 per record; a packed buffer is align_up(ceil(rows / 1024) x frame + 256, 256)
bytes, frame = 512 (H) or 1 536 (T), which is what `scan_cache_bytes` reports for it.

One launch that mixes dictionaries of 15 and 300 entries for one column cannot agree on a packed form (H and T) nor on a byte width (1 and
2), so — as before the packed forms — it reads that column's uint32 indices; 15 beside 200 entries (H and none) meet at the 1-byte form."""
import os
import subprocess
import sys

import numpy as np
import pytest

from frostdb_amd import physicalplan as pp
from frostdb_amd.logicalplan import Col, Count, Max, Min, Sum
from tests import test_gpu_narrow_scan as ns

pytestmark = pytest.mark.gpu

P = 4 << 20  # kScanCachePackedMinRows, restated
ROWS = [P + d for d in (0, 1, 3, 1023, 1024, 1025)]
H, T = "H", "T"
BITS = {H: 4, 1: 8, T: 12, 2: 16, 4: 32}


def form_of(entries: int, nulls: bool, rows: int):
    if rows >= P and entries + nulls <= 16:
        return H
    if entries <= 256:
        return 1
    if rows >= P and entries + nulls <= 4096:
        return T
    return 2 if entries <= 65536 else 4


def buffer_bytes(rows: int, form) -> int:
    if form in (H, T):
        return ((rows + 1023) // 1024 * (512 if form == H else 1536) + 256 + 255) // 256 * 256
    return ns.values_slot(rows, form)


def scanned_bytes(tables, filt, groups, forms, with_i):
    total = 0
    for t in tables:
        for name in dict.fromkeys(([filt] if filt else []) + list(groups)):
            total += (t.rows * BITS[forms[name]] + 7) // 8 + ((t.rows + 7) // 8 if t.dicts[name][1] else 0)
        total += t.rows * 8 * (2 if with_i else 1)
    return total


def run(tables, filt, groups, forms, with_i=False, ordered=False, kernel="fdb_plan_kernel"):
    """ns.run with the algorithmic bytes of the packed forms: scans `tables` in one launch, checks kernel, bytes and every group."""
    t0 = tables[0]
    aggs = [Sum(Col("v"))] + ([] if ordered else [Count(Col("v"))]) + ([Min(Col("i")), Max(Col("i"))] if with_i else [])
    fexpr = None if filt is None else Col(filt) == "%s%d" % (filt, t0.dicts[filt][0] - 1)
    plan = pp.HashAggregatePlan(fexpr, aggs, [Col(g) for g in groups], ordered=ordered)
    try:
        plan.CallbackResident([t.rb for t in tables])
        assert plan.last_kernel() == kernel, plan.last_kernel()
        assert plan.stats()["algorithmic_bytes"] == scanned_bytes(tables, filt, groups, forms, with_i), (filt, groups, forms)
        out = plan.Finish()
    finally:
        plan.Close()
    keys, sums, counts, mins, maxs = ns.expected(tables, filt, groups, with_i)
    assert out.num_rows == len(keys), (out.num_rows, len(keys))
    flat = np.zeros(out.num_rows, dtype=np.int64)
    for g in groups:
        c = out.column(g)
        entry = np.array([int(x.decode()[len(g):]) for x in c.dictionary.to_pylist()] + [-1], dtype=np.int64)
        ind = c.indices.fill_null(len(entry) - 1).to_numpy(zero_copy_only=False).astype(np.int64)
        flat = flat * (t0.dicts[g][0] + 1) + (entry[ind] + 1)
    order = np.argsort(flat, kind="stable")
    assert np.array_equal(flat[order], keys)
    assert ordered or np.array_equal(out.column("count(v)").to_numpy()[order], counts)
    got = out.column("v" if ordered else "sum(v)").to_numpy()[order]
    assert np.all(np.abs(got - sums) <= 1e-9 * np.abs(sums)), float(np.max(np.abs(got - sums) / np.abs(sums)))
    if with_i:
        assert np.array_equal(out.column("min(i)").to_numpy()[order], mins) and np.array_equal(out.column("max(i)").to_numpy()[order], maxs)
    return out


@pytest.mark.parametrize("small,big", [(1, 257), (15, 4095), (16, 4096)])
@pytest.mark.parametrize("rows", ROWS, ids=["P+%d" % (r - P) for r in ROWS])
def test_rows_and_forms(rows, small, big):
    """A column at the H / byte edge (`a`) and one at the T / 2-byte edge (`b`), with and without NULLs (junk indices above 70 000 under a
    NULL, the last row holds the last entry: ns.dict_column), each as filter only, as group only, as both, and as the late slot of a
    two-phase shape beside a 1-byte column."""
    for nulls in (False, True):
        t = ns.Table(rows, {"a": (small, nulls), "b": (big, nulls), "h": (50, nulls)}, seed=rows + small + nulls)
        forms = {"a": form_of(small, nulls, rows), "b": form_of(big, nulls, rows), "h": 1}
        try:
            run([t], "a", [], forms, with_i=True)
            run([t], "b", [], forms, with_i=True)
            run([t], None, ["a"], forms)
            run([t], None, ["b"], forms)
            run([t], "a", ["b"], forms)
            run([t], "b", ["a"], forms)
            run([t], "a", ["b", "h"], forms, with_i=True)
            run([t], "b", ["a", "h"], forms, with_i=True)
            assert t.rb.scan_cache_bytes == sum(buffer_bytes(rows, forms[c]) for c in "abh"), (small, big, nulls, forms)
        finally:
            t.close()


def test_a_record_below_the_threshold_takes_the_launch_to_the_byte_forms():
    """One launch over records of 4 Mi and 4 Mi - 1 rows reads both at the byte forms. The same two records pushed one launch each — the
    first then at H / T, the second at 1 / 2 bytes — give the same groups and counts, and sums equal to 1e-9 relative."""
    a = ns.Table(P, {"a": (15, True), "b": (300, False)}, seed=1)
    b = ns.Table(P - 1, {"a": (15, True), "b": (300, False)}, seed=2)
    try:
        both = run([a, b], "a", ["b"], {"a": 1, "b": 2})
        assert a.rb.scan_cache_bytes == ns.values_slot(P, 1) + ns.values_slot(P, 2) and b.rb.scan_cache_bytes == ns.values_slot(P - 1, 1) + ns.values_slot(P - 1, 2)
        plan = pp.HashAggregatePlan(Col("a") == "a14", [Sum(Col("v")), Count(Col("v"))], [Col("b")])
        try:
            plan.CallbackResident([a.rb])
            assert plan.stats()["algorithmic_bytes"] == scanned_bytes([a], "a", ["b"], {"a": H, "b": T}, False)
            plan.CallbackResident([b.rb])
            apart = plan.Finish()
        finally:
            plan.Close()
        # scanned alone the first record took its packed forms, and now holds both
        assert a.rb.scan_cache_bytes == ns.values_slot(P, 1) + ns.values_slot(P, 2) + buffer_bytes(P, H) + buffer_bytes(P, T)

        def groups(out):
            return {k: (c, x) for k, c, x in zip(out.column("b").dictionary_decode().to_pylist(), out.column("count(v)").to_pylist(), out.column("sum(v)").to_pylist())}

        one, two = groups(both), groups(apart)
        assert sorted(one) == sorted(two) and len(one) == 300
        assert all(one[k][0] == two[k][0] and abs(one[k][1] - two[k][1]) <= 1e-9 * one[k][1] for k in one)
    finally:
        a.close(); b.close()


def test_mixed_dictionaries_of_one_column():
    live0 = pp.live_allocations()
    a = ns.Table(P, {"a": (15, False)}, seed=3)
    try:
        for other, forms in ((200, {"a": 1}), (300, {"a": 4})):  # H beside none: 1 byte; H beside T, 1 byte beside 2: the uint32 column
            b = ns.Table(P, {"a": (other, False)}, seed=4)
            try:
                plan = pp.HashAggregatePlan(None, [Sum(Col("v")), Count(Col("v"))], [Col("a")])
                try:
                    plan.CallbackResident([a.rb, b.rb])
                    assert plan.stats()["algorithmic_bytes"] == scanned_bytes([a, b], None, ["a"], forms, False)
                    out = plan.Finish()
                finally:
                    plan.Close()
                want = np.bincount(a.idx["a"], minlength=other) + np.bincount(b.idx["a"], minlength=other)
                got = dict(zip(out.column("a").dictionary_decode().to_pylist(), out.column("count(v)").to_pylist()))
                assert got == {b"a%d" % k: int(n) for k, n in enumerate(want) if n}
                assert a.rb.scan_cache_bytes == ns.values_slot(P, 1)  # (the second launch builds nothing, and the first one's buffer stays)
            finally:
                b.close()
    finally:
        a.close()
    assert pp.live_allocations() == live0


def test_is_null_leaf_reads_a_packed_slot_with_its_bitmap():
    """The filter `a IS NULL` reads slot a's bitmap; the group column `a` is the same column at H, null-folded: every selected row is in NULL's group."""
    live0 = pp.live_allocations()
    t = ns.Table(P + 5, {"a": (9, True)}, seed=5)
    try:
        plan = pp.HashAggregatePlan(Col("a") == None, [Count(Col("v")), Sum(Col("v"))], [Col("a")])  # noqa: E711
        try:
            plan.CallbackResident([t.rb])
            assert plan.last_kernel() == "fdb_plan_kernel"
            out = plan.Finish()
        finally:
            plan.Close()
        null = t.idx["a"] < 0
        assert out.num_rows == 1 and out.column("count(v)").to_pylist() == [int(null.sum())] and out.column("a").null_count == 1
        assert abs(out.column("sum(v)").to_pylist()[0] - t.v[null].sum()) <= 1e-9 * t.v[null].sum()
        assert t.rb.scan_cache_bytes == buffer_bytes(P + 5, H)
    finally:
        t.close()
    assert pp.live_allocations() == live0


def test_ordered_plan_over_a_sorted_record():
    t = ns.Table(P + 3, {"a": (12, True), "b": (1000, False)}, seed=6, sort_by="b")
    try:
        run([t], "a", ["b"], {"a": H, "b": T}, ordered=True)
    finally:
        t.close()


def test_interpreting_path_builds_nothing():
    code = ("import numpy as np\nfrom frostdb_amd import physicalplan as pp\nfrom tests import test_gpu_narrow_scan as ns\nfrom tests import test_gpu_packed_scan as ps\n"
            "live0 = pp.live_allocations()\nt = ns.Table(ps.P, {'a': (15, True), 'b': (1000, False)}, seed=8)\nlive1 = pp.live_allocations()\n"
            "ps.run([t], 'a', ['b'], {'a': 4, 'b': 4}, kernel='scan_slots_kernel')\nassert t.rb.scan_cache_bytes == 0 and pp.live_allocations() == live1\n"
            "t.close()\nassert pp.live_allocations() == live0\nprint('ok')\n")
    env = dict(os.environ, FDB_NO_JIT="1")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stderr[-2000:]


def test_closing_the_record_returns_the_pool():
    live0 = pp.live_allocations()
    t = ns.Table(P, {"a": (5, True), "b": (1024, False)}, seed=9)
    run([t], "a", ["b"], {"a": H, "b": T})
    assert t.rb.scan_cache_bytes == buffer_bytes(P, H) + buffer_bytes(P, T)
    t.close()
    assert pp.live_allocations() == live0


# ---- the builder's bytes ------------------------------------------------------------------------------------------------------------------
def packed_positions(i: np.ndarray, rows: int, form):
    """scan_cache_packed_position, restated: (byte of the low 8 bits — T only —, byte of the nibble, its shift)."""
    frame, plane = (512, 0) if form == H else (1536, 1024)
    b, j = i // 1024, i % 1024
    u, l, r = j // 256, (j % 256) // 4, j % 4
    e = np.where(i < rows // 1024 * 1024, 16 * l + 4 * u + r, j)
    return b * frame + e, b * frame + plane + e // 2, (e % 2) * 4


@pytest.mark.parametrize("form,entries,nulls", [(H, 15, True), (H, 16, False), (H, 0, True), (T, 4095, True), (T, 4096, False), (T, 300, True)])
@pytest.mark.parametrize("rows", [1024 * k + d for k in (0, 1, 3) for d in (0, 1, 1023) if 1024 * k + d > 0])
def test_selftest_scan_cache_packed(rows, form, entries, nulls):
    """Every byte of the frames: S = entries under a NULL row, the truncated index elsewhere, each at its position, 0 from the last row to the frame's end."""
    i = np.arange(rows, dtype=np.int64)
    valid = np.ones(rows, dtype=bool)
    if nulls:
        valid = i % 7 != 3
        valid[0] = valid[rows - 1] = False
        valid[256:320] = False
    modulus = max(entries, 1)
    indices = ((i * 7 + 3) % modulus).astype(np.uint32)
    indices[~valid] = np.uint32(70000) + (i[~valid] % 4096).astype(np.uint32)
    bits = np.packbits(valid, bitorder="little")
    frames = (rows + 1023) // 1024
    out = np.full(frames * (512 if form == H else 1536), 0xAB, dtype=np.uint8)
    L = pp.lib()
    rc = L.fdb_selftest_scan_cache_packed(indices.ctypes.data, bits.ctypes.data if nulls else None, rows, entries, 5 if form == H else 6, 0, out.ctypes.data, len(out))
    assert rc == 0, L.fdb_last_error().decode("utf-8", "replace")
    value = np.where(valid, (i * 7 + 3) % modulus, entries)
    want = np.zeros(len(out), dtype=np.uint8)
    lo, nib, shift = packed_positions(i, rows, form)
    if form == T:
        want[lo] = value & 0xFF
    np.bitwise_or.at(want, nib, (((value >> 8) if form == T else value) & 0xF) << shift)
    assert np.array_equal(out, want), np.flatnonzero(out != want)[:8]


def test_selftest_scan_cache_packed_bad_arguments():
    L = pp.lib()
    src, bits, out = np.zeros(16, dtype=np.uint32), np.zeros(2, dtype=np.uint8), np.zeros(1536, dtype=np.uint8)
    call = lambda *a: L.fdb_selftest_scan_cache_packed(*a)  # noqa: E731
    assert call(src.ctypes.data, bits.ctypes.data, 16, 16, 5, 0, out.ctypes.data, 512) == pp.FDB_ERR_INVALID     # 16 entries and NULL do not fit 4 bits
    assert call(src.ctypes.data, bits.ctypes.data, 16, 4096, 6, 0, out.ctypes.data, 1536) == pp.FDB_ERR_INVALID  # nor 4 096 and NULL 12
    assert call(src.ctypes.data, None, 16, 17, 5, 0, out.ctypes.data, 512) == pp.FDB_ERR_INVALID
    assert call(src.ctypes.data, None, 16, 5, 1, 0, out.ctypes.data, 512) == pp.FDB_ERR_INVALID   # not a packed form
    assert call(src.ctypes.data, None, 16, 5, 5, 0, out.ctypes.data, 1536) == pp.FDB_ERR_INVALID  # out_bytes is not the frames
