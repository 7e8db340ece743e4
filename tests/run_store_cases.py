"""Cases for the table-free OrderedAggregate — the run store: the run kernels of fdb_jitgen.cpp (narrow, medium and wide run records), the
segments push_hash lays out for them, and the run store's Finish (scan_u32_*, runs_map_kernel, runs_flags_kernel, runs_flags_wide_kernel,
runs_sort_keys_kernel, runs_expand_kernel, runs_translate_kernel of fdb_kernels.hip) — and, beside every case, the CLAIM of what it makes
the bookkeeping do: per launch the run record (Plan::runs_format), per wave the events of its (rb, rp, ps) state (`wave_model`), the number
of runs, whether the keys arrive in order.

The claims come from a Python RESTATEMENT of the C++; every part names the lines it restates. It can drift from them: when fdb_jitgen.cpp
changes how a wave stages, flushes or changes chunks, when push_hash changes the tile order or the grid, or when Plan::runs_format /
Plan::runs_wanted change a limit, the restatement has to follow, or the coverage it promises is of the old code. Not restated: the default
grid (a device property): a launch with the default grid is modelled as one workgroup per 1 024-row tile, which holds while the record has
at most DEFAULT_GRID_AT_LEAST tiles (tests/test_gpu_run_store.py reads the device's grid off the launch and holds it to that); beyond that
a case claims no wave events at the default grid.

The EXPECTED ROWS come from a plain numpy group-by in this file (`reference`): np.unique over the key tuples, then bincount, add.at,
minimum.at and maximum.at — never from another plan of the library. Rows come out in the plan's key order (every group column ascending
bytewise, NULLs last) and are compared row for row, in order. A NULL slot of the aggregated column reads as its zeroed value (as
tests/ordered_oracle.py has it), int64 sums wrap modulo 2^64. Where keys are NULL in the first columns the reference's own merge leaves a
group in several rows; the device brings such a group out whole and so does `reference`.

No test lives here. `cases(family)` is the one generator both test modules run; it is seeded and deterministic.
tests/test_run_store_cases_cpu.py pins the restatement on hand-worked claims, holds the families to claiming every event, every format
boundary and both sides of the segment limit, and the reference to the oracle; tests/test_gpu_run_store.py runs the cases on the device."""
import functools
import math

import numpy as np
import pyarrow as pa

from frostdb_amd.logicalplan import Col, Count, Max, Min, Sum

SCAN_FAMILIES = ("per_tile_k", "edges", "filter", "formats", "segments", "extremes")
FINISH_FAMILIES = ("run_counts", "violation", "translate", "many_runs")
FAMILIES = SCAN_FAMILIES + FINISH_FAMILIES

# ---- geometry, restated --------------------------------------------------------------------------------------------------------------------
WAVE_ROWS = 256        # HashGen::source: a lane owns 4 consecutive rows (`tid * 4`, fdb_jitgen.cpp:1147), a wave 64 lanes
TILE_ROWS = 1024       # BLK * 4 (fdb_jitgen.cpp:1106); one directory entry per (tile, wave): `h.runs.dir + (tile * 4 + wv) * 2` (:1404, :1441)
CHUNK = 4096           # FDB_RUN_CHUNK (fdb_kernels.h:198)
RUN_WAVE_LDS = 256 * 48  # FDB_RUN_WAVE_LDS = FDB_RUN_STAGE × FDB_RUN_BYTES (fdb_kernels.h:200-202)
MAX_SEGMENTS = 64      # FDB_MAX_RUN_SEGMENTS (fdb_kernels.h:542)
NARROW_MOST, MEDIUM_MOST, NARROW_COLUMNS = 254, 65534, 32  # Plan::runs_format (fdb_hash.cpp:1361-1369), FDB_RUN_TUPLE_BYTES
DEFAULT_GRID_AT_LEAST = 128
KERNEL = {0: "fdb_hash_kernel(runs)", 1: "fdb_hash_kernel(runs, medium)", 2: "fdb_hash_kernel(runs, wide)"}
SORTED_FINISH = "runs_sort_keys_kernel + runs_expand_kernel"  # what Plan::runs_sort leaves in last_kernel() (fdb_hash.cpp:1566)
TRANSLATE = "runs_translate_kernel"

EVENTS = frozenset((
    "flush_stage_full", "flush_with_fewer_than_64_active_lanes", "writer_lane_not_0", "switch_exact_fit", "switch_abandoning",
    "switch_with_runs_pending", "direct", "direct_and_switch_same_tile", "final_flush_empty", "final_flush_pending", "wave_tile_without_runs"))

AGGS = {"sum_i": Sum(Col("v")), "sum_f": Sum(Col("f")), "min": Min(Col("v")), "max": Max(Col("f")), "count": Count(Col("v"))}
FIVE = ("sum_i", "sum_f", "min", "max", "count")
I64_MIN, I64_MAX = np.iinfo(np.int64).min, np.iinfo(np.int64).max


def stage_cap(fmt, n_cols):
    """push_hash (fdb_hash.cpp:331-333): the runs a wave's LDS stage holds. A wide record is the table's key tuple — 4 words of header, a
    word per dictionary column, rounded up to 4 (hash_layout) — and 4 words of count and aggregate."""
    if fmt == 0:
        return 256
    if fmt == 1:
        return RUN_WAVE_LDS // 80
    key_words = (4 + n_cols + 3) & ~3
    return RUN_WAVE_LDS // (4 * (key_words + 4))


def run_ends(sel, gid):
    """Which rows end a run of their wave (fdb_jitgen.cpp:1241-1286). Inside a lane row k − 1 is folded into row k when both are selected and
    their keys are equal (:1241-1246); a lane's last selected row is folded into the next lane of the wave when that lane is active and its
    first selected row has the same key (:1286). A lane that left the tile (past the record's end :1147, nothing selected :1162) ends
    every run. → (ends [rows, padded to whole tiles], active [lanes])"""
    n = len(sel)
    n_pad = -(-max(n, 1) // TILE_ROWS) * TILE_ROWS
    s = np.zeros(n_pad, bool); s[:n] = sel
    g = np.full(n_pad, -1, np.int64); g[:n] = gid
    s4, g4 = s.reshape(-1, 4), g.reshape(-1, 4)
    ends = s4.copy()
    for k in range(3):
        ends[:, k] &= ~(s4[:, k + 1] & (g4[:, k] == g4[:, k + 1]))
    active = s4.any(axis=1)
    kf = np.argmax(s4, axis=1)                   # first selected row of the lane
    kl = 3 - np.argmax(s4[:, ::-1], axis=1)      # last selected row
    lanes = np.arange(len(s4))
    first_key, last_key = g4[lanes, kf], g4[lanes, kl]
    hand_on = np.zeros(len(s4), bool)
    hand_on[:-1] = active[:-1] & active[1:] & (last_key[:-1] == first_key[1:]) & (lanes[:-1] % 64 != 63)
    ends[lanes[hand_on], kl[hand_on]] = False
    return ends.reshape(-1), active


def wave_model(sel, gid, fmt, n_cols, grid):
    """One launch of the run kernel over a record: `sel` the rows the filter keeps, `gid` a code per row that is equal exactly where the key
    tuples are, `fmt` the run record, `grid` the workgroups (0: the default grid, taken as one workgroup per tile).
    → dict(events, runs, chunks, chunk_of [(tile, wave) → (workgroup, wave, chunk number of that wave) or None], n_w)

    Restated: the tile loop `for (tile = blockIdx.x; tile < n_tiles; tile += gridDim.x)` (fdb_jitgen.cpp:1140) with gridDim = min(grid,
    n_tiles) (fdb_hash.cpp:356); s_runs = (0, 4096, 4096) at the start (:1120); per wave tile with runs: sw = rp + n_w > 4096, direct =
    n_w > CAP (wide and medium only), the stage is copied out when sw, direct or (rp − ps) + n_w > CAP (:1396-1400, :1433-1437) by the
    ACTIVE lanes — stride n_act, lane first2 takes the next chunk and writes the state and the directory entry (:1401-1404, :1438-1441);
    the final copy (:1496-1511)."""
    ends, active = run_ends(sel, gid)
    n_tiles = len(ends) // TILE_ROWS
    n_w = ends.reshape(-1, WAVE_ROWS).sum(axis=1)
    act = active.reshape(-1, 64)
    n_act, first2 = act.sum(axis=1), np.argmax(act, axis=1)
    cap = stage_cap(fmt, n_cols)
    G = n_tiles if grid == 0 else min(grid, n_tiles)
    if grid == 0 and n_tiles > DEFAULT_GRID_AT_LEAST:
        return dict(events=None, runs=int(n_w.sum()), chunks=None, chunk_of=None, n_w=n_w)
    events, chunks, chunk_of = set(), 0, [None] * (n_tiles * 4)
    for b in range(G):
        for wv in range(4):
            rp = ps = CHUNK
            had, gap, gen = False, False, -1
            for tile in range(b, n_tiles, G):
                i = tile * 4 + wv
                if n_act[i] == 0:
                    gap = had
                    continue
                n = int(n_w[i])
                assert n > 0  # (an active lane has a selected row, and the wave's last one ends a run)
                if gap:
                    events.add("wave_tile_without_runs")
                    gap = False
                sw, direct, pend = rp + n > CHUNK, fmt != 0 and n > cap, rp - ps
                if sw or direct or pend + n > cap:
                    if pend > 0:
                        if pend + n > cap:
                            events.add("flush_stage_full")
                        if n_act[i] < 64:
                            events.add("flush_with_fewer_than_64_active_lanes")
                    ps = rp
                if sw:
                    if had:  # (the first tile of a wave always takes a chunk: that is the branch every test reaches)
                        events.add("switch_exact_fit" if rp == CHUNK else "switch_abandoning")
                        if pend > 0:
                            events.add("switch_with_runs_pending")
                        if direct:
                            events.add("direct_and_switch_same_tile")
                    rp = ps = 0
                    gen += 1
                    chunks += 1
                if direct:
                    events.add("direct")
                if first2[i] != 0:
                    events.add("writer_lane_not_0")
                chunk_of[i] = (b, wv, gen)
                rp += n
                if direct:
                    ps = rp
                had = True
            if had:
                events.add("final_flush_pending" if rp > ps else "final_flush_empty")
    return dict(events=events, runs=int(n_w.sum()), chunks=chunks, chunk_of=chunk_of, n_w=n_w)


def segment_chunks(rows, grid):
    """push_hash (fdb_hash.cpp:355-360): the chunks a segment is sized for"""
    n_tiles = -(-rows // TILE_ROWS)
    G = n_tiles if grid == 0 else min(grid, n_tiles)
    return rows // (CHUNK - 256) + G * 4 + 2


class FormatModel:
    """Plan::runs_format (fdb_hash.cpp:1361-1369) over the pushes of one plan: the plan's columns in first-seen order, every column's values
    interned in dictionary order (resolve_batch). `force`: $FDB_RUNS_WIDE."""

    def __init__(self, force=None):
        self.cols, self.values, self.force = [], {}, force

    def push(self, batch):
        present = [f for f in batch.schema.names if f.startswith("labels.")]
        for name in present:
            if name not in self.values:
                self.cols.append(name)
                self.values[name] = {}
            known = self.values[name]
            for v in batch.column(batch.schema.get_field_index(name)).dictionary.to_pylist():
                known.setdefault(v, len(known) + 1)
        most = max(len(self.values[c]) for c in self.cols)
        if self.force == "1" or len(self.cols) > NARROW_COLUMNS or present != self.cols or most > MEDIUM_MOST:
            return 2
        return 1 if most > NARROW_MOST or self.force == "m" else 0


# ---- records -----------------------------------------------------------------------------------------------------------------------------------
def value(tag, x):
    return b"%s%05d" % (tag, x)


def dict_col(k, x, tag=b"v", order=None):
    """A dictionary column of k values v00000 … ; x: the VALUE of every row (−1 = NULL). The dictionary lists the values in DESCENDING order
    (or in `order`, a permutation: entry i holds value order[i]), so neither indices nor key ids are ranks."""
    x = np.asarray(x, np.int64)
    order = np.arange(k - 1, -1, -1) if order is None else np.asarray(order)
    place = np.empty(k, np.int64)
    place[order] = np.arange(k)
    null = x < 0
    idx = pa.array(np.where(null, 0, place[np.where(null, 0, x)]).astype(np.uint32), mask=null if null.any() else None)
    return pa.DictionaryArray.from_arrays(idx, pa.array([value(tag, v) for v in order], type=pa.binary()))


def names_of(n_cols):
    return ["labels.l%02d" % c for c in range(n_cols)]


def record(keys, v, f=None, v_null=None, f_null=None, names=None):
    """keys: dictionary arrays in plan order; v: int64; f: float64 (default: small integers derived from v, so that float sums are exact)"""
    v = np.asarray(v, np.int64)
    f = np.asarray((v % 97 - 48).astype(np.float64) if f is None else f, np.float64)
    arrays = list(keys) + [pa.array(v, mask=v_null), pa.array(f, mask=f_null)]
    return pa.RecordBatch.from_arrays(arrays, names=(names or names_of(len(keys))) + ["v", "f"])


def values_for(n, seed, positive=True):
    rng = np.random.default_rng(seed)
    return rng.integers(1, 1000, n) if positive else rng.integers(-1000, 1000, n)


def radix_keys(g, sizes, cols=None):
    """Key number g → one value per column, lexicographic in g: the last len(sizes) columns count in mixed radix, the ones before are constant"""
    g = np.asarray(g, np.int64)
    out, div = [], 1
    for k in reversed(sizes):
        out.append((g // div) % k)
        div *= k
    assert g.max(initial=0) < div
    out = out[::-1]
    cols = cols or len(sizes)
    return [np.zeros(len(g), np.int64)] * (cols - len(sizes)) + out


def keyed_record(g, sizes=(200, 200, 200), cols=None, seed=0, dropped=(), null_last=False, **kw):
    """One record whose row r has key number g[r]. `dropped`: rows the filter v > 0 removes (0 and negative values alternate)."""
    g = np.asarray(g, np.int64)
    xs = radix_keys(g, sizes, cols)
    full = [1] * (len(xs) - len(sizes)) + list(sizes)
    if null_last:  # the largest value of every counting column becomes NULL: still in key order (NULLs last)
        xs = [np.where((x == k - 1) & (k > 1) & (c >= len(xs) - len(sizes)), -1, x) for c, (x, k) in enumerate(zip(xs, full))]
    v = values_for(len(g), seed + len(g))
    d = np.asarray(sorted(dropped), np.int64)
    if len(d):
        v[d] = np.where(np.arange(len(d)) % 2 == 0, 0, -v[d])
    return record([dict_col(k, x) for k, x in zip(full, xs)], v, **kw)


def runs_to_keys(lengths, keys=None):
    """[run length] (+ the key number of every run; default 0, 1, 2 …) → key number per row"""
    keys = np.arange(len(lengths)) if keys is None else np.asarray(keys)
    return np.repeat(keys, lengths)


def cut(batch, points):
    edges = [0] + list(points) + [batch.num_rows]
    return [batch.slice(a, b - a) for a, b in zip(edges, edges[1:])]


# ---- the reference: a numpy group-by ---------------------------------------------------------------------------------------------------------
def key_ranks(records, names):
    """Per column: the rank of every row's value among ALL values of the column (bytes ascending), NULL and absent = the largest → [rows] each"""
    out, shown = [], []
    for name in names:
        vals = set()
        for b in records:
            i = b.schema.get_field_index(name)
            if i >= 0:
                vals.update(b.column(i).dictionary.to_pylist())
        order = sorted(vals)
        rank = {v: r for r, v in enumerate(order)}
        per = []
        for b in records:
            i = b.schema.get_field_index(name)
            if i < 0:
                per.append(np.full(b.num_rows, len(order), np.int64))
                continue
            a = b.column(i)
            lut = np.array([rank[v] for v in a.dictionary.to_pylist()] + [len(order)], np.int64)
            per.append(lut[a.indices.fill_null(len(lut) - 1).to_numpy(zero_copy_only=False).astype(np.int64)])
        out.append(np.concatenate(per) if per else np.zeros(0, np.int64))
        shown.append(order + [None])
    return out, shown


def selected(batch, filt):
    """filt: None or "v > 0" (a NULL never matches)"""
    if filt is None:
        return np.ones(batch.num_rows, bool)
    a = batch.column(batch.schema.get_field_index("v"))
    return (a.fill_null(0).to_numpy(zero_copy_only=False) > 0) & ~a.is_null().to_numpy(zero_copy_only=False)


def group_codes(ranks, shown):
    """→ (code per row, equal exactly where the key tuples are and ordered like them; None when 63 bits do not hold the tuple)"""
    code, span = np.zeros(len(ranks[0]) if ranks else 0, np.int64), 1
    for r, s in zip(ranks, shown):
        span *= len(s)
        if span >= 1 << 62:
            return None
        code = code * len(s) + r
    return code


def reference(records, names, agg, filt=None, fsum=False):
    """→ (key rank columns [groups] each, shown values per column, aggregate [groups]) in key order. agg: a name of AGGS."""
    ranks, shown = key_ranks(records, names)
    sel = np.concatenate([selected(b, filt) for b in records]) if records else np.zeros(0, bool)
    rows = np.flatnonzero(sel)
    code = group_codes(ranks, shown)
    if code is not None:
        uniq, first, inv = np.unique(code[rows], return_index=True, return_inverse=True)
    else:
        tuples = np.stack([r[rows] for r in ranks], axis=1)
        uniq, first, inv = np.unique(tuples, axis=0, return_index=True, return_inverse=True)
    inv = inv.reshape(-1)
    n = len(first)
    keys = [r[rows][first] for r in ranks]
    if agg == "count":
        return keys, shown, np.bincount(inv, minlength=n).astype(np.int64)
    col = "f" if agg in ("sum_f", "max") else "v"
    arr = [b.column(b.schema.get_field_index(col)) for b in records]
    x = np.concatenate([a.fill_null(0).to_numpy(zero_copy_only=False) for a in arr])[rows]  # a NULL slot reads as its zeroed value
    if agg in ("sum_i", "sum_f"):
        if fsum:
            order = np.argsort(inv, kind="stable")
            bounds = np.searchsorted(inv[order], np.arange(n + 1))
            return keys, shown, np.array([math.fsum(x[order[a:b]]) for a, b in zip(bounds, bounds[1:])])
        acc = np.zeros(n, x.dtype)
        with np.errstate(over="ignore", invalid="ignore"):
            np.add.at(acc, inv, x)
        return keys, shown, acc
    if x.dtype == np.float64:
        acc = np.full(n, np.inf if agg == "min" else -np.inf)
    else:
        acc = np.full(n, I64_MAX if agg == "min" else I64_MIN, np.int64)
    (np.minimum if agg == "min" else np.maximum).at(acc, inv, x)
    return keys, shown, acc


def reference_rows(records, names, agg, filt=None, fsum=False):
    keys, shown, acc = reference(records, names, agg, filt, fsum)
    cols = [[s[k] for k in kc] for kc, s in zip(keys, shown)]
    return list(zip(*cols, acc.tolist())) if len(acc) else []


def fsum_bounds(records, names, filt=None):
    """Per group (n − 1) · 2^-53 · Σ|v| over column f: the error bound of a float64 sum in ANY order"""
    ranks, shown = key_ranks(records, names)
    rows = np.flatnonzero(np.concatenate([selected(b, filt) for b in records]))
    _, inv = np.unique(group_codes(ranks, shown)[rows], return_inverse=True)
    inv = inv.reshape(-1)
    x = np.concatenate([b.column(b.schema.get_field_index("f")).fill_null(0).to_numpy(zero_copy_only=False) for b in records])[rows]
    cnt = np.bincount(inv)
    mag = np.zeros(len(cnt)); np.add.at(mag, inv, np.abs(x))
    return (cnt - 1) * 2.0 ** -53 * mag * (1 + 2.0 ** -50)  # (the factor covers the rounding of Σ|v| itself)


# ---- cases ----------------------------------------------------------------------------------------------------------------------------------------
class Case:
    """`records` go through ONE ordered plan, `pushes` says how: a list of calls, each ("host", i) — Callback of record i — or ("resident",
    [i …]) — CallbackResident of those records at once; default: one host Callback per record. `grids`: the grid_blocks to run at (0 =
    the default grid). `formats`: per record the run record it is claimed to write (None: the record is not scanned by the run kernel).
    `in_order`: whether the keys arrive in order — the sorted Finish runs exactly when they do not. `source`: records of a SECOND plan,
    merged into the first as runs before Finish (family translate). `claims`: names this case must deliver (checked by the CPU module)."""

    def __init__(self, id, family, records, aggs=FIVE, grids=(0,), filt=None, force=None, pushes=None, in_order=True, source=None, fsum=False,
                 claims=()):
        self.id, self.family, self.records, self.aggs, self.grids = id, family, list(records), tuple(aggs), tuple(grids)
        self.filt, self.force, self.in_order, self.source, self.fsum, self.claims = filt, force, in_order, source, fsum, tuple(claims)
        self.names = []
        for b in self.records + list(source or []):
            self.names += [f for f in b.schema.names if f.startswith("labels.") and f not in self.names]
        self.pushes = pushes if pushes is not None else [("host", i) for i in range(len(self.records))]
        self.formats = self._formats()

    def _formats(self):
        """Plan::runs_wanted's segment limit (fdb_hash.cpp:1331) and runs_format per record; a record without rows launches nothing"""
        m, out, segs, left = FormatModel(self.force), [None] * len(self.records), 0, False
        for how, what in self.pushes:
            idx = [what] if how == "host" else list(what)
            live = [i for i in idx if self.records[i].num_rows > 0]
            fmts = {i: m.push(self.records[i]) for i in idx}  # (every record of a call is resolved before the first launch)
            if not live:
                continue
            if left or segs + len(live) > MAX_SEGMENTS:
                left = True
                continue
            for i in live:
                out[i] = fmts[i]
            segs += len(live)
        self.leaves_the_path = left
        return out

    def filter_expr(self):
        return None if self.filt is None else Col("v") > 0

    def all_records(self):
        return self.records + list(self.source or [])

    def rows(self):
        return sum(b.num_rows for b in self.all_records())

    def want(self, agg):
        return reference(self.all_records(), self.names, agg, self.filt, self.fsum and agg == "sum_f")

    def want_rows(self, agg):
        return reference_rows(self.all_records(), self.names, agg, self.filt, self.fsum and agg == "sum_f")

    @functools.lru_cache(maxsize=None)
    def launches(self, grid):
        """wave_model of every record that the run kernel scans → [(record index, model result)]"""
        ranks, shown = key_ranks(self.records, self.names)
        code = group_codes(ranks, shown)
        if code is None:
            code = np.unique(np.stack(ranks, axis=1), axis=0, return_inverse=True)[1].reshape(-1)
        out, at = [], 0
        m = FormatModel(self.force)
        for i, b in enumerate(self.records):
            m.push(b)
            if self.formats[i] is not None:
                out.append((i, wave_model(selected(b, self.filt), code[at:at + b.num_rows], self.formats[i], len(m.cols), grid)))
            at += b.num_rows
        return out

    def events(self, grid):
        ev = set()
        for _, r in self.launches(grid):
            if r["events"] is None:
                return None
            ev |= r["events"]
        return ev

    def runs(self, grid=0):
        return sum(r["runs"] for _, r in self.launches(grid))

    def __repr__(self):
        return self.id


# -- per_tile_k: every wave tile ends exactly k runs ----------------------------------------------------------------------------------------
# tiles per k: enough for the event the k is there for at grid 1 AND grid 2 (a wave of grid 2 sees every second tile)
PER_TILE = {1: 4, 3: 172, 128: 66, 255: 34, 256: 34}


def per_tile_keys(k, tiles, join):
    """Key number per row: wave tile w (256 rows) is cut into k runs of 256 / k rows (the remainder goes to the later runs). `join`: the last
    run of every EVEN wave tile and the first run of the next one share their key — one group in two runs, cut by the wave's edge."""
    w = np.arange(tiles * 4 * WAVE_ROWS) // WAVE_ROWS
    j = (np.arange(tiles * 4 * WAVE_ROWS) % WAVE_ROWS) * k // WAVE_ROWS
    return w * k + j - ((w + 1) // 2 if join else 0)


def per_tile_cases():
    out = []
    for k, tiles in PER_TILE.items():
        join = k in (3, 128, 255)
        out.append(Case("per_tile_k-%d_runs_over_%d_tiles%s" % (k, tiles, "_joined" if join else ""), "per_tile_k", [keyed_record(per_tile_keys(k, tiles, join), seed=100 + k)], grids=(1, 2, 0)))
    return out


# -- edges -----------------------------------------------------------------------------------------------------------------------------------------
EDGE_LAYOUTS = {
    # last rows of runs: 255, 256, 257 (wave edge), 1 023, 1 024, 1 025 (tile edge), 1 299 (the ragged end: 1 300 is no multiple of 256)
    "runs_end_on_rows_255_256_257_1023_1024_1025": ([256, 1, 1, 766, 1, 1, 274], ()),
    # last rows 3 (lane 0's last), 4 (lane 1's first), 7, 8, 252 + 255 …
    "runs_end_on_a_lanes_last_row_and_the_next_lanes_first": ([4, 1, 3, 1, 244, 3, 1, 4, 2], ()),
    "one_run_over_three_whole_tiles": ([1000, 24 + 3072 + 10, 50], ()),
    "one_key_ends_a_record_and_starts_the_next": ([300, 500, 227], (550,)),
    "one_key_across_a_one_row_record_and_an_empty_record": ([300, 500, 227], (640, 641, 641)),
    "records_of_777_and_1027_rows": ([5, 700, 72 + 100, 900, 27], (777,)),
    "one_run_is_the_whole_record_of_2049_rows": ([2049], ()),
}


def edges_cases():
    out = []
    for name, (lengths, cuts) in EDGE_LAYOUTS.items():
        rec = keyed_record(runs_to_keys(lengths, np.arange(len(lengths)) * 7 + 3), seed=200 + len(lengths))
        out.append(Case("edges-" + name, "edges", cut(rec, cuts), grids=(1, 2, 0)))
    return out


# -- filter: v > 0, the dropped rows placed ------------------------------------------------------------------------------------------------------
def filter_cases():
    out = []
    dense = per_tile_keys(128, 4, False)   # 4 tiles, every wave tile 128 runs of 2 rows: a stage is full after two tiles
    for lanes in (1, 5, 63):  # wave 0 of tile 2 (the tile whose runs make the stage flush at grid 1): its first lanes leave the tile
        out.append(Case("filter-first_%d_lanes_of_a_wave_tile_emptied" % lanes, "filter", [keyed_record(dense, seed=300 + lanes, dropped=range(2048, 2048 + 4 * lanes))],
                        filt="v > 0", grids=(1, 2, 0), claims=("flush_with_fewer_than_64_active_lanes", "writer_lane_not_0")))
    out.append(Case("filter-a_whole_wave_tile_emptied_between_two_with_runs", "filter", [keyed_record(dense, seed=310, dropped=range(1024, 1280))], filt="v > 0", grids=(1, 2, 0),
                    claims=("wave_tile_without_runs",)))
    # runs of 85 / 86 rows: lanes 0, 1 and 63 of wave tile 1 lose their middle rows — rows 0 and 3 of such a lane are two runs of one key
    long_runs = per_tile_keys(3, 3, True)
    mid = [256 + 4 * lane + k for lane in (0, 1, 63) for k in (1, 2)]
    out.append(Case("filter-middle_rows_of_a_lane_removed", "filter", [keyed_record(long_runs, seed=320, dropped=mid)], filt="v > 0", grids=(1, 2, 0)))
    rec = keyed_record(per_tile_keys(3, 3, True), seed=330, dropped=range(1000, 2100))
    out.append(Case("filter-all_of_a_record_removed", "filter", cut(rec, (1000, 2100)), filt="v > 0", grids=(1, 2, 0)))
    return out


# -- formats: the limits of Plan::runs_format -------------------------------------------------------------------------------------------------------
def sorted_sample(sizes, n, seed, always=()):
    """n key numbers drawn from the mixed-radix space, ascending, `always` among them"""
    space = int(np.prod([int(s) for s in sizes]))
    rng = np.random.default_rng(seed)
    return np.sort(np.concatenate([rng.integers(0, space, n - len(always)), np.asarray(always, np.int64)]))


def formats_cases():
    out = []
    two = ("sum_i", "max")
    for most, fmt in ((254, 0), (255, 1), (65534, 1), (65535, 2)):
        sizes = (3, most, 4)
        g = sorted_sample(sizes, 1500, 400 + most, always=(0, 4 * most * 3 - 1, 4 * (most - 1) + 1))  # (the column's smallest and largest value are used)
        out.append(Case("formats-largest_column_of_%d_values" % most, "formats", [keyed_record(g, sizes, seed=410)], aggs=two, grids=(1, 2, 0), claims=("format_%d" % fmt,)))
    for cols, fmt in ((32, 0), (33, 2)):
        g = sorted_sample((5, 6, 7), 1500, 420 + cols)
        out.append(Case("formats-%d_group_columns" % cols, "formats", [keyed_record(g, (5, 6, 7), cols=cols, seed=421)], aggs=("sum_i",), grids=(1, 2, 0), claims=("format_%d" % fmt,)))
    for cols in (13, 40):  # every row its own run: 256 runs per wave tile > CAP = 128 / 64 → straight into the chunk; the 17th tile of a wave changes chunks
        out.append(Case("formats-%d_columns_wide_every_row_its_own_run" % cols, "formats", [keyed_record(np.arange(17 * TILE_ROWS + 5), cols=cols, seed=430 + cols)], aggs=("sum_i",),
                        force="1", grids=(1, 2, 0), claims=("format_2", "direct", "direct_and_switch_same_tile", "final_flush_empty")))
    # one plan, three pushes in key order: 3 columns of ≤ 254 values (narrow); the second record's dictionary brings column 1 to 300 values (medium);
    # the third lacks column 2 (wide; NULL there). Column 0 rises from record to record.
    a = keyed_record(sorted_sample((2, 200, 5), 700, 440), (2, 200, 5), seed=441)
    gb = sorted_sample((2, 300, 5), 700, 442)
    xb = radix_keys(gb, (2, 300, 5))
    b = record([dict_col(4, xb[0] + 2), dict_col(300, xb[1]), dict_col(5, xb[2])], values_for(700, 443))
    gc = sorted_sample((2, 300), 700, 444)
    xc = radix_keys(gc, (2, 300))
    c = record([dict_col(6, xc[0] + 4), dict_col(300, xc[1])], values_for(700, 445), names=names_of(2))
    out.append(Case("formats-narrow_then_medium_then_wide_segments_in_key_order", "formats", [a, b, c], aggs=two, grids=(1, 2, 0), claims=("format_0", "format_1", "format_2")))
    # the stage of the wider records carried across tiles, filled and taken through a change of chunks, as per_tile_k does for the narrow one:
    # medium (CAP = 153), 100 runs per wave tile: the second tile fills the stage; the 41st finds 4 000 runs in the chunk and abandons 96 slots.
    # wide with 3 columns (CAP = 256), 255 runs per wave tile: as per_tile_k's k = 255
    out.append(Case("formats-medium_100_runs_per_wave_tile_over_84_tiles", "formats", [keyed_record(per_tile_keys(100, 84, True), seed=450)], aggs=("sum_i", "sum_f"), force="m", grids=(1, 2, 0),
                    claims=("format_1", "flush_stage_full", "switch_abandoning", "switch_with_runs_pending")))
    out.append(Case("formats-wide_255_runs_per_wave_tile_over_34_tiles", "formats", [keyed_record(per_tile_keys(255, 34, True), seed=451)], aggs=("sum_i", "sum_f"), force="1", grids=(1, 2, 0),
                    claims=("format_2", "flush_stage_full", "switch_abandoning", "switch_with_runs_pending")))
    return out


# -- segments: FDB_MAX_RUN_SEGMENTS -------------------------------------------------------------------------------------------------------------------
def segments_cases():
    out = []
    for n in (64, 65):
        lengths = np.random.default_rng(500 + n).integers(1, 40, 3 * n)
        rec = keyed_record(runs_to_keys(lengths), seed=510)
        cuts = np.sort(np.random.default_rng(520 + n).choice(np.arange(1, rec.num_rows), n - 1, replace=False))
        recs = cut(rec, cuts)
        claim = ("segments_at_limit",) if n == 64 else ("segments_beyond_limit",)
        out.append(Case("segments-%d_host_records" % n, "segments", recs, aggs=FIVE if n == 64 else ("sum_i", "sum_f"), grids=(1, 2, 0), claims=claim))
        out.append(Case("segments-%d_resident_records_in_one_call" % n, "segments", recs, aggs=("sum_i",), pushes=[("resident", list(range(n)))], grids=(1, 2, 0), claims=claim))
    return out


# -- extremes ---------------------------------------------------------------------------------------------------------------------------------------
def extremes_cases():
    out = []
    lengths = np.random.default_rng(600).integers(1, 300, 24)
    g = runs_to_keys(lengths, np.arange(24) * 5)
    n = len(g)
    grp = g // 5
    rng = np.random.default_rng(601)
    v = rng.integers(-1000, 1000, n)
    v[grp == 0] = I64_MAX                       # SUM wraps
    v[grp == 1] = I64_MIN
    v[grp == 2] = np.where(np.arange((grp == 2).sum()) % 2 == 0, I64_MAX, I64_MIN)
    v[np.flatnonzero(grp == 3)[0]] = I64_MIN    # one extreme among ordinary values
    v[np.flatnonzero(grp == 4)[-1]] = I64_MAX
    f = rng.integers(-50, 50, n).astype(np.float64)
    f[np.flatnonzero(grp == 5)[::3]] = np.inf   # +inf among finite values (no −inf beside it: the sum is +inf in any order)
    f[np.flatnonzero(grp == 6)[::2]] = -np.inf
    f[grp == 7] = -0.0                          # a group of nothing but −0.0 (compared with ==: the device reports +0.0)
    f[grp == 8] = 5e-324 * rng.integers(1, 1000, (grp == 8).sum())   # subnormals: their sums are exact
    f[grp == 9] = 1e308                         # overflows to +inf in any order
    f[grp == 10] = -1e308
    f[np.flatnonzero(grp == 11)[1::2]] = -0.0   # −0.0 among small integers
    out.append(Case("extremes-int64_limits_and_special_floats", "extremes", [keyed_record(g, seed=0, f=f).set_column(3, "v", pa.array(v))], grids=(1, 2, 0)))
    # NULLs in the aggregated columns: scattered, on wave and lane edges, a group of nothing but NULLs (its SUM, MIN and MAX read 0)
    v2 = rng.integers(1, 1000, n)
    null = rng.random(n) < 0.2
    null[[0, 3, 4, 255, 256, n - 1]] = True
    null[grp == 12] = True
    null[grp == 13] = False
    out.append(Case("extremes-nulls_in_the_aggregated_column", "extremes", [keyed_record(g, seed=0).set_column(3, "v", pa.array(v2, mask=null)).set_column(4, "f", pa.array((v2 % 97 - 48).astype(np.float64), mask=null))],
                    grids=(1, 2, 0)))
    # general floats: SUM(f) against math.fsum within (n − 1) · 2^-53 · Σ|v| per group
    f3 = rng.normal(0, 1, n) * 10.0 ** rng.integers(-8, 9, n)
    out.append(Case("extremes-general_floats_against_fsum", "extremes", [keyed_record(g, seed=0, f=f3)], aggs=("sum_f",), grids=(1, 2, 0), fsum=True))
    return out


# -- run_counts: the Finish kernels at their block edges (default grid: every row its own key → run i is row i) ------------------------------------
RUN_COUNTS = (1, 255, 256, 257, 1023, 1024, 1025, 4096, 4097)
BLOCK_EDGES = (256, 1024, 4096)   # 256-thread blocks (runs_map / runs_flags / runs_expand), 1 024-element scan blocks (scan_u32), a chunk's worth


def run_counts_cases():
    out = []
    for n in RUN_COUNTS:
        out.append(Case("run_counts-%d_runs" % n, "run_counts", [keyed_record(np.arange(n) * 3, seed=700 + n)], claims=("runs=%d" % n,)))
        for e in BLOCK_EDGES:
            if e < n:  # rows e − 1 and e lie in two waves: equal keys there are two runs of one group, on either side of the block edge
                g = np.arange(n) * 3
                g[e:] -= 3
                out.append(Case("run_counts-%d_runs_one_group_across_run_%d" % (n, e), "run_counts", [keyed_record(g, seed=710 + n)], aggs=("sum_i", "sum_f", "max", "count"),
                                claims=("runs=%d" % n, "two_chunks")))
    g = np.arange(1025) * 3
    g[300:] -= 3
    out.append(Case("run_counts-a_group_in_two_segments", "run_counts", cut(keyed_record(g, seed=720), (300,)), claims=("runs=1025",)))
    # a one-run group (runs_expand_kernel's plain store) between groups of 3 and 4 runs (its atomics): 600 rows, 1 row, 700 rows
    out.append(Case("run_counts-a_one_run_group_between_many_run_groups", "run_counts", [keyed_record(runs_to_keys([600, 1, 700, 1, 1, 300]), seed=730)], claims=("runs=12",)))
    # NULL keys, last in every column: the largest value of every column is NULL
    gn = sorted_sample((4, 5, 6), 1025, 740, always=(119, 118, 113, 89))
    out.append(Case("run_counts-null_keys_sort_last", "run_counts", [keyed_record(gn, (4, 5, 6), seed=741, null_last=True)], aggs=("sum_i", "count")))
    return out


# -- violation: exactly one out-of-order pair -----------------------------------------------------------------------------------------------------
def swapped(n, i):
    """0, 3, 6 … with the keys of rows i − 1 and i exchanged: (i − 1, i) is the one pair out of order"""
    g = np.arange(n) * 3
    g[[i - 1, i]] = g[[i, i - 1]]
    return g


def violation_cases():
    out = []
    for force, tag in ((None, "narrow"), ("1", "wide")):
        aggs = ("sum_i", "min") if force is None else ("sum_i",)
        out.append(Case("violation-%s_in_order" % tag, "violation", [keyed_record(np.arange(600) * 3, seed=800)], aggs=aggs, force=force))
        out.append(Case("violation-%s_at_run_256" % tag, "violation", [keyed_record(swapped(600, 256), seed=801)], aggs=aggs, force=force, in_order=False))
        out.append(Case("violation-%s_as_the_last_pair" % tag, "violation", [keyed_record(swapped(600, 599), seed=802)], aggs=aggs, force=force, in_order=False))
        out.append(Case("violation-%s_between_two_segments" % tag, "violation", cut(keyed_record(swapped(600, 300), seed=803), (300,)), aggs=aggs, force=force, in_order=False))
        out.append(Case("violation-%s_in_the_32nd_column_only" % tag, "violation", [keyed_record(swapped(600, 411), (200, 200, 200), cols=32, seed=804)], aggs=("sum_i",), force=force, in_order=False))
        out.append(Case("violation-%s_32_columns_in_order" % tag, "violation", [keyed_record(np.arange(600) * 3, (200, 200, 200), cols=32, seed=805)], aggs=("sum_i",), force=force))
        # column 2 counts 0 … 5 with 5 = NULL; rows 4 and 5 exchanged: (0, 0, 3), (0, 0, NULL), (0, 0, 4), (0, 1, 0) — "NULL, then the value 4"
        gn = np.arange(120)
        gn[[4, 5]] = gn[[5, 4]]
        out.append(Case("violation-%s_null_then_a_value" % tag, "violation", [keyed_record(gn, (4, 5, 6), seed=806, null_last=True)], aggs=("sum_i",), force=force, in_order=False))
        out.append(Case("violation-%s_null_keys_in_order" % tag, "violation", [keyed_record(np.arange(120), (4, 5, 6), seed=807, null_last=True)], aggs=("sum_i",), force=force))
    return out


# -- translate: two ordered plans merged as runs ---------------------------------------------------------------------------------------------------
def translate_cases():
    out = []
    for dest_most, tag in ((200, "narrow"), (300, "medium")):
        for n in (255, 256, 257):
            rng = np.random.default_rng(900 + n + dest_most)
            sizes = (3, dest_most, 5)
            gd = sorted_sample(sizes, 900, 910 + n)
            xd = radix_keys(gd, sizes)
            dest = record([dict_col(3, xd[0], order=rng.permutation(3)), dict_col(dest_most, xd[1], order=rng.permutation(dest_most)), dict_col(5, xd[2], order=rng.permutation(5))], values_for(900, 911))
            # the source: n rows, every one its own key, over values the destination partly lacks (column 1 has 230 values, 30 beyond the narrow destination's)
            ssz = (3, 230, 7)
            gs = np.sort(rng.choice(3 * 230 * 7, n, replace=False))
            xs = radix_keys(gs, ssz)
            src = record([dict_col(3, xs[0], order=rng.permutation(3)), dict_col(230, xs[1], order=rng.permutation(230)), dict_col(7, xs[2], order=rng.permutation(7))], values_for(n, 912))
            out.append(Case("translate-%d_runs_into_a_%s_destination" % (n, tag), "translate", [dest], aggs=("sum_i", "min", "count"), source=[src], in_order=False,
                            claims=("source_runs=%d" % n, "format_%d" % (0 if tag == "narrow" else 1))))
    return out


# -- many_runs: the second round of scan_u64_single_kernel ----------------------------------------------------------------------------------------
MANY_RUNS = 1024 * 1024 + 1   # more than 1 024 scan blocks of 1 024 runs


def many_runs_cases():
    return [Case("many_runs-%d_rows_every_one_its_own_key" % MANY_RUNS, "many_runs", [keyed_record(np.arange(MANY_RUNS), (102, 102, 102), seed=1000)], aggs=("sum_i",), claims=("runs=%d" % MANY_RUNS,))]


@functools.lru_cache(maxsize=None)
def cases(family):
    """The cases of one family (built once per process: the records are shared and must be left unchanged)"""
    return tuple({"per_tile_k": per_tile_cases, "edges": edges_cases, "filter": filter_cases, "formats": formats_cases, "segments": segments_cases, "extremes": extremes_cases,
                  "run_counts": run_counts_cases, "violation": violation_cases, "translate": translate_cases, "many_runs": many_runs_cases}[family]())


def all_cases(families=FAMILIES):
    return [c for f in families for c in cases(f)]
