"""Cases for the kernels of fdb_merge.hip — hash_merge_wave_kernel<TABLE_SRC>, hash_partition_wave_kernel<PASS>, partition_bases_kernel —
and, beside every case, the LAUNCH SHAPE it claims to produce: which template instance runs, whether the tuple is translated in place
(`alias`) or through two tiles, fetched as 16-byte quads or word by word, through id LUTs or not, how many waves a workgroup has, how
much dynamic LDS it asks for, how many waves the launch has, how full the source table is. The kernels' branches hang on the column
order of the records, the order of the dictionary values, the column count and the row count; a case says here which side it lands on,
tests/test_hash_merge_cases_cpu.py checks that the families together reach every side, and tests/test_gpu_hash_merge.py runs the cases
on the device against the oracle.

The shapes are computed by a Python RESTATEMENT of the host arithmetic (class PlanModel and the functions in front of it); every part
names the lines it restates. It can drift from the C++: when fdb_hash.cpp or fdb_merge.hip change how a launch is shaped, the
restatement has to follow, or the coverage it promises is of the old code.

No test lives here. `cases(family)` is the one generator both test modules run; it is seeded and deterministic. Every count is a number
of DISTINCT GROUPS; a record has about 2–4 rows per group, except where the claimed table size fixes the row count (a fresh table is
sized from the ROWS of its first scan, so load 0.5 of 65 536 slots takes 32 768 rows of 32 768 groups)."""
import functools
from collections import Counter, namedtuple

import numpy as np
import pyarrow as pa

from frostdb_amd.logicalplan import Col, Count, DynCol, Max, Min, Sum

CUS = 256                  # MI355X; fdb_scan_default_grid returns the device's CU count
MIN_SLOTS = 1 << 16        # hash_reserve's floor
MAX_PARTS = 64             # FDB_MAX_PARTS
MAX_DENSE_GCOLS = 8        # FDB_MAX_DENSE_GCOLS
DENSE_KEY_SPACE = 1 << 22  # push_batches: a larger key space goes to the hash table
PART_EXTRA = MAX_PARTS * 8  # FDB_PART_EXTRA: a wave's row positions, one per partition
FAMILIES = ("widths", "layouts", "counts", "packed", "reducers", "exports")


# ---- the host arithmetic, restated ------------------------------------------------------------------------------------------------------
def next_pow2(v):
    p = 1
    while p < v:
        p <<= 1
    return p


def hash_layout(kinds, n_aggs):
    """Plan::hash_layout (fdb_hash.cpp:36-61). kinds: 0 dictionary column (1 word), 1 int64 / uint64 / bool column (2 words).
    → (word of every column, words used, key words, entry words)"""
    kw, words = 4, []
    for k in kinds:
        words.append(kw)
        kw += 1 if k == 0 else 2
    return words, kw, (kw + 3) & ~3, (3 + n_aggs + 3) // 4 * 4


def merge_reach(cols, in_stride_words, key_words):
    """Plan::hash_merge_args (fdb_hash.cpp:186-194). cols: (kind, word, src_word) per DESTINATION column. → (in_words, same_layout)"""
    reach, same = 2, True
    for kind, word, src_word in cols:
        if src_word != word:
            same = False
        if src_word >= 0:
            reach = max(reach, src_word + (1 if kind == 0 else 2))
    in_words = min((reach + 3) & ~3, in_stride_words)
    return in_words, same and in_words <= key_words


def wave_lds_bytes(in_words, out_words, alias):
    """fdb_merge.hip, wave_lds_bytes: the tiles, the slot queue, the inserting lanes' slots and lanes"""
    return 4 * 64 * (max(in_words, out_words) if alias else in_words + out_words) + 128 * 8 + 64 * 8 + 64 * 4


def geometry(per_wave, batches, cus=CUS):
    """fdb_merge.hip, geometry → (waves per workgroup, workgroups, dynamic LDS bytes)"""
    waves = max(1, min(4, (40 << 10) // per_wave))
    lds = per_wave * waves
    per_cu = max(1, min(4, (156 << 10) // (lds + 64)))
    blocks = max(1, min((cus // 2) * per_cu, (batches + waves - 1) // waves))
    return waves, blocks, lds


def quads_ok(stride_words, in_words):
    """fdb_merge.hip, quads_ok (the allocator's base addresses are 16-byte aligned)"""
    return stride_words % 4 == 0 and in_words % 4 == 0


def table_batches(capacity):
    """fdb_launch_hash_merge / part_plan: sixteen 64-slot batches per wave of a table source"""
    return ((capacity + 63) // 64) // 16 + 1


def merge_launch(table_src, in_words, key_words, same_layout, stride_words, batches):
    """fdb_launch_hash_merge (fdb_merge.hip)"""
    in_words = max(2, in_words)
    alias = bool(same_layout) and in_words <= key_words
    waves, blocks, lds = geometry(wave_lds_bytes(in_words, key_words, alias), batches)
    return dict(kernel="merge", table_src=int(table_src), in_words=in_words, out_words=key_words, alias=int(alias), quads=int(quads_ok(stride_words, in_words)),
                waves=waves, lds=lds, launch_waves=waves * blocks)


def partition_launch(in_words, key_words, row_words, same_layout, capacity):
    """part_plan (fdb_merge.hip): both passes share it"""
    in_words = max(2, in_words)
    alias = bool(same_layout) and in_words <= row_words
    waves, blocks, lds = geometry(wave_lds_bytes(in_words, row_words, alias) + PART_EXTRA, table_batches(capacity))
    return dict(kernel="partition", table_src=1, in_words=in_words, out_words=row_words, alias=int(alias), quads=int(quads_ok(key_words, in_words)),
                waves=waves, lds=lds, launch_waves=waves * blocks)


def packed_row_words(dst_key_words, n_vals):
    """fdb_packed_row_words (fdb_kernels.h)"""
    return (dst_key_words + 2 * n_vals + 3) & ~3


class PlanModel:
    """What a plan's host side knows when it shapes a launch: its group columns in the field order of the first records that bring them,
    each dictionary column's values in order of first appearance (key id = position + 1), dense or hash mode, the table's capacity and
    group count. Every method that launches one of the kernels under test appends the launch's shape to `shapes`."""

    def __init__(self, n_aggs, shapes):
        self.n_aggs, self.shapes = n_aggs, shapes
        self.cols = []          # [name, kind, values]
        self.hash = False       # TableMode
        self.cap = 0            # h_capacity_ (0: no table)
        self.kw = self.used = 0
        self.ew = (3 + n_aggs + 3) // 4 * 4
        self.groups = 0         # what hash_groups() would read
        self.bound = 0          # h_groups_bound_
        self.stale = False      # h_bound_stale_
        self.dirty = False      # state_dirty_

    def kinds(self):
        return [c[1] for c in self.cols]

    def words(self):
        return hash_layout(self.kinds(), self.n_aggs)[0]

    def adopt(self, name, kind, values):
        """resolve_batch / merge_hash_tables / hash_export / seed_groups: → (column index, key id of every value in `values`)"""
        for gi, c in enumerate(self.cols):
            if c[0] == name:
                break
        else:
            gi = len(self.cols)
            self.cols.append([name, kind, []])
        c = self.cols[gi]
        assert c[1] == kind, name
        ids = []
        if kind == 0:
            known = {v: i + 1 for i, v in enumerate(c[2])}
            for v in values:
                if v not in known:
                    c[2].append(v)
                    known[v] = len(c[2])
                ids.append(known[v])
        return gi, ids

    def layout(self):
        """hash_layout: a table that gains a column is re-hashed, into wider tuples or — the column landing on tail padding — into the
        same width with the new words zero; the launch shapes depend on neither"""
        _, self.used, self.kw, _ = hash_layout(self.kinds(), self.n_aggs)

    def reserve(self, extra, expected=0):
        """hash_reserve (fdb_hash.cpp:71-96)"""
        need = next_pow2(max(2 * (max(self.bound, expected) + extra), MIN_SLOTS))
        if self.cap != 0 and need <= self.cap:
            return
        if self.cap != 0 and self.bound > 0 and expected == 0:
            need *= 2
        self.cap = need

    def wants_hash(self):
        """push_batches (fdb_plan.cpp:1418-1427)"""
        space = 1
        for _, kind, values in self.cols:
            if kind != 0:
                return True
            space *= len(values) + 1
        return len(self.cols) > MAX_DENSE_GCOLS or space > DENSE_KEY_SPACE

    def switch_to_hash(self):
        """switch_to_hash (fdb_hash.cpp:210-244): the occupied dense slots leave as packed rows of 2 + (columns the plan has NOW) words"""
        n = self.groups if self.dirty else 0
        self.hash = True
        self.layout()
        self.bound = 0
        self.reserve(max(n, 1))
        if n > 0:
            in_kw = 2 + len(self.cols)
            cols = [(k, w, 2 + c if k == 0 else -1) for c, (k, w) in enumerate(zip(self.kinds(), self.words()))]
            self.packed_rows_launch(cols, in_kw, n, lut=False, why="migrate", groups_now=0)  # (into the fresh table)

    def packed_rows_launch(self, cols, in_kw, n, lut, why, groups_now):
        """hash_insert_entries + hash_merge_device (fdb_hash.cpp:159-207); groups_now: what the table holds (hash_groups)"""
        self.bound = groups_now
        self.reserve(n)
        in_words, same = merge_reach(cols, in_kw, self.kw)
        s = merge_launch(False, in_words, self.kw, same, in_kw, (n + 63) // 64)
        s.update(why=why, lut=int(lut), absent=int(any(sw < 0 for _, _, sw in cols)), incoming=n, entry_words=self.ew, src_load=None)
        self.shapes.append(s)

    def push(self, rec, groups_after):
        """push_batch of one resident record: resolve_batch, the mode decision, push_hash's reservation for one chunk"""
        for name, kind, values in rec.key_fields:
            self.adopt(name, kind, values)
        if rec.batch.num_rows == 0:
            return
        if not self.hash and self.wants_hash():
            self.switch_to_hash()
        if self.hash:
            self.layout()
            rows = rec.batch.num_rows
            assert rows < 1 << 20  # (one chunk: fdb_hash.cpp:381-450)
            room = self.cap // 2 - self.bound if self.cap // 2 > self.bound else 0
            if room < rows and self.cap != 0 and self.stale:
                self.bound, self.stale = self.groups, False
                room = self.cap // 2 - self.bound if self.cap // 2 > self.bound else 0
            if room < rows:
                self.reserve(rows)
            self.bound += rows
            self.stale = True
        self.groups = groups_after
        self.dirty = True

    def merge(self, src, groups_after):
        """merge_from (fdb_plan.cpp:2123-2143) → merge_hash / merge_hash_tables (fdb_hash.cpp:1182-1319)"""
        assert self.hash or src.hash, "dense into dense does not reach fdb_merge.hip"
        if not src.dirty:
            return
        kw_before, used_before = (self.kw, self.used) if self.cap != 0 else (None, None)
        if src.hash:
            src.layout()
            if not self.hash:
                    self.switch_to_hash()
            n_src = src.groups if src.cap != 0 else 0
        else:
            n_src = src.groups
            if n_src == 0:
                return
        cols_of, lut = {}, False
        src_words = src.words() if src.hash else None
        w = 2
        for sc, (name, kind, values) in enumerate(src.cols):
            gi, ids = self.adopt(name, kind, values)
            identity = ids == list(range(1, len(ids) + 1))
            if kind == 0 and not (src.hash and identity):  # (packed rows of a dense source always come with a LUT: fdb_hash.cpp:1314)
                lut = True
            cols_of[gi] = src_words[sc] if src.hash else w
            w += 1 if kind == 0 else 2
        if not src.hash and not self.hash:
            self.switch_to_hash()
        self.layout()
        cols = [(k, wd, cols_of.get(c, -1)) for c, (k, wd) in enumerate(zip(self.kinds(), self.words()))]
        if src.hash:
            if n_src == 0:
                self.reserve(0)
                return
            self.bound = self.groups
            self.reserve(n_src)
            in_words, same = merge_reach(cols, src.kw, self.kw)
            s = merge_launch(True, in_words, self.kw, same, src.kw, table_batches(src.cap))
            s.update(why="merge", lut=int(lut), absent=int(any(sw < 0 for _, _, sw in cols)), incoming=n_src, entry_words=self.ew, src_load=n_src / src.cap,
                     kw_before=kw_before, kw_after=self.kw, used_before=used_before, used_after=self.used)
            self.shapes.append(s)
            self.bound += n_src
            self.stale = True
        else:
            self.packed_rows_launch(cols, w, n_src, lut=lut, why="dense_into_hash", groups_now=self.groups)
            self.shapes[-1].update(kw_before=kw_before, kw_after=self.kw, used_before=used_before, used_after=self.used)
        self.groups = groups_after
        self.dirty = True

    def seed(self, schema):
        """seed_groups (fdb_hash.cpp:994-1034). schema: [(name, kind, values)]"""
        if not self.hash:
            self.switch_to_hash()
        for name, kind, values in schema:
            self.adopt(name, kind, values)
        self.layout()
        self.reserve(0)

    def export(self, layout, n_parts):
        """hash_export (fdb_hash.cpp:1036-1125): `in_words`, `same_layout` and `same_ids` are lines 1104-1113"""
        assert 1 <= n_parts <= MAX_PARTS
        if not self.hash:
            self.switch_to_hash()
        self.layout()
        self.reserve(0)
        maps = [layout.adopt(name, kind, values) for name, kind, values in self.cols]
        layout.layout()
        lwords = layout.words()
        dkw = layout.kw
        row_words = packed_row_words(dkw, 1 + self.n_aggs)
        if self.groups == 0:
            return
        in_words = min((self.used + 3) & ~3, self.kw)
        same = dkw >= in_words and len(layout.cols) == len(self.cols)
        for (gi, _), word in zip(maps, self.words()):
            if lwords[gi] != word:
                same = False
        same_ids = same and all(gi == sc and ids == list(range(1, len(ids) + 1)) for sc, (gi, ids) in enumerate(maps))
        s = partition_launch(in_words, self.kw, row_words, same, self.cap)
        s.update(why="export", same_ids=int(same_ids), n_parts=n_parts, incoming=self.groups, entry_words=self.ew, src_load=self.groups / self.cap, lut=None, absent=0)
        self.shapes.append(s)

    def imported(self):
        """hash_import (fdb_hash.cpp:1127-1177): packed rows in the owner's own layout — in place, quads, no LUT; their number is the hash's"""
        s = merge_launch(False, self.kw, self.kw, True, packed_row_words(self.kw, 1 + self.n_aggs), 1)
        s.update(why="import", lut=0, absent=0, incoming=None, entry_words=self.ew, src_load=None, launch_waves=None)
        self.shapes.append(s)


# ---- records ------------------------------------------------------------------------------------------------------------------------------
# A key space: `n_dict` dictionary columns labels.l00 …, then the wide columns (name, "i64" | "u64" | "bool"). Group g's tuple: the
# dictionary columns are the digits of g in base `card` (as many as it takes to tell `span` groups apart), the columns after them a
# hash of g; a wide column is an injective non-zero function of g (the hash table files an int64 key 0 under NULL's fingerprint, as the
# reference does — fdb_kernels.hip:823 — so no case holds both), bool keys its low bit.
Space = namedtuple("Space", "n_dict wide card span nulls")
Rec = namedtuple("Rec", "batch key_fields codes")  # key_fields: [(name, kind 0 | 1, dictionary values)] in field order; codes: {name: int64 per row, 0 = NULL}
ARROW = {"i64": pa.int64(), "u64": pa.uint64(), "bool": pa.bool_()}


def space(n_dict, wide=(), span=1 << 18, card=None, nulls=False):
    if card is None:
        card = 4 if n_dict >= 9 else 3
        while n_dict and card ** min(n_dict, 9) < span:
            card += 1
    return Space(n_dict, tuple(wide), card, span, nulls)


def dict_name(j):
    return "labels.l%02d" % j


def column_names(sp):
    return [dict_name(j) for j in range(sp.n_dict)] + [n for n, _ in sp.wide]


def digits(sp, j, g):
    telling = 1
    while sp.card ** telling < sp.span:
        telling += 1
    d = (g // sp.card ** j) % sp.card if j < telling else (g * (j + 3) + j) % sp.card
    if sp.nulls:  # about one id in eight of every column is NULL (digit −1), by a hash of (g, j) that the telling digits do not share
        d = np.where(((g * 2654435761 + j * 40503) >> 9) % 8 == 0, -1, d)
    return d


def wide_values(sp, i, kind, g):
    if kind == "bool":
        return (g & 1).astype(np.int64)
    if kind == "u64":
        return ((g % 1000) + 1).astype(np.int64) << 53
    v = (g + 1) * (0x100000001 if i % 2 else 1) * (-1 if i % 3 == 2 else 1)  # high words, negative values
    return v.astype(np.int64)


def make_record(sp, gids, seed, fields=None, dict_order="natural", wide_null=False, value_sign=0):
    """A record over the groups `gids` (one row each, in this order). `fields`: the key columns it carries, in field order (default: all).
    dict_order "permuted": every dictionary lists two values no row uses, then the space's values backwards.
    wide_null: every eighth group's wide keys are NULL. value_sign: +1 / −1 makes `value` ≥ 0 / < 0 (for filters)."""
    rng = np.random.default_rng(seed)
    g = np.asarray(gids, dtype=np.int64)
    n = len(g)
    fields = column_names(sp) if fields is None else list(fields)
    arrays, key_fields, codes = [], [], {}
    kinds = dict(sp.wide)
    for name in fields:
        if name in kinds:
            i = [w for w, _ in sp.wide].index(name)
            v = wide_values(sp, i, kinds[name], g)
            null = (g * 40503 + i) % 8 == 3 if wide_null else np.zeros(n, bool)
            if kinds[name] == "bool":
                arrays.append(pa.array(v.astype(bool), type=pa.bool_(), mask=null))
                codes[name] = np.where(null, 0, v + 1)
            else:
                arrays.append(pa.array(v.view(np.uint64) if kinds[name] == "u64" else v, type=ARROW[kinds[name]], mask=null))
                codes[name] = np.where(null, 0, v)
            key_fields.append((name, 1, []))
        else:
            j = int(name[-2:])
            d = digits(sp, j, g)
            values = [b"l%02d=%03d" % (j, k) for k in range(sp.card)]
            idx = np.where(d < 0, 0, d)
            if dict_order == "permuted":
                values = [b"l%02d=x0" % j, b"l%02d=x1" % j] + values[::-1]
                idx = 2 + (sp.card - 1 - idx)
            arrays.append(pa.DictionaryArray.from_arrays(pa.array(idx.astype(np.uint32), mask=d < 0), pa.array(values, type=pa.binary())))
            codes[name] = d + 1
            key_fields.append((name, 0, values))
    value = rng.integers(-100, 100, n)
    if value_sign:
        value = value_sign * np.abs(value) - (1 if value_sign < 0 else 0)
    arrays += [pa.array(value.astype(np.int64)), pa.array(rng.integers(-50, 50, n).astype(np.float64))]  # (small integers as float64: SUM is exact in any order)
    return Rec(pa.RecordBatch.from_arrays(arrays, names=fields + ["value", "floatvalue"]), key_fields, codes)


def rows_over(groups, per_group, seed):
    """`per_group` rows of every group of `groups`, shuffled"""
    g = np.repeat(np.asarray(groups, dtype=np.int64), per_group)
    np.random.default_rng(seed).shuffle(g)
    return g


def distinct_groups(recs, names, selected=None):
    """Distinct key tuples over the rows of `recs` (a column a record lacks is NULL there) — numpy's count, the oracle is held to it"""
    mats = []
    for r in recs:
        n = r.batch.num_rows
        m = np.stack([r.codes.get(c, np.zeros(n, np.int64)) for c in names], axis=1) if names else np.zeros((n, 0), np.int64)
        if selected is not None:
            m = m[selected(r)]
        mats.append(m)
    m = np.concatenate(mats) if mats else np.zeros((0, len(names)), np.int64)
    if len(m) == 0:
        return 0
    key = np.zeros(len(m), np.int64)  # rows → dense ranks, column by column (a lexicographic sort of wide rows is slow)
    for c in range(m.shape[1]):
        values, inv = np.unique(m[:, c], return_inverse=True)
        if len(values) > 1:
            key = np.unique(key * len(values) + inv, return_inverse=True)[1]
    return int(key.max()) + 1


# ---- cases --------------------------------------------------------------------------------------------------------------------------------
COUNT_SUM = (Count(Col("value")), Sum(Col("value")))
EVERY_REDUCER = (Count(Col("value")), Sum(Col("value")), Sum(Col("floatvalue")), Min(Col("value")), Max(Col("value")), Min(Col("floatvalue")), Max(Col("floatvalue")))


class Case:
    """op "merge" / "dense_into_hash": plan A scans `dst`, plan B scans `srcs[0]`, A.Merge(B). "migrate": one plan scans `dst` record by
    record. "export_import": plan s scans `srcs[s]` and exports for `n_parts` owners seeded with the unified schema; owner p imports
    region p of every source. `shapes`: the launches of fdb_merge.hip's kernels the case claims, in order; `groups`: distinct groups of
    the whole case; `src_groups`: of each source."""

    def __init__(self, id, family, op, names, dst=(), srcs=(), aggs=COUNT_SUM, n_parts=0, filt=None, final_stage=False, raw=None):
        self.id, self.family, self.op, self.names = id, family, op, list(names)
        self.dst, self.srcs, self.aggs, self.n_parts = list(dst), [list(s) for s in srcs], list(aggs), n_parts
        self.filt, self.final_stage = filt, final_stage
        self.raw = raw  # final-stage plans scan partial results: the oracle gets the raw records these came from
        self.matchers = [DynCol("labels")] + [Col(n) for n in self.names if not n.startswith("labels.")]
        self.shapes = []
        count = lambda recs: distinct_groups(recs, self.names, (lambda r: selected(self, r)) if filt is not None else None)  # noqa: E731
        self.groups = count(self.oracle_recs())
        self.src_groups = [count(s) for s in self.srcs]
        self.dst_groups = count(self.dst)
        n_aggs = len(self.aggs)
        if op == "migrate":
            a = PlanModel(n_aggs, self.shapes)
            for i, r in enumerate(self.dst):
                a.push(r, count(self.dst[: i + 1]))
        elif op in ("merge", "dense_into_hash"):
            a, b = PlanModel(n_aggs, self.shapes), PlanModel(n_aggs, self.shapes)
            for i, r in enumerate(self.dst):
                a.push(r, count(self.dst[: i + 1]))
            for i, r in enumerate(self.srcs[0]):
                b.push(r, count(self.srcs[0][: i + 1]))
            a.merge(b, self.groups)
        elif op == "export_import":
            plans = []
            for s in self.srcs:
                p = PlanModel(n_aggs, self.shapes)
                for i, r in enumerate(s):
                    p.push(r, count(s[: i + 1]))
                plans.append(p)
            owner = PlanModel(n_aggs, self.shapes)
            owner.seed(unified_schema(plans))
            for p in plans:
                p.export(owner, n_parts)
            owner.imported()

    def oracle_recs(self):
        return self.raw if self.raw is not None else self.dst + [r for s in self.srcs for r in s]

    def all_records(self):
        """The records the oracle answers for: every row of the case, the key columns in the case's one order. The reference hashes a
        row's key columns in the record's field order (aggregate.go:245-247, hashCombine is not commutative) and its records always carry
        them sorted by name; the library keys a group by its columns' NAMES, so a source whose fields come in another order still means
        the same groups — which is what the reversed-fields cases are about."""
        out = []
        for r in self.oracle_recs():
            have = r.batch.schema.names
            out.append(r.batch.select([n for n in self.names if n in have] + [n for n in have if n not in self.names]))
        return out

    def out_columns(self):
        return self.names + [a.Name() for a in self.aggs]

    def __repr__(self):
        return self.id


def selected(case, rec):
    """The rows of `rec` the case's filter keeps (the one filter the cases use is value >= 0)"""
    if case.filt is None:
        return np.ones(rec.batch.num_rows, bool)
    return rec.batch.column(rec.batch.schema.get_field_index("value")).to_numpy() >= 0


def unified_schema(plans):
    """distributed.unify_group_schemas: columns first seen first, a column's values first seen first"""
    model = PlanModel(0, [])
    for p in plans:
        for name, kind, values in p.cols:
            model.adopt(name, kind, values)
    return [(n, k, list(v)) for n, k, v in model.cols]


def halves(n, base=0):
    """(destination groups, source groups): n each, half of them shared"""
    return np.arange(base, base + n), np.arange(base + n // 2, base + n // 2 + n)


def table_pair(id, family, sp, dst_groups, src_groups, seed, **kw):
    """table → table: both plans hold hash tables over the whole space; 3 rows per group. `fields`, `dict_order`: of the source's record"""
    src_kw = {k: kw.pop(k) for k in ("fields", "dict_order", "wide_null") if k in kw}
    dst = [make_record(sp, rows_over(dst_groups, 3, seed), seed + 1, wide_null=src_kw.get("wide_null", False))] if len(dst_groups) else []
    src = [make_record(sp, rows_over(src_groups, 3, seed + 2), seed + 3, **src_kw)] if len(src_groups) else []
    return Case(id, family, "merge", column_names(sp), dst, [src], **kw)


def widths_cases():
    out = []
    shapes = [("1_int64", space(0, [("bucket", "i64")])), ("9_dict", space(9)), ("12_dict", space(12)), ("13_dict", space(13)), ("28_dict", space(28)),
              ("29_dict", space(29)), ("64_dict", space(64)), ("10_dict_int64_uint64_bool", space(10, [("bucket", "i64"), ("shard", "u64"), ("flag", "bool")])),
              ("64_int64", space(0, [("k%02d" % i, "i64") for i in range(64)]))]
    for i, (name, sp) in enumerate(shapes):
        d, s = halves(3000)
        out.append(table_pair("widths-" + name, "widths", sp, d, s, 100 + 10 * i))
    return out


def layouts_cases():
    sp = space(12, [("bucket", "i64")])
    names = column_names(sp)
    d, s = halves(3000)
    out = [table_pair("layouts-same_order_same_dictionaries", "layouts", sp, d, s, 200),
           table_pair("layouts-permuted_larger_dictionaries", "layouts", sp, d, s, 210, dict_order="permuted"),
           table_pair("layouts-reversed_fields", "layouts", sp, d, s, 220, fields=names[::-1]),
           table_pair("layouts-source_lacks_two_columns", "layouts", sp, d, s, 230, fields=names[:10] + names[12:])]
    # the source brings a 13th dictionary column, NULL in none of its rows: none of its groups is one of the destination's
    sp13 = space(13)
    dst = [make_record(sp13, rows_over(d, 3, 240), 241, fields=column_names(sp13)[:12])]
    src = [make_record(sp13, rows_over(s, 3, 242), 243)]
    out.append(Case("layouts-source_brings_a_13th_column", "layouts", "merge", column_names(sp13), dst, [src]))
    # … and a 10th column beside nine: 13 → 14 words of 16, the new column lands on what was the tuples' tail padding — which the
    # specialised scan does not write, so hash_layout has to (tests/test_gpu_hash_merge.py runs this one behind that scan as well)
    sp10 = space(10)
    dst = [make_record(sp10, rows_over(d, 3, 244), 245, fields=column_names(sp10)[:9])]
    src = [make_record(sp10, rows_over(s, 3, 246), 247)]
    out.append(Case("layouts-source_brings_a_10th_column_onto_the_padding", "layouts", "merge", column_names(sp10), dst, [src]))
    sp64 = space(0, [("k%02d" % i, "i64") for i in range(64)])
    out.append(table_pair("layouts-64_int64_reversed_fields", "layouts", sp64, d, s, 250, fields=column_names(sp64)[::-1]))
    spn = space(12, [("bucket", "i64")], nulls=True)
    out.append(table_pair("layouts-null_ids_and_null_int64_keys", "layouts", spn, d, s, 260, wide_null=True))
    # NULL int64 keys beside valid ones that are never 0, and a permuted dictionary on top: NULL ids must stay NULL through the LUT
    out.append(table_pair("layouts-nulls_through_the_lut", "layouts", spn, d, s, 270, wide_null=True, dict_order="permuted"))
    return out


def counts_cases():
    sp = space(12)
    out = []
    d = np.arange(3000)
    # a source plan that never scanned anything, and one whose filter selected nothing (its table exists and is empty)
    out.append(Case("counts-0_no_table", "counts", "merge", column_names(sp), [make_record(sp, rows_over(d, 3, 300), 301)], [[]]))
    out.append(Case("counts-0_filter_selects_nothing", "counts", "merge", column_names(sp), [make_record(sp, rows_over(d, 3, 302), 303, value_sign=1)],
                    [[make_record(sp, rows_over(d, 3, 304), 305, value_sign=-1)]], filt=Col("value") >= 0))
    for i, n in enumerate((1, 63, 64, 65, 127, 128, 129)):  # half of the incoming groups are the destination's
        out.append(table_pair("counts-%d_into_3000_half_shared" % n, "counts", sp, np.arange(3000), np.arange(3000 - n // 2, 3000 - n // 2 + n), 310 + 4 * i))
    for kind in ("empty", "identical", "disjoint", "half_shared"):
        for n in (65, 32768):
            src = np.arange(n)
            dst = {"empty": np.arange(0), "identical": src, "disjoint": src + n, "half_shared": src + n // 2}[kind]
            seed = 400 + 8 * len(out)
            if n == 32768:  # one row per group: 32 768 rows size the tables at 65 536 slots, load 0.5
                dr = [make_record(sp, rows_over(dst, 1, seed), seed + 1)] if len(dst) else []
                out.append(Case("counts-32768_into_%s" % kind, "counts", "merge", column_names(sp), dr, [[make_record(sp, rows_over(src, 1, seed + 2), seed + 3)]]))
            else:
                out.append(table_pair("counts-65_into_%s" % kind, "counts", sp, dst, src, seed))
    # 70 000 groups in 105 000 rows: 2^18 slots, 260 waves
    src = np.arange(35_000, 105_000)
    g = np.concatenate([src, src[:35_000]])
    np.random.default_rng(490).shuffle(g)
    out.append(Case("counts-70000_into_70000_half_shared", "counts", "merge", column_names(sp),
                    [make_record(sp, np.random.default_rng(491).permutation(np.concatenate([np.arange(70_000), np.arange(35_000)])), 492)], [[make_record(sp, g, 493)]]))
    return out


def packed_cases():
    out = []
    sp12 = space(12, span=1 << 13)
    for k in (1, 2, 3, 4, 8):
        for n in (1, 63, 64, 65, 4097):
            seed = 500 + 40 * k + (n % 37)
            # the dense source's columns are the destination's first k: its groups have NULL in the other 12 − k, the destination's never do
            sps = Space(k, (), space(k, span=4097).card, 4097, False)
            dst = make_record(sp12, rows_over(np.arange(3000), 3, seed), seed + 1)
            src = make_record(sps, rows_over(np.arange(n), 3, seed + 2), seed + 3)
            out.append(Case("packed-dense_%d_columns_%d_groups_into_hash" % (k, n), "packed", "dense_into_hash", column_names(sp12), [dst], [[src]]))
            # migration: a dense plan of k label columns meets a record with an int64 key on top
            spm = Space(k, (("bucket", "i64"),), sps.card, 4097, False)
            first = make_record(spm, rows_over(np.arange(n), 3, seed + 6), seed + 7, fields=column_names(spm)[:k])
            second = make_record(spm, rows_over(np.arange(n // 2, n // 2 + 200), 2, seed + 8), seed + 9)
            out.append(Case("packed-migrate_%d_columns_%d_groups" % (k, n), "packed", "migrate", column_names(spm), [first, second]))
    return out


def reducers_cases():
    sp = space(12)
    d, s = halves(3000)
    out = [table_pair("reducers-count_alone", "reducers", sp, d, s, 600, aggs=(Count(Col("value")),)),
           table_pair("reducers-every_reducer", "reducers", sp, d, s, 610, aggs=EVERY_REDUCER),
           table_pair("reducers-eight_aggregations", "reducers", sp, d, s, 620, aggs=(Count(Col("floatvalue")),) + EVERY_REDUCER),
           # the same reducers over packed rows: atomics instead of plain stores where the group is already there
           Case("reducers-every_reducer_from_a_dense_source", "reducers", "dense_into_hash", column_names(sp),
                [make_record(sp, rows_over(d, 3, 630), 631)],
                [[make_record(sp, rows_over(np.arange(200), 3, 632), 633, fields=column_names(sp)[:4])]], aggs=EVERY_REDUCER)]
    return out


def final_stage_case(partial_of):
    """Two final-stage plans scan the partial results of two partial plans (`partial_of(records, aggs, matchers)` → record: the oracle's
    partial aggregate) and are merged: COUNT's accumulator is a sum. The oracle's answer is over the raw records."""
    sp = space(12)
    d, s = halves(3000)
    aggs = (Count(Col("value")), Sum(Col("value")), Min(Col("value")), Max(Col("floatvalue")))
    raw = [make_record(sp, rows_over(d, 3, 640), 641), make_record(sp, rows_over(s, 3, 642), 643)]
    parts = []
    for r in raw:
        b = partial_of([r.batch], list(aggs), [DynCol("labels")])
        key_fields, codes = [], {}
        for i, f in enumerate(b.schema):
            if f.name.startswith("labels."):
                values = b.column(i).dictionary.to_pylist()
                key_fields.append((f.name, 0, values))
                digit = np.array([int(v.split(b"=")[1]) + 1 for v in values], dtype=np.int64)
                codes[f.name] = np.where(b.column(i).is_null().to_numpy(zero_copy_only=False), 0, digit[b.column(i).indices.fill_null(0).to_numpy()])
        parts.append(Rec(b, key_fields, codes))
    return Case("reducers-final_stage_destination", "reducers", "merge", column_names(sp), [parts[0]], [[parts[1]]], aggs=aggs, final_stage=True, raw=raw)


EXPORT_PARTS = (1, 2, 3, 15, 16, 17, 32, 33, 63, 64)


def source_record(sp, n, seed, base=0, **kw):
    """n groups from `base` on; 3 rows per group, except where the rows size the table: 32 768 groups in 32 768 rows (65 536 slots, load
    0.5), 70 000 in 105 000 (2^18 slots)"""
    g = np.arange(base, base + n)
    if n == 32768:
        rows = rows_over(g, 1, seed)
    elif n == 70_000:
        rows = np.random.default_rng(seed).permutation(np.concatenate([g, g[:35_000]]))
    else:
        rows = rows_over(g, 3, seed)
    return make_record(sp, rows, seed + 1, **kw)


def exports_cases():
    sp = space(12)
    names = column_names(sp)
    out = []
    for P in EXPORT_PARTS:
        out.append(Case("exports-3000_groups_%d_parts" % P, "exports", "export_import", names, srcs=[[source_record(sp, 3000, 700 + P)]], n_parts=P))
    for n in (1, 65, 32768, 70_000):
        for P in (17, 64):
            out.append(Case("exports-%d_groups_%d_parts" % (n, P), "exports", "export_import", names, srcs=[[source_record(sp, n, 800 + P + n % 91)]], n_parts=P))
    two = lambda seed, **kw: [[source_record(sp, 3000, seed)], [source_record(sp, 3000, seed + 2, base=1500, **kw)]]  # noqa: E731
    out.append(Case("exports-two_sources_equal_dictionaries", "exports", "export_import", names, srcs=two(900), n_parts=17))
    out.append(Case("exports-two_sources_permuted_dictionaries", "exports", "export_import", names, srcs=two(910, dict_order="permuted"), n_parts=17))
    out.append(Case("exports-two_sources_reversed_fields", "exports", "export_import", names, srcs=two(920, fields=names[::-1]), n_parts=17))
    sp13 = space(13)
    out.append(Case("exports-one_source_with_an_extra_column", "exports", "export_import", column_names(sp13),
                    srcs=[[source_record(sp13, 3000, 930, fields=names)], [source_record(sp13, 3000, 932, base=1500)]], n_parts=17))
    return out


@functools.lru_cache(maxsize=None)
def cases(family):
    """The cases of one family (built once per process: the records are shared and must be left unchanged)"""
    if family == "reducers":
        return tuple(reducers_cases() + [final_stage_case(oracle_partial)])
    return tuple({"widths": widths_cases, "layouts": layouts_cases, "counts": counts_cases, "packed": packed_cases, "exports": exports_cases}[family]())


def all_cases():
    return [c for f in FAMILIES for c in cases(f)]


# ---- the oracle's answers, computed once per process --------------------------------------------------------------------------------------
def oracle_partial(records, aggs, matchers):
    return oracle_partial_filtered(records, None, aggs, matchers)


def oracle_partial_filtered(records, filt, aggs, matchers):
    from oracle import OraclePlan
    o = OraclePlan(filt, aggs, matchers)
    for r in records:
        o.push(r)
    out = o.finish().to_arrow()
    o.close()
    return out


def record_rows(batch, columns):
    """A result record as a multiset of rows over `columns` (a column the record lacks is NULL); dictionary columns by value"""
    n = batch.num_rows
    cols = []
    for c in columns:
        i = batch.schema.get_field_index(c)
        if i < 0:
            cols.append([None] * n)
            continue
        a = batch.column(i)
        if pa.types.is_dictionary(a.type):
            values = np.array(a.dictionary.to_pylist() + [None], dtype=object)
            idx = a.indices.fill_null(len(values) - 1).to_numpy().astype(np.int64)
            cols.append(values[idx].tolist())
        else:
            cols.append(a.to_pylist())
    return Counter(zip(*cols)) if n else Counter()


def oracle_rows_of(records, filt, aggs, matchers, columns):
    """The oracle's result over `records` as a multiset of rows over `columns`"""
    return record_rows(oracle_partial_filtered(records, filt, aggs, matchers), columns)


_WANT = {}


def oracle_rows(case):
    if case.id not in _WANT:
        _WANT[case.id] = oracle_rows_of(case.all_records(), case.filt, case.aggs, case.matchers, case.out_columns())
    return _WANT[case.id]
