"""Cases for what feeds the hash table and what empties it — the specialised fdb_hash_kernel (fdb_jitgen.cpp), the interpreting
scan_hash_kernel, push_hash's chunk walk, hash_reserve → hash_rehash_kernel, and the device Finish of a table (hash_chunk_counts /
hash_gather_rows / group_rows_to_columns / present_ids / rank_ids, the transport widths and slices of finish_columns_hash,
hash_compact_kernel behind fetch_compact_hash) — and, beside every case, the CLAIM of which branch it takes: per push the chunk list,
the capacity afterwards, whether a re-hash ran and the key words before and after; per record and column an identity / LDS / global
key-id LUT; canonical or not; the quads stored with one 16-byte store; the kernel's name per variant; for Finish the group count, the
slice count, every column's transport width before and after the present-id pass, the columns that ship a bitmap and, where a case
puts its one NULL group on a chosen row of the result, that row (home_slot restates the fingerprint's low half: Finish emits in slot order).

The claims are computed by a Python RESTATEMENT of the host arithmetic (class ScanModel and finish_claim); every part names the lines
it restates. It can drift from the C++: when fdb_hash.cpp changes how a push is chunked, a table grown, a LUT placed or a width chosen,
the restatement has to follow, or the coverage it promises is of the old code. Not restated: the cardinality estimate of push_hash
(fdb_hash.cpp:395-405, only reached after 2^20 rows with the table out of room — ScanModel refuses such a case).

The EXPECTED ROWS come from a plain numpy group-by in this file (`reference`), not from the oracle: np.unique for the groups, bincount /
add.at / minimum.at / maximum.at for the reducers. All data are integers — int64 values, float64 values that are small integers — so
every partial sum is exact in any order and every output column is compared exactly. A NULL in an aggregated column counts as a row and
contributes the builder's zeroed slot, 0, to SUM, MIN and MAX, as in the reference.

No test lives here. `cases(family)` is the one generator both test modules run; it is seeded and deterministic.
tests/test_hash_scan_cases_cpu.py pins the restatement on hand-worked claims, holds the families to claiming every side of every branch
and the reference to the oracle; tests/test_gpu_hash_scan.py runs the cases on the device in both variants and checks what of a claim
can be observed: the kernel's name, the launch count, the group count, the result's schema and NULL counts.

Hash mode is reached on purpose; `why_hash` says how: an int64 / uint64 / bool / computed key, 9 or more dictionary columns, a key
space above 2^22 (two dictionaries of 2 048 values: 2 049² > 2^22), or exact sums (such a plan lives in the table from its first row).
An int64 key that is NULL and one that is 0 hash alike and the inserting row decides which of the two the group shows, so 0 stays out of
nullable wide columns — except in runs-null_and_zero_share_a_group, whose expected key is "NULL or 0" (NULL_OR_ZERO)."""
import functools
from collections import Counter

import numpy as np
import pyarrow as pa

from frostdb_amd.logicalplan import Col, Count, DynCol, Max, Min, Sum
from tests.hash_merge_cases import COUNT_SUM, DENSE_KEY_SPACE, EVERY_REDUCER, MAX_DENSE_GCOLS, MIN_SLOTS, column_names, hash_layout, make_record, next_pow2, record_rows, rows_over, space

FAMILIES = ("rows", "runs", "columns", "luts", "growth", "finish")
FIRST_CHUNK = 1 << 20   # kFirstChunkRows
CHUNK = 4 << 20         # kChunkRows
GROUP = 8               # HashGen::source GROUP, HASH_UNROLL
NULL_OR_ZERO = "NULL or 0"
FIVE = (Count(Col("value")), Sum(Col("value")), Sum(Col("floatvalue")), Min(Col("value")), Max(Col("floatvalue")))
THREE = COUNT_SUM + (Sum(Col("floatvalue")),)


# ---- the host arithmetic, restated ------------------------------------------------------------------------------------------------------
def key_fields(batch, matched):
    """resolve_batch (fdb_plan.cpp:1203-1237): the matched fields in the record's field order → [(name, kind, dictionary values, has validity)]"""
    out = []
    for i, f in enumerate(batch.schema):
        if not matched(f.name):
            continue
        a = batch.column(i)
        if pa.types.is_dictionary(f.type):
            out.append((f.name, 0, a.dictionary.to_pylist(), a.null_count > 0))
        else:
            out.append((f.name, 1, [], a.null_count > 0))
    return out


def lut_places(luts, predicate_bytes=0):
    """push_hash's LUT placement (fdb_hash.cpp:293-317). luts: per column None (a wide key) or the key id of every dictionary entry →
    ("identity" | "lds" | "global" | None per column, bytes of LDS)"""
    off, out = predicate_bytes, []
    for L in luts:
        if L is None:
            out.append(None)
        elif len(L) > 0 and L == list(range(1, len(L) + 1)):
            out.append("identity")
        elif 4 * len(L) <= 8192 and off + 4 * len(L) <= 60 * 1024:
            out.append("lds")
            off = (off + 4 * len(L) + 15) & ~15
        else:
            out.append("global")
    return out, (off + 15) & ~15


def stored_quads(kinds, words, canonical):
    """HashGen::emit_tuple_stores (fdb_jitgen.cpp, "stores: aligned quads …"): inside every group of 8 columns, four dictionary columns that
    start on a word divisible by 4 leave as one 16-byte store — in a canonical record only. → first column of every such quad"""
    out = []
    if not canonical:
        return out
    for c0 in range(0, len(kinds), GROUP):
        c1, c = min(len(kinds), c0 + GROUP), c0
        while c + 4 <= c1:
            if words[c] % 4 == 0 and kinds[c:c + 4] == [0, 0, 0, 0]:
                out.append(c)
                c += 4
            else:
                c += 1
    return out


class ScanModel:
    """What the host side of one plan knows from push to push (push_batches' mode decision, switch_to_hash on a plan without state,
    hash_layout, push_hash). `push` returns the claim of one record."""

    def __init__(self, n_aggs, exact=False):
        self.n_aggs, self.exact = n_aggs, exact
        self.cols = []          # [name, kind, values]
        self.hash = exact       # set_exact_sums: TableMode::HASH from the start (fdb_hash.cpp:99-107)
        self.cap = self.bound = self.seen = self.launches = 0
        self.stale = False
        self.kw = self.used = 0

    def kinds(self):
        return [c[1] for c in self.cols]

    def room(self):
        return self.cap // 2 - self.bound if self.cap and self.cap // 2 > self.bound else 0

    def reserve(self, extra):
        """hash_reserve without an estimate (fdb_hash.cpp:71-96) → whether a re-hash ran"""
        need = next_pow2(max(2 * (self.bound + extra), MIN_SLOTS))
        if self.cap and need <= self.cap:
            return False
        if self.cap and self.bound > 0:
            need *= 2
        rehash, self.cap = self.cap != 0, need
        return rehash

    def push(self, fields, rows, groups_at, predicate_bytes=0):
        """fields: key_fields of the record (computed keys last); groups_at(r): the groups in the table once rows [0, r) of this record
        are in — what hash_groups() reads when push_hash refreshes its bound in front of row r."""
        luts, present = [], []
        for name, kind, values, _ in fields:  # resolve_batch: new columns are appended, new values interned in dictionary order
            for gi, c in enumerate(self.cols):
                if c[0] == name:
                    break
            else:
                gi = len(self.cols)
                self.cols.append([name, kind, []])
            c = self.cols[gi]
            assert c[1] == kind, name
            present.append(gi)
            if kind != 0:
                luts.append(None)
                continue
            known = {v: i + 1 for i, v in enumerate(c[2])}
            L = []
            for v in values:
                if v not in known:
                    c[2].append(v)
                    known[v] = len(c[2])
                L.append(known[v])
            luts.append(L)
        claim = dict(rows=rows, chunks=[], rehash=False, layout_rehash=False, refreshed=False, kw_before=self.kw if self.cap else None, used_before=self.used if self.cap else None)
        if rows == 0:  # push_batches: no live record, nothing happens
            claim.update(cap_after=self.cap, kw_after=self.kw, launches=self.launches, lut=[], canonical=None, quads=[])
            return claim
        if not self.hash:  # push_batches (fdb_plan.cpp:1418-1427); the cases reach hash mode with their first rows
            sp = 1
            for _, kind, values in self.cols:
                sp *= len(values) + 1
            assert any(k != 0 for k in self.kinds()) or len(self.cols) > MAX_DENSE_GCOLS or sp > DENSE_KEY_SPACE, "the case would scan into the dense table"
            assert self.seen == 0
            self.hash = True  # switch_to_hash without dense state (fdb_hash.cpp:210-217): layout, bound 0, hash_reserve(1)
            self.bound = 0
            self.reserve(1)
        words, used, kw, _ = hash_layout(self.kinds(), self.n_aggs)  # push_hash: hash_layout()
        if self.cap and self.seen and (kw != self.kw or used > self.used):  # (fdb_hash.cpp:47) — a table that has tuples is re-hashed
            claim["layout_rehash"] = True
        self.kw, self.used = kw, used
        # canonical (fdb_hash.cpp:306-308): every column of the plan, at the plan's words
        w, canonical = 4, len(present) == len(self.cols)
        for gi in present:
            if not canonical:
                break
            canonical = words[gi] == w
            w += 1 if self.cols[gi][1] == 0 else 2
        places, lds = lut_places(luts, predicate_bytes)
        r0 = 0
        while r0 < rows:  # the chunk walk (fdb_hash.cpp:381-450)
            left = rows - r0
            min_chunk = min(left, FIRST_CHUNK if self.seen == 0 and self.bound == 0 else CHUNK)
            room = self.room()
            if room < min_chunk and self.cap and self.stale:
                self.bound, self.stale = groups_at(r0), False
                claim["refreshed"] = True
                room = self.room()
            if room < min_chunk:
                assert self.stale or self.seen < 1 << 20 or self.bound == 0, "the cardinality estimate is not restated"
                claim["rehash"] = self.reserve(min_chunk) or claim["rehash"]
                room = self.room()
            if room < left:
                room &= ~1023
            r1 = r0 + min(left, room)
            assert r1 > r0
            claim["chunks"].append((r0, r1))
            self.bound += r1 - r0
            self.stale = True
            self.seen += r1 - r0
            self.launches += 1
            r0 = r1
        claim.update(cap_after=self.cap, kw_after=self.kw, used_after=self.used, launches=self.launches, lut=places, lds_lut_bytes=lds, canonical=canonical,
                     quads=stored_quads([self.cols[gi][1] for gi in present], [words[gi] for gi in present], canonical), n_cols=len(present),
                     vmask_bits=[gi for gi in present if self.cols[gi][1] != 0], wide_words=[words[gi] for gi in present if self.cols[gi][1] != 0])
        return claim


M64 = (1 << 64) - 1


def fmix64(k):
    """fdb_fmix64 (fdb_kernels.h)"""
    k ^= k >> 33
    k = k * 0xff51afd7ed558ccd & M64
    k ^= k >> 33
    k = k * 0xc4ceb9fe1a85ec53 & M64
    return k ^ k >> 33


def home_slot(ids, mask):
    """The slot a key tuple probes first: the low half of its fingerprint (fdb_fp_k1, fp_add32, fp_add, fp_final, hash_find_or_insert —
    fdb_kernels.h). ids: per plan column ("d", key id, 0 = NULL) or ("w", int64 value | None). Finish emits the groups in slot order."""
    h1 = 0
    for gi, (kind, v) in enumerate(ids):
        k1 = fmix64(0x9E3779B97F4A7C15 * (gi + 1) & M64) | 1
        if kind == "d":
            h1 = (h1 + v * k1) & M64
        elif v:
            h1 = (h1 + (fmix64((v & M64) ^ 0x9FB21C651E98DF25) | 1) * k1) & M64
    return (fmix64((h1 + 0x243F6A8885A308D3) & M64) or 1) & mask


def transport_width(n):
    """finish_columns_hash (fdb_hash.cpp:555-563 by dictionary size, :709-718 by the ids present): negative = bits per index"""
    return -2 if n <= 4 else -4 if n <= 16 else 1 if n <= 256 else 2 if n <= 65536 else 4


def finish_claim(model, rows, names, env):
    """Finish of the model's table holding `rows` (the expected rows): group count, slices (fdb_hash.cpp:549-553), widths, bitmaps (:858-860)"""
    n = len(rows)
    shift = 6
    knob = int(env.get("FDB_FINISH_SLICE_SHIFT", 20))
    while shift < knob and (1 << shift) < n:
        shift += 1
    slices = (n + (1 << shift) - 1) >> shift
    before, after, bitmaps = [], [], []
    min_bytes = int(env.get("FDB_PRESENT_IDS_MIN_BYTES", 32 << 20))
    at_stake = 0
    for name, kind, values in model.cols:
        w = 8 if kind != 0 else transport_width(len(values))
        before.append(w)
        if kind == 0 and w in (1, 2):
            at_stake += n * w
    for c, (name, kind, values) in enumerate(model.cols):
        col = [r[names.index(name)] for r in rows]
        w = before[c]
        if kind == 0 and w in (1, 2) and n > 0 and "FDB_NO_PRESENT_IDS" not in env and at_stake >= min_bytes:
            cnt = len({v for v in col if v is not None})
            nw = -2 if cnt <= 4 else -4 if cnt <= 16 else 1 if cnt <= 256 else w
            w = nw
        after.append(w)
        if any(v is None for v in col):
            bitmaps.append(name)
    return dict(groups=n, slices=slices, slice_rows=1 << shift, width_before=before, width_after=after, bitmaps=bitmaps)


# ---- the reference: a numpy group-by over the records themselves --------------------------------------------------------------------------
def column_codes(batches, name, computed, null_or_zero):
    """Per batch: a code per row (0 = NULL) that is equal exactly where the column's values are, and the values to show"""
    vals, valid, typ = [], [], None
    for b in batches:
        n = b.num_rows
        if name in computed:
            v, ok = computed[name](b)
            typ = "i64"
        else:
            i = b.schema.get_field_index(name)
            if i < 0:
                vals.append(np.zeros(n, np.int64)); valid.append(np.zeros(n, bool))
                continue
            a = b.column(i)
            ok = ~a.is_null().to_numpy(zero_copy_only=False)
            if pa.types.is_dictionary(a.type):
                typ = "dict"
                v = a.indices.fill_null(0).to_numpy().astype(np.int64)
                vals.append(("d", a.dictionary.to_pylist(), v)); valid.append(ok)
                continue
            typ = {pa.int64(): "i64", pa.uint64(): "u64", pa.bool_(): "bool"}[a.type]
            v = a.fill_null(False if typ == "bool" else 0).to_numpy(zero_copy_only=False)
            v = v.astype(np.int64) if typ != "u64" else v.astype(np.uint64).view(np.int64)
        vals.append(v); valid.append(ok)
    if typ == "dict":
        ids, out = {}, []
        for v, ok in zip(vals, valid):
            if isinstance(v, tuple):
                lut = np.array([ids.setdefault(x, len(ids) + 1) for x in v[1]] + [0], dtype=np.int64)
                out.append(np.where(ok, lut[v[2]], 0))
            else:
                out.append(v)
        shown = [None] + sorted(ids, key=ids.get)
        return out, shown
    flat, ok = np.concatenate(vals) if vals else np.zeros(0, np.int64), np.concatenate(valid) if valid else np.zeros(0, bool)
    if null_or_zero:
        ok = ok & (flat != 0)
    uniq, inv = np.unique(flat[ok], return_inverse=True)
    code = np.zeros(len(flat), np.int64)
    code[ok] = inv + 1
    conv = {"i64": int, "u64": lambda x: int(x) & (2 ** 64 - 1), "bool": bool, None: int}[typ]
    shown = [NULL_OR_ZERO if null_or_zero else None] + [conv(x) for x in uniq]
    out, at = [], 0
    for b in batches:
        out.append(code[at:at + b.num_rows]); at += b.num_rows
    return out, shown


def reference(batches, names, aggs, select=None, computed=None, null_or_zero=False):
    """→ (rows as a Counter over names + aggregations, first selected row of every group in scan order, rows selected). Key tuples show
    None for NULL; int64 sums wrap modulo 2^64 (numpy's int64 addition does)."""
    computed = computed or {}
    sel = np.concatenate([np.ones(b.num_rows, bool) if select is None else select(b) for b in batches]) if batches else np.zeros(0, bool)
    gid = np.zeros(len(sel), np.int64)
    shown_of, codes_of = [], []
    for name in names:
        per, shown = column_codes(batches, name, computed, null_or_zero)
        code = np.concatenate(per) if per else np.zeros(0, np.int64)
        codes_of.append(code); shown_of.append(shown)
        gid = np.unique(gid * (len(shown) + 1) + code, return_inverse=True)[1].reshape(-1)  # (dense ranks: at most one per row, no overflow)
    rows_sel = np.flatnonzero(sel)
    if len(rows_sel) == 0:
        return Counter(), np.zeros(0, np.int64), 0
    g, first, inv = np.unique(gid[rows_sel], return_index=True, return_inverse=True)
    inv = inv.reshape(-1)
    n = len(g)
    cols = [[shown_of[c][k] for k in codes_of[c][rows_sel[first]]] for c in range(len(names))]
    for a in aggs:
        fn, col = a.Name().split("(")[0], a.Name().split("(")[1][:-1]
        if fn == "count":
            cols.append(np.bincount(inv, minlength=n).tolist())
            continue
        arr = [b.column(b.schema.get_field_index(col)) for b in batches]
        is_f = pa.types.is_floating(arr[0].type)
        v = np.concatenate([x.fill_null(0.0 if is_f else 0).to_numpy(zero_copy_only=False) for x in arr])[rows_sel]  # NULL ⇒ the builder's zeroed slot
        if fn == "sum":
            acc = np.zeros(n, np.float64 if is_f else np.int64)
            np.add.at(acc, inv, v)
        else:
            acc = np.full(n, (np.inf if fn == "min" else -np.inf) if is_f else (np.iinfo(np.int64).max if fn == "min" else np.iinfo(np.int64).min), v.dtype)
            (np.minimum if fn == "min" else np.maximum).at(acc, inv, v)
        cols.append(acc.tolist())
    return Counter(zip(*cols)), np.sort(rows_sel[first]), len(rows_sel)


# ---- cases --------------------------------------------------------------------------------------------------------------------------------
class Case:
    """`records` are scanned one Callback each by ONE plan. `pushes`: the claim of every record; `groups_after`: the table's groups after
    every record (numpy's count); `finish`: the Finish claim; `want`: the expected rows; `counts`: {key tuple: rows} where the case's
    construction fixes them. `variants`: "jit" (fdb_hash_kernel) and / or "interp" (scan_hash_kernel under FDB_NO_JIT); `kernels`:
    what last_kernel() says per variant — "unsupported" where the interpreting kernel refuses the case: it has no computed keys, the push
    fails with FDB_ERR_UNSUPPORTED. `through`: "finish" (Finish), "resident" (FinishResident → to_arrow), "partial" (partial keys and states).
    `before_rehash`: the push that re-hashes the table — the groups of the records in front of it must survive it. `oracle`: False for the two
    records of 2^20 rows and more, which are checked against the numpy reference alone."""

    def __init__(self, id, family, why_hash, records, aggs, names=None, filt=None, select=None, env=None, exact=False, computed=None, matchers=None,
                 null_or_zero=False, counts=None, variants=("jit", "interp"), oracle=True, predicate_bytes=0, through=("finish",), before_rehash=None):
        self.id, self.family, self.why_hash = id, family, why_hash
        self.records, self.aggs, self.filt, self.select = list(records), list(aggs), filt, select
        self.env, self.exact, self.computed, self.null_or_zero = dict(env or {}), exact, computed or {}, null_or_zero
        self.counts, self.variants, self.oracle, self.through, self.before_rehash = counts, variants, oracle, through, before_rehash
        self.final_stage = False
        if names is None:  # the plan's column order: first seen first, in field order; computed keys behind the stored ones of their record
            names = []
            for b in self.records:
                names += [f for f in b.schema.names if f not in names and f not in ("value", "floatvalue", "timestamp")]
                names += [c for c in self.computed if c not in names]
        self.names = list(names)
        self.matchers = matchers if matchers is not None else [DynCol("labels")] + [Col(n) for n in self.names if not n.startswith("labels.")]
        self.want, first, self.selected = reference(self.records, self.names, self.aggs, select, self.computed, null_or_zero)
        starts = np.cumsum([0] + [b.num_rows for b in self.records])
        model = ScanModel(len(self.aggs), exact)
        self.pushes, self.groups_after = [], []
        matched = lambda n: n in self.names and n not in self.computed  # noqa: E731
        for i, b in enumerate(self.records):
            fields = key_fields(b, matched) + [(c, 1, [], True) for c in self.computed]
            self.pushes.append(model.push(fields, b.num_rows, lambda r, s=starts[i]: int(np.searchsorted(first, s + r)), predicate_bytes or 0))
            # (a filter leaf's LUT goes to LDS in front of the key-id LUTs, place_luts: such a case keeps 16 KiB clear of the 60 KiB limit, so its claims hold wherever they start)
            assert predicate_bytes is not None or self.pushes[-1]["lds_lut_bytes"] + (16 << 10) <= 60 << 10, id
            self.groups_after.append(int(np.searchsorted(first, starts[i + 1])))
        self.model = model
        self.finish = finish_claim(model, list(self.want.elements()), self.out_columns(), self.env)
        self.kernels = {"jit": "fdb_hash_kernel", "interp": "unsupported" if self.computed else "scan_hash_kernel"}

    def out_columns(self):
        return self.names + [a.Name() for a in self.aggs]

    def oracle_records(self):
        """Every record with its key columns in the case's one order (hash_merge_cases.Case.all_records says why)"""
        out = []
        for b in self.records:
            have = b.schema.names
            out.append(b.select([n for n in self.names if n in have] + [n for n in have if n not in self.names]))
        return out

    def normalise(self, rows):
        """NULL-or-0: both kinds of key show as one"""
        if not self.null_or_zero:
            return rows
        wide = [i for i, n in enumerate(self.names) if not n.startswith("labels.")]
        return Counter({tuple(NULL_OR_ZERO if i in wide and (v is None or v == 0) else v for i, v in enumerate(r)): k for r, k in rows.items()})

    def __repr__(self):
        return self.id


def dict_col(values, idx):
    """idx: int array, −1 = NULL"""
    idx = np.asarray(idx)
    return pa.DictionaryArray.from_arrays(pa.array(np.where(idx < 0, 0, idx).astype(np.uint32), mask=idx < 0), pa.array(values, type=pa.binary()))


def i64_col(v, null=None, typ=pa.int64()):
    return pa.array(np.asarray(v), type=typ, mask=None if null is None else np.asarray(null, bool))


def record(keys, value, fvalue, value_null=None, extra=()):
    """keys: [(name, array)]; value / fvalue: integers"""
    cols = list(keys) + [("value", i64_col(value, value_null)), ("floatvalue", pa.array(np.asarray(fvalue, dtype=np.float64)))] + list(extra)
    return pa.RecordBatch.from_arrays([a for _, a in cols], names=[n for n, _ in cols])


def labels(prefix, n):
    return [b"%s=%05d" % (prefix, k) for k in range(n)]


def mark(n, rows):
    m = np.zeros(n, bool)
    m[[r for r in rows if 0 <= r < n]] = True
    return m


# -- rows: 4 rows per lane, 256 per wave, 1 024 per tile ----------------------------------------------------------------------------------------
ROW_COUNTS = (1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2047, 2049, 4097)
EDGE_ROWS = (0, 255, 256, 1023, 1024)
A5, B4 = labels(b"a", 5), labels(b"b", 4)


def rows_record(n, seed, nulls, value=None):
    """about 40 groups: labels.a × labels.b × two int64 buckets; `nulls`: labels.b, bucket and value are NULL on the record's first and last
    row and on rows 255 / 256 / 1 023 / 1 024 (two shapes in all: with and without validity bitmaps; the row count is not part of a shape)"""
    rng = np.random.default_rng(seed)
    g = rng.integers(0, 40, n)
    m = mark(n, EDGE_ROWS + (n - 1,)) if nulls else np.zeros(n, bool)
    value = rng.integers(-100, 100, n) if value is None else value
    return record([("labels.a", dict_col(A5, g % 5)), ("labels.b", dict_col(B4, np.where(m, -1, (g // 5) % 4))), ("bucket", i64_col((g // 20 + 1) * 1000, m if nulls else None))],
                  value, rng.integers(-50, 50, n), m if nulls else None)


def cut(batch, points):
    edges = [0] + list(points) + [batch.num_rows]
    return [batch.slice(a, b - a) for a, b in zip(edges, edges[1:])]


def rows_cases():
    out = []
    why = "an int64 key"
    for nulls in (False, True):
        tag = "nulls" if nulls else "plain"
        for n in ROW_COUNTS:
            out.append(Case("rows-%s_%d" % (tag, n), "rows", why, [rows_record(n, 1000 + n, nulls)], EVERY_REDUCER))
            a = max(1, (n // 2) | 1)
            if a < n:  # two records, the boundary odd; every record carries its own NULL rows
                out.append(Case("rows-%s_%d_in_two" % (tag, n), "rows", why, [rows_record(a, 2000 + n, nulls), rows_record(n - a, 2100 + n, nulls)], EVERY_REDUCER))
            a = max(1, (n // 3) | 1)
            b = a + max(1, ((n - a) // 2) | 1)
            if b < n:
                out.append(Case("rows-%s_%d_in_three" % (tag, n), "rows", why, [rows_record(a, 3000 + n, nulls), rows_record(b - a, 3100 + n, nulls), rows_record(n - b, 3200 + n, nulls)], EVERY_REDUCER))
    # one filter, value > t, at three thresholds over one record of 2 049 rows: wave 1 (rows 256 … 511), lanes 3 and 4 of wave 0 (rows 12 … 19) and
    # lane 0 of the second tile (rows 1 024 … 1 027) hold −50, every other row 1 … 99
    n = 2049
    v = np.random.default_rng(77).integers(1, 100, n)
    v[256:512] = -50; v[12:20] = -50; v[1024:1028] = -50
    rec = rows_record(n, 4000, True, value=v)
    for name, t in (("everything", -51), ("nothing_in_whole_lanes_and_waves", 0), ("nothing_at_all", 1000)):
        out.append(Case("rows-filter_selects_%s" % name, "rows", why, [rec], EVERY_REDUCER, filt=Col("value") > t, select=lambda b, t=t: value_gt(b, t)))
    return out


def value_gt(b, t):
    a = b.column(b.schema.get_field_index("value"))
    return (a.fill_null(0).to_numpy(zero_copy_only=False) > t) & ~a.is_null().to_numpy(zero_copy_only=False)  # (a NULL never matches)


# -- runs: rows ordered by group, the layout given run by run -------------------------------------------------------------------------------------
A50 = labels(b"r", 50)


def runs_record(layout, dropped=(), zero_groups=(), null_groups=()):
    """layout: [(group, rows)] in row order; `dropped`: rows the filter (value > 0) removes. Group g: labels.a = g % 50, bucket = 1000 · (g / 50 + 1)
    (zero_groups: bucket 0; null_groups: bucket NULL)"""
    g = np.concatenate([np.full(k, grp) for grp, k in layout])
    n = len(g)
    rng = np.random.default_rng(n + len(layout))
    v = rng.integers(1, 100, n)
    v[list(dropped)] = -rng.integers(1, 100, len(dropped)) if len(dropped) else 0
    bucket = np.where(np.isin(g, zero_groups), 0, (g // 50 + 1) * 1000)
    null = np.isin(g, null_groups)
    return record([("labels.a", dict_col(A50, g % 50)), ("bucket", i64_col(bucket, null if len(null_groups) else None))], v, rng.integers(-50, 50, n))


def runs_counts(layouts, dropped_of):
    c = Counter()
    for layout, dropped in zip(layouts, dropped_of):
        at = 0
        for grp, k in layout:
            c[(A50[grp % 50], (grp // 50 + 1) * 1000)] += k - sum(1 for r in dropped if at <= r < at + k)
            at += k
    return {k: v for k, v in c.items() if v}


def distinct(lengths, base=0):
    return [(base + i, k) for i, k in enumerate(lengths)]


RUN_LAYOUTS = {
    # (records as run layouts, rows dropped per record)
    "lengths_1_2_3_4_5_8": ([distinct([1, 2, 3, 4, 5, 8] * 3 + [8, 5, 4, 3, 2, 1])], [()]),
    # rows 1 … 7 end on the last row of lane 1, rows 8 … 12 on the first row of lane 3
    "ends_on_a_lanes_last_row_and_on_the_next_lanes_first": ([distinct([1, 7, 5, 3, 4, 4, 1])], [()]),
    # wave 0 is one run; 255 rows end one row before the wave edge at 512, 257 rows cross it and end on wave 2's last row
    "one_wave_and_255_and_257_rows_at_the_wave_edge": ([distinct([256, 255, 257, 256, 3])], [()]),
    "crosses_the_tile_edge_at_row_1024": ([distinct([1000, 48, 100])], [()]),
    "the_whole_record_of_1500_rows": ([distinct([1500])], [()]),
    "equal_keys_that_are_not_adjacent": ([[(0, 3), (1, 2), (0, 3), (2, 4), (3, 4), (2, 4), (4, 256), (5, 1), (4, 256)]], [()]),
    # lane 0 keeps rows 0 and 3 (sel 0b1001), lane 1 rows 4 and 7
    "middle_rows_removed_by_the_filter": ([distinct([8, 4, 3])], [(1, 2, 5, 6)]),
    "through_a_lane_the_filter_empties": ([distinct([12, 9])], [(4, 5, 6, 7, 16, 17, 18, 19)]),
    "ends_in_the_ragged_tail_of_1027_rows": ([distinct([1020, 7])], [()]),
    "the_same_key_ends_one_record_and_starts_the_next": ([[(0, 5), (1, 6)], [(1, 7), (2, 3)]], [(), ()]),
}


def runs_cases():
    out = []
    filt, sel = Col("value") > 0, lambda b: value_gt(b, 0)
    for exact in (False, True):
        for name, (layouts, dropped) in RUN_LAYOUTS.items():
            out.append(Case("runs-%s%s" % (name, "_exact" if exact else ""), "runs", "an int64 key" + (" and exact sums" if exact else ""),
                            [runs_record(l, d) for l, d in zip(layouts, dropped)], EVERY_REDUCER, filt=filt, select=sel, exact=exact, counts=runs_counts(layouts, dropped)))
    # the one case about NULL and 0: groups 0 / 1 share labels.a = r0 … and differ in bucket 0 / NULL only; so do 2 / 3 in the other order
    lay = [(0, 5), (1, 3), (2, 6), (3, 2), (7, 4)]
    rec = runs_record(lay, zero_groups=(0, 3), null_groups=(1, 2))
    a = pa.DictionaryArray.from_arrays(pa.array(np.repeat([0, 0, 1, 1, 2], [5, 3, 6, 2, 4]).astype(np.uint32)), pa.array(A50, type=pa.binary()))
    rec = rec.set_column(0, "labels.a", a)
    out.append(Case("runs-null_and_zero_share_a_group", "runs", "an int64 key", [rec], EVERY_REDUCER, filt=filt, select=sel, null_or_zero=True,
                    counts={(A50[0], NULL_OR_ZERO): 8, (A50[1], NULL_OR_ZERO): 8, (A50[2], 1000): 4}))
    return out


# -- columns: groups of 8, quads, int64 words, vmask bits ---------------------------------------------------------------------------------------
def col_case(id, sp, why, fields_of=None, aggs=FIVE, groups=200, seed=0, variants=("jit", "interp"), **kw):
    recs = []
    for i, fields in enumerate(fields_of or [None]):
        recs.append(make_record(sp, rows_over(np.arange(groups // 2 * i, groups // 2 * i + groups), 3, seed + i), seed + 10 + i, fields=fields, wide_null=bool(sp.wide), **kw).batch)
    return Case("columns-" + id, "columns", why, recs, aggs, variants=variants)


BUCKET = [("bucket", "i64")]


def columns_cases():
    out = []
    for n in (1, 7, 8):
        out.append(col_case("%d_dict_and_int64" % n, space(n, BUCKET, span=512), "an int64 key", seed=5000 + n))
    for n in (9, 12, 16, 17, 31, 32, 33, 63):
        out.append(col_case("%d_dict" % n, space(n, span=512, nulls=True), ">= 9 dictionary columns", seed=5000 + n))
    # 64 columns compile slowest: the specialised variant gets ONE 64-column case, the one with the int64 key on vmask's top bit
    out.append(col_case("64_dict", space(64, span=512, nulls=True), ">= 9 dictionary columns", seed=5064, variants=("interp",)))
    for k in (0, 2, 3):  # (k = 1 is 1_dict_and_int64) the key's two words start at tuple word 4 + k
        out.append(col_case("int64_at_word_%d" % (4 + k), space(k, BUCKET, span=512), "an int64 key", seed=5100 + k))
    for k in (31, 32, 63):  # bit gi of vmask: word 0's top bit, word 1's bottom bit, word 1's top bit
        sp = space(k, BUCKET, span=512, nulls=True)
        out.append(col_case("int64_as_column_%d" % k, sp, "an int64 key", seed=5200 + k))
    out.append(col_case("uint64_and_bool_keys", space(2, [("shard", "u64"), ("flag", "bool")], span=512), "a uint64 and a bool key", seed=5300))
    sp = space(12, span=512, nulls=True)  # (the shapes of 12_dict and 9_dict again: no compile of their own for the canonical records)
    names = column_names(sp)
    out.append(col_case("a_record_lacks_two_columns", sp, ">= 9 dictionary columns", [None, names[:5] + names[7:]], seed=5400))
    out.append(col_case("a_record_with_reversed_fields", sp, ">= 9 dictionary columns", [None, names[::-1]], seed=5410))
    sp13 = space(13, span=512, nulls=True)
    out.append(col_case("a_13th_column_widens_the_tuples", sp13, ">= 9 dictionary columns", [column_names(sp13)[:12], None], seed=5420))
    sp10 = space(10, span=512, nulls=True)
    out.append(col_case("a_10th_column_lands_on_the_padding", sp10, ">= 9 dictionary columns", [column_names(sp10)[:9], None], seed=5430))
    # a computed key: timestamp / 1000 * 1000 beside one dictionary column
    rng = np.random.default_rng(5500)
    n = 600
    ts = rng.integers(1, 20, n) * 500 + rng.integers(0, 500, n)
    rec = record([("labels.a", dict_col(A5, rng.integers(0, 5, n)))], rng.integers(-100, 100, n), rng.integers(-50, 50, n), extra=[("timestamp", i64_col(ts))])
    alias = (Col("timestamp") / 1000 * 1000).Alias("timestamp_bucket")
    out.append(Case("columns-a_computed_key", "columns", "a computed int64 key", [rec], FIVE, matchers=[DynCol("labels"), alias],
                    computed={"timestamp_bucket": lambda b: (b.column(b.schema.get_field_index("timestamp")).to_numpy() // 1000 * 1000, np.ones(b.num_rows, bool))}))
    return out


# -- luts: identity, LDS, global -------------------------------------------------------------------------------------------------------------------
def lut_record(dicts, perms, n, seed, null_every=11):
    """dicts: value lists; perms: per column None (the list as it is) or a permutation of it; rows draw entries uniformly, every 11th is NULL"""
    rng = np.random.default_rng(seed)
    keys = []
    for c, (values, perm) in enumerate(zip(dicts, perms)):
        want = rng.integers(0, len(values), n)  # the VALUE of the row, as an index into `values`
        if perm is None:
            listed, idx = values, want
        else:
            listed = [values[p] for p in perm]
            idx = np.argsort(perm)[want]
        keys.append(("labels.l%02d" % c, dict_col(listed, np.where((np.arange(n) + c) % null_every == 0, -1, idx))))
    return record(keys, rng.integers(-100, 100, n), rng.integers(-50, 50, n))


def luts_cases():
    out = []
    why = "a key space above 2^22"
    for size in (2048, 2049):  # 8 192 bytes: the last LUT that goes to LDS; 8 196: global
        d = [labels(b"x", size), labels(b"y", size)]
        p = [np.random.default_rng(size + c).permutation(size) for c in range(2)]
        q = [np.random.default_rng(size + 9 + c).permutation(size) for c in range(2)]
        out.append(Case("luts-%d_entries_identity_then_two_permutations" % size, "luts", why,
                        [lut_record(d, [None, None], 3000, 6000 + size), lut_record(d, p, 3000, 6100 + size), lut_record(d, q, 3000, 6200 + size)], THREE))
    d = [labels(b"c%d" % c, 2000) for c in range(8)]
    p = [np.random.default_rng(70 + c).permutation(2000) for c in range(8)]
    out.append(Case("luts-eight_permuted_columns_of_2000_entries", "luts", why, [lut_record(d, [None] * 8, 2500, 6300), lut_record(d, p, 2500, 6301)], THREE))
    # filter leaves with LUTs of their own beside the key-id LUTs: != on a dictionary column, and a regex
    d = [labels(b"x", 2048), labels(b"y", 2100)]
    p = [np.random.default_rng(80 + c).permutation(len(d[c])) for c in range(2)]
    recs = [lut_record(d, [None, None], 3000, 6400), lut_record(d, p, 3000, 6401)]

    def decoded(b, name):
        a = b.column(b.schema.get_field_index(name))
        vals = np.array(a.dictionary.to_pylist() + [None], dtype=object)
        return vals[a.indices.fill_null(len(vals) - 1).to_numpy().astype(np.int64)]

    out.append(Case("luts-a_not_equal_leaf_beside_them", "luts", why, recs, THREE, filt=Col("labels.l01") != b"y=00007",
                    select=lambda b: np.array([v is not None and v != b"y=00007" for v in decoded(b, "labels.l01")]), predicate_bytes=None))
    out.append(Case("luts-a_regex_leaf_beside_them", "luts", why, recs, THREE, filt=Col("labels.l01").RegexMatch("y=0001.$"),
                    select=lambda b: np.array([v is not None and v.startswith(b"y=0001") and len(v) == 7 for v in decoded(b, "labels.l01")]), predicate_bytes=None))
    return out


# -- growth: chunks, the pessimistic bound, hash_reserve, the re-hash ------------------------------------------------------------------------------
def growth_record(groups, seed, nulls=()):
    g = np.asarray(groups, dtype=np.int64)
    rng = np.random.default_rng(seed)
    m = mark(len(g), nulls)
    return record([("bucket", i64_col(g + 1, m if len(nulls) else None))], rng.integers(-100, 100, len(g)), rng.integers(-50, 50, len(g)), m if len(nulls) else None)


def growth_cases():
    out = []
    why = "an int64 key"
    out.append(Case("growth-32768_groups_fill_half_of_65536_then_one_more", "growth", why, [growth_record(np.arange(32768), 7000), growth_record([40000], 7001)], THREE, before_rehash=1))
    out.append(Case("growth-four_records_of_10000_distinct_groups", "growth", why, [growth_record(np.arange(10000 * i, 10000 * (i + 1)), 7010 + i) for i in range(4)], THREE, before_rehash=3))
    out.append(Case("growth-four_records_of_10000_rows_in_10_groups", "growth", why, [growth_record(np.arange(10000) % 10, 7020 + i) for i in range(4)], THREE))
    out.append(Case("growth-four_records_of_10000_distinct_groups_exact", "growth", why + " and exact sums", [growth_record(np.arange(10000 * i, 10000 * (i + 1)), 7030 + i) for i in range(4)], THREE,
                    exact=True, before_rehash=3))
    sp10 = space(10, span=1 << 16)
    first = make_record(sp10, np.arange(20000), 7040, fields=column_names(sp10)[:9]).batch
    second = make_record(sp10, np.arange(20000, 40000), 7041).batch
    out.append(Case("growth-a_rehash_after_a_column_was_added", "growth", ">= 9 dictionary columns", [first, second], THREE, before_rehash=1))
    for t in (1, 1025):  # the one big shape: a chunk boundary inside a record (checked against the numpy reference only)
        n = (1 << 20) + t
        g = np.random.default_rng(7050 + t).integers(0, 1000, n)
        out.append(Case("growth-a_record_of_2^20_plus_%d_rows_in_two_chunks" % t, "growth", why, [growth_record(g, 7060 + t, nulls=((1 << 20) - 1, 1 << 20, n - 1))], FIVE, oracle=False))
    return out


# -- finish: 64-slot chunks, rows in groups of 64, widths, slices, bitmaps ---------------------------------------------------------------------
def finish_record(n_groups, seed, dict_sizes=(7,), used=None, null_groups=(), all_null=()):
    """n_groups groups, 2 rows each: bucket = 1000 · (g + 1); dictionary column c has dict_sizes[c] entries of which the rows use `used[c]` (default:
    all it can); null_groups: the groups whose column 0 is NULL; all_null: columns NULL in every row"""
    g = np.repeat(np.arange(n_groups) if np.isscalar(n_groups) else np.asarray(n_groups), 2)
    rng = np.random.default_rng(seed)
    keys = []
    for c, size in enumerate(dict_sizes):
        u = size if used is None else used[c]
        idx = (g * (c + 1)) % u * (size // u)  # (spread over the dictionary: present ids are not a prefix)
        if c == 0:
            idx = np.where(np.isin(g, null_groups), -1, idx)
        if c in all_null:
            idx = np.full(len(g), -1)
        keys.append(("labels.l%02d" % c, dict_col(labels(b"f%d" % c, size), idx)))
    keys.append(("bucket", i64_col((g + 1) * 1000)))  # (the reference's 64-bit group hash, which the oracle restates, merges buckets 673 and 680 beside f0=00000)
    return record(keys, rng.integers(-100, 100, len(g)), rng.integers(-50, 50, len(g)))


def finish_cases():
    out = []
    why = "an int64 key"
    for n in (1, 63, 64, 65, 127, 128, 129, 4097):
        out.append(Case("finish-%d_groups" % n, "finish", why, [finish_record(n, 8000 + n)], EVERY_REDUCER, through=("finish", "resident")))
    for n in (64, 65, 129):
        out.append(Case("finish-%d_groups_in_slices_of_64" % n, "finish", why, [finish_record(n, 8100 + n)], THREE, env={"FDB_FINISH_SLICE_SHIFT": "6"}))
    sizes = (4, 5, 16, 17, 256, 257)
    out.append(Case("finish-dictionaries_of_4_5_16_17_256_257", "finish", why, [finish_record(600, 8200, sizes)], THREE))
    out.append(Case("finish-dictionaries_of_4_5_16_17_256_257_present_ids", "finish", why, [finish_record(600, 8201, sizes)], THREE, env={"FDB_PRESENT_IDS_MIN_BYTES": "0"}))
    out.append(Case("finish-300_entries_of_which_4_5_16_17_256_257_are_used", "finish", why, [finish_record(600, 8202, (300,) * 6, used=sizes)], THREE, env={"FDB_PRESENT_IDS_MIN_BYTES": "0"}))
    out.append(Case("finish-300_entries_no_present_ids", "finish", why, [finish_record(600, 8203, (300,) * 6, used=sizes)], THREE, env={"FDB_PRESENT_IDS_MIN_BYTES": "0", "FDB_NO_PRESENT_IDS": "1"}))
    out.append(Case("finish-a_column_null_in_every_group", "finish", why, [finish_record(65, 8204, (7, 300), all_null=(1,))], THREE, env={"FDB_PRESENT_IDS_MIN_BYTES": "0"}))
    # a column without a NULL beside one with exactly one NULL group (of 1 group: row 0 is the last row too)
    for n in (1, 64, 65):
        out.append(Case("finish-one_null_group_of_%d" % n, "finish", why, [finish_record(n, 8300 + n, (7, 5), null_groups=(n - 1,))], THREE))
    # … and that group on a row of the result chosen here: Finish emits the groups in slot order, and home_slot restates where a key goes.
    # Group g is (f0 = g % 7, f1 = 2 g % 5, bucket = 1000 (g + 1)), f0 NULL in the one group; no two chosen groups share a home slot.
    slot = {g: home_slot([("d", g % 7 + 1), ("d", 2 * g % 5 + 1), ("w", 1000 * (g + 1))], MIN_SLOTS - 1) for g in range(600)}
    g0 = min(range(10), key=lambda g: abs(home_slot([("d", 0), ("d", 2 * g % 5 + 1), ("w", 1000 * (g + 1))], MIN_SLOTS - 1) - MIN_SLOTS // 2))
    s0 = home_slot([("d", 0), ("d", 2 * g0 % 5 + 1), ("w", 1000 * (g0 + 1))], MIN_SLOTS - 1)
    taken, below, above = {s0}, [], []
    for g in range(10, 600):
        if slot[g] not in taken:
            taken.add(slot[g])
            (below if slot[g] < s0 else above).append(g)
    for n, row in ((65, 0), (65, 63), (65, 64), (130, 63), (130, 64), (130, 129)):
        c = Case("finish-the_null_group_of_%d_on_row_%d" % (n, row), "finish", why, [finish_record([g0] + below[:row] + above[:n - 1 - row], 8310 + n + row, (7, 5), null_groups=(g0,))], THREE)
        c.finish["null_row"] = row
        out.append(c)
    out.append(Case("finish-65537_entries_three_used", "finish", why, [finish_record(90, 8400, (65537,), used=(3,))], THREE, env={"FDB_PRESENT_IDS_MIN_BYTES": "0"}))
    for n in (63, 64, 65):
        out.append(Case("finish-partial_keys_and_states_of_%d_groups" % n, "finish", why, [finish_record(n, 8500 + n)], THREE, through=("partial",)))
    return out


@functools.lru_cache(maxsize=None)
def cases(family):
    """The cases of one family (built once per process: the records are shared and must be left unchanged)"""
    return tuple({"rows": rows_cases, "runs": runs_cases, "columns": columns_cases, "luts": luts_cases, "growth": growth_cases, "finish": finish_cases}[family]())


def all_cases():
    return [c for f in FAMILIES for c in cases(f)]


def oracle_rows(case):
    """The oracle's rows for the case (tests/test_hash_scan_cases_cpu.py holds `want` to them)"""
    from tests.hash_merge_cases import oracle_rows_of
    return oracle_rows_of(case.oracle_records(), case.filt, case.aggs, case.matchers, case.out_columns())


__all__ = ["FAMILIES", "cases", "all_cases", "record_rows", "oracle_rows", "NULL_OR_ZERO"]
