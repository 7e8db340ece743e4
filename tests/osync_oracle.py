"""The expected results of the merge of records with differing field lists (fdb_batches_merge_named) and of the OrderedSynchronizer on
top of it, over pyarrow records. A restatement of OrderedSynchronizer.ensureSameSchema / Callback / Finish
(query/physicalplan/ordered_synchronizer.go:59-241) that shares no code with the library: the schema rules over Python lists, absent
columns as real `pa.nulls` arrays, the merge by tests/merge_oracle.py (pairwise comparison of the concatenation), the rounds by counting.

Where the library deviates from the reference this file states the library's promise: leftover fields in first-seen order (the reference
iterates a Go map), no field twice (the reference duplicates sorting columns among the leftovers when there are several expressions), a
direction and NULL placement per expression, rounds that answer instead of blocking, a round's records merged in input order."""
import pyarrow as pa

from tests import merge_oracle


def normalize(order_by):
    """[(name, dynamic, descending, nulls_first)] from `Col` / `DynCol`-like objects (.name, .dynamic), bare names, or
    (expr[, descending[, nulls_first]]) tuples."""
    if isinstance(order_by, str) or hasattr(order_by, "name"):
        order_by = [order_by]
    out = []
    for o in order_by:
        o = tuple(o) if isinstance(o, (tuple, list)) else (o,)
        expr = o[0]
        name, dynamic = (expr, False) if isinstance(expr, str) else (expr.name, bool(expr.dynamic))
        out.append((name, dynamic, bool(len(o) > 1 and o[1]), bool(len(o) > 2 and o[2])))
    return out


def matches(name, dynamic, field):
    """logicalplan.Column.MatchColumn / DynamicColumn.MatchColumn (expr.go:353-355, :564-566)"""
    return field.startswith(name + ".") if dynamic else field == name


def unify_fields(field_lists, order_by):
    """The schema rules over lists of (name, type-like). Returns (names, n_sort, sort_exprs): the unified column order, how many leading
    columns sort, and for each of those the order expression it matched. Raises ValueError where the library refuses."""
    order = normalize(order_by)
    first_seen = {}
    for r, fields in enumerate(field_lists):
        names = [n for n, _ in fields]
        for n in names:
            if names.count(n) > 1:
                raise ValueError("found multiple fields for name %s" % n)
        for n, t in fields:
            if n in first_seen and first_seen[n][1] != t:
                raise ValueError("field %s differs between records %d and %d" % (n, first_seen[n][0], r))
            first_seen.setdefault(n, (r, t))
    out, sort_exprs = [], []
    for e, (name, dynamic, _, _) in enumerate(order):
        found = sorted((n for n in first_seen if n not in out and matches(name, dynamic, n)), key=lambda n: n.encode("utf-8"))  # sort.Strings
        out += found
        sort_exprs += [e] * len(found)
    n_sort = len(out)
    out += [n for n in first_seen if n not in out]  # (dict order = first-seen order)
    return out, n_sort, sort_exprs


def unify(records, order_by):
    """→ (pa.Schema of the unified columns — each with the type of its first occurrence —, sorting columns as merge_oracle wants them:
    [(position, descending, nulls_first)])"""
    order = normalize(order_by)
    lists = [[(f.name, f.type) for f in r.schema] for r in records]
    names, n_sort, sort_exprs = unify_fields(lists, order_by)
    types = {}
    for fields in lists:
        for n, t in fields:
            types.setdefault(n, t)
    schema = pa.schema([pa.field(n, types[n]) for n in names])
    return schema, [(k, order[sort_exprs[k]][2], order[sort_exprs[k]][3]) for k in range(n_sort)]


def pad(record: pa.RecordBatch, schema: pa.Schema) -> pa.RecordBatch:
    """`record` with the schema's columns in the schema's order; a column it lacks is all NULL (≙ MakeVirtualNullArray)."""
    cols = []
    for f in schema:
        k = record.schema.get_field_index(f.name)
        cols.append(record.column(k) if k >= 0 else pa.nulls(record.num_rows, f.type))
    return pa.RecordBatch.from_arrays(cols, schema=pa.schema([pa.field(f.name, c.type) for f, c in zip(schema, cols)]))


def merge(records, order_by, limit: int = 0) -> pa.RecordBatch:
    """The expected record (dictionaries decoded): merge_oracle.merge over the padded records; under an empty key, or for a single
    record, the concatenation in input order."""
    schema, columns = unify(records, order_by)
    padded = [pad(r, schema) for r in records]
    if columns and len(records) > 1:
        return merge_oracle.merge(padded, columns, limit)
    whole = merge_oracle.concatenation(padded)
    return whole.slice(0, limit) if limit > 0 else whole


class Rounds:
    """The synchronizer's counting: who waits, who runs, when a round is complete. push / finish return the list of (input, record) of
    the round they complete (in input order) or None; StateError where the library answers FDB_ERR_STATE."""

    class StateError(Exception):
        pass

    def __init__(self, inputs):
        self.parked = {}
        self.finished = set()
        self.inputs = inputs

    @property
    def running(self):
        return self.inputs - len(self.finished)

    def _complete(self):
        round_ = sorted(self.parked.items())
        self.parked = {}
        return round_

    def push(self, i, record):
        if i in self.finished or i in self.parked:
            raise Rounds.StateError(i)
        self.parked[i] = record
        return self._complete() if len(self.parked) == self.running else None

    def finish(self, i):
        """→ (round or None, done)"""
        if self.running == 0 or i in self.finished or i in self.parked:
            raise Rounds.StateError(i)
        self.finished.add(i)
        if self.running > 0 and self.running == len(self.parked):
            return self._complete(), False
        return None, self.running == 0
