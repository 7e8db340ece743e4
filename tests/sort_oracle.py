"""A Python restatement of the reference's record sort (pqarrow/arrowutils/sort.go: multiColSorter.compare :534-564 and Less :517-532)
over a pyarrow.RecordBatch, sorted with Python's STABLE sort through functools.cmp_to_key. It shares nothing with the library: no radix
keys, no ranks — rows are compared pairwise, column by column, exactly as the reference does.

The reference sorts with sort.Sort, which is not stable: where two rows are equal on every sorting column any order is legal there. The
library promises the stable one, so that is what this oracle gives.

Values are compared as Go compares them:
  int64 / uint64 / timestamp     cmp.Compare on the integers
  float64                        cmp.Compare: a NaN is equal to any NaN and less than every non-NaN (so below -Inf); -0.0 == +0.0.
                                 Not numpy's order (NaN last) and not pyarrow's.
  string / binary / dictionary   bytes.Compare on the entry's bytes (Go's string `<` agrees); two dictionary entries with the same bytes
                                 are equal
"""
import functools
import math

import pyarrow as pa

ASCENDING, DESCENDING = 0, 1


def go_cmp(a, b) -> int:
    """cmp.Compare[T] for ordered T (go/src/cmp/cmp.go): -1 if a < b, +1 if a > b, 0 if equal — NaNs first, all equal."""
    if isinstance(a, float) or isinstance(b, float):
        a_nan, b_nan = math.isnan(a), math.isnan(b)
        if a_nan:
            return 0 if b_nan else -1
        if b_nan:
            return 1
    return -1 if a < b else 1 if a > b else 0


def _column_values(col: pa.Array):
    """The column as Python values: None for NULL, bytes for every string-like value, int / float otherwise."""
    if pa.types.is_dictionary(col.type):
        col = col.dictionary_decode()
    if pa.types.is_timestamp(col.type):
        col = col.cast(pa.int64())
    t = col.type
    if not (pa.types.is_integer(t) or pa.types.is_floating(t) or pa.types.is_string(t) or pa.types.is_large_string(t) or pa.types.is_binary(t)
            or pa.types.is_large_binary(t)):
        raise TypeError("unsupported column type for sorting %s" % t)
    vals = col.to_pylist()
    return [v.encode() if isinstance(v, str) else v for v in vals]


def normalize(columns):
    """(index, direction, nulls_first) triples from (index[, descending[, nulls_first]]) tuples or bare indices."""
    out = []
    for c in columns:
        c = (c,) if isinstance(c, int) else tuple(c)
        out.append((int(c[0]), DESCENDING if len(c) > 1 and c[1] else ASCENDING, bool(len(c) > 2 and c[2])))
    return out


def sort_indices(record: pa.RecordBatch, columns):
    """≙ SortRecord(record, columns): the list p with row p[i] of `record` = row i of the sorted record. `columns` index the record's
    columns by position."""
    columns = normalize(columns)
    if not columns:
        raise ValueError("at least one column is needed for sorting")
    if record.num_rows <= 1:  # sort.go:412-417: the columns are not looked at
        return list(range(record.num_rows))
    data = [_column_values(record.column(ix)) for ix, _, _ in columns]
    # Direction.comparison(): the value compare() must return for Less to be true
    want = [-1 if d == ASCENDING else 1 for _, d, _ in columns]
    nulls_first = [nf for _, _, nf in columns]

    def compare(k, i, j):  # multiColSorter.compare
        x = data[k]
        if x[i] is None:
            if x[j] is None:
                return 0
            if want[k] == 1:
                return 1 if nulls_first[k] else -1
            return -1 if nulls_first[k] else 1
        if x[j] is None:
            if want[k] == 1:
                return -1 if nulls_first[k] else 1
            return 1 if nulls_first[k] else -1
        return go_cmp(x[i], x[j])

    def less(i, j):  # multiColSorter.Less
        for k in range(len(columns)):
            c = compare(k, i, j)
            if c != 0:
                return c == want[k]
        return False

    def three_way(i, j):
        # = -1 if less(i, j) else 1 if less(j, i) else 0, in one walk over the columns (compare(k, j, i) == -compare(k, i, j))
        for k in range(len(columns)):
            c = compare(k, i, j)
            if c != 0:
                return -1 if c == want[k] else 1
        return 0

    if record.num_rows <= 64:  # small records: through Less itself, both ways round
        for i in range(record.num_rows):
            for j in range(record.num_rows):
                assert three_way(i, j) == (-1 if less(i, j) else 1 if less(j, i) else 0)

    return sorted(range(record.num_rows), key=functools.cmp_to_key(three_way))
