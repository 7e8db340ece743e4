"""The expected result of the device MergeRecords (fdb_batches_merge) over pyarrow records: the STABLE order of the concatenation
records[0] ‖ records[1] ‖ … under the reference's comparison as tests/sort_oracle.py restates it (pairwise, column by column, in Python),
cut to `limit` rows when limit > 0. It shares no code with the library: no keys, no ranks, no merge path.

For inputs that are each ordered by the sorting columns this is what a k-way merge that breaks ties by record, then by row, produces —
one of the orders arrowutils.MergeRecords (container/heap, no promise about ties) may give, and the one the library promises.

Dictionary and plain string / binary columns are decoded before anything is compared or concatenated, so inputs with different
dictionaries concatenate, and the expected record holds plain values."""
import pyarrow as pa

from tests import sort_oracle


def decoded(col: pa.Array) -> pa.Array:
    """The column without its dictionary; string-like values as binary (they compare, and are compared, by their bytes)."""
    if isinstance(col, pa.ChunkedArray):
        col = col.combine_chunks()
    if pa.types.is_dictionary(col.type):
        col = col.dictionary_decode()
    t = col.type
    if pa.types.is_string(t) or pa.types.is_large_string(t) or pa.types.is_large_binary(t):
        col = col.cast(pa.binary())
    return col


def decoded_record(record: pa.RecordBatch) -> pa.RecordBatch:
    return pa.RecordBatch.from_arrays([decoded(c) for c in record.columns], names=record.schema.names)


def concatenation(records) -> pa.RecordBatch:
    recs = [decoded_record(r) for r in records]
    names = recs[0].schema.names
    assert all(r.schema.names == names for r in recs)
    return pa.RecordBatch.from_arrays([pa.concat_arrays([r.column(k) for r in recs]) for k in range(len(names))], names=names)


def is_ordered(record: pa.RecordBatch, columns) -> bool:
    return sort_oracle.sort_indices(decoded_record(record), columns) == list(range(record.num_rows))


def merge_indices(records, columns, limit: int = 0):
    """Rows of the concatenation, in output order. `columns`: (index[, descending[, nulls_first]]) by position, as for sort_oracle."""
    order = sort_oracle.sort_indices(concatenation(records), columns)
    return order[:limit] if limit > 0 else order


def merge(records, columns, limit: int = 0) -> pa.RecordBatch:
    """The expected record, dictionaries decoded."""
    order = merge_indices(records, columns, limit)
    return concatenation(records).take(pa.array(order, type=pa.int64()))
