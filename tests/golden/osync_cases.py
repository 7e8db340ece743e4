"""The reference's vectors for records of differing schemas and for the OrderedSynchronizer, as data.

ENSURE_SAME_SCHEMA — TestEnsureSameSchema (pqarrow/arrowutils/schema_test.go:14-91): three records of int64 fields — record1 has
Field1, Field2; record2 has Field1, Field3; record3 has all three — and the six rows the reference reads back after giving every record
the fields it lacks. A row of `records` lists the record's own fields in its own order; a row of `expected` is (Field1, Field2, Field3)
with None where the record lacks the field: the reference's reader shows 0 there (the zero value of int64 under a NULL of the virtual
NULL array), so the expected VALUE under an absent field is 0 and its validity is NULL.

ORDERED_SYNCHRONIZER — the parameters of TestOrderedSynchronizer (query/physicalplan/ordered_synchronizer_test.go:19-88): 8 inputs feed
one synchronizer ordered by one int64 column; inputs 0 and 4 (`inputI % (inputs / 2) == 0`) call Finish without ever calling Callback;
the other six draw consecutive values from one ascending source (the reference: 0 … 9999) and push each as a one-row record until the
source is dry, then call Finish; everything the synchronizer emits, concatenated, is the source in order."""

SCHEMA_FILE = "pqarrow/arrowutils/schema_test.go"
OSYNC_FILE = "query/physicalplan/ordered_synchronizer_test.go"

ENSURE_SAME_SCHEMA = dict(
    cite=f"{SCHEMA_FILE}:14-91",
    fields=["Field1", "Field2", "Field3"],
    records=[
        dict(fields=["Field1", "Field2"], rows=[(1, 2), (1, 3)]),
        dict(fields=["Field1", "Field3"], rows=[(1, 2), (1, 3)]),
        dict(fields=["Field1", "Field2", "Field3"], rows=[(1, 1, 1), (2, 2, 2)]),
    ],
    expected=[
        (1, 2, None), (1, 3, None),  # record1
        (1, None, 2), (1, None, 3),  # record2
        (1, 1, 1), (2, 2, 2),        # record3
    ],
    value_under_absent=0,
)

ORDERED_SYNCHRONIZER = dict(
    cite=f"{OSYNC_FILE}:19-88",
    inputs=8,
    order_by="colName",
    finish_without_pushing=[0, 4],
    reference_source_len=10000,
)
