"""The reference's TestMerge cases as data (pqarrow/arrowutils/merge_test.go:51-241): the rows of every input record, the sorting columns,
the limit and the rows the reference expects.

A row is (number, text): `Number *int64` and `Text *string` of the test's row struct (merge_test.go:17-20), None = nil. The record has
two columns, COLUMNS: a nullable int64 and a nullable plain string (no `rle_dict` tag: records.NewBuild makes a string column, not a
dictionary). A sorting column is (index, direction, nulls_first) with direction 0 = Ascending, 1 = Descending. limit 0 = no limit.

Every expected list is what the stable merge gives too: where two rows tie on the sorting columns (the two 5s of the first four cases)
they are equal in every column, so the order of ties does not show — tests/test_merge_cpu.py checks each case against
tests/merge_oracle.py."""

MERGE_FILE = "pqarrow/arrowutils/merge_test.go"

ASC, DESC = 0, 1

COLUMNS = [("number", "int64"), ("text", "string")]


def n(*numbers):
    """rows that set Number only"""
    return [(v, None) for v in numbers]


CASES = [
    dict(id="merge_ascending", cite=f"{MERGE_FILE}:52-81",
         records=[n(None, 0, 2, 4, 5), n(1, 3, 5, 6, 7)], columns=[(0, ASC, True)], limit=0,
         expected=n(None, 0, 1, 2, 3, 4, 5, 5, 6, 7)),
    dict(id="merge_ascending_limit", cite=f"{MERGE_FILE}:83-106",
         records=[n(None, 0, 2, 4, 5), n(1, 3, 5, 6, 7)], columns=[(0, ASC, True)], limit=3,
         expected=n(None, 0, 1)),
    dict(id="merge_descending", cite=f"{MERGE_FILE}:108-135",
         records=[n(None, 5, 3, 1, 0), n(7, 6, 5, 4)], columns=[(0, DESC, True)], limit=0,
         expected=n(None, 7, 6, 5, 5, 4, 3, 1, 0)),
    dict(id="merge_descending_limit", cite=f"{MERGE_FILE}:137-162",
         records=[n(None, 5, 3, 1, 0), n(7, 6, 5, 4)], columns=[(0, DESC, True)], limit=6,
         expected=n(None, 7, 6, 5, 5, 4)),
    dict(id="multiple_ascending", cite=f"{MERGE_FILE}:164-188",
         records=[[(0, "a"), (0, "c"), (1, "e")], [(None, None), (0, "b"), (1, "d"), (2, "f")]],
         columns=[(0, ASC, True), (1, ASC, True)], limit=0,
         expected=[(None, None), (0, "a"), (0, "b"), (0, "c"), (1, "d"), (1, "e"), (2, "f")]),
    dict(id="multiple_descending", cite=f"{MERGE_FILE}:190-214",
         records=[[(1, "e"), (0, "c"), (0, "a")], [(None, None), (2, "f"), (1, "d"), (0, "b")]],
         columns=[(0, DESC, True), (1, DESC, True)], limit=0,
         expected=[(None, None), (2, "f"), (1, "e"), (1, "d"), (0, "c"), (0, "b"), (0, "a")]),
    dict(id="multiple_mixed", cite=f"{MERGE_FILE}:216-240",
         records=[[(1, "e"), (0, "a"), (0, "c")], [(None, None), (2, "f"), (1, "d"), (0, "b")]],
         columns=[(0, DESC, True), (1, ASC, True)], limit=0,
         expected=[(None, None), (2, "f"), (1, "d"), (1, "e"), (0, "a"), (0, "b"), (0, "c")]),
]
