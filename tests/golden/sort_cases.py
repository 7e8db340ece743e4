"""The reference's TestSortRecord cases as data (pqarrow/arrowutils/sort_test.go:22-241): the sample rows, the sorting columns and the
indices the reference expects.

A sample row gives only the fields it sets; the others take the zero value of the reference's `Sample` struct (sort_test.go:672-680) as
`Samples.Record()` appends it (:684-752): int 0, double 0.0, string "", dict "", nullable NULL — and a timestamp of 0 is appended as
NULL. COLUMNS is the record's schema in the reference's order; a sorting column is (index into the reference's schema, direction,
nulls_first) with direction 0 = Ascending, 1 = Descending.

Left out: "By DictFixed column ascending" / "… descending" (sort_test.go:153-172). They sort by column 4, a dictionary of
fixed_size_binary[2], which a resident record cannot hold (the issue's out-of-scope list); the column is left out of COLUMNS too, so the
reference's indices 5 and 6 (nullable, timestamp) are positions 4 and 5 of the record built here — INDEX_OF maps them.

Every expected index list is what a STABLE sort gives (the reference's sort.Sort promises no order of equal rows; on these 3- and 4-row
inputs its insertion sort happens to be stable) — tests/test_sort_cpu.py checks each against tests/sort_oracle.py."""

SORT_FILE = "pqarrow/arrowutils/sort_test.go"

ASC, DESC = 0, 1

# name, type of the column as the tests build it. "dict" = dictionary<uint32, binary>. "timestamp": the reference's column is an Arrow
# timestamp[s], compared as the integer it is (cmp.Compare on arrow.Timestamp, an int64); a resident record holds no Arrow timestamp
# type, timestamps reach it as int64 (as in every schema of the reference's that this project reads), so the tests build an int64 column
COLUMNS = [("int", "int64"), ("double", "float64"), ("string", "string"), ("dict", "dict"), ("nullable", "int64"), ("timestamp", "timestamp")]
# the reference's column index → the position in COLUMNS (4, dictFixed, is not there)
INDEX_OF = {0: 0, 1: 1, 2: 2, 3: 3, 5: 4, 6: 5}
ZERO = dict(int=0, double=0.0, string="", dict="", nullable=None, timestamp=0)


def col(index, direction=ASC, nulls_first=False):
    return (index, direction, nulls_first)


CASES = [
    dict(id="no_columns", cite=f"{SORT_FILE}:23-29", samples=[{}], columns=[], error="at least one column is needed for sorting"),
    dict(id="no_rows", cite=f"{SORT_FILE}:31-35", samples=[], columns=[col(0)], indices=[]),
    dict(id="one_row", cite=f"{SORT_FILE}:36-47", samples=[{}], columns=[col(0)], indices=[0]),
    dict(id="int_asc", cite=f"{SORT_FILE}:48-59", samples=[dict(int=3), dict(int=2), dict(int=1)], columns=[col(0)], indices=[2, 1, 0]),
    dict(id="int_desc", cite=f"{SORT_FILE}:60-72", samples=[dict(int=1), dict(int=2), dict(int=3)], columns=[col(0, DESC)], indices=[2, 1, 0]),
    dict(id="double_asc", cite=f"{SORT_FILE}:73-82", samples=[dict(double=3.0), dict(double=2.0), dict(double=1.0)], columns=[col(1)], indices=[2, 1, 0]),
    dict(id="double_desc", cite=f"{SORT_FILE}:83-92", samples=[dict(double=1.0), dict(double=2.0), dict(double=3.0)], columns=[col(1, DESC)], indices=[2, 1, 0]),
    dict(id="string_asc", cite=f"{SORT_FILE}:93-102", samples=[dict(string="3"), dict(string="2"), dict(string="1")], columns=[col(2)], indices=[2, 1, 0]),
    dict(id="string_desc", cite=f"{SORT_FILE}:103-112", samples=[dict(string="1"), dict(string="2"), dict(string="3")], columns=[col(2, DESC)], indices=[2, 1, 0]),
    dict(id="timestamp_asc", cite=f"{SORT_FILE}:113-122", samples=[dict(timestamp=3), dict(timestamp=2), dict(timestamp=1)], columns=[col(6)], indices=[2, 1, 0]),
    dict(id="timestamp_desc", cite=f"{SORT_FILE}:123-132", samples=[dict(timestamp=1), dict(timestamp=2), dict(timestamp=3)], columns=[col(6, DESC)],
         indices=[2, 1, 0]),
    dict(id="dict_asc", cite=f"{SORT_FILE}:133-142", samples=[dict(dict="3"), dict(dict="2"), dict(dict="1")], columns=[col(3)], indices=[2, 1, 0]),
    dict(id="dict_desc", cite=f"{SORT_FILE}:143-152", samples=[dict(dict="1"), dict(dict="2"), dict(dict="3")], columns=[col(3, DESC)], indices=[2, 1, 0]),
    dict(id="null_asc", cite=f"{SORT_FILE}:173-182", samples=[{}, {}, dict(nullable=1)], columns=[col(5)], indices=[2, 0, 1]),
    dict(id="null_asc_nulls_first", cite=f"{SORT_FILE}:183-192", samples=[{}, {}, dict(nullable=1)], columns=[col(5, ASC, True)], indices=[0, 1, 2]),
    dict(id="null_desc", cite=f"{SORT_FILE}:193-202", samples=[{}, {}, dict(nullable=1)], columns=[col(5, DESC)], indices=[2, 0, 1]),
    dict(id="null_desc_nulls_first", cite=f"{SORT_FILE}:203-212", samples=[{}, {}, dict(nullable=1)], columns=[col(5, DESC, True)], indices=[0, 1, 2]),
    dict(id="two_columns_same_direction", cite=f"{SORT_FILE}:213-226",
         samples=[dict(string="1", int=3), dict(string="2", int=2), dict(string="3", int=2), dict(string="4", int=1)],
         columns=[col(0), col(2)], indices=[3, 1, 2, 0]),
    dict(id="two_columns_different_direction", cite=f"{SORT_FILE}:227-240",
         samples=[dict(string="1", int=3), dict(string="2", int=2), dict(string="3", int=2), dict(string="4", int=1)],
         columns=[col(0, ASC), col(2, DESC)], indices=[3, 2, 1, 0]),
]
