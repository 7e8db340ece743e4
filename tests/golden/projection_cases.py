"""The reference's exec/projection vectors as data (logictest/testdata/exec/projection/*), and the expression sets of the Projection
operator's differential test with the kernel shape each of them compiles to.

A vector: the table's columns and rows as the reference inserts them, the output list of the `select`, the optional `where`, and the
rows the reference prints. `None` is a NULL label.
"""
from frostdb_amd.logicalplan import OP_GT, OP_LT, AliasExpr, And, BinaryExpr, Col, Convert, If, IsNull, Literal, Or

MATH_FILE = "logictest/testdata/exec/projection/math_projection"
CONVERT_FILE = "logictest/testdata/exec/projection/convert"
PROJECTION_FILE = "logictest/testdata/exec/projection/projection"
BOOL_FILE = "logictest/testdata/exec/projection/bool"

VECTORS = [
    dict(id="value_times_timestamp", cite=f"{MATH_FILE}:10-15",
         cols=[("labels.label1", "dict"), ("stacktrace", "dict"), ("timestamp", "int64"), ("value", "int64")],
         rows=[("value1", "stack1", 1, 2), ("value1", "stack1", 3, 4), ("value1", "stack2", 5, 6)],
         select=[Col("value") * Col("timestamp")], where=None,
         out=["value * timestamp"], expected=[(2,), (12,), (30,)]),
    dict(id="convert_value_times_floatvalue", cite=f"{CONVERT_FILE}:10-15",
         cols=[("labels.label1", "dict"), ("stacktrace", "dict"), ("timestamp", "int64"), ("value", "int64"), ("floatvalue", "float64")],
         rows=[("value1", "stack1", 1, 2, 1.1), ("value1", "stack1", 3, 4, 1.1), ("value1", "stack2", 5, 6, 1.1)],
         select=[Convert(Col("value"), "float") * Col("floatvalue")], where=None,
         out=["convert(value, float) * floatvalue"], expected=[(2 * 1.1,), (4 * 1.1,), (6 * 1.1,)]),  # printed as 2.200000 4.400000 6.600000
    dict(id="label1", cite=f"{PROJECTION_FILE}:10-15",
         cols=[("labels.label1", "dict"), ("labels.label2", "dict"), ("labels.label3", "dict"), ("labels.label4", "dict"), ("labels.label5", "dict")],
         rows=[("value1", "value1", None, None, "value1"), ("value2", "value2", "value3", None, "value1"), ("value3", "value1", None, "value4", "value1")],
         select=[Col("labels.label1")], where=None,
         out=["labels.label1"], expected=[("value1",), ("value2",), ("value3",)]),
    dict(id="label1_label2", cite=f"{PROJECTION_FILE}:17-22",
         cols=[("labels.label1", "dict"), ("labels.label2", "dict"), ("labels.label3", "dict"), ("labels.label4", "dict"), ("labels.label5", "dict")],
         rows=[("value1", "value1", None, None, "value1"), ("value2", "value2", "value3", None, "value1"), ("value3", "value1", None, "value4", "value1")],
         select=[Col("labels.label1"), Col("labels.label2")], where=None,
         out=["labels.label1", "labels.label2"], expected=[("value1", "value1"), ("value2", "value2"), ("value3", "value1")]),
    # schema simple_bool (logictest/logic_test.go:43-60); the SQL front end turns the quoted true into a boolean literal (sqlparse/visitor.go:265-271)
    dict(id="name_where_found", cite=f"{BOOL_FILE}:10-14",
         cols=[("name", "dict"), ("found", "bool")],
         rows=[("test0", True), ("test1", True), ("test2", False)],
         select=[Col("name")], where=Col("found") == True,  # noqa: E712
         out=["name"], expected=[("test0",), ("test1",), ("test2",)][:2]),
]

# ---- differential test: one entry = one Projection call = one generated kernel --------------------------------------------------------
# Columns of the test record: a, b int64 with NULLs (raw slots under the NULLs set), c int64 without; f, g float64 with NULLs, h float64
# without; u, v uint64 without; d a dictionary column with NULLs (5 entries), w a dictionary column of 100 entries, s a plain utf8 column.
# `shape`: the same expressions for tools/jit_dump.cpp's `project` mode (the kernel source is compiled offline in the CPU suite).
A, B, C, F, G, H, U, V, D, W, S = (Col(n) for n in "abcfghuvdws")
DIFF_CASES = [
    dict(id="int_add_sub_mul", exprs=[A + B, A - B, A * B], shape="ci0n,ci1n,+;ci0n,ci1n,-;ci0n,ci1n,*"),
    dict(id="int_div_nested", exprs=[A / B, (A / B) + C, A / 1000 * 1000], shape="ci0n,ci1n,/;ci0n,ci1n,/,ci2,+;ci0n,li,/,li,*"),
    dict(id="int_div_never_null", exprs=[A / 7, IsNull(C)], shape="ci0n,li,/;ci1,nu"),
    dict(id="float_arith", exprs=[F + G, F - G, F * G, F / G, F * G + H], shape="cf0n,cf1n,+;cf0n,cf1n,-;cf0n,cf1n,*;cf0n,cf1n,/;cf0n,cf1n,*,cf2,+"),
    dict(id="uint_arith", exprs=[U + V, U * V, U / V, U - V], shape="cu0,cu1,+;cu0,cu1,*;cu0,cu1,/;cu0,cu1,-"),
    dict(id="compare_isnull", exprs=[BinaryExpr(A, OP_GT, B), A == 1, BinaryExpr(F, OP_LT, G), IsNull(A)], shape="ci0n,ci1n,q5;ci0n,li,q1;cf2n,cf3n,q3;ci0n,nu"),
    dict(id="if_convert_logic", exprs=[If(A > 0, A, C), Convert(A) * F, And(A > 0, F < 1.5), Or(A > 0, F < 1.5)],
         shape="ci0n,li,q5,ci0n,ci1,if;ci0n,cv,cf2n,*;ci0n,li,q5,cf2n,lf,q3,and;ci0n,li,q5,cf2n,lf,q3,or"),
    dict(id="strings", exprs=[D == "v2", W == "w77", S == "s1", And(D == "v2", A > 0)], shape="db0n;dl1;db2;db0n,ci0n,li,q5,and"),
    dict(id="literal_and_alias", exprs=[AliasExpr(Literal(7), "seven"), A.Alias("aa"), Literal(2.5) * H],
         shape="li;ci0n;lf,cf1,*"),
]
