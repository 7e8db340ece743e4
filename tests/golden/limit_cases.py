"""The reference's exec/limit vectors as data (logictest/testdata/exec/limit/limit): the table's columns and rows as the reference
inserts them, and per `select … limit N` the selected columns, the count and the rows the reference prints. `None` is a NULL label."""

LIMIT_FILE = "logictest/testdata/exec/limit/limit"

TABLE = dict(
    cols=["labels.label1", "labels.label2", "labels.label3", "labels.label4", "labels.label5"],
    rows=[("value1", "value1", None, None, "value1"),
          ("value2", "value2", "value3", None, "value1"),
          ("value3", "value1", None, "value4", "value1")],
)

CASES = [
    dict(id="label3_limit_0", cite=f"{LIMIT_FILE}:10-12", select=["labels.label3"], count=0, expected=[]),
    dict(id="label1_limit_4", cite=f"{LIMIT_FILE}:14-19", select=["labels.label1"], count=4, expected=[("value1",), ("value2",), ("value3",)]),
    dict(id="label2_limit_3", cite=f"{LIMIT_FILE}:21-26", select=["labels.label2"], count=3, expected=[("value1",), ("value2",), ("value1",)]),
    dict(id="label3_limit_2", cite=f"{LIMIT_FILE}:28-32", select=["labels.label3"], count=2, expected=[(None,), ("value3",)]),
    dict(id="label1_label2_limit_5", cite=f"{LIMIT_FILE}:34-39", select=["labels.label1", "labels.label2"], count=5,
         expected=[("value1", "value1"), ("value2", "value2"), ("value3", "value1")]),
]
