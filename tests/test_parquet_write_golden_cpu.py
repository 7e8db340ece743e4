"""The Parquet writer's bytes, pinned (selftest_parquet_write): no GPU.

tests/golden/parquet_write_digests.json holds, for every (rows, option set) below, the length and SHA-256 of the file the host walk
returned at the commit before the writer's plumbing was rewritten around one spec and one plan. The records are arithmetic patterns
only — np.arange, modulo, comparisons; no random generator — so the digests depend on the writer alone. Every option set goes through
the narrowest entry point that carries it (which selftest_parquet_write chooses), "all" through fdb_selftest_parquet_write_runs.

    python -m tests.test_parquet_write_golden_cpu --write     # writes the fixture anew: only ever with a library whose bytes are trusted
"""
import hashlib
import json
import os
import sys

import numpy as np
import pyarrow as pa

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "parquet_write_digests.json")
PAGE = 64
ROWS = [0, 1, 63, 64, 65, 129, 1000]
OPTION_SETS = {
    "none": {},
    "delta": {"encodings": {"i64": "delta", "u64": "delta"}},
    "snappy": {"compression": "snappy"},
    "page_index": {"statistics": "page", "sorting_columns": [("d5",), ("i64", True)], "index_size_limit": 4},
    "bloom": {"bloom_filters": ["i64", "d257"]},
    "runs": {"runs": True},
}
OPTION_SETS["all"] = {k: v for kw in list(OPTION_SETS.values()) for k, v in kw.items()}


def record(rows: int) -> pa.RecordBatch:
    """int64, uint64 (past 2^63), float64 with NULLs, bool, a dictionary of 5 entries in stretches, one of 257 with NULLs — scattered
    and in whole pages — and a plain string column."""
    i = np.arange(rows, dtype=np.int64)
    d5 = pa.DictionaryArray.from_arrays(pa.array(((i // 40) % 5).astype(np.int32)), pa.array(["entry-%d" % e for e in range(5)]))
    d257 = pa.DictionaryArray.from_arrays(pa.array(((i * 7) % 257).astype(np.int32), mask=(i % 11 == 0) | ((i // PAGE) % 4 == 2)),
                                          pa.array(["value-%03d" % (e * 3 % 257) for e in range(257)]))
    cols = [pa.array((i * i) % 1009 * 1000 - 3 * i - 500),
            pa.array(i.astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15)),
            pa.array((i % 17 - 8) * 0.25, mask=i % 5 == 3),
            pa.array(i % 3 == 0),
            d5, d257,
            pa.array(["s%d" % (v % 13) for v in i.tolist()], type=pa.string())]
    return pa.RecordBatch.from_arrays(cols, names=["i64", "u64", "f64", "flag", "d5", "d257", "text"])


def digests() -> dict:
    from frostdb_amd import physicalplan as pp
    out = {}
    for rows in ROWS:
        rec = record(rows)
        for name, kw in OPTION_SETS.items():
            data = pp.selftest_parquet_write(rec, page_rows=PAGE, **kw)
            out["%d/%s" % (rows, name)] = {"bytes": len(data), "sha256": hashlib.sha256(data).hexdigest()}
    return out


def test_the_fixture_lists_every_rows_and_option_set():
    golden = json.load(open(GOLDEN))
    assert len(golden) == len(ROWS) * len(OPTION_SETS) == 49
    assert sorted(golden) == sorted("%d/%s" % (rows, name) for rows in ROWS for name in OPTION_SETS)


def test_every_file_is_byte_for_byte_what_it_was():
    golden, got = json.load(open(GOLDEN)), digests()
    assert sorted(got) == sorted(golden)
    for key in golden:
        assert got[key]["bytes"] == golden[key]["bytes"], key
        assert got[key]["sha256"] == golden[key]["sha256"], key


if __name__ == "__main__":
    assert sys.argv[1:] == ["--write"], __doc__
    with open(GOLDEN, "w") as f:
        json.dump(digests(), f, indent=0, sort_keys=True)
        f.write("\n")
