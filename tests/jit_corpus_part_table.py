"""The shapes whose source is pinned WITH the packed part table on (tools/jit_dump.cpp, `ptab`; JitShape::part_table): (name, jit_dump
arguments without `ptab`). Each has its twin without the table in tests/jit_corpus.py or is compiled beside it by
tests/test_jit_part_table_cpu.py; tests/golden/jit_part_table_digests.json holds the digests. A shape added here gets its entry with
FDB_WRITE_JIT_DIGESTS=1 (see that test)."""

PART_TABLE = [
    ("headline", ["plan", "lds", "narrow", "256", "sum"]),                # bench.py's query, dictionary slots with bitmaps
    ("headline_nonull", ["plan", "lds", "narrow", "256", "sum", "nonull"]),  # … over null-folded caches: what the benchmark launches
    ("quad_two_phase", ["plan", "two", "narrow", "256"]),
    ("quad_wave_tables", ["plan", "wave", "narrow", "256"]),
    ("quad_cfg3", ["plan", "two", "narrow", "256", "cfg3"]),
]
