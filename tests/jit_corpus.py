"""Every shape the CPU suite asks tools/jit_dump.cpp for, in one place: (name, jit_dump arguments). The tests that compile the generated
sources take their shapes from the groups below; tests/test_jit_source_identity_cpu.py pins the text of every one of them
(tests/golden/jit_source_digests.json). A shape added here gets its digest with FDB_WRITE_JIT_DIGESTS=1 (see that test)."""
from tests.golden.projection_cases import DIFF_CASES

# tests/test_jit_sources_cpu.py: one representative shape per kernel and mode
SOURCES = [
    ("plan_lds", ["plan", "lds"]),
    ("plan_wave_tables", ["plan", "wave"]),       # fdb_plan_set_deterministic
    ("plan_reg_slots", ["plan", "reg"]),
    ("plan_cache", ["plan", "cache"]),
    ("plan_two_phase", ["plan", "two"]),
    ("flags", ["flags"]),
    ("select_value", ["select", "1"]),            # filter() in one pass: one 8-byte column fused
    ("select_value_and_dict", ["select"]),        # … next to an unfused dictionary leaf with a LUT in LDS
    ("hash_32_columns", ["32"]),                  # cfg 5
    ("hash_int64_key", ["8", "1"]),
    ("runs_32_columns", ["32", "2"]),             # the table-free OrderedAggregate's run kernel
    ("runs_wide_32_columns", ["32", "3"]),        # … writing wide records (any cardinality: tuples from re-loaded columns)
    ("runs_wide_int64_key", ["3", "4"]),          # … with an int64 key column
    ("runs_medium_32_columns", ["32", "5"]),      # … writing medium records (two bytes per key id, ids kept in registers)
]

# tests/test_jit_narrow_sources_cpu.py / test_jit_quad_sources_cpu.py: a 1-byte filter slot plus a 2-byte group slot — the same three
# launches under both names — and the single-phase shape at 512 and 256 threads per workgroup
NARROW = [
    ("narrow_lds", ["plan", "lds", "narrow"]),
    ("narrow_two_phase", ["plan", "two", "narrow"]),
    ("narrow_wave_tables", ["plan", "wave", "narrow"]),
]
QUAD = [("quad_" + name[len("narrow_"):], args) for name, args in NARROW] + [
    ("quad_lds_512", ["plan", "lds", "narrow", "512"]),
    ("quad_lds_256", ["plan", "lds", "narrow", "256"]),
]
# tests/test_jit_quad_isa_cpu.py: the quad shapes and bench.py's headline query
QUAD_ISA = QUAD + [("quad_lds_256_sum", ["plan", "lds", "narrow", "256", "sum"])]

# tests/test_exact_sums_jit_cpu.py
EXACT = [
    ("exact_32_columns", ["32", "0", "exact"]),  # cfg 5's key shape, two exact SUMs (one with NULLs) and a COUNT
    ("exact_int64_key", ["3", "1", "exact"]),    # an int64 (time bucket) key
    ("exact_no_groups", ["0", "0", "exact"]),    # no group column: one group
]

# tests/test_hash_scan_cases_cpu.py: the column counts of tests/hash_scan_cases.py — N dictionary columns with validity (the first 8 LUTs
# in LDS), SUM(float64) + COUNT; "1": the last column an int64 key; "exact": exact sums
HASH_CASES = [("hash_scan_" + "_".join(a), a) for a in
              [[str(n)] for n in (9, 12, 16, 17, 31, 32, 33, 63, 64)] + [[str(n + 1), "1"] for n in (0, 1, 2, 3, 7, 8, 31, 32, 63)] + [["2", "1", "exact"]]]

# tests/test_project_cpu.py: the expression sets of the Projection operator's differential test
PROJECT = [(case["id"], ["project", case["shape"]]) for case in DIFF_CASES]

# Shapes no test compiles, pinned for their text: computed aggregate inputs, computed keys, expression columns of the hash kernel,
# kernels without a predicate, a fused 4-byte slot.
DIV = "ci0n,ci1n,/"                               # a division at the root: the input can be NULL
IF7 = "db0n,ci0,li,q5,and,ci0,ci1,if"             # a compared dictionary column (an expression node of kind 7) inside an if
COMPUTED = [
    ("plan_lds_sum_div", ["plan", "lds", "agg=sumf:" + DIV]),          # the uniform fold and the per-row LDS atomics
    ("plan_reg_sum_div", ["plan", "reg", "agg=sumf:" + DIV]),          # the register table
    ("plan_cache_sum_div", ["plan", "cache", "agg=sumf:" + DIV]),      # the combining cache
    ("plan_two_sum_div", ["plan", "two", "agg=sumf:" + DIV]),          # late registers
    ("plan_lds_sum_float_div", ["plan", "lds", "agg=sumf:cf0n,cf1n,/"]),
    ("plan_lds_min_add", ["plan", "lds", "agg=mini:ci0,li,+"]),
    ("plan_wave_max_float", ["plan", "wave", "agg=maxf:cf0n,lf,*"]),
    ("plan_lds_sum_if_leaf", ["plan", "lds", "agg=sumi:" + IF7]),
    ("plan_reg_sum_if_leaf", ["plan", "reg", "agg=sumi:" + IF7]),
    ("plan_quad_sum_div", ["plan", "lds", "narrow", "256", "agg=sumf:" + DIV]),
    ("hash_8_computed_agg_and_key", ["8", "0", "agg=sumf:cf0n,cf1n,*", "key=ci2,li,/"]),
    ("hash_8_min_if_leaf", ["8", "0", "agg=mini:" + IF7]),
    ("runs_wide_computed_key", ["8", "3", "key=ci0,li,/"]),
    ("runs_medium_computed_agg", ["8", "5", "agg=sumi:ci0n,ci1,*"]),
    ("exact_computed_sum", ["8", "0", "exact", "agg=sumf:cf0n,cf1n,*"]),
    ("flags_no_predicate", ["flags", "nopred"]),
    ("select_no_predicate", ["select", "nopred"]),
    ("select_fuse8_fuse4", ["select", "fuse4"]),                       # (`select 1 1` has no 4-byte slot left to fuse)
    ("select_value_fuse4_bit", ["select", "1", "1"]),
]


def kernel_of(args):
    """The kernel a jit_dump invocation prints."""
    return {"plan": "fdb_plan_kernel", "flags": "fdb_flags_kernel", "select": "fdb_select_kernel", "project": "fdb_project_kernel"}.get(args[0], "fdb_hash_kernel")


def _distinct(groups):
    seen, out = set(), []
    for name, args in (s for g in groups for s in g):
        if tuple(args) not in seen:
            seen.add(tuple(args))
            out.append((name, args))
    assert len({n for n, _ in out}) == len(out)
    return out


# one entry per distinct invocation (the narrow shapes go by their quad names)
CORPUS = _distinct([SOURCES, QUAD_ISA, NARROW, EXACT, HASH_CASES, PROJECT, COMPUTED])
