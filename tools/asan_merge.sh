#!/bin/bash
# Host-only memory-safety check of the device MergeRecords' host code under AddressSanitizer + UBSan: the key layout across records
# (frostdb_amd/csrc/fdb_sortplan.h: pack_sort_fields, bits_for, dense_ranks), the dictionary plan of a column across the inputs with its
# union, translation and rank tables (fdb_mergerec.h: plan_merge_dict, with fdb_reservoir.h's DictUnion and fdb_arrow.cpp's dictionary
# constructors), the schema union and per-input column map of records whose field lists differ (fdb_mergerec.h: unify_merge_schema) and the merge-path walk behind fdb_selftest_merge_path (fdb_mergepath.h: the code the kernels compile, on host arrays).
# No GPU, no HIP, no python: a stand-alone program (tools/asan_merge_main.cpp) is compiled with g++ and run. Prints "asan merge ok".
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd)
OUT=${TMPDIR:-/tmp}/fdb_asan_merge
mkdir -p "$OUT"
g++ -std=c++17 -g -O1 -Wall -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -DFDB_MERGEREC_HOST_ONLY -I"$ROOT/include" -I"$ROOT/frostdb_amd/csrc" \
    "$ROOT/tools/asan_merge_main.cpp" "$ROOT/frostdb_amd/csrc/fdb_arrow.cpp" -o "$OUT/asan_merge" -lpthread
"$OUT/asan_merge"
