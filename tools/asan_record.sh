#!/bin/bash
# Host-only check of the resident record's layout contract under AddressSanitizer + UBSan (frostdb_amd/csrc/fdb_record.h, compiled with
# FDB_RECORD_HOST_ONLY): the slots of 2 000 random column lists are 256-aligned, disjoint, padded and add up; the three ways a bitmap's
# size has been written give the same slot for every row count up to 70 000; finish_column counts a bool as bits and keeps a bitmap only
# for a column with a NULL. No GPU, no HIP, no python: a stand-alone program (tools/asan_record_main.cpp) is compiled with g++ and run.
# Prints "asan record ok".
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd)
OUT=${TMPDIR:-/tmp}/fdb_asan_record
mkdir -p "$OUT"
g++ -std=c++17 -g -O1 -Wall -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -DFDB_RECORD_HOST_ONLY -I"$ROOT/include" -I"$ROOT/frostdb_amd/csrc" \
    "$ROOT/tools/asan_record_main.cpp" -o "$OUT/asan_record"
"$OUT/asan_record"
