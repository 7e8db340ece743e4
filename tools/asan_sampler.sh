#!/bin/bash
# Host-only memory-safety check of the Sampler's and Take's host code (frostdb_amd/csrc/fdb_reservoir.h: ReservoirSelect,
# keep_last_per_slot, DictUnion, check_take_indices — with fdb_arrow.cpp's dictionary constructors) under AddressSanitizer + UBSan.
# No GPU, no HIP, no python: a stand-alone program (tools/asan_sampler_main.cpp) is compiled with g++ and run. Prints "asan sampler ok".
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd)
OUT=${TMPDIR:-/tmp}/fdb_asan_sampler
mkdir -p "$OUT"
g++ -std=c++17 -g -O1 -Wall -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -I"$ROOT/include" -I"$ROOT/frostdb_amd/csrc" \
    "$ROOT/tools/asan_sampler_main.cpp" "$ROOT/frostdb_amd/csrc/fdb_arrow.cpp" -o "$OUT/asan_sampler" -lpthread
"$OUT/asan_sampler"
