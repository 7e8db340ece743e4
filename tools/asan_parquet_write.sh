#!/bin/bash
# Host-only memory-safety check of the Parquet writer's host half under AddressSanitizer + UBSan: options and column checks, layout
# planning, the thrift compact writer, the dictionary page builder and the tail (frostdb_amd/csrc/fdb_pqwrite.cpp), and the host walk of
# the survey and encode passes (fdb_pqwrite.h: the page geometry, bit positions and word assembly the kernels compile) and of the
# DELTA_BINARY_PACKED passes (fdb_pqdelta.h) over seeded random records and options, with fdb_arrow.cpp's dictionary constructors; and the
# SNAPPY compressor's host walk (fdb_pqsnappy.h) over the same records with codecs per column at random and over bodies around one and
# two fragments, every page inflated again by the library's host decoder (fdb_codec.cpp); the codec drawn per column is UNCOMPRESSED,
# SNAPPY or LZ4_RAW, and the LZ4_RAW compressor's host walk (fdb_pqlz4.h) runs over the same pages and bodies, inflated again by fdb::lz4_raw.
# Every record is also written with index options at random — statistics, a cut limit, sorting columns: the min / max pass's host walk
# (fdb_pqstats.h), chunk bounds, ColumnIndex and OffsetIndex — and the index is read back by a small thrift reader of the program's own.
# … and with bloom filter options at random — columns and bits per value: the insert pass's host walk (fdb_pqbloom.h), the filters'
# headers and bitsets between the pages and the index — and a reader of the program's own, with its own XXH64, finds every non-NULL
# value in its column's filter and no bit that no value set.
# … and with run options at random — per column the dictionary indices, the definition levels, both or none: the run passes' host walk
# (fdb_pqruns.h), every stream cut into runs decoded by a hybrid reader of the program's own and held to "never longer than packed".
# … and with group options at random — a row_group_rows that leaves one row group, dictionaries of used entries only: the present and
# remap passes' host walk (fdb_pqdict.h), every re-keyed index checked, and a dictionary reader of the program's own finds in every
# pruned chunk exactly the used entries.
# … and with a string form drawn per byte-array column — dictionary, PLAIN or DELTA_LENGTH_BYTE_ARRAY: the byte survey's and the byte
# encode pass's host walk (fdb_pqbytes.h), the lengths through the DELTA walk, and a PLAIN reader and a DELTA_LENGTH reader of the
# program's own find every page's values in exactly the bytes the layout gave it.
# No GPU, no HIP runtime (fdb_codec.h takes its types from the HIP headers), no python: a stand-alone program (tools/asan_parquet_write_main.cpp) is compiled with g++ and run. Prints "asan parquet write ok".
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd)
OUT=${TMPDIR:-/tmp}/fdb_asan_parquet_write
mkdir -p "$OUT"
g++ -std=c++17 -g -O1 -Wall -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -DFDB_PQWRITE_HOST_ONLY -D__HIP_PLATFORM_AMD__ -I"${ROCM_PATH:-/opt/rocm}/include" -I"$ROOT/include" -I"$ROOT/frostdb_amd/csrc" \
    "$ROOT/tools/asan_parquet_write_main.cpp" "$ROOT/frostdb_amd/csrc/fdb_pqwrite.cpp" "$ROOT/frostdb_amd/csrc/fdb_codec.cpp" "$ROOT/frostdb_amd/csrc/fdb_arrow.cpp" -o "$OUT/asan_parquet_write" -lpthread
"$OUT/asan_parquet_write"
