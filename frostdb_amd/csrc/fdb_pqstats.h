// fdb_pqstats.h — the min / max pass of the Parquet writer (kernel: fdb_pqstats.hip; host side: fdb_pqwrite.cpp): what the kernel and the
// host walk behind fdb_selftest_parquet_write_indexed share — ONE definition of the order every column kind is compared in, as
// fdb_pqwrite.h is for the page geometry and fdb_pqdelta.h for the DELTA arithmetic.
//
// Every value that counts is mapped to an unsigned 64-bit KEY whose unsigned order is the column's order in Parquet (TypeDefinedOrder):
//   I64    the sign bit flipped                                   signed
//   U64    the bits as they are                                   unsigned, Int(64, unsigned)
//   F64    the total-order flip (negative: every bit, else the    numeric; a NaN does not count (tested on the bits). −0.0 sorts below
//          sign bit)                                              +0.0 here, so the fold does not depend on which zero it meets first;
//                                                                 parquet-format's zero rule is the host's, after the fold
//   BOOL   0 / 1 (the resident form holds 1 = false, 2 = true)   false < true
//   INDEX  ranks[index]: the dense rank of the entry's bytes      unsigned bytes, shorter first on a common prefix (dense_ranks of
//                                                                 fdb_sortplan.h: equal entries share a rank, so duplicates are one value)
// An index at or past `rank_len` does not count: it is the survey's to refuse (fdb_pqwrite.cpp), and is never used as a subscript here.
// The inverse (fdb_pqx_value) gives the 8 bytes of a V64 key back, 0 / 1 of a BOOL key, and the rank of an INDEX key, which the host
// turns into an entry.
//
// The table: per (column, page) the smallest and the largest key of the page's non-NULL rows that count — mins at [item], maxes at
// [items + item], item = column × n_pages + page. It starts EMPTY (min = all ones, max = zero) and every tile folds its own pair in with
// one min and one max: both commute, so the table does not depend on the order of the tiles. min > max after the pass: the page has no
// value that counts — no separate counter. (A page whose only key is 0 has min = max = 0: not empty.)
#pragma once

#include "fdb_pqwrite.h"

enum { FDB_PQX_I64 = 0, FDB_PQX_U64 = 1, FDB_PQX_F64 = 2, FDB_PQX_BOOL = 3, FDB_PQX_INDEX = 4 };

#define FDB_PQX_EMPTY_MIN (~0ull)
#define FDB_PQX_EMPTY_MAX 0ull

// One column as the pass sees it. `validity` == nullptr: every row counts.
struct FdbPqxCol {
  const void* values;             // 8 bytes per row (16-byte aligned on the device), or a uint32 index per row
  const unsigned char* validity;  // as FdbPqwCol's
  const uint32_t* ranks;          // INDEX: rank_len dense ranks
  uint32_t rank_len;
  int32_t mode;
};

FDB_PQW_HD bool fdb_pqx_is_nan(uint64_t bits) { return (bits & 0x7FFFFFFFFFFFFFFFull) > 0x7FF0000000000000ull; }

// The key of an 8-byte value (I64 / U64 / F64 / BOOL); false: the value does not count.
FDB_PQW_HD bool fdb_pqx_key(int mode, uint64_t bits, uint64_t* key) {
  switch (mode) {
    case FDB_PQX_I64: *key = bits ^ 0x8000000000000000ull; return true;
    case FDB_PQX_F64:
      if (fdb_pqx_is_nan(bits)) return false;
      *key = (bits >> 63) != 0 ? ~bits : bits ^ 0x8000000000000000ull;
      return true;
    case FDB_PQX_BOOL: *key = (int64_t)bits >= 2 ? 1 : 0; return true;
    default: *key = bits; return true;
  }
}
// … of a dictionary index.
FDB_PQW_HD bool fdb_pqx_index_key(const uint32_t* ranks, uint32_t rank_len, uint32_t index, uint64_t* key) {
  if (index >= rank_len) return false;
  *key = ranks[index];
  return true;
}
// The inverse: the value's 8 bytes (I64 / U64 / F64), 0 / 1 (BOOL), the rank (INDEX).
FDB_PQW_HD uint64_t fdb_pqx_value(int mode, uint64_t key) {
  switch (mode) {
    case FDB_PQX_I64: return key ^ 0x8000000000000000ull;
    case FDB_PQX_F64: return (key >> 63) != 0 ? key ^ 0x8000000000000000ull : ~key;
    default: return key;
  }
}

FDB_PQW_HD void fdb_pqx_fold(uint64_t key, uint64_t* mn, uint64_t* mx) {
  *mn = key < *mn ? key : *mn;
  *mx = key > *mx ? key : *mx;
}

// The rows a lane folds at a time: a UNIT is 16 bytes of values — two 8-byte values or four indices — and never crosses a validity word.
#define FDB_PQX_UNIT_V64 2
#define FDB_PQX_UNIT_INDEX 4
// Unit `u` of the tile whose rows are [first, end) (first a multiple of 64): its rows start at first + u × per, `bits` are their
// validity bits (bit i = row i of the unit holds a value; rows at or past `end` are cleared). `v`: the unit's values, read by the caller
// only as far as `bits` or `end` allow.
FDB_PQW_HD uint32_t fdb_pqx_unit_bits(const unsigned char* validity, int64_t first, int64_t end, uint32_t u, uint32_t per) {
  const uint32_t lr = u * per;
  return (uint32_t)(fdb_pqw_valid_word(validity, first, (int)(lr >> 6), end) >> (lr & 63)) & ((1u << per) - 1);
}

#ifndef FDB_PQWRITE_HOST_ONLY
#include <hip/hip_runtime_api.h>
// table: 2 × n_cols × n_pages keys, set to EMPTY by the caller on the same stream (mins: all ones, maxes: zero).
hipError_t fdb_launch_pqx_minmax(const FdbPqxCol* cols, FdbPqwGeom g, unsigned long long* table, hipStream_t stream);
#endif
