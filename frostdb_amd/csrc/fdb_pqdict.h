// fdb_pqdict.h — used-entry dictionaries of the Parquet writer (kernels: fdb_pqdict.hip; host walk and layout: fdb_pqwrite.cpp): ONE
// definition of which entries a chunk's dictionary page keeps and of what an index becomes, for the kernels and for the host walk behind
// fdb_selftest_parquet_write_grouped — as fdb_pqbloom.h is for the filters and fdb_pqruns.h for the runs.
//
// A chunk's PRESENCE bitmap has one bit per entry of the column's dictionary, ⌈entries / 64⌉ 64-bit words, bit (i & 63) of word
// (i >> 6) for entry i: set when at least one non-NULL row of the chunk holds index i. The dictionary page keeps the entries whose bit
// is set, in entry order — two entries of equal bytes are two entries, both kept when both are used — and an index i becomes its RANK
// among them: before[i >> 6], the used entries in the words in front of i's (an exclusive count the host makes after the wait), plus
// the bits of i's own word below bit (i & 63). U, the bits set, is the page's num_values, and bits(U − 1) the chunk's width. An index at
// or past `entries` sets no bit and has no rank (the survey's to refuse, fdb_pqwrite.cpp); a NULL row's slot is written as 0.
#pragma once

#include "fdb_pqwrite.h"
#include "fdb_pqstats.h"

// The present pass collects a tile's bits in an LDS copy of the bitmap when the dictionary has at most this many entries: 128 words, 1 KiB.
#define FDB_PQG_LDS_WORDS 128
#define FDB_PQG_LDS_ENTRIES (64 * FDB_PQG_LDS_WORDS)

// One pruned column as the two passes see it.
struct FdbPqgCol {
  const uint32_t* values;          // a uint32 index per row (16-byte aligned on the device)
  const unsigned char* validity;   // as FdbPqwCol's
  unsigned long long* bits;        // the presence bitmap: fdb_pqg_words(entries) words, zeroed before the present pass
  const uint32_t* before;          // per word: the used entries in front of it (remap pass)
  uint32_t* out;                   // the re-keyed copy: an index per row, whole units of 4 rows writable (remap pass)
  uint32_t entries, pad;
};

FDB_PQW_HD uint64_t fdb_pqg_words(uint64_t entries) { return (entries + 63) / 64; }
FDB_PQW_HD uint64_t fdb_pqg_bit(uint32_t index) { return 1ull << (index & 63); }
FDB_PQW_HD bool fdb_pqg_used(const unsigned long long* bits, uint32_t index) { return ((uint64_t)bits[index >> 6] & fdb_pqg_bit(index)) != 0; }
// The rank of a used entry among the used ones (index < entries).
FDB_PQW_HD uint32_t fdb_pqg_rank(const unsigned long long* bits, const uint32_t* before, uint32_t index) {
  return before[index >> 6] + (uint32_t)fdb_pqw_popc((uint64_t)bits[index >> 6] & (fdb_pqg_bit(index) - 1));
}

#ifndef FDB_PQWRITE_HOST_ONLY
#include <hip/hip_runtime_api.h>
// Present: every non-NULL row's index sets its bit in its column's bitmap (zeroed by the caller on the same stream).
hipError_t fdb_launch_pqg_present(const FdbPqgCol* cols, int32_t n_cols, FdbPqwGeom g, hipStream_t stream);
// Remap: out[row] = the rank of values[row]; 0 for a NULL row and for an index at or past `entries`.
hipError_t fdb_launch_pqg_remap(const FdbPqgCol* cols, int32_t n_cols, FdbPqwGeom g, hipStream_t stream);
#endif
