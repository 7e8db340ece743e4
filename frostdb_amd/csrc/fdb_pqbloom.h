// fdb_pqbloom.h — the bloom filter pass of the Parquet writer (kernel: fdb_pqbloom.hip; host side: fdb_pqwrite.cpp): what the kernel and the
// host walk behind fdb_selftest_parquet_write_filtered share — ONE definition of the hash, the block, the bits and the size of a
// split-block bloom filter (parquet-format's BloomFilter.md), as fdb_pqstats.h is for the order of the min / max pass.
//
//   hash    XXH64, seed 0, of the value's PLAIN bytes: an I64 / U64 / F64 value's 8 bytes, little-endian, the bits as they are (a NaN with
//           its payload, −0.0 and +0.0 as two values); a dictionary or plain string / binary entry's bytes without a length prefix.
//   block   ((hash >> 32) × n_blocks) >> 32. A block is 32 bytes: eight 32-bit little-endian words.
//   bits    in word i of the block bit (((uint32)hash × SALT[i]) >> 27).
//   size    n values at b bits each: 32 × max(1, ⌈⌈n × b / 8⌉ / 32⌉) bytes, at most FDB_PQB_MAX_BYTES — not rounded to a power of two,
//           which the block rule does not need. n: the column's non-NULL rows, of an index column the smaller of that and the
//           dictionary's length. No value: one zero block.
//   header  BloomFilterHeader in thrift compact: numBytes, BLOCK, XXHASH, UNCOMPRESSED (fdb_pqb_header).
// A pair of words is one aligned 64-bit word of the bitset (word 2p in its low half): the kernel sets a value's eight bits with at most
// four 64-bit atomic ORs. OR commutes, so the bitset does not depend on the order the values went in.
#pragma once

#include "fdb_pqstats.h"  // (the units a lane reads at a time: fdb_pqx_unit_bits)

#define FDB_PQB_BLOCK_BYTES 32
#define FDB_PQB_MAX_BYTES (128u << 20)
#define FDB_PQB_DEFAULT_BITS 10  // ≙ bloomFilterBitsPerValue (dynparquet/schema.go)
#define FDB_PQB_MAX_HEADER 19

// One filtered column as the pass sees it. `validity` == nullptr: every row counts.
struct FdbPqbCol {
  const void* values;             // 8 bytes per row (16-byte aligned on the device), or a uint32 index per row
  const unsigned char* validity;  // as FdbPqwCol's
  const uint64_t* hashes;         // index column: hash_len entry hashes
  unsigned long long* bits;       // the column's bitset: n_blocks × 32 bytes, 32-byte aligned, zeroed by the caller
  uint32_t hash_len, n_blocks;
  int32_t index, pad;             // index != 0: an index column
};

#define FDB_PQB_P1 0x9E3779B185EBCA87ull
#define FDB_PQB_P2 0xC2B2AE3D27D4EB4Full
#define FDB_PQB_P3 0x165667B19E3779F9ull
#define FDB_PQB_P4 0x85EBCA77C2B2AE63ull
#define FDB_PQB_P5 0x27D4EB2F165667C5ull

FDB_PQW_HD uint64_t fdb_pqb_rotl(uint64_t x, int r) { return (x << r) | (x >> (64 - r)); }
FDB_PQW_HD uint64_t fdb_pqb_round(uint64_t acc, uint64_t in) { return fdb_pqb_rotl(acc + in * FDB_PQB_P2, 31) * FDB_PQB_P1; }
FDB_PQW_HD uint64_t fdb_pqb_merge(uint64_t h, uint64_t v) { return (h ^ fdb_pqb_round(0, v)) * FDB_PQB_P1 + FDB_PQB_P4; }
FDB_PQW_HD uint64_t fdb_pqb_avalanche(uint64_t h) {
  h ^= h >> 33; h *= FDB_PQB_P2;
  h ^= h >> 29; h *= FDB_PQB_P3;
  return h ^ (h >> 32);
}

// XXH64 (seed 0) of an 8-byte value: the general function below at len == 8, a handful of multiplies.
FDB_PQW_HD uint64_t fdb_pqb_hash8(uint64_t bits) {
  uint64_t h = FDB_PQB_P5 + 8;
  h ^= fdb_pqb_round(0, bits);
  h = fdb_pqb_rotl(h, 27) * FDB_PQB_P1 + FDB_PQB_P4;
  return fdb_pqb_avalanche(h);
}

// XXH64 (seed 0) of `len` bytes: stripes of 32, then tails of 8, 4 and 1.
FDB_PQW_HD uint64_t fdb_pqb_hash(const unsigned char* p, uint64_t len) {
  const unsigned char* const end = p + len;
  uint64_t h;
  if (len >= 32) {
    uint64_t v1 = FDB_PQB_P1 + FDB_PQB_P2, v2 = FDB_PQB_P2, v3 = 0, v4 = 0ull - FDB_PQB_P1, w;
    do {
      __builtin_memcpy(&w, p, 8); v1 = fdb_pqb_round(v1, w);
      __builtin_memcpy(&w, p + 8, 8); v2 = fdb_pqb_round(v2, w);
      __builtin_memcpy(&w, p + 16, 8); v3 = fdb_pqb_round(v3, w);
      __builtin_memcpy(&w, p + 24, 8); v4 = fdb_pqb_round(v4, w);
      p += 32;
    } while (end - p >= 32);
    h = fdb_pqb_rotl(v1, 1) + fdb_pqb_rotl(v2, 7) + fdb_pqb_rotl(v3, 12) + fdb_pqb_rotl(v4, 18);
    h = fdb_pqb_merge(h, v1); h = fdb_pqb_merge(h, v2); h = fdb_pqb_merge(h, v3); h = fdb_pqb_merge(h, v4);
  } else {
    h = FDB_PQB_P5;
  }
  h += len;
  for (; end - p >= 8; p += 8) {
    uint64_t w;
    __builtin_memcpy(&w, p, 8);
    h ^= fdb_pqb_round(0, w);
    h = fdb_pqb_rotl(h, 27) * FDB_PQB_P1 + FDB_PQB_P4;
  }
  if (end - p >= 4) {
    uint32_t w;
    __builtin_memcpy(&w, p, 4);
    h ^= (uint64_t)w * FDB_PQB_P1;
    h = fdb_pqb_rotl(h, 23) * FDB_PQB_P2 + FDB_PQB_P3;
    p += 4;
  }
  for (; p < end; p++) {
    h ^= (uint64_t)*p * FDB_PQB_P5;
    h = fdb_pqb_rotl(h, 11) * FDB_PQB_P1;
  }
  return fdb_pqb_avalanche(h);
}

FDB_PQW_HD uint32_t fdb_pqb_salt(int i) {
  switch (i) {
    case 0: return 0x47b6137bu;
    case 1: return 0x44974d91u;
    case 2: return 0x8824ad5bu;
    case 3: return 0xa2b7289du;
    case 4: return 0x705495c7u;
    case 5: return 0x2df1424bu;
    case 6: return 0x9efc4947u;
    default: return 0x5c6bfb31u;
  }
}

FDB_PQW_HD uint32_t fdb_pqb_block(uint64_t hash, uint32_t n_blocks) { return (uint32_t)(((hash >> 32) * (uint64_t)n_blocks) >> 32); }
// The bit of word `i` (0 … 7) of the block.
FDB_PQW_HD uint32_t fdb_pqb_word_mask(uint64_t hash, int i) { return 1u << (((uint32_t)hash * fdb_pqb_salt(i)) >> 27); }
// … of words 2p and 2p + 1 (p: 0 … 3) as one little-endian 64-bit word.
FDB_PQW_HD uint64_t fdb_pqb_pair_mask(uint64_t hash, int p) { return (uint64_t)fdb_pqb_word_mask(hash, 2 * p) | ((uint64_t)fdb_pqb_word_mask(hash, 2 * p + 1) << 32); }

// bits_per_value as asked (0: the default) → as used.
FDB_PQW_HD uint32_t fdb_pqb_bits_per_value(int32_t asked) { return asked == 0 ? FDB_PQB_DEFAULT_BITS : (uint32_t)asked; }
// The bitset's bytes for `n` values at `b` bits (1 … 64) each.
FDB_PQW_HD uint32_t fdb_pqb_bytes(uint64_t n, uint32_t b) {
  const uint64_t bytes = (n * b + 7) / 8;
  uint64_t blocks = (bytes + FDB_PQB_BLOCK_BYTES - 1) / FDB_PQB_BLOCK_BYTES;
  if (blocks < 1) blocks = 1;
  const uint64_t out = blocks * FDB_PQB_BLOCK_BYTES;
  return out > FDB_PQB_MAX_BYTES ? FDB_PQB_MAX_BYTES : (uint32_t)out;
}

// BloomFilterHeader for a bitset of `bytes` bytes, as pyarrow writes it: 15 zigzag-varint(numBytes) 1c 1c 00 00 1c 1c 00 00 1c 1c 00 00 00
// — 1: numBytes; 2: algorithm { 1: BLOCK {} }; 3: hash { 1: XXHASH {} }; 4: compression { 1: UNCOMPRESSED {} }. Returns its length
// (at most FDB_PQB_MAX_HEADER).
FDB_PQW_HD uint32_t fdb_pqb_header(uint32_t bytes, unsigned char* out) {
  uint32_t n = 0;
  out[n++] = 0x15;
  uint64_t z = (uint64_t)bytes << 1;
  while (z >= 0x80) { out[n++] = (unsigned char)(z | 0x80); z >>= 7; }
  out[n++] = (unsigned char)z;
  for (int f = 0; f < 3; f++) { out[n++] = 0x1c; out[n++] = 0x1c; out[n++] = 0; out[n++] = 0; }
  out[n++] = 0;
  return n;
}

#ifndef FDB_PQWRITE_HOST_ONLY
#include <hip/hip_runtime_api.h>
// Every non-NULL row's value of the `n_cols` columns into their bitsets, which the caller zeroed on the same stream. g: the record's
// geometry (its n_cols is not looked at).
hipError_t fdb_launch_pqb_insert(const FdbPqbCol* cols, int32_t n_cols, FdbPqwGeom g, hipStream_t stream);
#endif
