// fdb_pqdelta.h — the arithmetic of the Parquet writer's DELTA_BINARY_PACKED pages (kernels: fdb_pqdelta.hip; host walk: fdb_pqwrite.cpp):
// ONE definition of deltas, minimum, widths, sizes, header bytes and of how an output word of a miniblock is put together, for the
// kernels and for the host walk behind fdb_selftest_parquet_write_encoded — as fdb_pqwrite.h is for the PLAIN / bit-packed passes.
//
// A page's non-NULL values v[0 … count) in rank order (8-byte bit patterns; INT64 and UINT64 alike) are written as
//   varint(128) varint(4) varint(count) zigzag(v[0])                                   the page header, 5 … 18 bytes
//   per BLOCK of up to 128 deltas d[i] = v[i + 1] − v[i] (wrapping), count − 1 of them in all:
//     zigzag(min)  the smallest delta of the block taken as signed int64, 1 … 10 bytes
//     4 width bytes: miniblock m (32 deltas) is as wide as the bit length of its largest d − min (unsigned, wrapping), 0 … 64;
//                    0 for a miniblock of the last block that holds no delta
//     the miniblocks that hold a delta, each exactly `width` 32-bit words: d − min at bit j × width, least significant bit first, the
//                    last one padded to 32 values with zero bits
// A page of one value is its header alone; a page without a value is varint(128) varint(4) 0 0. A block's parts are whole bytes and a
// miniblock whole 4-byte words — at any byte of the file, so they are stored unaligned and nobody shares a byte with a neighbour.
#pragma once

#include "fdb_pqwrite.h"

#define FDB_PQD_BLOCK 128        // deltas per block
#define FDB_PQD_MINI 32          // deltas per miniblock: a miniblock at width w is w 32-bit words
#define FDB_PQD_MINIS 4
#define FDB_PQD_THREADS 256      // four waves, each working on a block (or a page) of its own
#define FDB_PQD_WAVES (FDB_PQD_THREADS / 64)
#define FDB_PQD_MAX_HEADER 18    // 80 01 | 04 | varint(count: 32 bits) <= 5 | zigzag(first value) <= 10

// One DELTA column as the kernels see it. `dense`: the column's non-NULL values, those of page p in rank order from dense[first row of p]
// on — the column itself when it has no bitmap, else scratch the compaction pass fills.
struct FdbPqdCol {
  const uint64_t* values;
  const unsigned char* validity;
  uint64_t* dense;
  int32_t col, pad;              // its place in the survey's tables (FdbPqwPageStat, tile_base)
};
// What the block survey leaves per (DELTA column, page, block); `off` is filled in by the page walk: where the block starts, from the
// page's first value byte on.
struct FdbPqdBlock {
  int64_t min;
  uint32_t widths;               // byte m = width of miniblock m
  uint32_t bytes, off, pad;
};

FDB_PQW_HD int32_t fdb_pqd_blocks_per_page(int32_t page_rows) { return (page_rows + FDB_PQD_BLOCK - 1) / FDB_PQD_BLOCK; }  // (a page of n rows has at most n − 1 deltas)
FDB_PQW_HD uint32_t fdb_pqd_deltas(uint32_t count) { return count > 0 ? count - 1 : 0; }
FDB_PQW_HD uint32_t fdb_pqd_blocks(uint32_t deltas) { return (deltas + FDB_PQD_BLOCK - 1) / FDB_PQD_BLOCK; }
// Deltas of block b of a page with `deltas` of them (0: the block does not exist), and the miniblocks that hold one.
FDB_PQW_HD uint32_t fdb_pqd_block_deltas(uint32_t deltas, uint32_t b) {
  const uint64_t first = (uint64_t)b * FDB_PQD_BLOCK;
  return first >= deltas ? 0 : (deltas - first < FDB_PQD_BLOCK ? (uint32_t)(deltas - first) : FDB_PQD_BLOCK);
}
FDB_PQW_HD uint32_t fdb_pqd_minis(uint32_t block_deltas) { return (block_deltas + FDB_PQD_MINI - 1) / FDB_PQD_MINI; }

FDB_PQW_HD uint64_t fdb_pqd_delta(const uint64_t* v, uint64_t i) { return v[i + 1] - v[i]; }   // wraps
FDB_PQW_HD uint64_t fdb_pqd_rel(uint64_t delta, int64_t min) { return delta - (uint64_t)min; }  // wraps; < 2^width of its miniblock
FDB_PQW_HD uint32_t fdb_pqd_bit_length(uint64_t x) { return x == 0 ? 0u : 64u - (uint32_t)__builtin_clzll(x); }
FDB_PQW_HD uint32_t fdb_pqd_width(uint32_t widths, uint32_t m) { return (widths >> (8 * m)) & 0xFFu; }
FDB_PQW_HD uint32_t fdb_pqd_set_width(uint32_t widths, uint32_t m, uint32_t w) { return widths | (w << (8 * m)); }

FDB_PQW_HD uint64_t fdb_pqd_zigzag(int64_t v) { return ((uint64_t)v << 1) ^ (uint64_t)(v >> 63); }
FDB_PQW_HD uint32_t fdb_pqd_varint_len(uint64_t v) { uint32_t n = 1; while (v >= 0x80) { n++; v >>= 7; } return n; }
// Byte i (< fdb_pqd_varint_len(v)) of varint(v).
FDB_PQW_HD unsigned char fdb_pqd_varint_byte(uint64_t v, uint32_t i) {
  const uint64_t rest = v >> (7 * i);  // (i <= 9: the shift stays below 64)
  return (unsigned char)((rest & 0x7F) | (rest >= 0x80 ? 0x80 : 0));
}

// A block: zigzag(min), four width bytes, `minis` miniblocks of width × 4 bytes.
FDB_PQW_HD uint32_t fdb_pqd_block_head_len(int64_t min) { return fdb_pqd_varint_len(fdb_pqd_zigzag(min)) + FDB_PQD_MINIS; }
FDB_PQW_HD uint32_t fdb_pqd_block_words(uint32_t widths, uint32_t minis) {
  uint32_t words = 0;
  for (uint32_t m = 0; m < minis; m++) words += fdb_pqd_width(widths, m);
  return words;
}
FDB_PQW_HD uint32_t fdb_pqd_block_bytes(int64_t min, uint32_t widths, uint32_t minis) { return fdb_pqd_block_head_len(min) + 4 * fdb_pqd_block_words(widths, minis); }
// Byte i of a block's head.
FDB_PQW_HD unsigned char fdb_pqd_block_head_byte(int64_t min, uint32_t widths, uint32_t i) {
  const uint64_t zz = fdb_pqd_zigzag(min);
  const uint32_t n = fdb_pqd_varint_len(zz);
  return i < n ? fdb_pqd_varint_byte(zz, i) : (unsigned char)fdb_pqd_width(widths, i - n);
}

// The page header: 80 01 | 04 | varint(count) | zigzag(first value; 0 when there is none).
FDB_PQW_HD uint32_t fdb_pqd_header_len(uint32_t count, uint64_t first) { return 3 + fdb_pqd_varint_len(count) + fdb_pqd_varint_len(fdb_pqd_zigzag((int64_t)first)); }
FDB_PQW_HD unsigned char fdb_pqd_header_byte(uint32_t count, uint64_t first, uint32_t i) {
  if (i < 3) return i == 0 ? 0x80 : i == 1 ? 0x01 : (unsigned char)FDB_PQD_MINIS;
  const uint32_t n = fdb_pqd_varint_len(count);
  return i - 3 < n ? fdb_pqd_varint_byte(count, i - 3) : fdb_pqd_varint_byte(fdb_pqd_zigzag((int64_t)first), i - 3 - n);
}
// The most a page of `rows` rows can need: the host checks what the device reports against it.
FDB_PQW_HD uint64_t fdb_pqd_max_page_bytes(uint32_t rows) { return FDB_PQD_MAX_HEADER + (uint64_t)fdb_pqd_blocks(fdb_pqd_deltas(rows)) * (10 + FDB_PQD_MINIS) + (uint64_t)fdb_pqd_minis(fdb_pqd_deltas(rows)) * 256; }

// Output word k (< w) of a miniblock at width w (1 … 64): rel[j] (< 2^w) sits at bit j × w of the miniblock, j < 32. No shift reaches 64:
// a value starts less than 32 bits above the word's first bit or less than w <= 64 bits below it.
FDB_PQW_HD uint32_t fdb_pqd_assemble_word(const uint64_t* rel, uint32_t w, uint32_t k) {
  const uint32_t lo = k << 5, hi = lo + 32;
  uint32_t out = 0;
  for (uint32_t j = lo / w; j < FDB_PQD_MINI; j++) {
    const uint32_t s = j * w;
    if (s >= hi) break;
    out |= s >= lo ? (uint32_t)(rel[j] << (s - lo)) : (uint32_t)(rel[j] >> (lo - s));
  }
  return out;
}

#ifndef FDB_PQWRITE_HOST_ONLY
// Compaction: of every column with a bitmap, the non-NULL values of page p in rank order to dense[first row of p …] (tile_base: the survey's).
hipError_t fdb_launch_pqd_compact(const FdbPqdCol* dcols, int32_t n_dcols, FdbPqwGeom g, const uint32_t* tile_base, hipStream_t stream);
// Block survey, then the page walk: blocks[(dcol × n_pages + page) × blocks_per_page + b] and page_bytes[dcol × n_pages + page] = the
// page's value bytes, header included. `stats`: the survey's table (the counts).
hipError_t fdb_launch_pqd_survey(const FdbPqdCol* dcols, int32_t n_dcols, FdbPqwGeom g, const FdbPqwPageStat* stats, FdbPqdBlock* blocks, uint32_t* page_bytes, hipStream_t stream);
// Encode: every DELTA page's value bytes into `image` from values_off[dcol × n_pages + page] on.
hipError_t fdb_launch_pqd_encode(const FdbPqdCol* dcols, int32_t n_dcols, FdbPqwGeom g, const FdbPqwPageStat* stats, const FdbPqdBlock* blocks, const uint64_t* values_off,
                                 unsigned char* image, hipStream_t stream);
#endif
