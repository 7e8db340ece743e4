// fdb_pqbytes.h — the arithmetic of the Parquet writer's VALUE pages of BYTE_ARRAY columns (kernels: fdb_pqbytes.hip; host walk and layout:
// fdb_pqwrite.cpp): ONE definition of what a value costs, of where a byte of a tile's output comes from and of how an output word is put
// together, for the kernels and for the host walk behind fdb_selftest_parquet_write_strings — as fdb_pqdelta.h is for the DELTA pages.
//
// A dictionary / string / binary column written with a FORM (fdb_parquet_string_options) has no dictionary page: a page's non-NULL values
// follow its definition levels in row order, as
//   PLAIN                     per value the 4-byte little-endian length, then the entry's bytes;
//   DELTA_LENGTH_BYTE_ARRAY   the lengths as ONE DELTA_BINARY_PACKED block sequence (fdb_pqdelta.h: the lengths are handed to those passes
//                             as a 64-bit column in rank order), then every value's bytes back to back.
// The BYTE STREAM of a page is what the byte encode pass writes: everything of a PLAIN page, the bytes behind the lengths of a DELTA_LENGTH
// one. The entries are read from two tables per column: entry_off[e] … entry_off[e + 1] are entry e's bytes in entry_bytes (entries + 1
// offsets; the writer refuses a dictionary of 2^31 bytes or more, so they fit 32 bits). A tile's share of the stream starts at a byte the
// host knows from the byte survey's per-tile sums; inside the tile the values' exclusive byte offsets off[0 … count] (off[count]: the
// tile's bytes) are staged, and the output is produced BY OUTPUT POSITION: whoever owns output byte `pos` finds the value j with
// off[j] <= pos < off[j + 1] and reads its source byte — so stores are contiguous whatever the lengths are, one long entry and thousands of
// empty ones take the same code. An output WORD is an aligned 32-bit word of the image (fdb_pqwrite.h); a word the tile owns whole is
// stored, one it shares — with a neighbouring tile, page or bytes of the host — is OR-ed into the zeroed image, as in the encode pass.
#pragma once

#include "fdb_pqwrite.h"

#define FDB_PQY_THREADS 256
#define FDB_PQY_PER_THREAD (FDB_PQW_TILE / FDB_PQY_THREADS)  // values of a tile each thread scans

enum { FDB_PQY_DICTIONARY = 0, FDB_PQY_PLAIN = 1, FDB_PQY_DELTA_LENGTH = 2 };  // fdb_parquet_string_options::forms

// One column with a form as the kernels see it.
struct FdbPqyCol {
  const uint32_t* values;            // the column's index per row
  const unsigned char* validity;     // nullptr: every row counts
  const uint32_t* entry_off;         // entries + 1
  const unsigned char* entry_bytes;
  uint64_t* lengths;                 // DELTA_LENGTH: the non-NULL rows' lengths, those of page p in rank order from lengths[first row of p] on — the
                                     // scratch column the DELTA passes read (FdbPqdCol::dense); nullptr for PLAIN
  uint32_t entries;
  int32_t col;                       // its place in the survey's tables (FdbPqwPageStat, tile_base)
  int32_t plain, pad;                // 1: PLAIN — a value is its length bytes and its bytes
};

// An index at or past the dictionary is the layout's to refuse (the survey's table says so); until then it counts as an empty value.
FDB_PQW_HD uint32_t fdb_pqy_entry_len(const uint32_t* entry_off, uint32_t entries, uint32_t v) { return v < entries ? entry_off[v + 1] - entry_off[v] : 0u; }
// What a value of `len` bytes adds to the byte stream.
FDB_PQW_HD uint32_t fdb_pqy_value_bytes(uint32_t len, bool plain) { return len + (plain ? 4u : 0u); }

// The value that output byte `pos` (< off[count]) of a tile belongs to: the j with off[j] <= pos < off[j + 1]; values without a byte
// (off[j] == off[j + 1]) are never found.
FDB_PQW_HD uint32_t fdb_pqy_find(const uint32_t* off, uint32_t count, uint32_t pos) {
  uint32_t lo = 0, hi = count;  // off[lo] <= pos < off[hi]
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if (off[mid] <= pos) lo = mid; else hi = mid;
  }
  return lo;
}

// Output byte `pos` of the tile, which belongs to value j (of entry idx[j]).
FDB_PQW_HD unsigned char fdb_pqy_byte(const uint32_t* off, const uint32_t* idx, uint32_t j, uint32_t pos, bool plain, const uint32_t* entry_off, const unsigned char* entry_bytes) {
  uint32_t in = pos - off[j];
  if (plain) {
    if (in < 4) return (unsigned char)((off[j + 1] - off[j] - 4u) >> (8 * in));  // the length, little-endian
    in -= 4;
  }
  return entry_bytes[(uint64_t)entry_off[idx[j]] + in];
}

// The image words a tile's `total` (> 0) bytes from image byte `dst` on touch.
FDB_PQW_HD uint64_t fdb_pqy_first_word(uint64_t dst) { return dst >> 2; }
FDB_PQW_HD uint64_t fdb_pqy_last_word(uint64_t dst, uint32_t total) { return (dst + total - 1) >> 2; }

// What the tile contributes to image word k (first_word <= k <= last_word): its bytes of the word, and in *mask 0xFF for each of them —
// 0xFFFFFFFF: the word is the tile's alone.
FDB_PQW_HD uint32_t fdb_pqy_word(const uint32_t* off, const uint32_t* idx, uint32_t count, bool plain, const uint32_t* entry_off, const unsigned char* entry_bytes, uint64_t dst,
                                 uint32_t total, uint64_t k, uint32_t* mask) {
  const uint64_t lo = k << 2, end = dst + total;
  const uint32_t b0 = lo < dst ? (uint32_t)(dst - lo) : 0u, b1 = end - lo >= 4 ? 4u : (uint32_t)(end - lo);
  uint32_t pos = (uint32_t)(lo + b0 - dst), j = fdb_pqy_find(off, count, pos), word = 0, m = 0;
  for (uint32_t b = b0; b < b1; b++, pos++) {
    while (pos >= off[j + 1]) j++;  // (pos < off[count]: j stays below count)
    word |= (uint32_t)fdb_pqy_byte(off, idx, j, pos, plain, entry_off, entry_bytes) << (8 * b);
    m |= 0xFFu << (8 * b);
  }
  *mask = m;
  return word;
}

#ifndef FDB_PQWRITE_HOST_ONLY
// Byte survey: tile_bytes[(ycol × n_pages + page) × tiles_per_page + tile] = what the tile's non-NULL rows add to the page's byte stream;
// of a DELTA_LENGTH column the rows' lengths go to `lengths` on the way (tile_base: the survey's).
hipError_t fdb_launch_pqy_survey(const FdbPqyCol* ycols, int32_t n_ycols, FdbPqwGeom g, const uint32_t* tile_base, uint64_t* tile_bytes, hipStream_t stream);
// Byte encode: every tile's share of its page's byte stream into `image` (zeroed), from bytes_out[ycol × n_pages + page] (FDB_PQW_NONE: the
// page has no value) + byte_base[(ycol × n_pages + page) × tiles_per_page + tile] on.
hipError_t fdb_launch_pqy_encode(const FdbPqyCol* ycols, int32_t n_ycols, FdbPqwGeom g, const uint64_t* bytes_out, const uint64_t* byte_base, unsigned char* image, hipStream_t stream);
#endif
