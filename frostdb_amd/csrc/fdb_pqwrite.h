// fdb_pqwrite.h — the arithmetic of the Parquet writer (fdb_pqwrite.cpp; kernels in fdb_pqwrite.hip): ONE definition of the page geometry,
// of where a value's bits go and of how an output word is put together, for the kernels and for the host walk behind
// fdb_selftest_parquet_write — as fdb_mergepath.h is for the merge and fdb_sortkey.h for the key encoding.
//
// A record of `rows` rows is cut into pages of `page_rows` rows (a multiple of 64, so a page starts on a word of the validity bitmap) and
// a page into tiles of at most FDB_PQW_TILE rows; a tile is what one workgroup encodes at a time, and it never crosses a page. Parquet
// stores non-NULL values only: value number j of a page (its RANK: the non-NULL rows of the page before it) of a run bit-packed at width w
// starts at bit j × w of the run's payload, least significant bit first. The writer produces the whole file body in one image; `payload`
// below is the image byte where a run's first payload byte sits — in general neither word- nor even byte-pair-aligned — and an output
// WORD is an aligned 32-bit word of the image.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) || defined(__HIP__)
#include <hip/hip_runtime.h>
#define FDB_PQW_HD __host__ __device__ __forceinline__
#else
#define FDB_PQW_HD inline
#endif

#define FDB_PQW_BLOCK 256
#define FDB_PQW_TILE 4096        // rows per tile: 64 validity words, 16 KiB of staged indices
#define FDB_PQW_TILE_WORDS (FDB_PQW_TILE / 64)
#define FDB_PQW_STAGE_WORDS (FDB_PQW_TILE + FDB_PQW_TILE / 32)  // fdb_pqw_slot
#define FDB_PQW_MAX_GRID 1024    // workgroups per launch; more work items than that are strided over
#define FDB_PQW_NONE (~0ull)     // FdbPqwPageOut: nothing for the device to write there

enum { FDB_PQW_V64 = 0, FDB_PQW_BOOL = 1, FDB_PQW_INDEX = 2 };

// One column as the kernels see it. `validity` == nullptr: every row counts (no NULLs, or a required column).
struct FdbPqwCol {
  const void* values;             // 8 bytes per row (V64, BOOL: 1 = false / 2 = true) or a uint32 index per row
  const unsigned char* validity;  // bit i = row i is not NULL; bits past `rows` are undefined, whole 64-bit words are readable
  int32_t kind;
  int32_t width;                  // BOOL: 1, INDEX: bits of (entries - 1); 0 = nothing is packed
};
struct FdbPqwGeom {
  int64_t rows, n_pages;
  int32_t page_rows, tiles_per_page, n_cols, pad;
};
// What the survey leaves per (column, page): the non-NULL rows, and the smallest and largest index among them (INDEX columns; mn > mx
// when there is none).
struct FdbPqwPageStat { uint32_t count, mn, mx, pad; };
// Where the encode pass writes a (column, page)'s payloads in the image (FDB_PQW_NONE: an RLE run, written by the host).
struct FdbPqwPageOut { uint64_t levels_off, values_off; };

FDB_PQW_HD int64_t fdb_pqw_pages(int64_t rows, int32_t page_rows) { return (rows + page_rows - 1) / page_rows; }
FDB_PQW_HD int32_t fdb_pqw_tiles_per_page(int32_t page_rows) { return (page_rows + FDB_PQW_TILE - 1) / FDB_PQW_TILE; }
FDB_PQW_HD int64_t fdb_pqw_page_first(const FdbPqwGeom& g, int64_t page) { return page * g.page_rows; }
FDB_PQW_HD int64_t fdb_pqw_page_end(const FdbPqwGeom& g, int64_t page) {
  const int64_t e = (page + 1) * g.page_rows;
  return e < g.rows ? e : g.rows;
}
// Rows [first, end) of tile `t` of `page`; first >= end: the tile is empty (the record's last page is short).
FDB_PQW_HD void fdb_pqw_tile_rows(const FdbPqwGeom& g, int64_t page, int32_t t, int64_t* first, int64_t* end) {
  const int64_t pe = fdb_pqw_page_end(g, page), f = fdb_pqw_page_first(g, page) + (int64_t)t * FDB_PQW_TILE, e = f + FDB_PQW_TILE;
  *first = f;
  *end = e < pe ? e : pe;
}

FDB_PQW_HD int fdb_pqw_popc(uint64_t x) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __popcll(x);
#else
  return __builtin_popcountll(x);
#endif
}

// Validity word `wi` of the rows from `first` (a multiple of 64) on, with the bits of rows >= end cleared: what a page's definition
// levels hold for those rows, padding bits zero.
FDB_PQW_HD uint64_t fdb_pqw_valid_word(const unsigned char* validity, int64_t first, int wi, int64_t end) {
  const int64_t row = first + (int64_t)wi * 64;
  if (row >= end) return 0;
  const int64_t n = end - row;
  const uint64_t mask = n >= 64 ? ~0ull : ((1ull << n) - 1);
  if (validity == nullptr) return mask;
  uint64_t w;
  __builtin_memcpy(&w, validity + (row >> 3), 8);
  return w & mask;
}

// Sizes of a page's parts.
FDB_PQW_HD uint32_t fdb_pqw_level_bytes(uint32_t rows) { return (rows + 7) / 8; }    // a bit-packed level run: ⌈rows/8⌉ groups of one byte
FDB_PQW_HD uint32_t fdb_pqw_groups(uint32_t values) { return (values + 7) / 8; }     // groups of eight values of a bit-packed run
FDB_PQW_HD uint64_t fdb_pqw_packed_bytes(uint32_t values, uint32_t w) { return (uint64_t)fdb_pqw_groups(values) * w; }
FDB_PQW_HD uint32_t fdb_pqw_bits(uint64_t max_index) { uint32_t w = 0; while (max_index != 0) { w++; max_index >>= 1; } return w; }  // bits(entries − 1)

// Staged values sit at slot(j): one word of padding every 32, so that the lanes of a wave, which at width 1 start 32 values apart,
// do not all read one LDS bank.
FDB_PQW_HD uint32_t fdb_pqw_slot(uint32_t j) { return j + (j >> 5); }

// The image words a tile's values touch: ranks [first, first + count) of the run whose payload starts at image BIT `payload_bit`.
FDB_PQW_HD uint64_t fdb_pqw_first_word(uint64_t payload_bit, uint64_t first, uint32_t w) { return (payload_bit + first * w) >> 5; }
FDB_PQW_HD uint64_t fdb_pqw_last_word(uint64_t payload_bit, uint64_t first, uint32_t count, uint32_t w) { return (payload_bit + (first + count) * w - 1) >> 5; }

// What the tile's values contribute to image word `k`: vals[slot(j)] is the value of rank first + j (j < count), already cut to w bits
// (1 <= w <= 32). Values of other tiles that share the word are not seen here — the first and the last word of a tile are OR-ed into
// the zeroed image, the words between are stored.
FDB_PQW_HD uint32_t fdb_pqw_assemble_word(const uint32_t* vals, uint64_t first, uint32_t count, uint64_t payload_bit, uint32_t w, uint64_t k) {
  const uint64_t lo = k << 5, hi = lo + 32, run0 = payload_bit + first * w;
  uint32_t j = lo > run0 ? (uint32_t)(lo - run0) / w : 0;  // the value that holds bit `lo` (a tile's bits fit 32 bits: 4096 × 32)
  uint32_t out = 0;
  for (; j < count; j++) {
    const uint64_t s = run0 + (uint64_t)j * w;
    if (s >= hi) break;
    const uint32_t v = vals[fdb_pqw_slot(j)];
    out |= s >= lo ? v << (uint32_t)(s - lo) : v >> (uint32_t)(lo - s);
  }
  return out;
}

#ifndef FDB_PQWRITE_HOST_ONLY
#include <hip/hip_runtime_api.h>
// Survey: stats[col × n_pages + page] and tile_base[(col × n_pages + page) × tiles_per_page + tile] = the rank of the tile's first value.
hipError_t fdb_launch_pqw_survey(const FdbPqwCol* cols, FdbPqwGeom g, FdbPqwPageStat* stats, uint32_t* tile_base, hipStream_t stream);
// Encode: every payload of every page into `image` (zeroed, a multiple of 4 bytes long) at the offsets of `out`.
hipError_t fdb_launch_pqw_encode(const FdbPqwCol* cols, FdbPqwGeom g, const FdbPqwPageOut* out, const uint32_t* tile_base, unsigned char* image, hipStream_t stream);
#endif
