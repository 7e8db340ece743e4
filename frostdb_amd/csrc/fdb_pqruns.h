// fdb_pqruns.h — the rule by which the Parquet writer cuts a page's dictionary indices or definition levels into the runs of the RLE /
// bit-packed hybrid (kernels: fdb_pqruns.hip; host walk: fdb_pqwrite.cpp): ONE definition of what a group is worth, of which groups
// become an RLE run, of every run's size and of its bytes, for the kernels and for the host walk behind fdb_selftest_parquet_write_runs —
// as fdb_pqdelta.h is for the DELTA pages.
//
// A STREAM is n symbols s[0 … n) at width w >= 1: a page's definition levels (w = 1, n = the page's rows, s = the validity bit) or an
// INDEX column's page values (w = the column's width, n = the page's non-NULL rows, s = the index, by rank). The rule applies where the
// writer would otherwise emit ONE bit-packed run (fdb_pqr_active); a page that is one RLE run stays as it is.
//   G = n / 8 full groups, then n mod 8 tail symbols. A full group is UNIFORM when its 8 symbols are equal; a STRETCH is a maximal
//   range of consecutive uniform groups of one value. T = ⌈16 / w⌉: a stretch of at least T groups is an RLE run —
//   varint(count << 1), the value in ⌈w / 8⌉ little-endian bytes. The tail joins the last RLE run when the stretch ending at group
//   G − 1 is one and every tail symbol equals its value. Every maximal range of the remaining groups is a bit-packed run —
//   varint((groups << 1) | 1), groups × w bytes, LSB first; a tail that joined nothing is one more zero-padded group at the end of
//   the last bit-packed run, a run of its own when an RLE run comes right before it.
// An RLE run stands for at least 16 packed bytes and costs at most 4 + 4, and 4 more for the header of the bit-packed run it splits
// off (a page has at most 2^24 rows: every header is at most 4 bytes), so a stream is never longer than its one bit-packed run.
//
// A group's KEY is its value when it is uniform and FDB_PQR_MIXED otherwise (no index is 2^32 − 1: a dictionary has fewer than 2^32
// entries); its CLASS is its key when its stretch is long enough and FDB_PQR_MIXED — bit-packed — otherwise. Neighbouring groups of
// one class are one run. Whether a stretch reaches T is seen from T − 1 groups to either side, which is what lets the kernels decide
// it from a window.
#pragma once

#include "fdb_pqwrite.h"

#define FDB_PQR_MIXED 0xFFFFFFFFu
#define FDB_PQR_CHUNK 256        // groups a workgroup takes at a step, one per lane (1 024 measured no faster: §9)
#define FDB_PQR_HALO 16          // keys staged to either side of a chunk: T − 1 <= 15 for the class of the chunk's neighbours, + 1

// One stream of a column as the kernels see it. `dense`: an INDEX column's non-NULL indices, those of page p in rank order from
// dense[first row of p] on — the column itself when it has no bitmap, else scratch the compaction pass fills. `levels` != 0: the
// stream is the column's definition levels, read from `validity`.
struct FdbPqrStream {
  const uint32_t* values;
  const unsigned char* validity;
  uint32_t* dense;
  int32_t col, width;              // its place in the survey's tables (FdbPqwPageStat, tile_base); the symbols' width
  int32_t levels, pad;
};

FDB_PQW_HD uint32_t fdb_pqr_threshold(uint32_t w) { return (16 + w - 1) / w; }
FDB_PQW_HD uint32_t fdb_pqr_value_bytes(uint32_t w) { return (w + 7) / 8; }
FDB_PQW_HD uint32_t fdb_pqr_varint_len(uint32_t v) { return v < (1u << 7) ? 1 : v < (1u << 14) ? 2 : v < (1u << 21) ? 3 : v < (1u << 28) ? 4 : 5; }
FDB_PQW_HD unsigned char fdb_pqr_varint_byte(uint32_t v, uint32_t i) { return (unsigned char)(((v >> (7 * i)) & 0x7F) | ((v >> (7 * i)) >= 0x80 ? 0x80 : 0)); }  // i < fdb_pqr_varint_len(v)
FDB_PQW_HD uint32_t fdb_pqr_rle_header(uint32_t symbols) { return symbols << 1; }
FDB_PQW_HD uint32_t fdb_pqr_packed_header(uint32_t groups) { return (groups << 1) | 1; }
FDB_PQW_HD uint32_t fdb_pqr_rle_bytes(uint32_t symbols, uint32_t w) { return fdb_pqr_varint_len(fdb_pqr_rle_header(symbols)) + fdb_pqr_value_bytes(w); }
FDB_PQW_HD uint32_t fdb_pqr_packed_bytes(uint32_t groups, uint32_t w) { return fdb_pqr_varint_len(fdb_pqr_packed_header(groups)) + groups * w; }

// The stream of a page whose survey counted `count` non-NULL rows of `rows`, the indices among them from mn to mx: its symbols, and
// whether the rule applies — the page's levels or indices would be ONE bit-packed run.
FDB_PQW_HD uint32_t fdb_pqr_symbols(bool levels, uint32_t count, uint32_t rows) { return levels ? rows : count; }
FDB_PQW_HD bool fdb_pqr_active(bool levels, uint32_t count, uint32_t rows, uint32_t mn, uint32_t mx) { return levels ? (count > 0 && count < rows) : (count > 0 && mn != mx); }
// What the host holds a stream's size to before it trusts it: not more than the one bit-packed run, not less than the smallest run.
FDB_PQW_HD uint32_t fdb_pqr_max_bytes(uint32_t n, uint32_t w) { return fdb_pqr_packed_bytes(fdb_pqw_groups(n), w); }
FDB_PQW_HD uint32_t fdb_pqr_min_bytes(uint32_t w) { return 1 + fdb_pqr_value_bytes(w); }

// The key of k symbols (8: a full group; fewer: the tail).
FDB_PQW_HD uint32_t fdb_pqr_group_key(const uint32_t* sym, uint32_t k) {
  const uint32_t v = sym[0];
  for (uint32_t i = 1; i < k; i++)
    if (sym[i] != v) return FDB_PQR_MIXED;
  return v;
}
// … of k definition levels, bit i of `byte` the level of the group's row i (bits from k on are zero).
FDB_PQW_HD uint32_t fdb_pqr_level_key(uint32_t byte, uint32_t k) { return byte == 0 ? 0u : byte == (1u << k) - 1 ? 1u : FDB_PQR_MIXED; }

// Does the stretch of group i reach T groups? key[lo … hi) are the keys around it — of the page's full groups, FDB_PQR_MIXED where
// there is none (before the first, from the tail on) — and hold at least T − 1 to either side of i.
FDB_PQW_HD bool fdb_pqr_long(const uint32_t* key, int32_t i, int32_t lo, int32_t hi, uint32_t T) {
  const uint32_t v = key[i];
  if (v == FDB_PQR_MIXED) return false;
  uint32_t n = 1;
  for (int32_t k = i - 1; n < T && k >= lo && key[k] == v; k--) n++;
  for (int32_t k = i + 1; n < T && k < hi && key[k] == v; k++) n++;
  return n >= T;
}
FDB_PQW_HD uint32_t fdb_pqr_class(const uint32_t* key, int32_t i, int32_t lo, int32_t hi, uint32_t T) { return fdb_pqr_long(key, i, lo, hi, T) ? key[i] : FDB_PQR_MIXED; }
// The tail's class: the class of group G − 1 when that is an RLE run of the tail's key, else bit-packed.
FDB_PQW_HD uint32_t fdb_pqr_tail_class(uint32_t tail_key, bool has_group, uint32_t last_class) {
  return has_group && tail_key != FDB_PQR_MIXED && last_class == tail_key ? tail_key : FDB_PQR_MIXED;
}

// Byte b (< w) of a bit-packed group: sym[0 … 8) at w bits each (cut to w bits, padding zero), least significant bit first.
FDB_PQW_HD unsigned char fdb_pqr_group_byte(const uint32_t* sym, uint32_t w, uint32_t b) {
  const uint32_t lo = 8 * b;
  uint32_t out = 0;
  for (uint32_t k = lo / w; k < 8; k++) {
    const uint32_t s = k * w;
    if (s >= lo + 8) break;
    out |= s >= lo ? sym[k] << (s - lo) : sym[k] >> (lo - s);
  }
  return (unsigned char)out;
}

#ifndef FDB_PQWRITE_HOST_ONLY
#include <hip/hip_runtime_api.h>
// Compaction: the indices of every value stream with a bitmap, by rank, into its `dense`.
hipError_t fdb_launch_pqr_compact(const FdbPqrStream* streams, int32_t n_streams, FdbPqwGeom g, const uint32_t* tile_base, hipStream_t stream);
// Run survey: page_bytes[stream × n_pages + page] = the bytes of the page's stream cut into runs; 0 where the rule does not apply.
hipError_t fdb_launch_pqr_survey(const FdbPqrStream* streams, int32_t n_streams, FdbPqwGeom g, const FdbPqwPageStat* stats, uint32_t* page_bytes, hipStream_t stream);
// Run encode: every such stream's runs into `image`, from out[stream × n_pages + page] on (FDB_PQW_NONE: nothing to write).
hipError_t fdb_launch_pqr_encode(const FdbPqrStream* streams, int32_t n_streams, FdbPqwGeom g, const FdbPqwPageStat* stats, const uint32_t* page_bytes, const uint64_t* out,
                                 unsigned char* image, hipStream_t stream);
#endif
