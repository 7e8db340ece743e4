// fdb_pqsnappy.h — the rule of the Parquet writer's SNAPPY compressor (kernels: fdb_pqsnappy.hip; host walk: below, used by fdb_pqwrite.cpp
// and behind fdb_selftest_parquet_write_compressed): ONE definition of the hash, of which earlier position a position is held against, of
// which position of a step wins, of how far a match reaches and of how literals and copies are tagged and split, for the kernel and for
// the host walk — as fdb_pqdelta.h is for the DELTA pages. The device's file is then byte for byte the host walk's.
//
// A page body of U bytes becomes the Snappy block  varint(U) | elements of fragment 0 | elements of fragment 1 | …  — the body cut into
// FRAGMENTS of FDB_PQS_FRAGMENT bytes (the last one shorter; a body of 0 bytes has none and is the block `00`). Every fragment is
// compressed on its own: no copy reaches before its fragment's first byte, so the fragments' elements concatenate into one valid block,
// every offset is below FDB_PQS_FRAGMENT <= 65 472 (what the project's device decoder reaches back), and positions fit 16 bits.
//
// One fragment src[0 … n), walked in WINDOWS of 64 positions from `cursor` on (a position p is one where 4 bytes are left: p + 4 <= n):
//   - a position's CANDIDATE is the nearest earlier position of the same window, at most FDB_PQS_NEAR back, holding the same 4 bytes
//     (runs, and values repeated with a short period — bit-packed indices at width 10 repeat every 5 bytes); where there is none, the
//     position the table holds under the hash of its 4 bytes, if that one holds the same 4 bytes. The table knows the positions before
//     the window only: under each hash the LARGEST of them (atomicMax on the device — nothing depends on which lane comes first).
//   - the LOWEST position of the window with a candidate wins. The bytes before it that no copy covered yet go out as one literal; the
//     match is extended byte by byte as far as the fragment goes (it may run over its own source: a run); it goes out as copies;
//     the next window starts behind it. No position has a candidate: the next window starts 64 further, the literal stays pending.
//   - before the next window every position below its start that is not in the table yet is put in.
//   - when fewer than 4 bytes are left behind the cursor, what is pending goes out as the last literal.
// Elements: a literal of L bytes is tagged in 1 byte (L <= 60), 2 (L <= 256) or 3 (L <= 65 536); a copy of `len` bytes is cut into
// 64-byte elements while 68 or more are left, one of 60 if then more than 64 are, and the rest (4 … 64); an element of 4 … 11 bytes from
// less than 2 048 back takes the 1-byte-offset form (2 bytes), every other the 2-byte-offset form (3 bytes). A copy never takes more bytes
// than it stands for and a literal at most 3 more, so a fragment of n bytes stays within fdb_pqs_bound(n) = 32 + n + n / 6, Snappy's own.
#pragma once

#include <stdint.h>

#include "fdb_pqwrite.h"

#define FDB_PQS_FRAGMENT 32768   // bytes of a page body compressed on their own; <= FDB_PAGE_RING_REACH (65 472) and <= 65 536
#define FDB_PQS_HASH_BITS 12
#define FDB_PQS_TABLE (1 << FDB_PQS_HASH_BITS)  // entries of a wave's table: position + 1 (0: nothing yet), 32 bits each for LDS atomics
#define FDB_PQS_WINDOW 64
#define FDB_PQS_NEAR 16          // how far back inside its window a position looks for its 4 bytes: the periods of equal values bit-packed at 1 … 16 bits, and 8-byte values twice
#define FDB_PQS_THREADS 128      // two waves, each with a fragment and a table of its own: 32 KiB of LDS
#define FDB_PQS_WAVES (FDB_PQS_THREADS / 64)
#define FDB_PQS_COMPRESS_GRID 2048  // workgroups of the compress launch; more fragments than 2 × that are strided over
#define FDB_PQS_COPY_PIECE 65536 // bytes of an uncompressed column's chunk one workgroup of the gather moves at a time

static_assert(FDB_PQS_FRAGMENT <= 65472 && FDB_PQS_FRAGMENT <= 65536, "fragments stay within the device decoder's reach and 16-bit positions");

// One fragment as the compress kernel sees it (made by the host from the staging layout), and what it leaves behind.
struct FdbPqsFrag {
  uint64_t src_off;              // where the fragment's bytes start in the staging image
  uint32_t len, page;            // 1 … FDB_PQS_FRAGMENT; the compressed page it belongs to (index into the page tables)
};
// A compressed page: its fragments are first_frag … first_frag + n_frags − 1.
struct FdbPqsPage { uint32_t first_frag, n_frags; };
// A byte range the gather moves as it is, staging image → final image (an uncompressed column's chunk, in pieces), and a few bytes the
// host contributes inside a page body, blob → staging image.
struct FdbPqsRange { uint64_t src_off, dst_off; uint32_t len, pad; };

FDB_PQW_HD uint32_t fdb_pqs_bound(uint32_t n) { return 32 + n + n / 6; }
FDB_PQW_HD uint32_t fdb_pqs_slot_bytes() { return (fdb_pqs_bound(FDB_PQS_FRAGMENT) + 63u) & ~63u; }  // a fragment's scratch slot
FDB_PQW_HD uint32_t fdb_pqs_fragments(uint64_t body) { return (uint32_t)((body + FDB_PQS_FRAGMENT - 1) / FDB_PQS_FRAGMENT); }
FDB_PQW_HD uint32_t fdb_pqs_varint_len(uint64_t v) { uint32_t n = 1; while (v >= 0x80) { n++; v >>= 7; } return n; }

FDB_PQW_HD uint32_t fdb_pqs_load32(const unsigned char* p) { uint32_t x; __builtin_memcpy(&x, p, 4); return x; }
FDB_PQW_HD uint32_t fdb_pqs_hash(uint32_t x) { return (x * 0x1e35a7bdu) >> (32 - FDB_PQS_HASH_BITS); }

// A literal of L bytes (1 … 65 536): its tag bytes, then the L bytes.
FDB_PQW_HD uint32_t fdb_pqs_literal_tag_len(uint32_t L) { return L <= 60 ? 1u : L <= 256 ? 2u : 3u; }
FDB_PQW_HD unsigned char fdb_pqs_literal_tag_byte(uint32_t L, uint32_t i) {
  if (L <= 60) return (unsigned char)((L - 1) << 2);
  if (i == 0) return (unsigned char)((L <= 256 ? 60u : 61u) << 2);
  return (unsigned char)((L - 1) >> (8 * (i - 1)));
}

// A copy of `len` bytes (>= 4) from `off` back, as elements: `full` of 64 bytes, then one of 60 where more than 64 are left, then the
// rest (4 … 64).
FDB_PQW_HD uint32_t fdb_pqs_copy_full(uint32_t len) { return len >= 68 ? (len - 4) / 64 : 0; }
FDB_PQW_HD uint32_t fdb_pqs_copy_mid(uint32_t len) { return len - 64 * fdb_pqs_copy_full(len) > 64 ? 60u : 0u; }
FDB_PQW_HD uint32_t fdb_pqs_copy_rest(uint32_t len) { return len - 64 * fdb_pqs_copy_full(len) - fdb_pqs_copy_mid(len); }
FDB_PQW_HD uint32_t fdb_pqs_copy_elem_len(uint32_t n, uint32_t off) { return n <= 11 && off < 2048 ? 2u : 3u; }  // one element of n bytes (4 … 64)
FDB_PQW_HD unsigned char fdb_pqs_copy_elem_byte(uint32_t n, uint32_t off, uint32_t i) {
  if (n <= 11 && off < 2048) return i == 0 ? (unsigned char)(1u | ((n - 4) << 2) | ((off >> 8) << 5)) : (unsigned char)off;
  return i == 0 ? (unsigned char)(2u | ((n - 1) << 2)) : (unsigned char)(off >> (8 * (i - 1)));
}
FDB_PQW_HD uint32_t fdb_pqs_copy_bytes(uint32_t len, uint32_t off) {
  return 3 * fdb_pqs_copy_full(len) + (fdb_pqs_copy_mid(len) != 0 ? 3u : 0u) + fdb_pqs_copy_elem_len(fdb_pqs_copy_rest(len), off);
}

// ---- the host walk: what pqs_compress_kernel does with one fragment, position by position ------------------------------------------------
// `table`: FDB_PQS_TABLE words of the caller's (cleared here); `out`: fdb_pqs_bound(n) bytes. Returns the bytes written.
inline uint32_t fdb_pqs_put_literal(const unsigned char* src, uint32_t from, uint32_t to, unsigned char* out, uint32_t o) {
  const uint32_t L = to - from;
  if (L == 0) return o;
  for (uint32_t i = 0; i < fdb_pqs_literal_tag_len(L); i++) out[o++] = fdb_pqs_literal_tag_byte(L, i);
  __builtin_memcpy(out + o, src + from, L);
  return o + L;
}
inline uint32_t fdb_pqs_put_copy(uint32_t len, uint32_t off, unsigned char* out, uint32_t o) {
  for (uint32_t k = 0; k < fdb_pqs_copy_full(len); k++) for (uint32_t i = 0; i < 3; i++) out[o++] = fdb_pqs_copy_elem_byte(64, off, i);
  if (fdb_pqs_copy_mid(len) != 0) for (uint32_t i = 0; i < 3; i++) out[o++] = fdb_pqs_copy_elem_byte(60, off, i);
  const uint32_t rest = fdb_pqs_copy_rest(len);
  for (uint32_t i = 0; i < fdb_pqs_copy_elem_len(rest, off); i++) out[o++] = fdb_pqs_copy_elem_byte(rest, off, i);
  return o;
}
// The search, shared with the LZ4_RAW rule (fdb_pqlz4.h), which bounds it by the page body's end: positions 0 … stop − 1 may win (here
// every position with 4 bytes left: fdb_pqs_stop(n)), a match is extended up to position `reach` (here n).
FDB_PQW_HD uint32_t fdb_pqs_stop(uint32_t n) { return n >= 4 ? n - 3 : 0; }
// The window at `cursor`: the lowest position with a candidate, if any.
inline bool fdb_pqs_find_host(const unsigned char* src, uint32_t cursor, uint32_t stop, const uint32_t* table, uint32_t* win, uint32_t* cand) {
  for (uint32_t l = 0; l < FDB_PQS_WINDOW; l++) {
    const uint32_t p = cursor + l;
    if (p >= stop) break;
    const uint32_t x = fdb_pqs_load32(src + p);
    for (uint32_t q = p; q > cursor && p - (q - 1) <= FDB_PQS_NEAR; q--)
      if (fdb_pqs_load32(src + q - 1) == x) { *win = p; *cand = q - 1; return true; }
    const uint32_t t = table[fdb_pqs_hash(x)];
    if (t != 0 && fdb_pqs_load32(src + t - 1) == x) { *win = p; *cand = t - 1; return true; }
  }
  return false;
}
inline uint32_t fdb_pqs_extend_host(const unsigned char* src, uint32_t win, uint32_t cand, uint32_t reach) {
  uint32_t len = 4;
  while (win + len < reach && src[cand + len] == src[win + len]) len++;
  return len;
}
// Every position below `cursor` that is not in the table yet is put in; returns the new `filled`.
inline uint32_t fdb_pqs_fill_host(const unsigned char* src, uint32_t* table, uint32_t filled, uint32_t cursor, uint32_t stop) {
  for (; filled < cursor && filled < stop; filled++) {
    uint32_t* e = table + fdb_pqs_hash(fdb_pqs_load32(src + filled));
    if (filled + 1 > *e) *e = filled + 1;
  }
  return filled;
}
inline uint32_t fdb_pqs_compress_fragment_host(const unsigned char* src, uint32_t n, uint32_t* table, unsigned char* out) {
  for (uint32_t i = 0; i < FDB_PQS_TABLE; i++) table[i] = 0;
  const uint32_t stop = fdb_pqs_stop(n);
  uint32_t cursor = 0, lit = 0, filled = 0, o = 0;
  while (cursor < stop) {
    uint32_t win = 0, cand = 0;
    if (fdb_pqs_find_host(src, cursor, stop, table, &win, &cand)) {
      const uint32_t len = fdb_pqs_extend_host(src, win, cand, n);
      o = fdb_pqs_put_literal(src, lit, win, out, o);
      o = fdb_pqs_put_copy(len, win - cand, out, o);
      cursor = lit = win + len;
    } else {
      cursor += FDB_PQS_WINDOW;
    }
    filled = fdb_pqs_fill_host(src, table, filled, cursor, stop);
  }
  return fdb_pqs_put_literal(src, lit, n, out, o);
}

#if defined(__HIPCC__) || defined(__HIP__)
// ---- the search on the device: what a wave does with one window, bounded by `stop` and `reach` — the LZ4_RAW compress kernel's ---------------
// (fdb_pqlz4.hip). pqs_compress_kernel holds the same steps inline, with stop = fdb_pqs_stop(n) and reach = n: calling these from it
// was measured and cost its compress pass 4 % (9.96 → 10.41 ms on 268 MB of page bodies, alternated runs), so it stays as it is.
// The lanes of one wave have written LDS and are about to read what the others wrote (or the other way round).
__device__ __forceinline__ void fdb_pqs_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ uint32_t fdb_pqs_lowest_lane(unsigned long long mask) { return mask != 0ull ? (uint32_t)__builtin_ctzll(mask) : 64u; }

// `len` bytes src → dst at any alignment, by the 64 lanes of a wave (or the `threads` threads of a workgroup).
__device__ __forceinline__ void fdb_pqs_copy_bytes(const unsigned char* __restrict__ src, unsigned char* __restrict__ dst, uint32_t len, uint32_t tid, uint32_t threads) {
  for (uint32_t i = tid * 4; i + 4 <= len; i += threads * 4) { const uint32_t x = fdb_pqs_load32(src + i); __builtin_memcpy(dst + i, &x, 4); }
  const uint32_t r = len & ~3u;
  if (r + tid < len) dst[r + tid] = src[r + tid];
}

// The 4 bytes of the position 64 further, loaded while this window is searched: the next window's, if nothing matches here.
struct FdbPqsAhead { uint32_t x = 0, at = ~0u; };

// The window at `cursor` (< stop), a lane a position: each lane looks its 4 bytes up in the table (positions before the window) and, by
// shuffles, in the FDB_PQS_NEAR lanes below it; a ballot finds the lowest lane with a candidate. True: *win and *cand are that position
// and what it is held against. False: no position has a candidate, and the window's own positions have gone into the table with the
// bytes the lanes hold (the caller's `filled` is cursor + FDB_PQS_WINDOW then).
__device__ __forceinline__ bool fdb_pqs_find(const unsigned char* __restrict__ src, uint32_t cursor, uint32_t stop, uint32_t* table, uint32_t lane, FdbPqsAhead* ahead, uint32_t* win,
                                             uint32_t* cand) {
  const uint32_t p = cursor + lane;
  const bool valid = p < stop;
  uint32_t x;
  if (ahead->at == cursor) x = ahead->x;
  else x = valid ? fdb_pqs_load32(src + p) : 0;
  const uint32_t t = valid ? table[fdb_pqs_hash(x)] : 0;
  const bool t_hit = t != 0 && fdb_pqs_load32(src + t - 1) == x;  // (t − 1 < cursor: 4 bytes are left there)
  ahead->x = p + FDB_PQS_WINDOW < stop ? fdb_pqs_load32(src + p + FDB_PQS_WINDOW) : 0;
  ahead->at = cursor + FDB_PQS_WINDOW;
  const unsigned long long t_mask = __ballot(t_hit);
  unsigned long long w_mask = 0;  // the lanes with a candidate inside the window, best_d back
  uint32_t best_d = 0, w = fdb_pqs_lowest_lane(t_mask);
  // the lanes up to the lowest one with a candidate try every distance up to FDB_PQS_NEAR, down to the window's first position:
  // a lane l has tried them all once d reaches l, so when d passes w no lane below w can turn up any more, and w's own nearest
  // is found. Eight distances at a step, so that the shuffles do not wait for each other's ballot (a distance past w finds
  // nothing below w).
  static_assert(FDB_PQS_NEAR % 8 == 0 && FDB_PQS_NEAR < FDB_PQS_WINDOW, "the distances are tried eight at a step");
  for (uint32_t d0 = 1; d0 <= FDB_PQS_NEAR && d0 <= w; d0 += 8) {
#pragma unroll
    for (uint32_t k = 0; k < 8; k++) {
      const uint32_t d = d0 + k;  // (FDB_PQS_NEAR at the most)
      const uint32_t y = (uint32_t)__shfl_up((int)x, d, 64);
      if (valid && lane >= d && y == x && best_d == 0) best_d = d;
    }
    w_mask = __ballot(best_d != 0);
    w = fdb_pqs_lowest_lane(w_mask | t_mask);
  }
  if (w < 64) {
    const uint32_t wd = (uint32_t)__shfl((int)best_d, (int)w, 64), wt = (uint32_t)__shfl((int)t, (int)w, 64);
    *win = cursor + w;
    *cand = wd != 0 ? cursor + w - wd : wt - 1;
    return true;
  }
  fdb_pqs_wave_sync();
  if (valid) atomicMax(&table[fdb_pqs_hash(x)], p + 1);
  fdb_pqs_wave_sync();
  return false;
}

// The match of `win` against `cand`, extended 64 bytes at a compare + ballot up to position `reach`.
__device__ __forceinline__ uint32_t fdb_pqs_extend(const unsigned char* __restrict__ src, uint32_t win, uint32_t cand, uint32_t reach, uint32_t lane) {
  uint32_t len = 4;
  for (;;) {
    const uint32_t i = len + lane;
    const bool same = win + i < reach && src[cand + i] == src[win + i];
    const unsigned long long mask = __ballot(same);
    if (mask != ~0ull) return len + (uint32_t)__builtin_ctzll(~mask);
    len += 64;
  }
}

// The positions filled … cursor − 1 go into the table: atomicMax of the position — the largest wins whatever lane comes first — and the
// wave waits before it looks anything up.
__device__ __forceinline__ void fdb_pqs_fill(const unsigned char* __restrict__ src, uint32_t* table, uint32_t filled, uint32_t cursor, uint32_t stop, uint32_t lane) {
  fdb_pqs_wave_sync();  // (every lane has looked up what it wanted)
  for (uint32_t base = filled; base < cursor; base += 64) {
    const uint32_t q = base + lane;
    if (q < cursor && q < stop) atomicMax(&table[fdb_pqs_hash(fdb_pqs_load32(src + q))], q + 1);
  }
  fdb_pqs_wave_sync();
}
#endif

#ifndef FDB_PQWRITE_HOST_ONLY
// Place: ranges[i].len bytes of blob[ranges[i].src_off …] → image[ranges[i].dst_off …] (the host's bytes inside the bodies of compressed pages).
hipError_t fdb_launch_pqs_place(const FdbPqsRange* ranges, int32_t n_ranges, const unsigned char* blob, unsigned char* image, hipStream_t stream);
// Compress: fragment f of `staging` → scratch[f × fdb_pqs_slot_bytes() …], its byte count → frag_bytes[f]. Then the scan: frag_off[f] = the
// bytes of the page's fragments before f, page_bytes[page] = those of all of them.
hipError_t fdb_launch_pqs_compress(const FdbPqsFrag* frags, int32_t n_frags, const unsigned char* staging, unsigned char* scratch, uint32_t* frag_bytes, hipStream_t stream);
hipError_t fdb_launch_pqs_scan(const FdbPqsPage* pages, int32_t n_pages, const uint32_t* frag_bytes, uint32_t* frag_off, uint32_t* page_bytes, hipStream_t stream);
// Gather: every fragment's elements → final[page_dst[page] + frag_off[f] …]; every range staging → final as it is.
hipError_t fdb_launch_pqs_gather(const FdbPqsFrag* frags, int32_t n_frags, const uint32_t* frag_bytes, const uint32_t* frag_off, const uint64_t* page_dst, const unsigned char* scratch,
                                 const FdbPqsRange* ranges, int32_t n_ranges, const unsigned char* staging, unsigned char* final_image, hipStream_t stream);
#endif
