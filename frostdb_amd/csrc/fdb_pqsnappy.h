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
inline uint32_t fdb_pqs_compress_fragment_host(const unsigned char* src, uint32_t n, uint32_t* table, unsigned char* out) {
  for (uint32_t i = 0; i < FDB_PQS_TABLE; i++) table[i] = 0;
  uint32_t cursor = 0, lit = 0, filled = 0, o = 0;
  while (cursor + 4 <= n) {
    uint32_t win = 0, cand = 0;
    bool found = false;
    for (uint32_t l = 0; l < FDB_PQS_WINDOW && !found; l++) {
      const uint32_t p = cursor + l;
      if (p + 4 > n) break;
      const uint32_t x = fdb_pqs_load32(src + p);
      for (uint32_t q = p; q > cursor && p - (q - 1) <= FDB_PQS_NEAR && !found; q--)
        if (fdb_pqs_load32(src + q - 1) == x) { found = true; win = p; cand = q - 1; }
      if (!found) {
        const uint32_t t = table[fdb_pqs_hash(x)];
        if (t != 0 && fdb_pqs_load32(src + t - 1) == x) { found = true; win = p; cand = t - 1; }
      }
    }
    if (found) {
      uint32_t len = 4;
      while (win + len < n && src[cand + len] == src[win + len]) len++;
      o = fdb_pqs_put_literal(src, lit, win, out, o);
      o = fdb_pqs_put_copy(len, win - cand, out, o);
      cursor = lit = win + len;
    } else {
      cursor += FDB_PQS_WINDOW;
    }
    for (; filled < cursor && filled + 4 <= n; filled++) {
      uint32_t* e = table + fdb_pqs_hash(fdb_pqs_load32(src + filled));
      if (filled + 1 > *e) *e = filled + 1;
    }
  }
  return fdb_pqs_put_literal(src, lit, n, out, o);
}

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
