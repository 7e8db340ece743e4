// fdb_pqlz4.h — the rule of the Parquet writer's LZ4_RAW compressor (kernels: fdb_pqlz4.hip; host walk: below, used by fdb_pqwrite.cpp
// for the dictionary pages and behind fdb_selftest_parquet_write_*): ONE definition of where a match may start and end, of what a
// fragment leaves behind and of how the fragments' sequences join into one block, for the kernels and for the host walk — as
// fdb_pqsnappy.h is for SNAPPY, whose match search (hash, windows, nearest candidate, table) this rule takes over as it is.
//
// A page body of U bytes becomes ONE LZ4 block, bare (Parquet's LZ4_RAW has no preamble): a chain of SEQUENCES, each a token, the
// literal length's extension, the literals, a 2-byte offset and the match length's extension; the last sequence has literals only. A
// length's nibble of the token is min(v, 15) — v the literal count, or the match length − 4 — and v >= 15 is followed by (v − 15) / 255
// bytes of 255 and one byte (v − 15) % 255. A body of 0 bytes is the one byte `00`.
//
// Matches: the body is cut into fragments of FDB_PQS_FRAGMENT bytes and every fragment is searched as fdb_pqsnappy.h searches it — no
// match reaches before its fragment's first byte, so offsets stay below 32 768 — with the block format's two end conditions, which are
// the BODY's and not the fragment's: a position may win only if it is at most U − 12 (fdb_pql_stop), and a match is extended only up
// to body position U − 5 (fdb_pql_reach). They touch the last fragment and, when that one is shorter than 12 bytes, the one before it.
//
// Block: the literals of a sequence are every body byte since the previous match's end, across fragment boundaries and across whole
// fragments without a match. So a fragment cannot finish its first sequence alone; it leaves (FdbPqlOut) `head`, the bytes before its
// first match; `tail`, the bytes behind its last; the first match's length; and in its scratch slot the MIDDLE: the first match's offset
// and length extension, then every later sequence whole, without the trailing literals. A walk over a page's fragments in order with a
// CARRY — the literal bytes pending in front of the fragment — then places them: a fragment with a match opens with a run of carry +
// head literals (token, extension, the run, then its middle) and leaves carry = tail; one without adds its length to the carry; the
// closing sequence holds the last carry. A match of m bytes takes 3 + its extension <= m − 1 bytes and literals one more byte per
// 255, so a page stays within fdb_pql_bound(U) = U + U / 255 + 16, LZ4_compressBound.
#pragma once

#include "fdb_pqsnappy.h"

// One fragment as the compress kernel sees it, and what it leaves behind.
struct FdbPqlFrag {
  uint64_t src_off;              // where the fragment's bytes start in the staging image
  uint32_t len, page;            // 1 … FDB_PQS_FRAGMENT; the LZ4 page it belongs to (index into the page tables)
  uint32_t stop, reach;          // fdb_pql_stop / fdb_pql_reach of the fragment in its body
};
struct FdbPqlOut { uint32_t head, tail, first_len, mid_bytes; };  // first_len == 0: no match — head is the fragment's length, tail and mid_bytes 0
// An LZ4 page: its fragments are first_frag … first_frag + n_frags − 1, its body ends at src_end in the staging image.
struct FdbPqlPage { uint64_t src_end; uint32_t first_frag, n_frags; };
// What the scan leaves: per fragment with a match where its share of the page's block starts and how many literals its first sequence
// holds (carry + head); per page where the closing sequence starts and its literals.
struct FdbPqlPlace { uint32_t off, run; };

FDB_PQW_HD uint64_t fdb_pql_bound(uint64_t n) { return n + n / 255 + 16; }
FDB_PQW_HD uint32_t fdb_pql_slot_bytes() { return ((uint32_t)fdb_pql_bound(FDB_PQS_FRAGMENT) + 63u) & ~63u; }  // a fragment's scratch slot

// The fragment of `n` bytes at `base` of a body of U: its positions 0 … stop − 1 may win, a match ends at position `reach` at the latest.
FDB_PQW_HD uint32_t fdb_pql_stop(uint64_t base, uint32_t n, uint64_t U) {
  if (U < base + 12) return 0;
  const uint64_t by_body = U - 12 - base + 1;
  const uint32_t by_frag = fdb_pqs_stop(n);
  return by_body < by_frag ? (uint32_t)by_body : by_frag;
}
FDB_PQW_HD uint32_t fdb_pql_reach(uint64_t base, uint32_t n, uint64_t U) {
  if (U < base + 5) return 0;
  const uint64_t by_body = U - 5 - base;
  return by_body < n ? (uint32_t)by_body : n;
}

// A length v (the literals, or the match length − 4): its nibble, and its extension bytes.
FDB_PQW_HD uint32_t fdb_pql_nibble(uint32_t v) { return v < 15 ? v : 15u; }
FDB_PQW_HD uint32_t fdb_pql_ext_len(uint32_t v) { return v < 15 ? 0u : (v - 15) / 255 + 1; }
FDB_PQW_HD unsigned char fdb_pql_ext_byte(uint32_t v, uint32_t i) { return i < (v - 15) / 255 ? (unsigned char)255 : (unsigned char)((v - 15) % 255); }
// The token of `literals` literals and a match of match_len bytes (0: the closing sequence, which has none).
FDB_PQW_HD unsigned char fdb_pql_token(uint32_t literals, uint32_t match_len) {
  return (unsigned char)((fdb_pql_nibble(literals) << 4) | (match_len != 0 ? fdb_pql_nibble(match_len - 4) : 0u));
}

// ---- the host walk: what the three kernels do, position by position ----------------------------------------------------------------------
inline uint32_t fdb_pql_put_ext(uint32_t v, unsigned char* out, uint32_t o) {
  for (uint32_t i = 0; i < fdb_pql_ext_len(v); i++) out[o++] = fdb_pql_ext_byte(v, i);
  return o;
}
// A sequence's front: token, literal extension, the literals src[0 … literals).
inline uint64_t fdb_pql_put_run(const unsigned char* src, uint32_t literals, uint32_t match_len, unsigned char* out, uint64_t o) {
  out[o++] = fdb_pql_token(literals, match_len);
  for (uint32_t i = 0; i < fdb_pql_ext_len(literals); i++) out[o++] = fdb_pql_ext_byte(literals, i);
  if (literals != 0) __builtin_memcpy(out + o, src, literals);  // (a body of 0 bytes may have no address)
  return o + literals;
}
// … and its back: the offset, the match length's extension.
inline uint32_t fdb_pql_put_match(uint32_t off, uint32_t match_len, unsigned char* out, uint32_t o) {
  out[o++] = (unsigned char)off;
  out[o++] = (unsigned char)(off >> 8);
  return fdb_pql_put_ext(match_len - 4, out, o);
}
// What pql_compress_kernel does with one fragment. `table`: FDB_PQS_TABLE words of the caller's (cleared here); `mid`: fdb_pql_slot_bytes().
inline FdbPqlOut fdb_pql_compress_fragment_host(const unsigned char* src, uint32_t n, uint32_t stop, uint32_t reach, uint32_t* table, unsigned char* mid) {
  for (uint32_t i = 0; i < FDB_PQS_TABLE; i++) table[i] = 0;
  uint32_t cursor = 0, lit = 0, filled = 0, o = 0;
  FdbPqlOut r{n, 0, 0, 0};
  while (cursor < stop) {
    uint32_t win = 0, cand = 0;
    if (fdb_pqs_find_host(src, cursor, stop, table, &win, &cand)) {
      const uint32_t len = fdb_pqs_extend_host(src, win, cand, reach);
      if (r.first_len == 0) { r.head = win; r.first_len = len; }
      else o = (uint32_t)fdb_pql_put_run(src + lit, win - lit, len, mid, o);
      o = fdb_pql_put_match(win - cand, len, mid, o);
      cursor = lit = win + len;
    } else {
      cursor += FDB_PQS_WINDOW;
    }
    filled = fdb_pqs_fill_host(src, table, filled, cursor, stop);
  }
  if (r.first_len != 0) { r.tail = n - lit; r.mid_bytes = o; }
  return r;
}
// A body of U bytes turned into its block: compress, scan and gather in one walk. `table`: FDB_PQS_TABLE words; `mid`:
// fdb_pql_slot_bytes(); `out`: fdb_pql_bound(U) bytes. Returns the bytes written.
inline uint64_t fdb_pql_block_host(const unsigned char* body, uint64_t U, uint32_t* table, unsigned char* mid, unsigned char* out) {
  uint64_t o = 0;
  uint32_t carry = 0;
  for (uint64_t at = 0; at < U; at += FDB_PQS_FRAGMENT) {
    const uint32_t n = (uint32_t)(U - at < FDB_PQS_FRAGMENT ? U - at : FDB_PQS_FRAGMENT);
    const FdbPqlOut r = fdb_pql_compress_fragment_host(body + at, n, fdb_pql_stop(at, n, U), fdb_pql_reach(at, n, U), table, mid);
    if (r.first_len == 0) { carry += n; continue; }
    o = fdb_pql_put_run(body + at - carry, carry + r.head, r.first_len, out, o);
    __builtin_memcpy(out + o, mid, r.mid_bytes);
    o += r.mid_bytes;
    carry = r.tail;
  }
  return fdb_pql_put_run(body + U - carry, carry, 0, out, o);
}

#ifndef FDB_PQWRITE_HOST_ONLY
// Compress: fragment f of `staging` → its middle in scratch[f × fdb_pql_slot_bytes() …], the rest of what it leaves → outs[f].
hipError_t fdb_launch_pql_compress(const FdbPqlFrag* frags, int32_t n_frags, const unsigned char* staging, unsigned char* scratch, FdbPqlOut* outs, hipStream_t stream);
// Scan: the walk with the carry over every page's fragments: places[f] (fragments with a match), closes[page], page_bytes[page] = the block's size.
hipError_t fdb_launch_pql_scan(const FdbPqlPage* pages, int32_t n_pages, const FdbPqlOut* outs, FdbPqlPlace* places, FdbPqlPlace* closes, uint32_t* page_bytes, hipStream_t stream);
// Gather: every fragment's first sequence front and middle, and every page's closing sequence → final[page_dst[page] + …].
hipError_t fdb_launch_pql_gather(const FdbPqlFrag* frags, int32_t n_frags, const FdbPqlPage* pages, int32_t n_pages, const FdbPqlOut* outs, const FdbPqlPlace* places,
                                 const FdbPqlPlace* closes, const uint64_t* page_dst, const unsigned char* scratch, const unsigned char* staging, unsigned char* final_image,
                                 hipStream_t stream);
#endif
