// frostdb_amd — host block decoders (see fdb_codec.h). Each format's grammar is walked by ONE function, which hands the elements — literal
// bytes, copies from the output — to a sink: BlockWriter produces the page (or a prefix of it), OffsetScan only looks at how far back
// the copies reach. The sinks are the formats' common half: an element means the same in both.
#include "fdb_codec.h"

#include <algorithm>
#include <cstring>

namespace fdb {
namespace {
// the elements → dst[0, min(want, cap)), in the kernels' order of refusals for an element: 4 bad offset, then 3 output overrun
struct BlockWriter {
  uint8_t* dst;
  size_t cap, want, op = 0;
  uint32_t begin(uint64_t announced) const { return announced == cap ? 0u : 1u; }
  bool full() const { return want < cap && op >= want; }  // a prefix, and it is there
  uint32_t literal(const uint8_t* p, size_t l) {
    if (l > cap - op) return 3;
    if (op < want) std::memcpy(dst + op, p, std::min(l, want - op));
    op += l;
    return 0;
  }
  uint32_t copy(size_t off, size_t l) {
    if (off == 0 || off > op) return 4;
    if (l > cap - op) return 3;
    const size_t m = op < want ? std::min(l, want - op) : 0;
    if (off >= m) std::memcpy(dst + op, dst + op - off, m);  // disjoint
    else if (off >= 8) { for (size_t i = 0; i < m; i += 8) std::memcpy(dst + op + i, dst + op - off + i, std::min<size_t>(8, m - i)); }  // a pattern of ≥ 8 bytes: 8 at a time
    else for (size_t i = 0; i < m; i++) dst[op + i] = dst[op - off + i];  // short pattern repeated: byte by byte
    op += l;
    return 0;
  }
  uint32_t end() const { return (want == cap ? op == cap : op >= want) ? 0u : 5u; }
};

// no output: "no" (6) to the first copy from beyond the ring's reach
struct OffsetScan {
  bool zero_is_no;  // LZ4's walk has always refused an offset of 0 here; Snappy's leaves it to the decoder that gets the page
  uint32_t begin(uint64_t) const { return 0; }
  bool full() const { return false; }
  uint32_t literal(const uint8_t*, size_t) const { return 0; }
  uint32_t copy(size_t off, size_t) const { return off > FDB_PAGE_RING_REACH || (off == 0 && zero_is_no) ? 6u : 0u; }
  uint32_t end() const { return 0; }
};

// The Snappy block format (format_description.txt): the uncompressed length as a varint, then elements — a tag byte whose low two bits
// say literal (length − 1 in the tag, or 60 … 63 for 1 … 4 length bytes behind it) or copy with a 1-, 2- or 4-byte offset.
template <class Sink>
uint32_t snappy_walk(const uint8_t* src, size_t n, Sink& out) {
  size_t ip = 0;
  uint64_t len = 0;
  for (int shift = 0;; shift += 7) {
    if (ip >= n || shift > 35) return 1;
    const uint8_t b = src[ip++];
    len |= (uint64_t)(b & 0x7F) << shift;
    if (!(b & 0x80)) break;
  }
  if (uint32_t e = out.begin(len)) return e;
  while (ip < n && !out.full()) {
    const uint8_t tag = src[ip++];
    const unsigned kind = tag & 3;
    size_t l = (size_t)(tag >> 2) + 1;
    if (kind == 0) {
      if (l > 60) {
        const size_t extra = l - 60;
        if (ip + extra > n) return 2;
        l = 0;
        for (size_t i = 0; i < extra; i++) l |= (size_t)src[ip + i] << (8 * i);
        l += 1;
        ip += extra;
      }
      if (l > n - ip) return 2;
      if (uint32_t e = out.literal(src + ip, l)) return e;
      ip += l;
      continue;
    }
    const size_t nb = kind == 3 ? 4 : kind;  // offset bytes; the 1-byte form keeps three more offset bits and a 3-bit length in the tag
    if (ip + nb > n) return 2;
    size_t off = 0;
    for (size_t i = 0; i < nb; i++) off |= (size_t)src[ip + i] << (8 * i);
    ip += nb;
    if (kind == 1) { l = 4 + ((tag >> 2) & 7); off |= (size_t)(tag >> 5) << 8; }
    if (uint32_t e = out.copy(off, l)) return e;
  }
  return out.end();
}

// The LZ4 block format (lz4_Block_format.md): a sequence = token (literal length << 4 | match length − 4), either length extended by
// bytes that add up to and including the first one ≠ 255, the literals, a 2-byte little-endian offset (1 … 65 535); the last sequence
// ends behind its literals. No frame and no length preamble.
template <class Sink>
uint32_t lz4_walk(const uint8_t* src, size_t n, Sink& out) {
  size_t ip = 0;
  auto extend = [&](size_t* len) {
    uint8_t b;
    do { if (ip >= n) return false; b = src[ip++]; *len += b; } while (b == 255);
    return true;
  };
  while (ip < n) {
    const uint8_t token = src[ip++];
    size_t ll = token >> 4, ml = token & 15;
    if (ll == 15 && !extend(&ll)) return 2;
    if (ll > n - ip) return 2;
    if (uint32_t e = out.literal(src + ip, ll)) return e;
    ip += ll;
    if (out.full()) return 0;
    if (ip == n) break;
    if (n - ip < 2) return 2;
    const size_t off = (size_t)src[ip] | ((size_t)src[ip + 1] << 8);
    ip += 2;
    if (ml == 15 && !extend(&ml)) return 2;
    if (uint32_t e = out.copy(off, ml + 4)) return e;
    if (out.full()) return 0;
  }
  return out.end();
}
}  // namespace

uint32_t snappy_block(const uint8_t* src, size_t n, uint8_t* dst, size_t cap, size_t want) {
  if (want > cap) return 3;
  BlockWriter w{dst, cap, want};
  return snappy_walk(src, n, w);
}
uint32_t lz4_block(const uint8_t* src, size_t n, uint8_t* dst, size_t cap, size_t want) {
  if (want > cap) return 3;
  BlockWriter w{dst, cap, want};
  return lz4_walk(src, n, w);
}
bool snappy_device_ok(const uint8_t* src, size_t n) { OffsetScan s{false}; return snappy_walk(src, n, s) == 0; }
bool lz4_device_ok(const uint8_t* src, size_t n) { OffsetScan s{true}; return lz4_walk(src, n, s) == 0; }

int32_t check_page_table(const FdbCodecPage* pages, int32_t n_pages, int64_t src_bytes, int64_t dst_bytes) {
  for (int32_t i = 0; i < n_pages; i++)
    if (pages[i].src_off > (uint64_t)src_bytes || pages[i].src_len > (uint64_t)src_bytes - pages[i].src_off || pages[i].dst_off > (uint64_t)dst_bytes ||
        pages[i].dst_len > (uint64_t)dst_bytes - pages[i].dst_off)
      return i;
  return -1;
}

void decode_pages_host(int codec, const uint8_t* src, const FdbCodecPage* pages, int32_t n_pages, uint8_t* dst, uint32_t* status) {
  const auto block = codec == FDB_CODEC_SNAPPY ? snappy_block : lz4_block;
  for (int32_t i = 0; i < n_pages; i++) status[i] = block(src + pages[i].src_off, pages[i].src_len, dst + pages[i].dst_off, pages[i].dst_len, pages[i].dst_len);
}
}  // namespace fdb
