// frostdb_amd — the host's block decoders for the two page formats the device inflates too (fdb_codec.hip): Snappy and LZ4. One walk
// over a format's elements serves the decoder, the prefix decoder and the "may the device take this page" answer.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "fdb_kernels.h"

namespace fdb {
// dst[0, cap) = the block src[0, n), `cap` = the page's announced uncompressed size (Snappy's preamble must say the same; LZ4 has
// none). Decodes until `want` bytes exist (want < cap: a prefix, nothing is written at or behind dst + want) or, with want == cap, the
// whole block, which must then fill dst exactly. Returns 0, or what failed first, in the device decoders' codes and order (fdb_kernels.h):
// 1 length preamble (Snappy), 2 truncated input, 3 output overrun, 4 bad offset, 5 output short. Never 6: any offset the format allows is fine here.
// lz4_block accepts what LZ4_decompress_safe accepts (and blocks that end in a match, which that one refuses).
uint32_t snappy_block(const uint8_t* src, size_t n, uint8_t* dst, size_t cap, size_t want);
uint32_t lz4_block(const uint8_t* src, size_t n, uint8_t* dst, size_t cap, size_t want);
inline bool snappy_raw(const uint8_t* src, size_t n, uint8_t* dst, size_t cap) { return snappy_block(src, n, dst, cap, cap) == 0; }
inline bool lz4_raw(const uint8_t* src, size_t n, uint8_t* dst, size_t cap) { return lz4_block(src, n, dst, cap, cap) == 0; }
// The first `want` bytes of a page (the definition levels at the head of a V1 page whose values are inflated on the device).
inline bool snappy_prefix(const uint8_t* src, size_t n, uint8_t* dst, size_t cap, size_t want) { return snappy_block(src, n, dst, cap, want) == 0; }
inline bool lz4_prefix(const uint8_t* src, size_t n, uint8_t* dst, size_t cap, size_t want) { return lz4_block(src, n, dst, cap, want) == 0; }

// May the device's decoder take this page? It keeps the page's last 64 KiB of output in an LDS ring, so a copy that reaches further
// back than FDB_PAGE_RING_REACH is beyond it (legal Snappy — a 4-byte-offset element, or a block longer than 64 KiB as klauspost/compress
// writes them for parquet-go, go.mod —, legal LZ4: offsets go up to 65 535; the host inflates such pages). Walks the elements only
// (literals are skipped, nothing is copied or allocated): a page of literals has a handful of them. A malformed stream also answers
// "no": the host's inflate then reports it.
bool snappy_device_ok(const uint8_t* src, size_t n);
bool lz4_device_ok(const uint8_t* src, size_t n);

// Every page of the table inside src[0, src_bytes) and dst[0, dst_bytes)? −1, or the first page that is not (the decoders check a page
// against its own lengths only).
int32_t check_page_table(const FdbCodecPage* pages, int32_t n_pages, int64_t src_bytes, int64_t dst_bytes);
// status[i] = the whole-page decode of page i by the host decoder of `codec` (FDB_CODEC_SNAPPY, else LZ4): fdb_launch_page_decode without a device.
void decode_pages_host(int codec, const uint8_t* src, const FdbCodecPage* pages, int32_t n_pages, uint8_t* dst, uint32_t* status);
}  // namespace fdb
