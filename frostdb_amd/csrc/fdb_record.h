// fdb_record.h — the layout contract of a record resident in HBM (DeviceBatch, fdb_plan.h) and the one builder of such records.
//
// A record is one arena of 256-byte aligned slots. Per column a value slot — uint32 dictionary indices or 8-byte values, bool widened to
// int64 — and, only if the column may hold NULLs, a bitmap slot; every slot ends kTailPad bytes past its payload. A finished column
// carries its bitmap iff it holds a NULL, and its value_bytes / validity_bytes are the algorithmic bytes every roofline figure counts.
//
// Three layers, smallest first: the slot arithmetic and finish_column are host-only (no device, no HIP: tools/asan_record.sh runs them
// under AddressSanitizer with FDB_RECORD_HOST_ONLY defined); RecordBuilder and the plumbing of a call that builds a record need both.
#pragma once

#include <cstddef>
#include <cstdint>
#include <memory>
#include <string>
#include <vector>

#include "fdb_arrow.h"

namespace fdb {

// ---- 1. slot arithmetic ------------------------------------------------------------------------------------------------------------------
inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
constexpr size_t kTailPad = 256;  // bytes readable past every column so tail lanes may over-read
constexpr size_t kNoSlot = (size_t)-1;

inline size_t value_width(ColKind kind) { return kind == ColKind::DICT || kind == ColKind::STR ? 4 : 8; }  // (a plain string column is staged as indices)
inline size_t values_slot(size_t rows, size_t width) { return align_up(rows * width + kTailPad, 256); }
// Whole 64-bit words, which is what the kernels write. Sizing the payload in bytes, (rows + 7) / 8, or in 32-bit words, (rows + 31) / 32 * 4,
// gives the same slot: the word forms round the byte count up to a multiple of 4 or 8, and the next multiple of 256 at or above the
// byte count is itself such a multiple, so the rounding never passes it.
inline size_t bitmap_slot(size_t rows) { return align_up((rows + 63) / 64 * 8 + kTailPad, 256); }

// Element position of row `i` in a narrow-index cache (ScanCache, below) of `rows` rows at `width` 1 or 2 bytes per index. The cache has one
// reader, fdb_plan_kernel, whose wave owns a block of 1 024 consecutive rows as four sub-steps of 256 rows; in sub-step u lane l owns rows
// 256 u + 4 l … + 3. The indices of a full block sit in the order the wave's 16-byte loads want them: lane l's load at byte 16 l of the
// block's 1 024 bytes (width 1), or its two loads at bytes 1 024 h + 16 l of the block's 2 048 (width 2), hold its rows of sub-steps
// 0 … 3, or 2 h and 2 h + 1. The rows of the record's last, partial block stay in row order. The layout follows from the wave
// (64 lanes × 4 rows) alone: not from a workgroup size, a query or a launch.
#if defined(__HIPCC__)
#define FDB_RECORD_HD __host__ __device__
#else
#define FDB_RECORD_HD
#endif
constexpr int64_t kScanCacheBlock = 1024;  // rows of a wave's block
FDB_RECORD_HD inline int64_t scan_cache_position(int64_t i, int64_t rows, int width) {
  if (i >= rows / kScanCacheBlock * kScanCacheBlock) return i;
  const int64_t b = i / kScanCacheBlock, j = i % kScanCacheBlock, u = j / 256, l = (j % 256) / 4, r = j % 4;
  return width == 1 ? kScanCacheBlock * b + 16 * l + 4 * u + r : kScanCacheBlock * b + 512 * (u / 2) + 8 * l + 4 * (u % 2) + r;
}

// What the cache holds for a dictionary column, from numbers alone (tools/scan_cache_dump.cpp prints them for a test to hold to a table).
constexpr int64_t kScanCacheMinRows = (int64_t)1 << 20;  // below it 3 B/row and column save less than a microsecond of a scan
// Bytes per index the cache can hold for a dictionary of `entries` entries; 4: none (the column itself).
inline int narrow_width(size_t entries) { return entries <= 256 ? 1 : entries <= 65536 ? 2 : 4; }
// … of a resident record of `rows` rows
inline int scan_cache_width_of(size_t entries, int64_t rows) { return rows < kScanCacheMinRows ? 4 : narrow_width(entries); }
// Null-folded: the buffer holds the index S = `entries`, one past the dictionary, under every NULL row, so that its reader needs no
// bitmap. The column has a bitmap (`nulls` > 0) and S fits the width: at most 255 entries at 1 byte, 65 535 at 2. Dictionaries of
// exactly 256 and 65 536 entries keep their width, are not folded, and are scanned with their bitmap.
inline bool scan_cache_folds(size_t entries, int64_t nulls, int64_t rows) {
  const int w = scan_cache_width_of(entries, rows);
  return nulls > 0 && w < 4 && entries < ((size_t)1 << (8 * w));
}

// ---- the packed forms: 4 and 12 bits per index ----------------------------------------------------------------------------------------
// Form H holds an index in 4 bits (a column whose entries plus one NULL value number at most 16), form T in 12 (at most 4 096) as two
// planes: the low byte of every index, laid out exactly as the 1-byte form, and the high nibble, laid out as form H. Unpacking T is
// lo | hi << 8: no bit field crosses a word. A buffer is a run of whole frames, one per 1 024-row block: 512 B for H; for T 1 024 B of
// bytes, then 512 B of nibbles. In a full block lane l's 16 nibbles (rows 256 u + 4 l + r, nibble 4 u + r, low nibble first) are the 8
// bytes at 8 l of the nibble plane, so sub-step u is bits 16 u … 16 u + 15 of the lane's 64-bit word. The record's last, partial block
// keeps the same frame in row order: row j of the block at byte j and nibble j, zeros behind the last row to the frame's end.
// A packed buffer of a column with NULLs is always null-folded (the rule below leaves S = entries room), so it needs no bitmap.
constexpr int kScanFormH = 5, kScanFormT = 6;  // as JitSlot::width / FdbScanArgs::w4 carry them, beside the byte widths 1, 2 and 4
constexpr int64_t kScanCachePackedMinRows = (int64_t)4 << 20;  // below it the 1 B a row the packed forms save on top of the byte forms is under a microsecond of a scan
inline bool scan_form_packed(int form) { return form == kScanFormH || form == kScanFormT; }
inline int scan_form_bits(int form) { return form == kScanFormH ? 4 : form == kScanFormT ? 12 : form == 1 ? 8 : form == 2 ? 16 : 32; }
inline int64_t scan_form_frame(int form) { return form == kScanFormH ? 512 : 1536; }  // bytes of a packed form's frame
inline size_t packed_slot(size_t rows, int form) { return align_up((rows + 1023) / 1024 * (size_t)scan_form_frame(form) + kTailPad, 256); }
// Bytes a scan of `rows` rows reads of an index column at `form` (any of the five): the algorithmic bytes of that slot.
inline int64_t scan_form_bytes(int64_t rows, int form) { return (rows * scan_form_bits(form) + 7) / 8; }
// The width rule. H where entries + (nulls > 0) ≤ 16; else nothing where the 1-byte form applies; else T where entries + (nulls > 0)
// ≤ 4 096; else nothing. 0: the column gets no packed buffer (it may get a byte one: scan_cache_width_of). A column of exactly 16 or
// 4 096 entries with NULLs falls to the byte forms, which fold it.
inline int scan_cache_packed_of(size_t entries, int64_t nulls, int64_t rows) {
  if (rows < kScanCachePackedMinRows) return 0;
  const size_t need = entries + (nulls > 0 ? 1 : 0);
  return need <= 16 ? kScanFormH : entries <= 256 ? 0 : need <= 4096 ? kScanFormT : 0;
}
// Where row `i` of a packed buffer of `rows` rows sits: the byte of its low 8 bits (T; −1 for H) and the byte and shift of its nibble.
struct PackedAt { int64_t byte; int64_t nibble_byte; int nibble_shift; };
FDB_RECORD_HD inline PackedAt scan_cache_packed_position(int64_t i, int64_t rows, int form) {
  const int64_t frame = form == kScanFormH ? 512 : 1536, plane = form == kScanFormH ? 0 : 1024;
  const int64_t b = i / kScanCacheBlock, j = i % kScanCacheBlock, u = j / 256, l = (j % 256) / 4, r = j % 4;
  const int64_t e = i >= rows / kScanCacheBlock * kScanCacheBlock ? j : 16 * l + 4 * u + r;  // element of the block: byte e, nibble e
  PackedAt at;
  at.byte = form == kScanFormH ? -1 : b * frame + e;
  at.nibble_byte = b * frame + plane + e / 2;
  at.nibble_shift = (int)(e % 2) * 4;
  return at;
}

// Offsets of the slots of one record, in column order: [values | bitmap] per column.
struct RecordLayout {
  struct Col { size_t val_off, bit_off; };  // bit_off == kNoSlot: no bitmap slot
  std::vector<Col> cols;
  size_t total = 0;
  void add(size_t rows, size_t width, bool bitmap) {
    Col c{total, kNoSlot};
    total += values_slot(rows, width);
    if (bitmap) { c.bit_off = total; total += bitmap_slot(rows); }
    cols.push_back(c);
  }
};

// ---- 2. a finished column ----------------------------------------------------------------------------------------------------------------
// One column of a record resident in HBM.
struct DevColumn {
  std::string name;
  std::string format;           // Arrow format of the column as received (index format for DICT)
  ColKind kind = ColKind::OTHER;
  int64_t length = 0;
  int64_t null_count = 0;
  void* d_values = nullptr;     // int64/uint64/double values, bool as int64 1 / 2, uint32 indices (DICT, and STR: encoded on import); nullptr for OTHER or not staged
  uint8_t* d_validity = nullptr;  // validity bitmap at bit offset 0; nullptr ⇔ null_count == 0
  std::shared_ptr<HostDict> dict;
  int64_t value_bytes = 0;      // algorithmic bytes: values/indices
  int64_t validity_bytes = 0;   // algorithmic bytes: bitmap (0 when the column has no nulls)
};

// `d` (its kind set) holds `rows` rows at `values`, `nulls` of them NULL; `bitmap` is kept only if there is a NULL. A bool counts as
// Arrow's bits, whatever it occupies. Returns what the column adds to its record's payload_bytes.
inline int64_t finish_column(DevColumn* d, int64_t rows, int64_t nulls, void* values, void* bitmap) {
  d->length = rows;
  d->null_count = nulls;
  d->d_values = values;
  d->value_bytes = d->kind == ColKind::BOOL ? (rows + 7) / 8 : rows * (int64_t)value_width(d->kind);
  if (nulls > 0 && bitmap != nullptr) { d->d_validity = (uint8_t*)bitmap; d->validity_bytes = (rows + 7) / 8; }
  return d->value_bytes + d->validity_bytes;
}

}  // namespace fdb

#ifndef FDB_RECORD_HOST_ONLY
#include <exception>

#include <hip/hip_runtime_api.h>

namespace fdb {

class Context;
struct DeviceBatch;

// Declared after the results it guards: an error that unwinds past it waits for the stream, so their arenas (and inputs the caller
// may release) go back to the pool only once no queued kernel uses them.
struct DrainOnUnwind {
  hipStream_t s; int n = std::uncaught_exceptions();
  ~DrainOnUnwind() { if (std::uncaught_exceptions() > n) (void)hipStreamSynchronize(s); }
};

// A pooled context for the length of one call: its stream, its staging ring, and device scratch that goes back to the context's pool
// when the call ends (synchronised).
struct CallScope {
  Context* ctx = nullptr;
  std::vector<void*> scratch;
  explicit CallScope(int device);
  ~CallScope();
  CallScope(const CallScope&) = delete;
  void* alloc(size_t bytes);
};

// ---- the narrow-index cache of a resident record -------------------------------------------------------------------------------------
// Beside the record, never part of it: per dictionary column at most one device buffer of the column's indices at 1 byte (dictionaries
// of ≤ 256 entries) or 2 bytes (≤ 65 536), which the dense generated scan (fdb_plan_kernel) reads instead of the uint32 column. It
// depends on the immutable record alone, so it is built once — by the first such scan that references the column — and freed with the
// record. The record's layout, arena_bytes (fdb_batch_device_bytes: the record's OWN columns) and every other operator are untouched by
// it: the cache is extra memory, up to 3 bytes per row and scanned dictionary column, reported by fdb_batch_scan_cache_bytes.
// A buffer is sized like a values slot and comes from the device pool, so fdb_live_allocations counts it. Its bytes are a private layout
// (scan_cache_position, above): no other operator, and nothing outside the library, reads them.
// NULL is an index of its own where it fits (scan_cache_folds, above): a null-folded buffer holds S = the dictionary's entry count
// under every NULL row, the answer a filter leaf's truth table keeps last and the entry a group LUT gets appended (digit 0), so the scan
// of such a column loads no bitmap. A buffer that is not folded holds the truncated uint32 of every row, a NULL row's included.
struct ScanCache {
  struct Col { void* d = nullptr; int width = 0; size_t bytes = 0; bool folded = false; };
  std::vector<Col> cols;  // column c's byte form at 2 c, its packed form (kScanFormH / kScanFormT in `width`) at 2 c + 1; empty until the first buffer
  int64_t bytes = 0;      // Σ values_slot(rows, width) / packed_slot(rows, form) of the buffers
};
// Width at which a dense generated scan may read column `c` of `b` — 1, 2, or 4 when the column gets no buffer: no dictionary column,
// a dictionary too large, a record below kScanCacheMinRows or a transient one (a host record is scanned once). Builds nothing.
int scan_cache_width(const DeviceBatch& b, size_t c);
// The packed form a dense generated scan may read column `c` at — kScanFormH, kScanFormT, or 0: none (scan_cache_packed_of; never for a
// transient record). A record scanned in different company may come to hold both forms of a column; both are counted and freed with it.
int scan_cache_packed(const DeviceBatch& b, size_t c);
// Whether that buffer is (or, once built, will be) null-folded: scan_cache_folds of the column's dictionary, NULL count and rows. Builds nothing.
bool scan_cache_folded(const DeviceBatch& b, size_t c);
// The buffer of column `c` (scan_cache_width(b, c) < 4), built on `stream` if it is not there yet. Two plans on two threads and two
// streams may meet the same fresh record: the record's mutex is held from the look-up to the publication, and a buffer is published
// only after the stream that built it has been synchronised — exactly one survives and nobody reads it early.
const void* scan_cache_get(const DeviceBatch& b, size_t c, hipStream_t stream);
// The same for the column's packed buffer (scan_cache_packed(b, c) != 0).
const void* scan_cache_get_packed(const DeviceBatch& b, size_t c, hipStream_t stream);

// FDB_ERR_UNSUPPORTED, naming `what`, if a column of `in` (rows > 0) is of a type the resident record cannot hold.
void require_values(const DeviceBatch& in, const char* what);

// finish_column for column `c` of `b` (b->rows rows), added to the record's payload_bytes.
void finish_column(DeviceBatch* b, size_t c, int64_t nulls, void* values, void* bitmap);

// ---- 3. a record of `rows` rows, column by column -----------------------------------------------------------------------------------------
// add() every column, allocate(), point the kernels at values() / validity(), and once the NULL counts are back finish(). Declare it
// before the DrainOnUnwind of the stream that writes the arena. Without rows nothing is laid out and finish() gives the bare schema.
class RecordBuilder {
 public:
  RecordBuilder(int device, int64_t rows);
  RecordBuilder(RecordBuilder&&) noexcept;
  ~RecordBuilder();
  void add(const std::string& name, const std::string& format, ColKind kind, std::shared_ptr<HostDict> dict, bool may_have_nulls);
  void allocate();  // the arena, from the device pool (nothing when there is nothing to hold)
  void* values(size_t c) const;
  uint8_t* validity(size_t c) const;  // nullptr: the column has no bitmap slot
  size_t bitmap_slot_bytes() const { return bitmap_slot((size_t)rows_); }  // (a bitmap that is OR-ed into is zeroed whole)
  std::unique_ptr<DeviceBatch> finish(const unsigned long long* nulls);  // nulls[c]: NULLs of column c (not read without rows)
  // `in` without rows: every column's name, format, kind and dictionary.
  static std::unique_ptr<DeviceBatch> schema_of(const DeviceBatch& in);

 private:
  std::unique_ptr<DeviceBatch> out_;
  RecordLayout layout_;
  int64_t rows_;
};

}  // namespace fdb
#endif
