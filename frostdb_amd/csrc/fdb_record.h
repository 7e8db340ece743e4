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

// ---- the forms of the narrow-index cache ----------------------------------------------------------------------------------------------
// A resident dictionary column is scanned (fdb_plan_kernel, the cache's one reader) at one of five forms: its own uint32 indices (4), or
// a buffer of the record's cache (ScanCache, below) that holds them at 1 or 2 bytes, or packed at 4 bits (H) or 12 bits (T: the low byte
// of every index, laid out exactly as form 1, then the high nibble, laid out as H — unpacking is lo | hi << 8, no bit field crosses a
// word). The codes are what FdbScanArgs::w4 / wl4, JitSlot::form and the launch description carry (an argument block writes 0 for 4).
//
// Layout. The reader's wave owns a block of 1 024 consecutive rows as four sub-steps of 256 rows; in sub-step u lane l owns rows
// 256 u + 4 l … + 3. The indices of a full block sit in the order the wave's loads want them: lane l's 16-byte load at byte 16 l of the
// block (forms 1 and T's byte plane), or its two loads at bytes 1 024 h + 16 l (form 2), hold its rows of sub-steps 0 … 3, or 2 h and
// 2 h + 1; its 16 nibbles (rows 256 u + 4 l + r, nibble 4 u + r, low nibble first) are the 8 bytes at 8 l of the nibble plane, so
// sub-step u is bits 16 u … 16 u + 15 of the lane's 64-bit word. The rows of the record's last, partial block stay in row order; a framed
// form (H, T) still gives that block a whole frame, zeros behind the last row. The layout follows from the wave (64 lanes × 4 rows) alone.
//
enum ScanForm : int { kScanForm1 = 1, kScanForm2 = 2, kScanForm4 = 4, kScanFormH = 5, kScanFormT = 6 };
constexpr int64_t kScanCacheBlock = 1024;  // rows of a wave's block
// Per form: bits per index; the largest index it holds; the bytes of a full block's indices; framed (the packed forms): a partial block
// occupies a whole frame too; the rows a record must have (below them the bytes the form saves are under a microsecond of a scan).
struct ScanFormRow { ScanForm form; const char* name; int bits; uint32_t max_index; int64_t block_bytes; bool framed; int64_t min_rows; };
constexpr ScanFormRow kScanForms[] = {
    {kScanForm1, "1", 8, 0xFFu, 1024, false, (int64_t)1 << 20},
    {kScanForm2, "2", 16, 0xFFFFu, 2048, false, (int64_t)1 << 20},
    {kScanForm4, "4", 32, 0xFFFFFFFFu, 4096, false, 0},
    {kScanFormH, "H", 4, 0xFu, 512, true, (int64_t)4 << 20},
    {kScanFormT, "T", 12, 0xFFFu, 1536, true, (int64_t)4 << 20},
};
constexpr const ScanFormRow* scan_form_row(int form) {  // nullptr: not a form's code
  for (const ScanFormRow& r : kScanForms) if (r.form == form) return &r;
  return nullptr;
}
inline const ScanFormRow& scan_form(ScanForm form) { return *scan_form_row(form); }
inline const char* scan_form_name(ScanForm form) { return scan_form(form).name; }
inline int scan_form_bits(ScanForm form) { return scan_form(form).bits; }
inline int64_t scan_form_bytes(int64_t rows, ScanForm form) { return (rows * scan_form_bits(form) + 7) / 8; }  // the algorithmic bytes a scan reads of such a slot
// Bytes of a buffer of `rows` rows: sized like a values slot, a framed form in whole frames.
inline size_t scan_form_slot(size_t rows, ScanForm form) {
  const ScanFormRow& f = scan_form(form);
  return align_up((f.framed ? (rows + kScanCacheBlock - 1) / kScanCacheBlock * (size_t)f.block_bytes : rows * (size_t)f.bits / 8) + kTailPad, 256);
}
// Null-folded: the buffer of a column with NULLs holds S = `entries`, the index one past the dictionary, under every NULL row where S fits
// the form, and its reader needs no bitmap. Dictionaries of exactly 256 and 65 536 entries keep their byte form and their bitmap.
inline bool scan_form_folds(ScanForm form, size_t entries, int64_t nulls) { return nulls > 0 && form != kScanForm4 && entries <= scan_form(form).max_index; }

// The rule: the forms a column of a record of `rows` rows may be scanned at, narrowest first, always ending in 4 (the column itself) —
// at most its packed form, its byte form and 4. A form applies from its minimum rows on where the dictionary fits it; a packed form must
// also leave room for S when the column has NULLs (so a packed buffer of such a column is always folded: 16 or 4 096 entries with NULLs
// fall to the byte forms, which fold them), and is offered only where it is narrower than the byte form (T never beside form 1).
struct ScanForms {  // (as constructed: the column itself only)
  int n = 1; ScanForm form[3] = {kScanForm4, kScanForm4, kScanForm4};
  bool has(ScanForm f) const { return (n > 0 && form[0] == f) || (n > 1 && form[1] == f) || (n > 2 && form[2] == f); }
};
inline ScanForms scan_forms_of(size_t entries, int64_t nulls, int64_t rows) {
  const ScanFormRow *packed = nullptr, *bytes = nullptr;
  for (const ScanFormRow& f : kScanForms) {
    if (f.form == kScanForm4 || rows < f.min_rows || entries + (f.framed && nulls > 0 ? 1 : 0) > (size_t)f.max_index + 1) continue;
    const ScanFormRow*& best = f.framed ? packed : bytes;
    if (best == nullptr || f.bits < best->bits) best = &f;
  }
  ScanForms out; out.n = 0;
  if (packed != nullptr && (bytes == nullptr || packed->bits < bytes->bits)) out.form[out.n++] = packed->form;
  if (bytes != nullptr) out.form[out.n++] = bytes->form;
  out.form[out.n++] = kScanForm4;
  return out;
}
// The form a launch over `n` > 0 parts reads a slot at: the first candidate of parts[0] that every part offers (4 always survives) —
// the same packed form in all parts, else the same byte form in all parts, else the uint32 columns.
inline ScanForm scan_form_common(const ScanForms* parts, size_t n) {
  for (int k = 0; k < parts[0].n; k++) {
    bool all = true;
    for (size_t p = 1; all && p < n; p++) all = parts[p].has(parts[0].form[k]);
    if (all) return parts[0].form[k];
  }
  return kScanForm4;
}

// Where row `i` of a buffer of `rows` rows at `form` sits: `n_bytes` bytes (little-endian; 0: none, form H) at `byte` hold the index's
// low bits, and the nibble at `nibble_byte` >> `nibble_shift` (nibble_byte < 0: none, the unpacked forms) the 4 bits above them.
struct ScanCacheAt { int64_t byte; int n_bytes; int64_t nibble_byte; int nibble_shift; };
inline ScanCacheAt scan_cache_at(int64_t i, int64_t rows, ScanForm form) {
  const ScanFormRow& f = scan_form(form);
  const int64_t b = i / kScanCacheBlock, j = i % kScanCacheBlock, u = j / 256, l = (j % 256) / 4, r = j % 4;
  const bool full = i < rows / kScanCacheBlock * kScanCacheBlock;
  const int64_t e = full ? 16 * l + 4 * u + r : j;                            // element of the block at one byte (and one nibble) each
  const int64_t e2 = full ? 512 * (u / 2) + 8 * l + 4 * (u % 2) + r : j;      // … at two bytes each
  ScanCacheAt at;
  at.n_bytes = f.bits / 8;  // the whole bytes of an index; a framed form keeps the nibble above them in a plane behind theirs
  at.byte = b * f.block_bytes + (at.n_bytes == 2 ? 2 * e2 : at.n_bytes == 4 ? 4 * j : e);
  at.nibble_byte = f.framed ? b * f.block_bytes + at.n_bytes * kScanCacheBlock + e / 2 : -1;
  at.nibble_shift = f.framed ? (int)(e % 2) * 4 : 0;
  return at;
}
// The index a buffer holds for row `i`.
inline uint32_t scan_cache_read(const uint8_t* buf, int64_t i, int64_t rows, ScanForm form) {
  const ScanCacheAt at = scan_cache_at(i, rows, form);
  uint32_t v = 0;
  for (int k = 0; k < at.n_bytes; k++) v |= (uint32_t)buf[at.byte + k] << (8 * k);
  if (at.nibble_byte >= 0) v |= (uint32_t)((buf[at.nibble_byte] >> at.nibble_shift) & 0xFu) << (8 * at.n_bytes);
  return v;
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
// Beside the record, never part of it: per dictionary column and form (ScanForm, above) at most one device buffer of the column's
// indices, which the dense generated scan (fdb_plan_kernel) reads instead of the uint32 column. It depends on the immutable record
// alone, so it is built once — by the first such scan that wants the column at that form — and freed with the record; a record scanned
// in different company may come to hold two forms of a column. The record's layout, arena_bytes (fdb_batch_device_bytes: the record's
// OWN columns) and every other operator are untouched by it: the cache is extra memory from the device pool (fdb_live_allocations
// counts it), reported by fdb_batch_scan_cache_bytes, in a private layout (scan_cache_at) that nothing else reads.
// A null-folded buffer (scan_form_folds) holds S under every NULL row, the answer a filter leaf's truth table keeps last and the entry
// a group LUT gets appended (digit 0); a buffer that is not folded holds the truncated uint32 of every row, a NULL row's included.
struct ScanCache {
  struct Entry { size_t column; ScanForm form; void* d; size_t bytes; bool folded; };
  std::vector<Entry> entries;  // looked up by (column, form)
  int64_t bytes = 0;           // Σ scan_form_slot(rows, form) of the buffers
};
// The forms a dense generated scan may read column `c` of `b` at (scan_forms_of) — just 4 when the column gets no buffer: no dictionary
// column, no values, or a transient or borrowed record (a host record is scanned once). Builds nothing.
ScanForms scan_cache_forms(const DeviceBatch& b, size_t c);
// Whether the column's buffer at `form` is (or, once built, will be) null-folded. Builds nothing.
bool scan_cache_folded(const DeviceBatch& b, size_t c, ScanForm form);
// … whether any candidate folds, for what is decided before a launch has chosen (a packed form folds whenever the byte form does).
bool scan_cache_may_fold(const DeviceBatch& b, size_t c);
// The buffer of column `c` at `form`, one of scan_cache_forms(b, c) below 4, built on `stream` if it is not there yet. Two plans on two
// threads and two streams may meet the same fresh record: the record's mutex is held from the look-up to the publication, and a buffer
// is published only after the stream that built it has been synchronised — exactly one survives and nobody reads it early.
const void* scan_cache_get(const DeviceBatch& b, size_t c, ScanForm form, hipStream_t stream);

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
