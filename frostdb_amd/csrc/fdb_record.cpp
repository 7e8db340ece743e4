// fdb_record.cpp — RecordBuilder and the plumbing of a call that builds a resident record (see fdb_record.h).
#include "fdb_record.h"

#include "fdb_context.h"
#include "fdb_plan.h"

namespace fdb {

CallScope::CallScope(int device) {
  hip_check(hipSetDevice(device), "hipSetDevice");
  ctx = Context::acquire(device);
}

CallScope::~CallScope() {
  (void)hipStreamSynchronize(ctx->stream);
  for (void* p : scratch) ctx->dev_free(p);
  ctx->reset_staging();
  Context::release(ctx);
}

void* CallScope::alloc(size_t bytes) {
  void* p = ctx->dev_alloc(bytes);
  scratch.push_back(p);
  return p;
}

int scan_cache_width(const DeviceBatch& b, size_t c) {
  if (b.arena_ctx != nullptr || b.arena_borrowed || b.rows < kScanCacheMinRows) return 4;
  const DevColumn& col = b.cols[c];
  if (col.kind != ColKind::DICT || col.dict == nullptr || col.d_values == nullptr) return 4;
  return narrow_width(col.dict->values.size());
}

bool scan_cache_folded(const DeviceBatch& b, size_t c) {
  if (scan_cache_width(b, c) >= 4) return false;
  const DevColumn& col = b.cols[c];
  return col.d_validity != nullptr && scan_cache_folds(col.dict->values.size(), col.null_count, b.rows);
}

int scan_cache_packed(const DeviceBatch& b, size_t c) {
  if (scan_cache_width(b, c) >= 4) return 0;  // (transient, below the byte forms' threshold, no dictionary column, or a dictionary too large for any form)
  const DevColumn& col = b.cols[c];
  return scan_cache_packed_of(col.dict->values.size(), col.d_validity != nullptr ? col.null_count : 0, b.rows);
}

static const void* scan_cache_build(const DeviceBatch& b, size_t c, int width, hipStream_t stream) {
  const bool packed = scan_form_packed(width);
  std::lock_guard<std::mutex> lk(b.scan_cache_mu);
  ScanCache& sc = b.scan_cache;
  if (sc.cols.empty()) sc.cols.resize(2 * b.cols.size());
  ScanCache::Col& e = sc.cols[2 * c + (packed ? 1 : 0)];
  if (e.d != nullptr) return e.d;
  const size_t bytes = packed ? packed_slot((size_t)b.rows, width) : values_slot((size_t)b.rows, (size_t)width);
  void* d = device_pool_alloc(b.device, bytes);
  const bool folded = scan_cache_folded(b, c);
  hipError_t err = folded ? fdb_launch_narrow_indices((const uint32_t*)b.cols[c].d_values, b.cols[c].d_validity, (uint32_t)b.cols[c].dict->values.size(), d, b.rows, width, stream)
                          : fdb_launch_narrow_indices((const uint32_t*)b.cols[c].d_values, d, b.rows, width, stream);
  if (err == hipSuccess) err = hipStreamSynchronize(stream);
  if (err != hipSuccess) { device_pool_free(b.device, d); hip_check(err, "narrow-index cache"); }
  e.d = d; e.width = width; e.bytes = bytes; e.folded = folded;
  sc.bytes += (int64_t)bytes;
  return d;
}

const void* scan_cache_get(const DeviceBatch& b, size_t c, hipStream_t stream) {
  const int width = scan_cache_width(b, c);
  if (width >= 4) throw Error(FDB_ERR_INVALID, "internal: no narrow-index cache for column " + b.cols[c].name);
  return scan_cache_build(b, c, width, stream);
}

const void* scan_cache_get_packed(const DeviceBatch& b, size_t c, hipStream_t stream) {
  const int form = scan_cache_packed(b, c);
  if (form == 0) throw Error(FDB_ERR_INVALID, "internal: no packed index cache for column " + b.cols[c].name);
  return scan_cache_build(b, c, form, stream);
}

void require_values(const DeviceBatch& in, const char* what) {
  for (const DevColumn& c : in.cols)
    if (c.d_values == nullptr && in.rows > 0)
      throw Error(FDB_ERR_UNSUPPORTED, std::string(what) + ": column type " + c.format + " (" + c.name + ") is not supported on the device path");
}

void finish_column(DeviceBatch* b, size_t c, int64_t nulls, void* values, void* bitmap) {
  b->payload_bytes += finish_column(&b->cols[c], b->rows, nulls, values, bitmap);
}

RecordBuilder::RecordBuilder(int device, int64_t rows) : out_(new DeviceBatch()), rows_(rows) {
  out_->device = device;
  out_->rows = rows;
}

RecordBuilder::RecordBuilder(RecordBuilder&&) noexcept = default;
RecordBuilder::~RecordBuilder() = default;

void RecordBuilder::add(const std::string& name, const std::string& format, ColKind kind, std::shared_ptr<HostDict> dict, bool may_have_nulls) {
  DevColumn d;
  d.name = name; d.format = format; d.kind = kind; d.dict = std::move(dict);
  out_->cols.push_back(std::move(d));
  layout_.add((size_t)rows_, value_width(kind), may_have_nulls);
}

void RecordBuilder::allocate() {
  if (rows_ == 0 || layout_.total == 0) return;
  out_->arena = device_pool_alloc(out_->device, layout_.total);
  out_->arena_bytes = layout_.total;
}

void* RecordBuilder::values(size_t c) const {
  return out_->arena != nullptr ? (unsigned char*)out_->arena + layout_.cols[c].val_off : nullptr;
}

uint8_t* RecordBuilder::validity(size_t c) const {
  return out_->arena != nullptr && layout_.cols[c].bit_off != kNoSlot ? (uint8_t*)out_->arena + layout_.cols[c].bit_off : nullptr;
}

std::unique_ptr<DeviceBatch> RecordBuilder::finish(const unsigned long long* nulls) {
  if (rows_ > 0)
    for (size_t c = 0; c < out_->cols.size(); c++) finish_column(out_.get(), c, (int64_t)nulls[c], values(c), validity(c));
  return std::move(out_);
}

std::unique_ptr<DeviceBatch> RecordBuilder::schema_of(const DeviceBatch& in) {
  RecordBuilder rb(in.device, 0);
  for (const DevColumn& c : in.cols) rb.add(c.name, c.format, c.kind, c.dict, false);
  return rb.finish(nullptr);
}

}  // namespace fdb
