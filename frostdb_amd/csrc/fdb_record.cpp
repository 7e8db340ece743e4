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

// NULLs as the cache sees them: a column without a bitmap has none
static int64_t cached_nulls(const DevColumn& col) { return col.d_validity != nullptr ? col.null_count : 0; }

ScanForms scan_cache_forms(const DeviceBatch& b, size_t c) {
  const DevColumn& col = b.cols[c];
  if (b.arena_ctx != nullptr || b.arena_borrowed || col.kind != ColKind::DICT || col.dict == nullptr || col.d_values == nullptr) return ScanForms();
  return scan_forms_of(col.dict->values.size(), cached_nulls(col), b.rows);
}

bool scan_cache_folded(const DeviceBatch& b, size_t c, ScanForm form) {
  return form != kScanForm4 && scan_cache_forms(b, c).has(form) && scan_form_folds(form, b.cols[c].dict->values.size(), cached_nulls(b.cols[c]));
}

bool scan_cache_may_fold(const DeviceBatch& b, size_t c) {
  const ScanForms f = scan_cache_forms(b, c);
  for (int k = 0; k + 1 < f.n; k++) if (scan_form_folds(f.form[k], b.cols[c].dict->values.size(), cached_nulls(b.cols[c]))) return true;  // (the closing 4 never folds)
  return false;
}

const void* scan_cache_get(const DeviceBatch& b, size_t c, ScanForm form, hipStream_t stream) {
  if (form == kScanForm4 || !scan_cache_forms(b, c).has(form)) throw Error(FDB_ERR_INVALID, "internal: no narrow-index cache at form " + std::string(scan_form_name(form)) + " for column " + b.cols[c].name);
  std::lock_guard<std::mutex> lk(b.scan_cache_mu);
  ScanCache& sc = b.scan_cache;
  for (const ScanCache::Entry& e : sc.entries) if (e.column == c && e.form == form) return e.d;
  sc.entries.reserve(sc.entries.size() + 1);  // (nothing may throw between the build and the publication)
  const size_t bytes = scan_form_slot((size_t)b.rows, form);
  void* d = device_pool_alloc(b.device, bytes);
  const bool folded = scan_form_folds(form, b.cols[c].dict->values.size(), cached_nulls(b.cols[c]));
  hipError_t err = fdb_launch_narrow_indices((const uint32_t*)b.cols[c].d_values, folded ? b.cols[c].d_validity : nullptr, (uint32_t)b.cols[c].dict->values.size(), d, b.rows, form, stream);
  if (err == hipSuccess) err = hipStreamSynchronize(stream);
  if (err != hipSuccess) { device_pool_free(b.device, d); hip_check(err, "narrow-index cache"); }
  sc.entries.push_back(ScanCache::Entry{c, form, d, bytes, folded});
  sc.bytes += (int64_t)bytes;
  return d;
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
