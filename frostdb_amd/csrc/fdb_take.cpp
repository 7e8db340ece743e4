// fdb_take.cpp — Take, Limit and the reservoir Sampler on records resident in HBM (see fdb_take.h).
//
// ≙ arrowutils.Take, Limiter.Callback (limit.go:63-98) and ReservoirSampler (sampler.go). The reference gathers on the host, column by
// column through builders; here one launch of take_kernel copies every column of a record (fdb_take.hip), the Sampler's reservoir is a
// record in HBM that scatter_kernel writes rows into as they are drawn, and what the host keeps is the selection itself (fdb_reservoir.h:
// Algorithm L, the dictionary unions, the index checks). None of the three belongs to a plan: each call borrows a pooled context (its
// stream, its staging ring, its scratch) — the Sampler for its lifetime — and ends synchronised, so an input may be released as soon as
// the call has returned.
#include "fdb_take.h"

#include "fdb_context.h"
#include "fdb_plan_internal.h"

#include <algorithm>
#include <cstring>

namespace fdb {

namespace {
struct GatherCol {
  std::string name, format;
  ColKind kind;
  std::shared_ptr<HostDict> dict;
  const void* src;
  const uint8_t* src_valid;  // nullptr: no NULLs in the source
  bool valid_bytes;
};

// Row d_rows[i] (nullptr: row i) of every column → row i of a new record of `n` > 0 rows: one launch, one wait. A column without a NULL
// among its n rows is emitted without a bitmap, as filter() does.
std::unique_ptr<DeviceBatch> gather(Context* ctx, std::vector<void*>* scratch, int device, const std::vector<GatherCol>& cols, const uint32_t* d_rows, int64_t n) {
  if (cols.size() > (size_t)FDB_TAKE_MAX_COLS) throw Error(FDB_ERR_UNSUPPORTED, "take: more than " + std::to_string(FDB_TAKE_MAX_COLS) + " columns");
  hipStream_t stream = ctx->stream;
  RecordBuilder out(device, n);
  DrainOnUnwind drain{stream};  // (after `out`: its arena outlives the queued kernel)
  for (const GatherCol& c : cols) out.add(c.name, c.format, c.kind, c.dict, c.src_valid != nullptr);
  out.allocate();
  std::vector<FdbTakeCol> tc(cols.size());
  for (size_t k = 0; k < cols.size(); k++) {
    FdbTakeCol& t = tc[k];
    std::memset(&t, 0, sizeof(t));
    t.src = cols[k].src;
    t.src_valid = cols[k].src_valid;
    t.dst = out.values(k);
    t.dst_valid = out.validity(k);
    t.width = (int32_t)value_width(cols[k].kind);
    t.valid_bytes = cols[k].valid_bytes ? 1 : 0;
  }
  std::vector<unsigned long long> h_nulls(cols.size(), 0);
  if (!cols.empty()) {
    const FdbTakeCol* d_cols = (const FdbTakeCol*)ctx->stage(tc.data(), tc.size() * sizeof(FdbTakeCol));
    unsigned long long* d_nulls = (unsigned long long*)ctx->dev_alloc(cols.size() * 8);
    scratch->push_back(d_nulls);
    hip_check(hipMemsetAsync(d_nulls, 0, cols.size() * 8, stream), "hipMemsetAsync(null counts)");
    hip_check(fdb_launch_take(d_cols, (int)cols.size(), d_rows, n, d_nulls, stream), "take launch");
    hip_check(hipMemcpyAsync(h_nulls.data(), d_nulls, cols.size() * 8, hipMemcpyDeviceToHost, stream), "hipMemcpyAsync(null counts)");
  }
  hip_check(hipStreamSynchronize(stream), "hipStreamSynchronize");
  return out.finish(h_nulls.data());
}

std::vector<GatherCol> columns_of(const DeviceBatch& in) {
  std::vector<GatherCol> cols;
  for (const DevColumn& c : in.cols) cols.push_back(GatherCol{c.name, c.format, c.kind, c.dict, c.d_values, c.d_validity, false});
  return cols;
}

// The whole record, device to device, into an arena of its own (as Projection passes a field through).
std::unique_ptr<DeviceBatch> copy_batch(const DeviceBatch& in) {
  CallScope cs(in.device);
  hipStream_t stream = cs.ctx->stream;
  RecordBuilder out(in.device, in.rows);
  DrainOnUnwind drain{stream};
  for (const DevColumn& c : in.cols) out.add(c.name, c.format, c.kind, c.dict, c.d_validity != nullptr);
  out.allocate();
  in.note_reader(stream);
  const size_t rows = (size_t)in.rows;
  std::vector<unsigned long long> nulls;
  for (size_t k = 0; k < in.cols.size(); k++) {
    const DevColumn& c = in.cols[k];
    nulls.push_back((unsigned long long)c.null_count);
    hip_check(hipMemcpyAsync(out.values(k), c.d_values, rows * value_width(c.kind), hipMemcpyDeviceToDevice, stream), "hipMemcpyAsync(limit column)");
    if (c.d_validity != nullptr) hip_check(hipMemcpyAsync(out.validity(k), c.d_validity, (rows + 7) / 8, hipMemcpyDeviceToDevice, stream), "hipMemcpyAsync(limit validity)");
  }
  hip_check(hipStreamSynchronize(stream), "hipStreamSynchronize");
  return out.finish(nulls.data());
}
}  // namespace

std::unique_ptr<DeviceBatch> take_batch(const DeviceBatch& in, const int32_t* indices, int64_t n) {
  check_take_indices(indices, n, in.rows);
  require_values(in, "take");
  if (n == 0) return RecordBuilder::schema_of(in);
  CallScope cs(in.device);
  uint32_t* d_rows = (uint32_t*)cs.ctx->dev_alloc((size_t)n * 4);
  cs.scratch.push_back(d_rows);
  // (validated: every index is ≥ 0, so the int32 bits are the uint32 row numbers; the call ends synchronised, the caller's array is only read until then)
  hip_check(hipMemcpyAsync(d_rows, indices, (size_t)n * 4, hipMemcpyHostToDevice, cs.ctx->stream), "hipMemcpyAsync(take indices)");
  return take_device_rows(in, &cs, d_rows, n);
}

std::unique_ptr<DeviceBatch> take_device_rows(const DeviceBatch& in, CallScope* cs, const uint32_t* d_rows, int64_t n) {
  in.note_reader(cs->ctx->stream);
  return gather(cs->ctx, &cs->scratch, in.device, columns_of(in), d_rows, n);
}

std::unique_ptr<DeviceBatch> limit_batch(const DeviceBatch& in, uint64_t count) {
  require_values(in, "limit");
  if (in.rows == 0 || count == 0) return RecordBuilder::schema_of(in);  // limit.go:64-70
  if ((uint64_t)in.rows <= count) return copy_batch(in);    // limit.go:72-74
  // the first `count` rows: take_kernel over the identity — a prefix copy of every column in one launch, the last validity word cut at
  // `count` and the prefix's NULLs counted on the way
  CallScope cs(in.device);
  in.note_reader(cs.ctx->stream);
  return gather(cs.ctx, &cs.scratch, in.device, columns_of(in), nullptr, (int64_t)count);
}

// ---------------------------------------------------------------------------------------------------------
// Sampler
// ---------------------------------------------------------------------------------------------------------
Sampler::Sampler(int64_t size, uint64_t seed, int device) : device_(device), select_(size, seed) {
  if (size < 0) throw Error(FDB_ERR_INVALID, "sampler: negative size");
  if (size > 0x7FFFFFFFll) throw Error(FDB_ERR_UNSUPPORTED, "sampler: more than 2^31 - 1 slots");
  if (device < 0 || device >= 16) throw Error(FDB_ERR_INVALID, "device index out of range");
}

Sampler::~Sampler() {
  if (ctx_ == nullptr) return;
  (void)hipSetDevice(device_);
  (void)hipStreamSynchronize(stream_);
  for (Field& f : fields_) ctx_->dev_free(f.block);
  ctx_->reset_staging();
  Context::release(ctx_);
}

void Sampler::ensure_context() {
  hip_check(hipSetDevice(device_), "hipSetDevice");
  if (ctx_ != nullptr) return;
  ctx_ = Context::acquire(device_);
  stream_ = ctx_->stream;
}

void Sampler::alloc_field(Field* f, int64_t cap) {
  const size_t values = align_up((size_t)cap * width(*f) + kTailPad, 256), bytes = values + align_up((size_t)cap + kTailPad, 256);
  f->block = ctx_->dev_alloc(bytes);
  f->valid = (uint8_t*)f->block + values;
  hip_check(hipMemsetAsync(f->block, 0, bytes, stream_), "hipMemsetAsync(reservoir)");  // every slot NULL, its value 0
}

void Sampler::grow(int64_t slots) {
  if (slots <= cap_) return;
  const int64_t cap = std::min<int64_t>(select_.size(), std::max<int64_t>(std::max<int64_t>(slots, 2 * cap_), 1024));
  std::vector<void*> old;
  for (Field& f : fields_) {
    void* from = f.block;
    const uint8_t* from_valid = f.valid;
    old.push_back(from);
    alloc_field(&f, cap);
    if (cap_ > 0) {
      hip_check(hipMemcpyAsync(f.block, from, (size_t)cap_ * width(f), hipMemcpyDeviceToDevice, stream_), "hipMemcpyAsync(reservoir)");
      hip_check(hipMemcpyAsync(f.valid, from_valid, (size_t)cap_, hipMemcpyDeviceToDevice, stream_), "hipMemcpyAsync(reservoir validity)");
    }
  }
  if (!old.empty()) hip_check(hipStreamSynchronize(stream_), "hipStreamSynchronize");
  for (void* p : old) ctx_->dev_free(p);
  cap_ = cap;
}

int Sampler::field_of(const DevColumn& c) {
  for (size_t f = 0; f < fields_.size(); f++) {
    Field& F = fields_[f];
    if (F.name != c.name) continue;
    const bool same = F.kind == c.kind && (c.kind == ColKind::DICT || F.format == c.format);
    if (!same) throw Error(FDB_ERR_UNSUPPORTED, "sampler: field " + c.name + " changes its type between records (" + F.format + " against " + c.format + ")");
    return (int)f;
  }
  return -1;
}

void Sampler::push_batch(const DeviceBatch& b) {
  if (b.rows == 0 || select_.size() == 0) return;
  if (b.device != device_) throw Error(FDB_ERR_INVALID, "batch lives on a different device than the sampler");
  if (b.rows > 0xFFFFFFFFll) throw Error(FDB_ERR_UNSUPPORTED, "sampler: more than 2^32 - 1 rows in one record");
  if (b.cols.size() > (size_t)FDB_TAKE_MAX_COLS) throw Error(FDB_ERR_UNSUPPORTED, "sampler: more than " + std::to_string(FDB_TAKE_MAX_COLS) + " columns");
  // everything that can refuse the record, before a draw is made
  require_values(b, "sampler");
  std::vector<int> col_field(b.cols.size(), -1);
  for (size_t c = 0; c < b.cols.size(); c++) {
    const DevColumn& C = b.cols[c];
    for (size_t q = 0; q < c; q++) if (b.cols[q].name == C.name) throw Error(FDB_ERR_UNSUPPORTED, "sampler: two fields named " + C.name + " in one record");
    if (C.kind == ColKind::DICT && !C.dict) throw Error(FDB_ERR_INVALID, "sampler: dictionary column without its dictionary: " + C.name);
    col_field[c] = field_of(C);
    if (col_field[c] >= 0 && C.kind == ColKind::DICT) fields_[(size_t)col_field[c]].dict.check_type(*C.dict, C.name);
  }
  // which rows enter, and where
  std::vector<uint32_t> pairs;
  const int64_t size = select_.size(), rows = b.rows;
  select_.push(rows, [&](int64_t row, int64_t slot) {
    if (row < 0 || row >= rows || slot < 0 || slot >= size) throw Error(FDB_ERR_STATE, "sampler: a draw left the record or the reservoir");
    pairs.push_back((uint32_t)row);
    pairs.push_back((uint32_t)slot);
  });
  if (pairs.empty()) return;
  ensure_context();
  DrainOnUnwind drain{stream_};
  const int64_t kept = select_.kept();
  grow(kept);
  std::vector<int> schema;
  for (size_t c = 0; c < b.cols.size(); c++) {
    if (col_field[c] < 0) {  // first seen: NULL in every slot so far
      Field f;
      f.name = b.cols[c].name; f.format = b.cols[c].format; f.kind = b.cols[c].kind;
      alloc_field(&f, cap_);
      fields_.push_back(std::move(f));
      col_field[c] = (int)fields_.size() - 1;
    }
    schema.push_back(col_field[c]);
  }
  std::sort(schema.begin(), schema.end());
  size_t sid = 0;
  while (sid < schemas_.size() && schemas_[sid] != schema) sid++;
  if (sid == schemas_.size()) schemas_.push_back(schema);
  slot_schema_.resize((size_t)kept, -1);
  for (size_t k = 0; k + 1 < pairs.size(); k += 2) slot_schema_[pairs[k + 1]] = (int32_t)sid;
  if (stamp_.size() < (size_t)kept) stamp_.resize((size_t)kept, 0);
  const size_t m = keep_last_per_slot(&pairs, &stamp_);

  std::vector<FdbTakeCol> tc(fields_.size());
  std::vector<std::shared_ptr<const std::vector<uint32_t>>> tables(fields_.size());
  for (size_t f = 0; f < fields_.size(); f++) {
    FdbTakeCol& t = tc[f];
    std::memset(&t, 0, sizeof(t));
    t.dst = fields_[f].block;
    t.dst_valid = fields_[f].valid;
    t.width = (int32_t)width(fields_[f]);
    t.absent = 1;
  }
  {
    StageScope stage_scope(ctx_);  // the translation tables and the descriptors leave with one copy
    for (size_t c = 0; c < b.cols.size(); c++) {
      const DevColumn& C = b.cols[c];
      const size_t f = (size_t)col_field[c];
      FdbTakeCol& t = tc[f];
      t.absent = 0;
      t.src = C.d_values;
      t.src_valid = C.d_validity;
      if (C.kind == ColKind::DICT) {
        tables[f] = fields_[f].dict.table_for(C.dict, C.name);
        t.table = (const uint32_t*)ctx_->stage(tables[f]->data(), tables[f]->size() * 4);
        t.table_len = (uint32_t)std::min<size_t>(tables[f]->size(), 0xFFFFFFFFu);
      }
    }
    const FdbTakeCol* d_cols = (const FdbTakeCol*)ctx_->stage(tc.data(), tc.size() * sizeof(FdbTakeCol));
    const uint32_t* d_pairs = (const uint32_t*)ctx_->stage(pairs.data(), pairs.size() * 4);
    ctx_->flush_staging();
    b.note_reader(stream_);
    hip_check(fdb_launch_scatter(d_cols, (int)tc.size(), d_pairs, (int64_t)m, stream_), "scatter launch");
  }
  hip_check(hipStreamSynchronize(stream_), "hipStreamSynchronize");
  ctx_->reset_staging();
}

void Sampler::push(const ArrowArray* array, const ArrowSchema* schema) {
  HostRecordView view;
  view_record(array, schema, &view);
  if (view.rows == 0 || select_.size() == 0) return;
  ensure_context();
  std::unique_ptr<DeviceBatch> b = import_batch(view, device_, nullptr, stream_);
  push_batch(*b);
}

std::unique_ptr<DeviceBatch> Sampler::finish_batch(int64_t* n_rows) {
  const int64_t kept = select_.kept();
  if (n_rows != nullptr) *n_rows = kept;
  if (kept == 0 || ctx_ == nullptr) {
    std::unique_ptr<DeviceBatch> out(new DeviceBatch());
    out->device = device_;
    return out;
  }
  hip_check(hipSetDevice(device_), "hipSetDevice");
  // the fields of the records whose rows are in the reservoir now (what materialize would find, sampler.go:230-242), sorted by name
  std::vector<char> used(fields_.size(), 0);
  for (int64_t s = 0; s < kept; s++)
    for (int f : schemas_[(size_t)slot_schema_[(size_t)s]]) used[(size_t)f] = 1;
  std::vector<size_t> order;
  for (size_t f = 0; f < fields_.size(); f++) if (used[f]) order.push_back(f);
  std::sort(order.begin(), order.end(), [&](size_t a, size_t b) { return fields_[a].name < fields_[b].name; });
  std::vector<GatherCol> cols;
  for (size_t f : order) {
    const Field& F = fields_[f];
    std::shared_ptr<HostDict> dict;
    if (F.kind == ColKind::DICT) {
      std::vector<std::string> values = F.dict.values();
      dict = F.dict.plain() ? make_plain_dictionary(std::move(values), F.dict.value_format()) : make_dictionary(std::move(values), F.dict.utf8() ? "u" : "z");
    }
    cols.push_back(GatherCol{F.name, F.format, F.kind, dict, F.block, F.valid, true});
  }
  std::vector<void*> scratch;
  struct Free { Context* c; std::vector<void*>* v; ~Free() { for (void* p : *v) c->dev_free(p); c->reset_staging(); } } free_scratch{ctx_, &scratch};
  return gather(ctx_, &scratch, device_, cols, nullptr, kept);
}

void Sampler::finish(ArrowArray* out, ArrowSchema* out_schema, int64_t* n_rows) {
  std::unique_ptr<DeviceBatch> b = finish_batch(n_rows);
  if (b->cols.empty()) { export_record(std::vector<OutColumn>(), 0, out, out_schema); return; }  // (nothing kept: no device to ask)
  export_batch(*b, out, out_schema);
}

}  // namespace fdb
