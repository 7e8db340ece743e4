// fdb_sort.cpp — Sort of a record resident in HBM (see fdb_sort.h).
//
// ≙ arrowutils.SortRecord, and SortRecord + Take as merge_test.go:356-375 uses the pair. The reference compares rows pairwise on the host,
// column by column (multiColSorter.Less); here the sorting columns are turned into radix keys whose unsigned order IS that comparison
// (fdb_sortkey.h) and the record's row numbers are sorted by them: a stable LSD radix sort over the 64-bit key words, last word first. Pass
// 1 builds its keys in row order with payload = row number; every later pass builds its word's keys through the permutation so far and
// sorts (key, row number) again, each pass over the bits its word uses only. What the host does is the plan: which field goes where, and
// the byte-order ranks of the dictionaries. Like Take the call borrows a pooled context, runs on its one stream and ends synchronised; all
// temporaries are the context's and go back to it before the call returns.
#include "fdb_sort.h"

#include <algorithm>
#include <cstring>

#include "fdb_context.h"
#include "fdb_plan_internal.h"
#include "fdb_sortkey.h"
#include "fdb_sortplan.h"
#include "fdb_take.h"

namespace fdb {

namespace {

struct SortPlan {
  std::vector<std::vector<FdbSortField>> words;  // [word][field], ranks = an OFFSET into `ranks` (in entries) + 1 until they are on the device
  std::vector<int> bits;
  std::vector<uint32_t> ranks;                   // the rank tables of the dictionary columns, back to back
};

// Everything that can refuse the call, and the plan of the keys. rows ≥ 2.
SortPlan plan_sort(const DeviceBatch& in, const fdb_sort_col* cols, int32_t n_cols) {
  if (in.rows > 0x7FFFFFFFll) throw Error(FDB_ERR_INVALID, "sort: more than 2^31 - 1 rows (indices are int32)");
  for (int32_t k = 0; k < n_cols; k++) {
    if (cols[k].index < 0 || (size_t)cols[k].index >= in.cols.size())
      throw Error(FDB_ERR_INVALID, "sort: column index " + std::to_string(cols[k].index) + " outside the record's " + std::to_string(in.cols.size()) + " columns");
    if (cols[k].direction > 1u) throw Error(FDB_ERR_INVALID, "sort: unexpected direction value " + std::to_string(cols[k].direction) + ", only 0 (ascending) and 1 (descending) are allowed");
  }
  for (int32_t k = 0; k < n_cols; k++) {
    const DevColumn& c = in.cols[(size_t)cols[k].index];
    const bool sorts = c.kind == ColKind::I64 || c.kind == ColKind::U64 || c.kind == ColKind::F64 || (c.kind == ColKind::DICT && c.dict);
    if (!sorts || c.d_values == nullptr) throw Error(FDB_ERR_UNSUPPORTED, "unsupported column type for sorting " + c.format + " for column " + c.name);
    if (((uintptr_t)c.d_values & 15u) != 0) throw Error(FDB_ERR_UNSUPPORTED, "sort: the values of column " + c.name + " are not 16-byte aligned");
  }
  SortPlan plan;
  std::vector<SortColBits> col_bits((size_t)n_cols);
  std::vector<size_t> rank_off((size_t)n_cols, 0), rank_len((size_t)n_cols, 0);
  for (int32_t k = 0; k < n_cols; k++) {
    const DevColumn& c = in.cols[(size_t)cols[k].index];
    int value_bits = 64;
    if (c.kind == ColKind::DICT) {
      uint32_t distinct = 0;
      const std::vector<uint32_t> r = dense_ranks(*c.dict, &distinct);
      value_bits = bits_for(distinct);
      if (value_bits > 0) {
        rank_off[(size_t)k] = plan.ranks.size();
        rank_len[(size_t)k] = r.size();
        plan.ranks.insert(plan.ranks.end(), r.begin(), r.end());
      }
    }
    col_bits[(size_t)k] = SortColBits{value_bits, c.null_count != 0 && c.d_validity != nullptr};
  }
  const std::vector<SortPart> parts = pack_sort_fields(col_bits, &plan.bits);
  plan.words.resize(plan.bits.size());
  for (const SortPart& p : parts) {
    const fdb_sort_col& sc = cols[p.col];
    const DevColumn& c = in.cols[(size_t)sc.index];
    FdbSortField f;
    std::memset(&f, 0, sizeof(f));
    f.values = c.d_values;
    f.validity = col_bits[(size_t)p.col].has_null_bit ? c.d_validity : nullptr;
    f.kind = (int32_t)c.kind;
    f.width = p.width; f.shift = p.shift; f.null_shift = p.null_shift;
    f.flags = (sc.direction == 1u ? FDB_SORT_DESC : 0u) | (sc.nulls_first != 0u ? FDB_SORT_NULLS_FIRST : 0u);
    if (c.kind == ColKind::DICT && p.width > 0) {
      f.ranks = (const uint32_t*)(uintptr_t)(rank_off[(size_t)p.col] + 1);
      f.rank_len = (uint32_t)std::min<size_t>(rank_len[(size_t)p.col], 0xFFFFFFFFu);
    }
    plan.words[(size_t)p.word].push_back(f);
  }
  return plan;
}

// The rank tables and the field descriptors of every word, on the device (the scope's scratch and staging ring).
std::vector<const FdbSortField*> stage_fields(SortPlan& plan, CallScope* cs) {
  Context* ctx = cs->ctx;
  const uint32_t* d_ranks = nullptr;
  if (!plan.ranks.empty()) {
    uint32_t* r = (uint32_t*)cs->alloc(plan.ranks.size() * 4 + kTailPad);
    ctx->copy_in(r, plan.ranks.data(), plan.ranks.size() * 4);  // (through the pinned ring: the host vector is read when this returns)
    d_ranks = r;
  }
  std::vector<const FdbSortField*> d_fields(plan.words.size(), nullptr);
  StageScope stage_scope(ctx);  // the descriptors of all words leave with one copy
  for (size_t w = 0; w < plan.words.size(); w++) {
    for (FdbSortField& f : plan.words[w])
      if (f.ranks != nullptr) f.ranks = d_ranks + ((size_t)(uintptr_t)f.ranks - 1);
    d_fields[w] = (const FdbSortField*)ctx->stage(plan.words[w].data(), plan.words[w].size() * sizeof(FdbSortField));
  }
  return d_fields;
}

// The permutation in device memory (the scope's scratch; valid until the scope ends). rows ≥ 2. Everything is queued on the scope's stream;
// nothing is waited for.
const uint32_t* sort_on_device(const DeviceBatch& in, SortPlan& plan, CallScope* cs) {
  Context* ctx = cs->ctx;
  hipStream_t stream = ctx->stream;
  const int64_t n = in.rows;
  const size_t rows = (size_t)n;
  uint32_t* pay_a = (uint32_t*)cs->alloc(rows * 4 + kTailPad);
  in.note_reader(stream);
  if (plan.words.empty()) {  // nothing tells two rows apart (every column one distinct value, no NULLs): the input order, by stability
    hip_check(fdb_launch_sort_iota(pay_a, n, stream), "sort iota launch");
    return pay_a;
  }
  uint32_t* pay_b = (uint32_t*)cs->alloc(rows * 4 + kTailPad);
  unsigned long long* keys_a = (unsigned long long*)cs->alloc(rows * 8 + kTailPad);
  unsigned long long* keys_b = (unsigned long long*)cs->alloc(rows * 8 + kTailPad);
  size_t temp_bytes = 0;
  hip_check(fdb_sort_pairs_u64_u32(nullptr, &temp_bytes, keys_a, keys_b, pay_a, pay_b, n, 64, stream), "sort scratch size");
  void* temp = cs->alloc(std::max<size_t>(temp_bytes, 256));
  const std::vector<const FdbSortField*> d_fields = stage_fields(plan, cs);
  bool first = true;
  for (size_t w = plan.words.size(); w-- > 0;) {  // least significant word first
    hip_check(fdb_launch_sort_keys(d_fields[w], (int)plan.words[w].size(), first ? nullptr : pay_a, n, keys_a, first ? pay_a : nullptr, stream), "sort keys launch");
    size_t tb = temp_bytes;
    hip_check(fdb_sort_pairs_u64_u32(temp, &tb, keys_a, keys_b, pay_a, pay_b, n, plan.bits[w], stream), "sort pairs");
    std::swap(pay_a, pay_b);
    first = false;
  }
  return pay_a;
}

void check_args(const fdb_sort_col* cols, int32_t n_cols) {
  if (n_cols == 0) throw Error(FDB_ERR_INVALID, "sort: at least one column is needed for sorting");
  if (n_cols < 0 || cols == nullptr) throw Error(FDB_ERR_INVALID, "sort: bad column list");
}

}  // namespace

void sort_batch_indices(const DeviceBatch& in, const fdb_sort_col* cols, int32_t n_cols, int32_t* indices_out) {
  check_args(cols, n_cols);
  if (in.rows <= 1) {  // sort.go:412-417
    if (in.rows == 1) {
      if (indices_out == nullptr) throw Error(FDB_ERR_INVALID, "null argument");
      indices_out[0] = 0;
    }
    return;
  }
  if (indices_out == nullptr) throw Error(FDB_ERR_INVALID, "null argument");
  SortPlan plan = plan_sort(in, cols, n_cols);
  CallScope cs(in.device);
  DrainOnUnwind drain{cs.ctx->stream};
  const uint32_t* d_perm = sort_on_device(in, plan, &cs);
  // (row numbers < 2^31: the uint32 bits are the int32 indices)
  hip_check(hipMemcpyAsync(indices_out, d_perm, (size_t)in.rows * 4, hipMemcpyDeviceToHost, cs.ctx->stream), "hipMemcpyAsync(sort indices)");
  hip_check(hipStreamSynchronize(cs.ctx->stream), "hipStreamSynchronize");
}

std::unique_ptr<DeviceBatch> sort_batch(const DeviceBatch& in, const fdb_sort_col* cols, int32_t n_cols) {
  check_args(cols, n_cols);
  if (in.rows <= 1) return limit_batch(in, 1);  // nothing to order: the (zero-row or one-row) record, copied
  SortPlan plan = plan_sort(in, cols, n_cols);
  require_values(in, "sort");
  CallScope cs(in.device);
  DrainOnUnwind drain{cs.ctx->stream};
  const uint32_t* d_perm = sort_on_device(in, plan, &cs);
  return take_device_rows(in, &cs, d_perm, in.rows);  // every entry is a row number of `in`: a permutation of 0 … rows - 1
}

// Measurement aid (tools/sort_bench.py): device time, between two events on the call's stream, of what sort_batch_indices queues before
// its copy-out — key kernels + radix passes — and of BARE fdb_sort_pairs_u64 calls with the same pass count and bit widths over keys of the
// record's last word (the yardstick: the key kernels' share is the difference). Medians over `reps` calls after `warmup` calls.
void sort_bench(const DeviceBatch& in, const fdb_sort_col* cols, int32_t n_cols, int32_t reps, int32_t warmup, double* sort_ms, double* bare_ms, int32_t* n_passes) {
  check_args(cols, n_cols);
  if (in.rows < 2 || reps < 1 || warmup < 0 || sort_ms == nullptr || bare_ms == nullptr) throw Error(FDB_ERR_INVALID, "sort bench: bad arguments");
  const SortPlan plan = plan_sort(in, cols, n_cols);
  if (plan.words.empty()) throw Error(FDB_ERR_INVALID, "sort bench: the columns hold nothing to sort by");
  if (n_passes != nullptr) *n_passes = (int32_t)plan.words.size();
  auto median = [](std::vector<float> v) { std::sort(v.begin(), v.end()); return (double)v[v.size() / 2]; };
  struct Events {
    Context* c; hipEvent_t a, b;
    explicit Events(Context* ctx) : c(ctx), a(ctx->get_event()), b(ctx->get_event()) {}
    ~Events() { c->put_event(a); c->put_event(b); }
  };
  std::vector<float> ms;
  for (int32_t r = 0; r < warmup + reps; r++) {
    SortPlan p = plan;
    CallScope cs(in.device);
    Events ev(cs.ctx);
    hip_check(hipEventRecord(ev.a, cs.ctx->stream), "hipEventRecord");
    (void)sort_on_device(in, p, &cs);
    hip_check(hipEventRecord(ev.b, cs.ctx->stream), "hipEventRecord");
    hip_check(hipStreamSynchronize(cs.ctx->stream), "hipStreamSynchronize");
    float t = 0;
    hip_check(hipEventElapsedTime(&t, ev.a, ev.b), "hipEventElapsedTime");
    if (r >= warmup) ms.push_back(t);
  }
  *sort_ms = median(ms);
  ms.clear();
  {
    SortPlan p = plan;
    CallScope cs(in.device);
    Events ev(cs.ctx);
    hipStream_t stream = cs.ctx->stream;
    const size_t rows = (size_t)in.rows;
    unsigned long long* keys_a = (unsigned long long*)cs.alloc(rows * 8 + kTailPad);
    unsigned long long* keys_b = (unsigned long long*)cs.alloc(rows * 8 + kTailPad);
    unsigned long long* vals_a = (unsigned long long*)cs.alloc(rows * 8 + kTailPad);
    unsigned long long* vals_b = (unsigned long long*)cs.alloc(rows * 8 + kTailPad);
    size_t temp_bytes = 0;
    hip_check(fdb_sort_pairs_u64(nullptr, &temp_bytes, keys_a, keys_b, vals_a, vals_b, in.rows, 64, stream), "sort scratch size");
    void* temp = cs.alloc(std::max<size_t>(temp_bytes, 256));
    hip_check(hipMemsetAsync(vals_a, 0, rows * 8, stream), "hipMemsetAsync");
    const std::vector<const FdbSortField*> d_fields = stage_fields(p, &cs);
    const size_t last = p.words.size() - 1;
    in.note_reader(stream);
    hip_check(fdb_launch_sort_keys(d_fields[last], (int)p.words[last].size(), nullptr, in.rows, keys_a, nullptr, stream), "sort keys launch");
    for (int32_t r = 0; r < warmup + reps; r++) {
      hip_check(hipEventRecord(ev.a, stream), "hipEventRecord");
      for (size_t w = p.words.size(); w-- > 0;) {
        size_t tb = temp_bytes;
        hip_check(fdb_sort_pairs_u64(temp, &tb, keys_a, keys_b, vals_a, vals_b, in.rows, p.bits[w], stream), "sort pairs");
      }
      hip_check(hipEventRecord(ev.b, stream), "hipEventRecord");
      hip_check(hipStreamSynchronize(stream), "hipStreamSynchronize");
      float t = 0;
      hip_check(hipEventElapsedTime(&t, ev.a, ev.b), "hipEventElapsedTime");
      if (r >= warmup) ms.push_back(t);
    }
  }
  *bare_ms = median(ms);
}

}  // namespace fdb
