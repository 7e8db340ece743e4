// fdb_capi.cpp — the extern "C" surface declared in include/frostdb_amd.h. Every entry point converts C++
// exceptions into fdb_status codes (never aborts: the Go side wraps chains in recovery.Do, physicalplan.go:142).
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "fdb_codec.h"
#include "fdb_comm.h"
#include "fdb_context.h"
#include "fdb_dynamic.h"
#include "fdb_jit.h"
#include "fdb_mergepath.h"
#include "fdb_mergerec.h"
#include "fdb_plan.h"
#include "fdb_pqwrite_host.h"
#include "fdb_record.h"
#include "fdb_regex.h"
#include "fdb_sort.h"
#include "fdb_sortkey.h"
#include "fdb_take.h"

// A plan handle: one operator chain. With aggregations over a DynamicColumn (fdb_dynamic.h) `plan` is the family's main plan
// (static aggregations / group keys) and `dyn` holds the children.
struct fdb_plan {
  std::unique_ptr<fdb::DynamicAggs> dyn;
  fdb_plan_desc main_desc;
  fdb::Plan plan;
  fdb_plan(const fdb_plan_desc* d, int dev)
      : dyn(fdb::DynamicAggs::wanted(d) ? new fdb::DynamicAggs(d, dev) : nullptr),
        main_desc(dyn ? dyn->main_desc() : (d ? *d : fdb_plan_desc())),
        plan(d ? &main_desc : nullptr, dev) {}
  // a fresh plan of `proto`'s descriptor (the shard of fdb_plan_exchange)
  explicit fdb_plan(const fdb::Plan& proto) : main_desc(), plan(proto, fdb::Plan::CloneTag()) {}
};
struct fdb_comm { std::unique_ptr<fdb::Comm> c; };
struct fdb_batch { std::unique_ptr<fdb::DeviceBatch> b; };
struct fdb_osync { fdb::OrderedSync s; fdb_osync(int32_t inputs, const fdb_order_col* order, int32_t n_order) : s(inputs, order, n_order) {} };
struct fdb_sampler { fdb::Sampler s; fdb_sampler(int64_t size, uint64_t seed, int device) : s(size, seed, device) {} };

namespace {
thread_local std::string g_last_error;

template <typename F>
int guard(fdb_plan* p, F&& f) {
  try {
    f();
    return FDB_OK;
  } catch (const fdb::Error& e) {
    if (p) p->plan.error = e.what(); else g_last_error = e.what();
    return e.code;
  } catch (const std::bad_alloc&) {
    if (p) p->plan.error = "out of host memory"; else g_last_error = "out of host memory";
    return FDB_ERR_OOM;
  } catch (const std::exception& e) {
    if (p) p->plan.error = e.what(); else g_last_error = e.what();
    return FDB_ERR_INVALID;
  } catch (...) {
    if (p) p->plan.error = "unknown error"; else g_last_error = "unknown error";
    return FDB_ERR_INVALID;
  }
}
// Entry points that expose ONE table (state arrays for the RCCL merges, the hash exchange) do not apply to a family of plans.
void single_table_only(const fdb_plan* p) {
  if (p->dyn) throw fdb::Error(FDB_ERR_UNSUPPORTED, "not available for a plan with aggregations over a dynamic column set (merge such plans with fdb_plan_merge)");
}
}  // namespace

namespace {
template <typename F>
int comm_guard(fdb_comm* c, F&& f) {
  try {
    f();
    return FDB_OK;
  } catch (const fdb::Error& e) {
    if (c && c->c) c->c->error = e.what();
    g_last_error = e.what();
    return e.code;
  } catch (const std::bad_alloc&) {
    g_last_error = "out of host memory";
    return FDB_ERR_OOM;
  } catch (const std::exception& e) {
    if (c && c->c) c->c->error = e.what();
    g_last_error = e.what();
    return FDB_ERR_INVALID;
  }
}
int wrap_all(std::vector<std::unique_ptr<fdb::Comm>>&& v, fdb_comm** out) {
  for (size_t i = 0; i < v.size(); i++) { out[i] = new fdb_comm(); out[i]->c = std::move(v[i]); }
  return FDB_OK;
}
}  // namespace

namespace fdb { void widen_indices(const void* src, int width, uint32_t* dst, size_t n); void widen_indices_mapped(const void* src, int width, const uint32_t* table, size_t table_len, uint32_t* dst, size_t n); }  // fdb_widen.cc

extern "C" {

const char* fdb_version(void) { return "frostdb_amd 0.1.0 (gfx950)"; }
const char* fdb_last_error(void) { return g_last_error.c_str(); }

int fdb_device_count(int* n_devices) {
  return guard(nullptr, [&] {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) { n = 0; (void)hipGetLastError(); }
    *n_devices = n;
  });
}

int fdb_plan_explain(const fdb_plan_desc* desc, char* buf, int64_t capacity, int64_t* needed) {
  return guard(nullptr, [&] {
    std::string s;
    if (fdb::DynamicAggs::wanted(desc)) {
      fdb::DynamicAggs dyn(desc, 0);
      const fdb_plan_desc md = dyn.main_desc();
      fdb::Plan plan(&md, 0, /*explain_only=*/true);
      s = dyn.draw(plan);
    } else {
      fdb::Plan plan(desc, 0, /*explain_only=*/true);
      s = plan.draw();
    }
    if (needed != nullptr) *needed = (int64_t)s.size() + 1;
    if (buf != nullptr && capacity > 0) {
      const size_t n = std::min((size_t)capacity - 1, s.size());
      std::memcpy(buf, s.data(), n);
      buf[n] = 0;
    }
  });
}

int fdb_selftest_widen(const void* src, int32_t width, uint32_t* dst, int64_t n) {
  return guard(nullptr, [&] {
    if ((width != 1 && width != 2 && width != 4 && width != -2 && width != -4 && width != -12 && width != -14) || n < 0 || ((src == nullptr || dst == nullptr) && n > 0))
      throw fdb::Error(FDB_ERR_INVALID, "widen: width 1, 2, 4 (bytes) or -2, -4 (bits) and non-null buffers");
    if (width == -12 || width == -14) {  // the rank → index road of the same widths, through the table t[r] = 3 r + 5 of 4 / 16 entries
      uint32_t table[16];
      for (uint32_t r = 0; r < 16; r++) table[r] = 3 * r + 5;
      fdb::widen_indices_mapped(src, width + 10, table, width == -12 ? 4 : 16, dst, (size_t)n);
      return;
    }
    fdb::widen_indices(src, width, dst, (size_t)n);
  });
}

// The three scan-cache selftests behind their fronts' argument rules: the builder as scan_cache_get runs it — a uint32 column (and its bitmap:
// the null-folded builder) in their slots, the cache in a slot of its form —, `out_bytes` of it copied out, every row read back where scan_cache_at says.
static void selftest_scan_cache(const char* what, const uint32_t* indices, const uint8_t* validity, int64_t rows, int64_t entries, fdb::ScanForm form, int device, uint8_t* out, int64_t out_bytes) {
  const std::string w = what;
  fdb::CallScope call(device);
  void* d_src = call.alloc(fdb::values_slot((size_t)rows, 4));
  uint8_t* d_bits = validity != nullptr ? (uint8_t*)call.alloc(fdb::bitmap_slot((size_t)rows)) : nullptr;
  void* d_dst = call.alloc(fdb::scan_form_slot((size_t)rows, form));
  fdb::hip_check(hipMemcpyAsync(d_src, indices, (size_t)rows * 4, hipMemcpyHostToDevice, call.ctx->stream), (w + ": copy in").c_str());
  if (validity != nullptr) fdb::hip_check(hipMemcpyAsync(d_bits, validity, (size_t)(rows + 7) / 8, hipMemcpyHostToDevice, call.ctx->stream), (w + ": copy in").c_str());
  fdb::hip_check(fdb_launch_narrow_indices((const uint32_t*)d_src, d_bits, (uint32_t)entries, d_dst, rows, form, call.ctx->stream), (w + ": builder").c_str());
  fdb::hip_check(hipMemcpyAsync(out, d_dst, (size_t)out_bytes, hipMemcpyDeviceToHost, call.ctx->stream), (w + ": copy out").c_str());
  fdb::hip_check(hipStreamSynchronize(call.ctx->stream), (w + ": wait").c_str());
  for (int64_t i = 0; i < rows; i++) {
    const bool null = validity != nullptr && ((validity[i >> 3] >> (i & 7)) & 1) == 0;
    const uint32_t want = null ? (uint32_t)entries : indices[i] & fdb::scan_form(form).max_index;
    if (fdb::scan_cache_read(out, i, rows, form) != want) throw fdb::Error(FDB_ERR_INVALID, w + ": row " + std::to_string(i) + " is not at its position");
  }
}

int fdb_selftest_scan_cache(const uint32_t* indices, int64_t rows, int32_t width, int device, uint8_t* out, int64_t out_bytes) {
  return guard(nullptr, [&] {
    if (indices == nullptr || out == nullptr || rows <= 0 || rows > ((int64_t)1 << 28) || (width != 1 && width != 2) || out_bytes != (rows * width + 15) / 16 * 16)
      throw fdb::Error(FDB_ERR_INVALID, "scan cache: 1 to 2^28 rows, width 1 or 2, out_bytes = rows * width rounded up to 16");
    selftest_scan_cache("scan cache", indices, nullptr, rows, 0, (fdb::ScanForm)width, device, out, out_bytes);
  });
}

int fdb_selftest_scan_cache_nulls(const uint32_t* indices, const uint8_t* validity, int64_t rows, int64_t entries, int32_t width, int device, uint8_t* out, int64_t out_bytes) {
  return guard(nullptr, [&] {
    if (indices == nullptr || validity == nullptr || out == nullptr || rows <= 0 || rows > ((int64_t)1 << 28) || (width != 1 && width != 2) ||
        entries < 0 || entries > (int64_t)fdb::scan_form((fdb::ScanForm)width).max_index || out_bytes != (rows * width + 15) / 16 * 16)
      throw fdb::Error(FDB_ERR_INVALID, "scan cache: 1 to 2^28 rows, width 1 or 2, entries <= 255 / 65 535, out_bytes = rows * width rounded up to 16");
    selftest_scan_cache("scan cache", indices, validity, rows, entries, (fdb::ScanForm)width, device, out, out_bytes);
  });
}

int fdb_selftest_scan_cache_packed(const uint32_t* indices, const uint8_t* validity, int64_t rows, int64_t entries, int32_t form, int device, uint8_t* out, int64_t out_bytes) {
  return guard(nullptr, [&] {
    const fdb::ScanFormRow* f = fdb::scan_form_row(form);
    if (indices == nullptr || out == nullptr || rows <= 0 || rows > ((int64_t)1 << 28) || f == nullptr || !f->framed || entries < 0 ||
        entries + (validity != nullptr ? 1 : 0) > (int64_t)f->max_index + 1 || out_bytes != (rows + fdb::kScanCacheBlock - 1) / fdb::kScanCacheBlock * f->block_bytes)
      throw fdb::Error(FDB_ERR_INVALID, "packed scan cache: 1 to 2^28 rows, form H (5) or T (6), entries (+ 1 with a bitmap) <= 16 / 4 096, out_bytes = whole frames");
    selftest_scan_cache("packed scan cache", indices, validity, rows, entries, f->form, device, out, out_bytes);
  });
}

// The device prefix sums, each launch sequence as the library runs it (scratch at the sizes fdb_kernels.h documents), over a caller's array.
int fdb_selftest_prefix_sums(int32_t kind, int device, const uint32_t* in, int64_t n, int32_t option, const int64_t* recs, int32_t n_recs, uint32_t* out,
                             uint64_t* totals) {
  return guard(nullptr, [&] {
    const int64_t max_n = (int64_t)1 << 28;
    const int64_t stride = kind == 2 ? option : 1;
    if (kind < 0 || kind > 2 || n < 0 || n > max_n || totals == nullptr || (n > 0 && (in == nullptr || out == nullptr)))
      throw fdb::Error(FDB_ERR_INVALID, "prefix sums: kind 0, 1 or 2, 0 to 2^28 entries, non-null buffers");
    if (kind == 0 && option != 0 && option != 1) throw fdb::Error(FDB_ERR_INVALID, "prefix sums: exclusive scan takes option 0 (block sums) or 1 (none)");
    if (kind == 2 && (stride < 1 || stride > 16 || n * stride > max_n)) throw fdb::Error(FDB_ERR_INVALID, "prefix sums: strided scan takes a stride of 1 to 16, 2^28 words in all");
    if (kind != 1 && (recs != nullptr || n_recs != 0)) throw fdb::Error(FDB_ERR_INVALID, "prefix sums: a record table goes with kind 1 only");
    if (kind == 1) {
      if (option < 0 || option > 2 || n < 1 || recs == nullptr || n_recs < 1 || n_recs > n)
        throw fdb::Error(FDB_ERR_INVALID, "prefix sums: filter scan takes option 0 (as filter() chooses), 1 (one level) or 2 (two levels), tiles and their records");
      // the table as filter() builds it: records with rows only, each owning the tiles of its rows, end to end from tile 0
      for (int32_t r = 0; r < n_recs; r++) {
        const int64_t begin = recs[2 * r], rows = recs[2 * r + 1], end = r + 1 < n_recs ? recs[2 * r + 2] : n;
        if (begin < 0 || begin >= n || (r == 0 && begin != 0) || rows < 1 || rows > max_n * FDB_COMPACT_TILE || begin + (rows + FDB_COMPACT_TILE - 1) / FDB_COMPACT_TILE != end)
          throw fdb::Error(FDB_ERR_INVALID, "prefix sums: record " + std::to_string(r) + " does not own the tiles of its rows, after its predecessor's");
      }
    }
    fdb::CallScope call(device);
    const hipStream_t stream = call.ctx->stream;
    const int64_t n_blocks = (n + 1023) / 1024;
    const size_t n_totals = kind == 1 ? (size_t)n_recs + 1 : 1;
    unsigned long long* d_totals = (unsigned long long*)call.alloc(n_totals * 8 + 64);
    // (what a launch leaves unwritten reads 0xA5… afterwards)
    fdb::hip_check(hipMemsetAsync(d_totals, 0xA5, n_totals * 8, stream), "prefix sums: fill");
    uint32_t* d_out = nullptr;
    if (kind == 0) {
      uint32_t* d_counts = (uint32_t*)call.alloc((size_t)n * 4 + 256);
      uint32_t* d_block_sums = option == 0 ? (uint32_t*)call.alloc(((size_t)n_blocks + 1) * 4) : nullptr;
      if (n > 0) fdb::hip_check(hipMemcpyAsync(d_counts, in, (size_t)n * 4, hipMemcpyHostToDevice, stream), "prefix sums: copy in");
      fdb::hip_check(fdb_launch_exclusive_scan(d_counts, n, d_block_sums, d_totals, stream), "prefix sums: exclusive scan");
      d_out = d_counts;
    } else if (kind == 1) {
      // block sums in front of the tile counts, as count_rows_two_pass lays them out
      unsigned char* d_counts = (unsigned char*)call.alloc((size_t)n_blocks * 8 + (size_t)n * 4 + 256);
      unsigned long long* d_block_sums = (unsigned long long*)d_counts;
      uint32_t* d_tile_counts = (uint32_t*)(d_counts + (size_t)n_blocks * 8);
      d_out = (uint32_t*)call.alloc((size_t)n * 4 + 256);
      FdbCompactRec* d_recs = (FdbCompactRec*)call.alloc((size_t)n_recs * sizeof(FdbCompactRec));
      static_assert(sizeof(FdbCompactRec) == 16, "the record table crosses the C ABI as pairs of int64");
      fdb::hip_check(hipMemcpyAsync(d_tile_counts, in, (size_t)n * 4, hipMemcpyHostToDevice, stream), "prefix sums: copy in");
      fdb::hip_check(hipMemcpyAsync(d_recs, recs, (size_t)n_recs * sizeof(FdbCompactRec), hipMemcpyHostToDevice, stream), "prefix sums: copy in");
      fdb::hip_check(hipMemsetAsync(d_out, 0xA5, (size_t)n * 4, stream), "prefix sums: fill");
      const bool two_level = option == 0 ? fdb_sel_scan_two_level(n) : option == 2;
      if (two_level) fdb::hip_check(fdb_launch_sel_block_sums(d_tile_counts, n, d_block_sums, stream), "prefix sums: block sums");
      fdb::hip_check(fdb_launch_sel_scan(d_tile_counts, two_level ? d_block_sums : nullptr, n, d_out, d_recs, n_recs, d_totals, stream), "prefix sums: filter scan");
    } else {
      uint32_t* d_in = (uint32_t*)call.alloc((size_t)(n * stride) * 4 + 256);
      d_out = (uint32_t*)call.alloc((size_t)n * 4 + 256);
      unsigned long long* d_scratch = (unsigned long long*)call.alloc(((size_t)n / 1024 + 2) * 8);
      if (n > 0) fdb::hip_check(hipMemcpyAsync(d_in, in, (size_t)(n * stride) * 4, hipMemcpyHostToDevice, stream), "prefix sums: copy in");
      if (n > 0) fdb::hip_check(hipMemsetAsync(d_out, 0xA5, (size_t)n * 4, stream), "prefix sums: fill");
      fdb::hip_check(fdb_launch_scan_u32(d_in, (int)stride, d_out, n, d_scratch, d_totals, stream), "prefix sums: strided scan");
    }
    if (n > 0) fdb::hip_check(hipMemcpyAsync(out, d_out, (size_t)n * 4, hipMemcpyDeviceToHost, stream), "prefix sums: copy out");
    fdb::hip_check(hipMemcpyAsync(totals, d_totals, n_totals * 8, hipMemcpyDeviceToHost, stream), "prefix sums: copy out");
    fdb::hip_check(hipStreamSynchronize(stream), "prefix sums: wait");
  });
}

int fdb_selftest_exact_sum(const double* x, int64_t n, double* out) {
  return guard(nullptr, [&] {
    if (n < 0 || out == nullptr || (n > 0 && x == nullptr)) throw fdb::Error(FDB_ERR_INVALID, "exact sum: n >= 0 and non-null buffers");
    // the host twin of the device path: the same digit split into the same limbs, the same normalize and rounding (fdb_kernels.h);
    // the adds run as the scan would between two normalizes
    long long limbs[FDB_EXACT_LIMBS] = {0};
    unsigned long long flags = 0;
    int64_t since = 0;
    for (int64_t i = 0; i < n; i++) {
      unsigned long long bits;
      std::memcpy(&bits, x + i, 8);
      int k; long long d0, d1, d2;
      const unsigned long long f = fdb_exact_split(bits, &k, &d0, &d1, &d2);
      if (f != 0ull) { flags |= f; continue; }
      limbs[k] += d0; limbs[k + 1] += d1; limbs[k + 2] += d2;
      if (++since == ((int64_t)1 << 30)) { fdb_exact_normalize(limbs); since = 0; }
    }
    const unsigned long long r = fdb_exact_round(limbs, flags);
    std::memcpy(out, &r, 8);
  });
}

int fdb_arrow_roundtrip(struct ArrowArray* batch, struct ArrowSchema* schema, struct ArrowArray* out, struct ArrowSchema* out_schema) {
  return guard(nullptr, [&] {
    if (out == nullptr || out_schema == nullptr) throw fdb::Error(FDB_ERR_INVALID, "null output");
    fdb::HostRecordView view;
    fdb::view_record(batch, schema, &view);
    fdb::roundtrip_record(view, out, out_schema);
  });
}

int fdb_read_ceiling(int device, int64_t bytes, int32_t reps, double* gb_per_s) {
  return guard(nullptr, [&] {
    if (gb_per_s == nullptr || bytes < (1 << 20) || reps < 1) throw fdb::Error(FDB_ERR_INVALID, "fdb_read_ceiling: bytes >= 1 MiB, reps >= 1");
    *gb_per_s = 0;
    bytes &= ~(int64_t)4095;
    if (hipSetDevice(device) != hipSuccess) throw fdb::Error(FDB_ERR_DEVICE, "hipSetDevice failed");
    void* buf = nullptr;
    unsigned long long* out = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    auto cleanup = [&] { if (buf) (void)hipFree(buf); if (out) (void)hipFree(out); if (e0) (void)hipEventDestroy(e0); if (e1) (void)hipEventDestroy(e1); };
    auto ck = [&](hipError_t e, const char* what) { if (e != hipSuccess) { cleanup(); throw fdb::Error(e == hipErrorOutOfMemory ? FDB_ERR_OOM : FDB_ERR_DEVICE, std::string(what) + ": " + hipGetErrorString(e)); } };
    ck(hipMalloc(&buf, (size_t)bytes), "hipMalloc");
    ck(hipMalloc((void**)&out, 64), "hipMalloc");
    ck(hipMemset(buf, 0, (size_t)bytes), "hipMemset");
    ck(hipEventCreate(&e0), "hipEventCreate");
    ck(hipEventCreate(&e1), "hipEventCreate");
    ck(fdb_launch_stream_read(buf, bytes, out, nullptr), "launch");  // warm-up
    float best = 0;
    for (int r = 0; r < reps; r++) {
      ck(hipEventRecord(e0, nullptr), "hipEventRecord");
      ck(fdb_launch_stream_read(buf, bytes, out, nullptr), "launch");
      ck(hipEventRecord(e1, nullptr), "hipEventRecord");
      ck(hipEventSynchronize(e1), "hipEventSynchronize");
      float ms = 0;
      ck(hipEventElapsedTime(&ms, e0, e1), "hipEventElapsedTime");
      if (ms > 0 && (best == 0 || ms < best)) best = ms;
    }
    cleanup();
    if (best > 0) *gb_per_s = (double)bytes / (best * 1e-3) / 1e9;
  });
}

int fdb_plan_create(const fdb_plan_desc* desc, int device, fdb_plan** out) {
  return guard(nullptr, [&] {
    if (out == nullptr) throw fdb::Error(FDB_ERR_INVALID, "null out pointer");
    if (desc != nullptr && desc->ordered != 0 && fdb::DynamicAggs::wanted(desc))
      throw fdb::Error(FDB_ERR_UNSUPPORTED, "OrderedAggregate over a dynamic column set is not supported");
    *out = new fdb_plan(desc, device);
  });
}

int fdb_plan_push(fdb_plan* plan, struct ArrowArray* batch, struct ArrowSchema* schema) {
  if (!plan) return FDB_ERR_INVALID;
  return guard(plan, [&] { if (plan->dyn) plan->dyn->push(plan->plan, batch, schema); else plan->plan.push(batch, schema); });
}

int fdb_plan_push_many(fdb_plan* plan, struct ArrowArray* const* batches, struct ArrowSchema* const* schemas, int32_t n, int32_t* n_pushed) {
  if (n_pushed) *n_pushed = 0;
  if (!plan || n < 0 || (n > 0 && (!batches || !schemas))) return FDB_ERR_INVALID;
  for (int32_t i = 0; i < n; i++) {
    const int rc = fdb_plan_push(plan, batches[i], schemas[i]);
    if (rc != 0) return rc;
    if (n_pushed) *n_pushed = i + 1;
  }
  return 0;
}

int fdb_plan_push_batch(fdb_plan* plan, const fdb_batch* batch) {
  if (!plan || !batch) return FDB_ERR_INVALID;
  return guard(plan, [&] {
    if (plan->dyn) { const fdb::DeviceBatch* b = batch->b.get(); plan->dyn->push_batches(plan->plan, &b, 1); return; }
    plan->plan.settle();
    plan->plan.push_batch(*batch->b);
  });
}

int fdb_plan_push_batches(fdb_plan* plan, const fdb_batch* const* batches, int32_t n) {
  if (!plan || (n > 0 && !batches)) return FDB_ERR_INVALID;
  return guard(plan, [&] {
    std::vector<const fdb::DeviceBatch*> v;
    for (int32_t i = 0; i < n; i++) {
      if (batches[i] == nullptr) throw fdb::Error(FDB_ERR_INVALID, "null batch");
      v.push_back(batches[i]->b.get());
    }
    if (plan->dyn) { plan->dyn->push_batches(plan->plan, v.data(), (int)v.size()); return; }
    plan->plan.settle();
    plan->plan.push_batches(v.data(), (int)v.size());
  });
}

int fdb_plan_finish(fdb_plan* plan, struct ArrowArray* out, struct ArrowSchema* out_schema, int64_t* n_rows) {
  if (!plan) return FDB_ERR_INVALID;
  return guard(plan, [&] {
    if (plan->dyn) { plan->dyn->finish(plan->plan, out, out_schema, n_rows); return; }
    plan->plan.settle();
    plan->plan.finish(out, out_schema, n_rows);
  });
}

int fdb_plan_finish_next(fdb_plan* plan, struct ArrowArray* out, struct ArrowSchema* out_schema, int64_t* n_rows, int32_t* emitted) {
  if (!plan || !out || !out_schema || !emitted) return FDB_ERR_INVALID;
  *emitted = 0;
  return guard(plan, [&] {
    std::memset(out, 0, sizeof(*out));
    std::memset(out_schema, 0, sizeof(*out_schema));
    *emitted = plan->plan.finish_next(out, out_schema, n_rows) ? 1 : 0;  // (a family of plans behind a dynamic aggregation emits one record: nothing pending)
  });
}

int fdb_plan_merge(fdb_plan* dst, fdb_plan* src) {
  if (!dst || !src) return FDB_ERR_INVALID;
  return guard(dst, [&] {
    if ((dst->dyn != nullptr) != (src->dyn != nullptr)) throw fdb::Error(FDB_ERR_INVALID, "plans have different aggregations");
    if (dst->dyn) { dst->dyn->merge_from(dst->plan, *src->dyn, src->plan); return; }
    src->plan.settle();
    dst->plan.settle();
    dst->plan.merge_from(src->plan);
  });
}

int fdb_plan_group_schema(fdb_plan* plan, struct ArrowArray* out, struct ArrowSchema* out_schema) {
  if (!plan || !out || !out_schema) return FDB_ERR_INVALID;
  return guard(plan, [&] { single_table_only(plan); plan->plan.refuse_exact("fdb_plan_group_schema"); plan->plan.settle(); plan->plan.group_schema(out, out_schema); });
}

int fdb_plan_seed_groups(fdb_plan* plan, struct ArrowArray* schema_record, struct ArrowSchema* schema) {
  if (!plan || !schema_record || !schema) return FDB_ERR_INVALID;
  return guard(plan, [&] { single_table_only(plan); plan->plan.settle(); plan->plan.seed_groups(schema_record, schema); });
}

int fdb_plan_hash_export(fdb_plan* src, fdb_plan* layout, int32_t n_parts, void** dev_rows, int64_t* counts, int32_t* row_words32) {
  if (!src || !layout || !dev_rows || !counts || !row_words32) return FDB_ERR_INVALID;
  return guard(src, [&] { single_table_only(src); single_table_only(layout); src->plan.refuse_exact("fdb_plan_hash_export"); layout->plan.refuse_exact("fdb_plan_hash_export"); src->plan.settle(); layout->plan.settle(); src->plan.hash_export(layout->plan, n_parts, dev_rows, counts, row_words32); });
}

int fdb_plan_hash_import(fdb_plan* plan, const void* dev_rows, int64_t n_rows) {
  if (!plan || (n_rows > 0 && !dev_rows)) return FDB_ERR_INVALID;
  return guard(plan, [&] { single_table_only(plan); plan->plan.refuse_exact("fdb_plan_hash_import"); plan->plan.settle(); plan->plan.hash_import(dev_rows, n_rows); });
}

int fdb_plan_filter(fdb_plan* plan, struct ArrowArray* batch, struct ArrowSchema* schema, struct ArrowArray* out,
                    struct ArrowSchema* out_schema, int64_t* n_selected) {
  if (!plan) return FDB_ERR_INVALID;
  return guard(plan, [&] { plan->plan.filter(batch, schema, out, out_schema, n_selected); });
}

int fdb_plan_select(fdb_plan* plan, struct ArrowArray* batch, struct ArrowSchema* schema, uint32_t* indices, int64_t capacity,
                    int64_t* n_selected) {
  if (!plan) return FDB_ERR_INVALID;
  return guard(plan, [&] { plan->plan.select(batch, schema, indices, capacity, n_selected); });
}

int fdb_plan_filter_batch(fdb_plan* plan, const fdb_batch* batch, fdb_batch** out, int64_t* n_selected) {
  if (!plan) return FDB_ERR_INVALID;
  return guard(plan, [&] {
    if (batch == nullptr || !batch->b || out == nullptr || n_selected == nullptr) throw fdb::Error(FDB_ERR_INVALID, "null argument");
    *out = nullptr;
    std::unique_ptr<fdb::DeviceBatch> r = plan->plan.filter_batch(*batch->b, n_selected);
    *out = new fdb_batch{std::move(r)};
  });
}

int fdb_plan_finish_batch(fdb_plan* plan, fdb_batch** out, int64_t* n_rows) {
  if (!plan) return FDB_ERR_INVALID;
  return guard(plan, [&] {
    if (out == nullptr) throw fdb::Error(FDB_ERR_INVALID, "null argument");
    *out = nullptr;
    single_table_only(plan);
    std::unique_ptr<fdb::DeviceBatch> r = plan->plan.finish_batch(n_rows);
    *out = new fdb_batch{std::move(r)};
  });
}

int fdb_plan_filter_batches(fdb_plan* plan, const fdb_batch* const* batches, int32_t n, fdb_batch** out, int64_t* n_selected) {
  if (!plan) return FDB_ERR_INVALID;
  return guard(plan, [&] {
    if (n < 0 || (n > 0 && (batches == nullptr || out == nullptr || n_selected == nullptr))) throw fdb::Error(FDB_ERR_INVALID, "null argument");
    std::vector<const fdb::DeviceBatch*> bs;
    for (int32_t i = 0; i < n; i++) {
      out[i] = nullptr;
      if (batches[i] == nullptr || !batches[i]->b) throw fdb::Error(FDB_ERR_INVALID, "null batch");
      bs.push_back(batches[i]->b.get());
    }
    std::vector<std::unique_ptr<fdb::DeviceBatch>> rs = plan->plan.filter_batches(bs.data(), n, n_selected);
    for (int32_t i = 0; i < n; i++) out[i] = new fdb_batch{std::move(rs[(size_t)i])};
  });
}

int fdb_plan_project_batch(fdb_plan* plan, const fdb_project_col* cols, int32_t n_cols, const fdb_batch* in, fdb_batch** out) {
  if (!plan) return FDB_ERR_INVALID;
  return guard(plan, [&] {
    if (in == nullptr || !in->b || out == nullptr) throw fdb::Error(FDB_ERR_INVALID, "null argument");
    *out = nullptr;
    std::unique_ptr<fdb::DeviceBatch> r = plan->plan.project_batch(cols, n_cols, *in->b);
    *out = new fdb_batch{std::move(r)};
  });
}

int fdb_plan_project_batches(fdb_plan* plan, const fdb_project_col* cols, int32_t n_cols, const fdb_batch* const* in, int32_t n, fdb_batch** out) {
  if (!plan) return FDB_ERR_INVALID;
  return guard(plan, [&] {
    if (n < 0 || (n > 0 && (in == nullptr || out == nullptr))) throw fdb::Error(FDB_ERR_INVALID, "null argument");
    std::vector<const fdb::DeviceBatch*> bs;
    for (int32_t i = 0; i < n; i++) {
      out[i] = nullptr;
      if (in[i] == nullptr || !in[i]->b) throw fdb::Error(FDB_ERR_INVALID, "null batch");
      bs.push_back(in[i]->b.get());
    }
    std::vector<std::unique_ptr<fdb::DeviceBatch>> rs = plan->plan.project_batches(cols, n_cols, bs.data(), n);
    for (int32_t i = 0; i < n; i++) out[i] = new fdb_batch{std::move(rs[(size_t)i])};
  });
}

int fdb_plan_project(fdb_plan* plan, const fdb_project_col* cols, int32_t n_cols, struct ArrowArray* batch, struct ArrowSchema* schema, struct ArrowArray* out,
                     struct ArrowSchema* out_schema) {
  if (!plan) return FDB_ERR_INVALID;
  return guard(plan, [&] {
    if (batch == nullptr || schema == nullptr || out == nullptr || out_schema == nullptr) throw fdb::Error(FDB_ERR_INVALID, "null argument");
    plan->plan.project(cols, n_cols, batch, schema, out, out_schema);
  });
}

int fdb_plan_select_batch(fdb_plan* plan, const fdb_batch* batch, uint32_t* dev_indices, int64_t capacity, int64_t* n_selected) {
  if (!plan) return FDB_ERR_INVALID;
  return guard(plan, [&] {
    if (batch == nullptr || !batch->b || dev_indices == nullptr || n_selected == nullptr) throw fdb::Error(FDB_ERR_INVALID, "null argument");
    *n_selected = plan->plan.select_batch(*batch->b, dev_indices, capacity);
  });
}

int fdb_batch_export(const fdb_batch* batch, struct ArrowArray* out, struct ArrowSchema* out_schema) {
  return guard(nullptr, [&] {
    if (batch == nullptr || !batch->b || out == nullptr || out_schema == nullptr) throw fdb::Error(FDB_ERR_INVALID, "null argument");
    fdb::export_batch(*batch->b, out, out_schema);
  });
}

int fdb_batch_take(const fdb_batch* in, const int32_t* indices, int64_t n, fdb_batch** out) {
  return guard(nullptr, [&] {
    if (in == nullptr || !in->b || out == nullptr) throw fdb::Error(FDB_ERR_INVALID, "null argument");
    *out = nullptr;
    std::unique_ptr<fdb::DeviceBatch> r = fdb::take_batch(*in->b, indices, n);
    *out = new fdb_batch{std::move(r)};
  });
}

int fdb_batch_limit(const fdb_batch* in, uint64_t count, fdb_batch** out) {
  return guard(nullptr, [&] {
    if (in == nullptr || !in->b || out == nullptr) throw fdb::Error(FDB_ERR_INVALID, "null argument");
    *out = nullptr;
    std::unique_ptr<fdb::DeviceBatch> r = fdb::limit_batch(*in->b, count);
    *out = new fdb_batch{std::move(r)};
  });
}

int fdb_batch_sort_indices(const fdb_batch* in, const fdb_sort_col* cols, int32_t n_cols, int32_t* indices_out) {
  return guard(nullptr, [&] {
    if (in == nullptr || !in->b) throw fdb::Error(FDB_ERR_INVALID, "null argument");
    fdb::sort_batch_indices(*in->b, cols, n_cols, indices_out);
  });
}

int fdb_batch_sort(const fdb_batch* in, const fdb_sort_col* cols, int32_t n_cols, fdb_batch** out) {
  return guard(nullptr, [&] {
    if (in == nullptr || !in->b || out == nullptr) throw fdb::Error(FDB_ERR_INVALID, "null argument");
    *out = nullptr;
    std::unique_ptr<fdb::DeviceBatch> r = fdb::sort_batch(*in->b, cols, n_cols);
    *out = new fdb_batch{std::move(r)};
  });
}

int fdb_selftest_sort_key(int32_t kind, uint32_t direction, uint64_t raw, uint64_t* key_out) {
  return guard(nullptr, [&] {
    if (key_out == nullptr) throw fdb::Error(FDB_ERR_INVALID, "null argument");
    if (kind != FDB_SORT_I64 && kind != FDB_SORT_U64 && kind != FDB_SORT_F64) throw fdb::Error(FDB_ERR_INVALID, "sort key: kind is not int64 (1), uint64 (2) or float64 (3)");
    if (direction > 1u) throw fdb::Error(FDB_ERR_INVALID, "sort key: direction is not 0 (ascending) or 1 (descending)");
    *key_out = fdb_sortkey_directed(fdb_sortkey_value(kind, raw), direction == 1u ? FDB_SORT_DESC : 0u, 64);
  });
}

int fdb_sort_bench(const fdb_batch* in, const fdb_sort_col* cols, int32_t n_cols, int32_t reps, int32_t warmup, double* sort_ms, double* bare_ms, int32_t* n_passes) {
  return guard(nullptr, [&] {
    if (in == nullptr || !in->b) throw fdb::Error(FDB_ERR_INVALID, "null argument");
    fdb::sort_bench(*in->b, cols, n_cols, reps, warmup, sort_ms, bare_ms, n_passes);
  });
}

extern "C++" {
static std::vector<const fdb::DeviceBatch*> merge_inputs(const fdb_batch* const* in, int32_t n) {
  if (n < 0 || (n > 0 && in == nullptr)) throw fdb::Error(FDB_ERR_INVALID, "merge: bad record list");
  std::vector<const fdb::DeviceBatch*> recs((size_t)n, nullptr);
  for (int32_t r = 0; r < n; r++) {
    if (in[r] == nullptr || !in[r]->b) throw fdb::Error(FDB_ERR_INVALID, "merge: record " + std::to_string(r) + " is null");
    recs[(size_t)r] = in[r]->b.get();
  }
  return recs;
}
}

int fdb_batches_merge(const fdb_batch* const* in, int32_t n, const fdb_sort_col* cols, int32_t n_cols, uint64_t limit, fdb_batch** out) {
  return guard(nullptr, [&] {
    if (out == nullptr) throw fdb::Error(FDB_ERR_INVALID, "null argument");
    *out = nullptr;
    const std::vector<const fdb::DeviceBatch*> recs = merge_inputs(in, n);
    std::unique_ptr<fdb::DeviceBatch> r = fdb::merge_batches(recs.data(), n, cols, n_cols, limit);
    *out = new fdb_batch{std::move(r)};
  });
}

int fdb_batches_merge_named(const fdb_batch* const* in, int32_t n, const fdb_order_col* order, int32_t n_order, uint64_t limit, fdb_batch** out) {
  return guard(nullptr, [&] {
    if (out == nullptr) throw fdb::Error(FDB_ERR_INVALID, "null argument");
    *out = nullptr;
    const std::vector<const fdb::DeviceBatch*> recs = merge_inputs(in, n);
    std::unique_ptr<fdb::DeviceBatch> r = fdb::merge_batches_named(recs.data(), n, order, n_order, limit);
    *out = new fdb_batch{std::move(r)};
  });
}

int fdb_selftest_merge_schema(const char* const* names, const int32_t* kinds, const int32_t* n_fields, int32_t n_records, const fdb_order_col* order, int32_t n_order,
                              int32_t* out_fields, int32_t* col_map, int32_t cap, int32_t* n_out, int32_t* n_sort) {
  return guard(nullptr, [&] {
    if (n_records < 0 || (n_records > 0 && n_fields == nullptr) || order == nullptr || n_order <= 0 || cap < 0 || n_out == nullptr || n_sort == nullptr)
      throw fdb::Error(FDB_ERR_INVALID, "merge schema: bad arguments");
    std::vector<fdb::MergeOrder> exprs;
    for (int32_t k = 0; k < n_order; k++) {
      if (order[k].name == nullptr) throw fdb::Error(FDB_ERR_INVALID, "merge schema: order expression " + std::to_string(k) + " has no name");
      exprs.push_back(fdb::MergeOrder{order[k].name, order[k].dynamic != 0});
    }
    std::vector<std::vector<fdb::MergeField>> lists((size_t)n_records);
    std::vector<int32_t> base((size_t)n_records, 0);
    int32_t flat = 0;
    for (int32_t r = 0; r < n_records; r++) {
      if (n_fields[r] < 0 || (n_fields[r] > 0 && (names == nullptr || kinds == nullptr))) throw fdb::Error(FDB_ERR_INVALID, "merge schema: bad field list");
      base[(size_t)r] = flat;
      for (int32_t f = 0; f < n_fields[r]; f++, flat++) {
        if (names[flat] == nullptr) throw fdb::Error(FDB_ERR_INVALID, "merge schema: field without a name");
        lists[(size_t)r].push_back(fdb::MergeField{names[flat], kinds[flat]});
      }
    }
    const fdb::MergeSchema u = fdb::unify_merge_schema(lists, exprs);
    *n_out = (int32_t)u.first.size();
    *n_sort = (int32_t)u.sort_expr.size();
    if (*n_out > cap) throw fdb::Error(FDB_ERR_INVALID, "merge schema: " + std::to_string(*n_out) + " output columns, room for " + std::to_string(cap));
    if (*n_out > 0 && (out_fields == nullptr || (n_records > 0 && col_map == nullptr))) throw fdb::Error(FDB_ERR_INVALID, "merge schema: null output");
    for (int32_t i = 0; i < *n_out; i++) {
      out_fields[i] = base[(size_t)u.first[(size_t)i].record] + u.first[(size_t)i].field;
      for (int32_t r = 0; r < n_records; r++) col_map[(size_t)r * (size_t)*n_out + (size_t)i] = u.map[(size_t)r][(size_t)i];
    }
  });
}

int fdb_osync_create(int32_t inputs, const fdb_order_col* order, int32_t n_order, fdb_osync** out) {
  return guard(nullptr, [&] {
    if (out == nullptr) throw fdb::Error(FDB_ERR_INVALID, "null argument");
    *out = nullptr;
    *out = new fdb_osync(inputs, order, n_order);
  });
}

int fdb_osync_push(fdb_osync* s, int32_t input, const fdb_batch* batch, fdb_batch** merged) {
  return guard(nullptr, [&] {
    if (s == nullptr || batch == nullptr || !batch->b || merged == nullptr) throw fdb::Error(FDB_ERR_INVALID, "null argument");
    *merged = nullptr;
    std::unique_ptr<fdb::DeviceBatch> r = s->s.push(input, batch->b.get());
    if (r) *merged = new fdb_batch{std::move(r)};
  });
}

int fdb_osync_finish(fdb_osync* s, int32_t input, fdb_batch** merged, int32_t* done) {
  return guard(nullptr, [&] {
    if (s == nullptr || merged == nullptr) throw fdb::Error(FDB_ERR_INVALID, "null argument");
    *merged = nullptr;
    bool last = false;
    std::unique_ptr<fdb::DeviceBatch> r = s->s.finish(input, &last);
    if (done != nullptr) *done = last ? 1 : 0;
    if (r) *merged = new fdb_batch{std::move(r)};
  });
}

void fdb_osync_close(fdb_osync* s) { delete s; }

int32_t fdb_merge_tile_rows(int32_t words) { return words < 0 ? 0 : (int32_t)fdb_merge_tile(words); }

int fdb_selftest_merge_path(const uint64_t* a, int64_t na, const uint64_t* b, int64_t nb, int32_t words, uint32_t* src_out) {
  return guard(nullptr, [&] {
    if (na < 0 || nb < 0 || words < 1 || words > 64 || na + nb > 0x7FFFFFFFll || (na > 0 && a == nullptr) || (nb > 0 && b == nullptr) || (na + nb > 0 && src_out == nullptr))
      throw fdb::Error(FDB_ERR_INVALID, "merge path: bad arguments");
    const int64_t bad = fdb_merge_path_host(a, na, b, nb, words, src_out);
    if (bad != 0) throw fdb::Error(FDB_ERR_INVALID, "merge path: the split points of tile " + std::to_string(bad - 1) + " cross (are both runs sorted?)");
  });
}

int fdb_merge_bench(const fdb_batch* const* in, int32_t n, const fdb_sort_col* cols, int32_t n_cols, int32_t reps, int32_t warmup, double* merge_ms, double* gather_ms,
                    double* round_ms, int32_t round_cap, int32_t* n_rounds, int32_t* words) {
  return guard(nullptr, [&] {
    const std::vector<const fdb::DeviceBatch*> recs = merge_inputs(in, n);
    fdb::merge_bench(recs.data(), n, cols, n_cols, reps, warmup, merge_ms, gather_ms, round_ms, round_cap, n_rounds, words);
  });
}

const char* fdb_batch_column_name(const fdb_batch* batch, int32_t index) {
  if (batch == nullptr || !batch->b || index < 0 || (size_t)index >= batch->b->cols.size()) return nullptr;
  return batch->b->cols[(size_t)index].name.c_str();
}

const char* fdb_batch_column_format(const fdb_batch* batch, int32_t index) {
  if (batch == nullptr || !batch->b || index < 0 || (size_t)index >= batch->b->cols.size()) return nullptr;
  return batch->b->cols[(size_t)index].format.c_str();
}

int fdb_sampler_create(int64_t size, uint64_t seed, int device, fdb_sampler** out) {
  return guard(nullptr, [&] {
    if (out == nullptr) throw fdb::Error(FDB_ERR_INVALID, "null argument");
    *out = nullptr;
    *out = new fdb_sampler(size, seed, device);
  });
}

int fdb_sampler_push_batch(fdb_sampler* sampler, const fdb_batch* batch) {
  return guard(nullptr, [&] {
    if (sampler == nullptr || batch == nullptr || !batch->b) throw fdb::Error(FDB_ERR_INVALID, "null argument");
    sampler->s.push_batch(*batch->b);
  });
}

int fdb_sampler_push(fdb_sampler* sampler, struct ArrowArray* batch, struct ArrowSchema* schema) {
  return guard(nullptr, [&] {
    if (sampler == nullptr || batch == nullptr || schema == nullptr) throw fdb::Error(FDB_ERR_INVALID, "null argument");
    sampler->s.push(batch, schema);
  });
}

int fdb_sampler_finish_batch(fdb_sampler* sampler, fdb_batch** out, int64_t* n_rows) {
  return guard(nullptr, [&] {
    if (sampler == nullptr || out == nullptr) throw fdb::Error(FDB_ERR_INVALID, "null argument");
    *out = nullptr;
    std::unique_ptr<fdb::DeviceBatch> r = sampler->s.finish_batch(n_rows);
    *out = new fdb_batch{std::move(r)};
  });
}

int fdb_sampler_finish(fdb_sampler* sampler, struct ArrowArray* out, struct ArrowSchema* out_schema, int64_t* n_rows) {
  return guard(nullptr, [&] {
    if (sampler == nullptr || out == nullptr || out_schema == nullptr) throw fdb::Error(FDB_ERR_INVALID, "null argument");
    sampler->s.finish(out, out_schema, n_rows);
  });
}

void fdb_sampler_close(fdb_sampler* sampler) { delete sampler; }

int fdb_selftest_reservoir(uint64_t seed, int64_t size, const int64_t* record_rows, int32_t n_records, int64_t* rows_out) {
  return guard(nullptr, [&] {
    if (size < 0 || n_records < 0 || (n_records > 0 && record_rows == nullptr)) throw fdb::Error(FDB_ERR_INVALID, "bad arguments");
    fdb::ReservoirSelect sel(size, seed);
    int64_t base = 0;
    for (int32_t r = 0; r < n_records; r++) {
      if (record_rows[r] < 0) throw fdb::Error(FDB_ERR_INVALID, "negative row count");
      if (rows_out == nullptr && record_rows[r] > 0 && size > 0) throw fdb::Error(FDB_ERR_INVALID, "null output");
      sel.push(record_rows[r], [&](int64_t row, int64_t slot) { rows_out[slot] = base + row; });
      base += record_rows[r];
    }
  });
}

const char* fdb_plan_draw(fdb_plan* plan) { return !plan ? "" : plan->dyn ? plan->dyn->draw(plan->plan) : plan->plan.draw(); }
const char* fdb_plan_last_error(const fdb_plan* plan) { return plan ? plan->plan.error.c_str() : g_last_error.c_str(); }
void fdb_plan_close(fdb_plan* plan) { delete plan; }

int fdb_plan_num_groups(fdb_plan* plan, int64_t* n_groups) {
  if (!plan) return FDB_ERR_INVALID;
  return guard(plan, [&] {
    if (plan->dyn) { *n_groups = plan->dyn->num_groups(plan->plan); return; }
    plan->plan.settle();
    *n_groups = plan->plan.num_groups();
  });
}

int fdb_plan_partial_keys(fdb_plan* plan, struct ArrowArray* out, struct ArrowSchema* out_schema) {
  if (!plan) return FDB_ERR_INVALID;
  return guard(plan, [&] { single_table_only(plan); plan->plan.settle(); plan->plan.partial_keys(out, out_schema); });
}

int fdb_plan_partial_state(fdb_plan* plan, int32_t agg, void* dst, int64_t capacity_bytes) {
  if (!plan) return FDB_ERR_INVALID;
  return guard(plan, [&] { single_table_only(plan); plan->plan.settle(); plan->plan.partial_state(agg, dst, capacity_bytes); });
}

int fdb_plan_state_signature(fdb_plan* plan, uint64_t* signature, int64_t* n_slots) {
  if (!plan) return FDB_ERR_INVALID;
  return guard(plan, [&] { single_table_only(plan); plan->plan.refuse_exact("fdb_plan_state_signature"); plan->plan.settle(); *signature = plan->plan.state_signature(n_slots); });
}

int fdb_plan_state_pointers(fdb_plan* plan, void** base, int64_t* array_stride, int64_t* n_slots) {
  if (!plan) return FDB_ERR_INVALID;
  return guard(plan, [&] { single_table_only(plan); plan->plan.refuse_exact("fdb_plan_state_pointers"); plan->plan.settle(); plan->plan.state_pointers(base, array_stride, n_slots); });
}

int fdb_plan_state_read(fdb_plan* plan, int32_t array, void* dst, int64_t capacity_bytes) {
  if (!plan) return FDB_ERR_INVALID;
  return guard(plan, [&] { single_table_only(plan); plan->plan.refuse_exact("fdb_plan_state_read"); plan->plan.settle(); plan->plan.state_read(array, dst, capacity_bytes); });
}

int fdb_plan_state_write(fdb_plan* plan, int32_t array, const void* src, int64_t bytes) {
  if (!plan) return FDB_ERR_INVALID;
  return guard(plan, [&] { single_table_only(plan); plan->plan.refuse_exact("fdb_plan_state_write"); plan->plan.settle(); plan->plan.state_write(array, src, bytes); });
}

int fdb_plan_state_arrays(fdb_plan* plan, int32_t* n_arrays) {
  if (!plan || !n_arrays) return FDB_ERR_INVALID;
  return guard(plan, [&] { single_table_only(plan); plan->plan.refuse_exact("fdb_plan_state_arrays"); *n_arrays = plan->plan.num_state_arrays(); });
}

int fdb_plan_state_array_op(fdb_plan* plan, int32_t array, int32_t* op) {
  if (!plan || !op) return FDB_ERR_INVALID;
  return guard(plan, [&] { single_table_only(plan); plan->plan.refuse_exact("fdb_plan_state_array_op"); plan->plan.settle(); *op = plan->plan.state_array_op(array); });
}

int fdb_plan_agg_type(fdb_plan* plan, int32_t agg, char* format_out) {
  if (!plan) return FDB_ERR_INVALID;
  return guard(plan, [&] { single_table_only(plan); plan->plan.settle(); *format_out = plan->plan.agg_format(agg); });
}

int fdb_batch_import(struct ArrowArray* batch, struct ArrowSchema* schema, int device, fdb_batch** out) {
  return guard(nullptr, [&] {
    fdb::HostRecordView view;
    fdb::view_record(batch, schema, &view);
    std::unique_ptr<fdb_batch> b(new fdb_batch());
    b->b = fdb::import_batch(view, device, nullptr, nullptr);
    *out = b.release();
  });
}

int fdb_batch_from_parquet(const fdb_parquet_chunk* chunks, int32_t n_chunks, int64_t n_rows, int device, fdb_batch** out) {
  return guard(nullptr, [&] {
    if (out == nullptr) throw fdb::Error(FDB_ERR_INVALID, "null output");
    *out = nullptr;
    std::unique_ptr<fdb_batch> b(new fdb_batch());
    b->b = fdb::batch_from_parquet(chunks, n_chunks, n_rows, device);
    *out = b.release();
  });
}

// The Parquet writer's entry points (fdb_batch_to_parquet* and fdb_selftest_parquet_write*): each fills as much of a PqwSpec as it has arguments for and goes through one of these two.
static int write_resident(const fdb_batch* batch, const fdb::PqwSpec& spec, uint8_t** bytes, int64_t* n_bytes) {
  return guard(nullptr, [&] {
    if (batch == nullptr || !batch->b || bytes == nullptr || n_bytes == nullptr) throw fdb::Error(FDB_ERR_INVALID, "null argument");
    *bytes = nullptr; *n_bytes = 0;
    fdb::batch_to_parquet(*batch->b, spec, bytes, n_bytes);
  });
}

static int write_selftest(struct ArrowArray* batch, struct ArrowSchema* schema, const fdb::PqwSpec& spec, uint8_t** bytes, int64_t* n_bytes) {
  return guard(nullptr, [&] {
    if (batch == nullptr || schema == nullptr || bytes == nullptr || n_bytes == nullptr) throw fdb::Error(FDB_ERR_INVALID, "null argument");
    *bytes = nullptr; *n_bytes = 0;
    fdb::HostRecordView view;
    fdb::view_record(batch, schema, &view);
    fdb::selftest_parquet_write(view, spec, bytes, n_bytes);
  });
}

int fdb_batch_to_parquet(const fdb_batch* batch, const fdb_parquet_write_options* options, uint8_t** bytes, int64_t* n_bytes) {
  return write_resident(batch, fdb::PqwSpec{options}, bytes, n_bytes);
}

int fdb_batch_to_parquet_encoded(const fdb_batch* batch, const fdb_parquet_write_options* options, const int8_t* encodings, int32_t n_encodings, uint8_t** bytes, int64_t* n_bytes) {
  return write_resident(batch, fdb::PqwSpec{options, encodings, n_encodings}, bytes, n_bytes);
}

void fdb_bytes_free(uint8_t* bytes) { fdb::pqw_free_bytes(bytes); }

int fdb_selftest_parquet_write(struct ArrowArray* batch, struct ArrowSchema* schema, const fdb_parquet_write_options* options, uint8_t** bytes, int64_t* n_bytes) {
  return write_selftest(batch, schema, fdb::PqwSpec{options}, bytes, n_bytes);
}

int fdb_selftest_parquet_write_encoded(struct ArrowArray* batch, struct ArrowSchema* schema, const fdb_parquet_write_options* options, const int8_t* encodings, int32_t n_encodings,
                                       uint8_t** bytes, int64_t* n_bytes) {
  return write_selftest(batch, schema, fdb::PqwSpec{options, encodings, n_encodings}, bytes, n_bytes);
}

int fdb_batch_to_parquet_compressed(const fdb_batch* batch, const fdb_parquet_write_options* options, const int8_t* encodings, int32_t n_encodings, const int8_t* codecs, int32_t n_codecs,
                                    uint8_t** bytes, int64_t* n_bytes) {
  return write_resident(batch, fdb::PqwSpec{options, encodings, n_encodings, codecs, n_codecs}, bytes, n_bytes);
}

int fdb_selftest_parquet_write_compressed(struct ArrowArray* batch, struct ArrowSchema* schema, const fdb_parquet_write_options* options, const int8_t* encodings, int32_t n_encodings,
                                          const int8_t* codecs, int32_t n_codecs, uint8_t** bytes, int64_t* n_bytes) {
  return write_selftest(batch, schema, fdb::PqwSpec{options, encodings, n_encodings, codecs, n_codecs}, bytes, n_bytes);
}

int fdb_batch_to_parquet_indexed(const fdb_batch* batch, const fdb_parquet_write_options* options, const int8_t* encodings, int32_t n_encodings, const int8_t* codecs, int32_t n_codecs,
                                 const fdb_parquet_index_options* index, uint8_t** bytes, int64_t* n_bytes) {
  return write_resident(batch, fdb::PqwSpec{options, encodings, n_encodings, codecs, n_codecs, index}, bytes, n_bytes);
}

int fdb_selftest_parquet_write_indexed(struct ArrowArray* batch, struct ArrowSchema* schema, const fdb_parquet_write_options* options, const int8_t* encodings, int32_t n_encodings,
                                       const int8_t* codecs, int32_t n_codecs, const fdb_parquet_index_options* index, uint8_t** bytes, int64_t* n_bytes) {
  return write_selftest(batch, schema, fdb::PqwSpec{options, encodings, n_encodings, codecs, n_codecs, index}, bytes, n_bytes);
}

int fdb_batch_to_parquet_filtered(const fdb_batch* batch, const fdb_parquet_write_options* options, const int8_t* encodings, int32_t n_encodings, const int8_t* codecs, int32_t n_codecs,
                                  const fdb_parquet_index_options* index, const fdb_parquet_bloom_options* bloom, uint8_t** bytes, int64_t* n_bytes) {
  return write_resident(batch, fdb::PqwSpec{options, encodings, n_encodings, codecs, n_codecs, index, bloom}, bytes, n_bytes);
}

int fdb_selftest_parquet_write_filtered(struct ArrowArray* batch, struct ArrowSchema* schema, const fdb_parquet_write_options* options, const int8_t* encodings, int32_t n_encodings,
                                        const int8_t* codecs, int32_t n_codecs, const fdb_parquet_index_options* index, const fdb_parquet_bloom_options* bloom, uint8_t** bytes,
                                        int64_t* n_bytes) {
  return write_selftest(batch, schema, fdb::PqwSpec{options, encodings, n_encodings, codecs, n_codecs, index, bloom}, bytes, n_bytes);
}

int fdb_batch_to_parquet_runs(const fdb_batch* batch, const fdb_parquet_write_options* options, const int8_t* encodings, int32_t n_encodings, const int8_t* codecs, int32_t n_codecs,
                              const fdb_parquet_index_options* index, const fdb_parquet_bloom_options* bloom, const fdb_parquet_run_options* runs, uint8_t** bytes, int64_t* n_bytes) {
  return write_resident(batch, fdb::PqwSpec{options, encodings, n_encodings, codecs, n_codecs, index, bloom, runs}, bytes, n_bytes);
}

int fdb_selftest_parquet_write_runs(struct ArrowArray* batch, struct ArrowSchema* schema, const fdb_parquet_write_options* options, const int8_t* encodings, int32_t n_encodings,
                                    const int8_t* codecs, int32_t n_codecs, const fdb_parquet_index_options* index, const fdb_parquet_bloom_options* bloom,
                                    const fdb_parquet_run_options* runs, uint8_t** bytes, int64_t* n_bytes) {
  return write_selftest(batch, schema, fdb::PqwSpec{options, encodings, n_encodings, codecs, n_codecs, index, bloom, runs}, bytes, n_bytes);
}

int fdb_batch_to_parquet_grouped(const fdb_batch* batch, const fdb_parquet_write_options* options, const int8_t* encodings, int32_t n_encodings, const int8_t* codecs, int32_t n_codecs,
                                 const fdb_parquet_index_options* index, const fdb_parquet_bloom_options* bloom, const fdb_parquet_run_options* runs,
                                 const fdb_parquet_group_options* groups, uint8_t** bytes, int64_t* n_bytes) {
  return write_resident(batch, fdb::PqwSpec{options, encodings, n_encodings, codecs, n_codecs, index, bloom, runs, groups}, bytes, n_bytes);
}

int fdb_selftest_parquet_write_grouped(struct ArrowArray* batch, struct ArrowSchema* schema, const fdb_parquet_write_options* options, const int8_t* encodings, int32_t n_encodings,
                                       const int8_t* codecs, int32_t n_codecs, const fdb_parquet_index_options* index, const fdb_parquet_bloom_options* bloom,
                                       const fdb_parquet_run_options* runs, const fdb_parquet_group_options* groups, uint8_t** bytes, int64_t* n_bytes) {
  return write_selftest(batch, schema, fdb::PqwSpec{options, encodings, n_encodings, codecs, n_codecs, index, bloom, runs, groups}, bytes, n_bytes);
}

int fdb_batch_to_parquet_strings(const fdb_batch* batch, const fdb_parquet_write_options* options, const int8_t* encodings, int32_t n_encodings, const int8_t* codecs, int32_t n_codecs,
                                 const fdb_parquet_index_options* index, const fdb_parquet_bloom_options* bloom, const fdb_parquet_run_options* runs,
                                 const fdb_parquet_group_options* groups, const fdb_parquet_string_options* strings, uint8_t** bytes, int64_t* n_bytes) {
  return write_resident(batch, fdb::PqwSpec{options, encodings, n_encodings, codecs, n_codecs, index, bloom, runs, groups, strings}, bytes, n_bytes);
}

int fdb_selftest_parquet_write_strings(struct ArrowArray* batch, struct ArrowSchema* schema, const fdb_parquet_write_options* options, const int8_t* encodings, int32_t n_encodings,
                                       const int8_t* codecs, int32_t n_codecs, const fdb_parquet_index_options* index, const fdb_parquet_bloom_options* bloom,
                                       const fdb_parquet_run_options* runs, const fdb_parquet_group_options* groups, const fdb_parquet_string_options* strings, uint8_t** bytes,
                                       int64_t* n_bytes) {
  return write_selftest(batch, schema, fdb::PqwSpec{options, encodings, n_encodings, codecs, n_codecs, index, bloom, runs, groups, strings}, bytes, n_bytes);
}

int fdb_batches_from_parquet(const fdb_parquet_row_group* groups, int32_t n_groups, int device, fdb_batch** out) {
  return guard(nullptr, [&] {
    if (out == nullptr || n_groups <= 0) throw fdb::Error(FDB_ERR_INVALID, "null output");
    for (int32_t g = 0; g < n_groups; g++) out[g] = nullptr;
    std::vector<std::unique_ptr<fdb::DeviceBatch>> bs = fdb::batches_from_parquet(groups, n_groups, device);
    std::vector<std::unique_ptr<fdb_batch>> hs;
    for (auto& b : bs) { hs.emplace_back(new fdb_batch()); hs.back()->b = std::move(b); }
    for (int32_t g = 0; g < n_groups; g++) out[g] = hs[(size_t)g].release();
  });
}

// fdb_snappy_decode_pages / fdb_lz4_decode_pages: `codec` is parquet.thrift's number, `what` the prefix of the error texts
static int decode_pages(int codec, const char* what, const uint8_t* src, int64_t src_bytes, const FdbCodecPage* pages, int32_t n_pages, uint8_t* dst, int64_t dst_bytes,
                        int device, uint32_t* status, double* kernel_ms) {
  return guard(nullptr, [&] {
    if (n_pages < 0 || src_bytes < 0 || dst_bytes < 0 || (n_pages > 0 && (pages == nullptr || status == nullptr))) throw fdb::Error(FDB_ERR_INVALID, std::string(what) + ": bad arguments");
    const int32_t outside = fdb::check_page_table(pages, n_pages, src_bytes, dst_bytes);
    if (outside >= 0) throw fdb::Error(FDB_ERR_INVALID, std::string(what) + ": page " + std::to_string(outside) + " lies outside the buffers");
    if (kernel_ms) *kernel_ms = 0.0;
    if (n_pages == 0) return;
    if (device < 0) { fdb::decode_pages_host(codec, src, pages, n_pages, dst, status); return; }  // the host decoder over the same table: no GPU is touched (the kernel's status codes; never 6)
    fdb::hip_check(hipSetDevice(device), "hipSetDevice");
    struct Dev { void* p = nullptr; ~Dev() { if (p) (void)hipFree(p); } } d_src, d_dst, d_pages, d_status;
    struct Ev { hipEvent_t e = nullptr; ~Ev() { if (e) (void)hipEventDestroy(e); } } e0, e1;
    const size_t pad = 64;  // (the kernel's 16-byte moves never start past a page's last byte, but may end up to 15 bytes behind it)
    fdb::hip_check(hipMalloc(&d_src.p, (size_t)src_bytes + pad), "hipMalloc");
    fdb::hip_check(hipMalloc(&d_dst.p, (size_t)dst_bytes + pad), "hipMalloc");
    fdb::hip_check(hipMalloc(&d_pages.p, (size_t)n_pages * sizeof(FdbCodecPage)), "hipMalloc");
    fdb::hip_check(hipMalloc(&d_status.p, (size_t)n_pages * 4), "hipMalloc");
    fdb::hip_check(hipMemcpy(d_src.p, src, (size_t)src_bytes, hipMemcpyHostToDevice), "hipMemcpy");
    fdb::hip_check(hipMemcpy(d_pages.p, pages, (size_t)n_pages * sizeof(FdbCodecPage), hipMemcpyHostToDevice), "hipMemcpy");
    fdb::hip_check(hipEventCreate(&e0.e), "hipEventCreate");
    fdb::hip_check(hipEventCreate(&e1.e), "hipEventCreate");
    fdb::hip_check(hipEventRecord(e0.e, nullptr), "hipEventRecord");
    fdb::hip_check(fdb_launch_page_decode(codec, (const uint8_t*)d_src.p, (const FdbCodecPage*)d_pages.p, n_pages, (uint8_t*)d_dst.p, (uint32_t*)d_status.p, nullptr), (std::string(what) + " launch").c_str());
    fdb::hip_check(hipEventRecord(e1.e, nullptr), "hipEventRecord");
    fdb::hip_check(hipDeviceSynchronize(), "hipDeviceSynchronize");
    float ms = 0.f;
    fdb::hip_check(hipEventElapsedTime(&ms, e0.e, e1.e), "hipEventElapsedTime");
    if (kernel_ms) *kernel_ms = (double)ms;
    fdb::hip_check(hipMemcpy(status, d_status.p, (size_t)n_pages * 4, hipMemcpyDeviceToHost), "hipMemcpy");
    if (dst_bytes > 0) fdb::hip_check(hipMemcpy(dst, d_dst.p, (size_t)dst_bytes, hipMemcpyDeviceToHost), "hipMemcpy");
  });
}
static_assert(sizeof(fdb_snappy_page) == sizeof(FdbCodecPage), "fdb_snappy_page (and fdb_lz4_page, the same type) mirrors FdbCodecPage");

int fdb_snappy_decode_pages(const uint8_t* src, int64_t src_bytes, const fdb_snappy_page* pages, int32_t n_pages, uint8_t* dst, int64_t dst_bytes,
                            int device, uint32_t* status, double* kernel_ms) {
  return decode_pages(FDB_CODEC_SNAPPY, "snappy", src, src_bytes, reinterpret_cast<const FdbCodecPage*>(pages), n_pages, dst, dst_bytes, device, status, kernel_ms);
}

int fdb_lz4_decode_pages(const uint8_t* src, int64_t src_bytes, const fdb_lz4_page* pages, int32_t n_pages, uint8_t* dst, int64_t dst_bytes,
                         int device, uint32_t* status, double* kernel_ms) {
  return decode_pages(FDB_CODEC_LZ4_RAW, "lz4", src, src_bytes, reinterpret_cast<const FdbCodecPage*>(pages), n_pages, dst, dst_bytes, device, status, kernel_ms);
}

int64_t fdb_batch_num_rows(const fdb_batch* batch) { return batch ? batch->b->rows : 0; }
int64_t fdb_batch_device_bytes(const fdb_batch* batch) { return batch ? (int64_t)batch->b->arena_bytes : 0; }
int64_t fdb_batch_scan_cache_bytes(const fdb_batch* batch) { return batch ? batch->b->scan_cache_bytes() : 0; }
void fdb_batch_release(fdb_batch* batch) { delete batch; }

int fdb_plan_stats(fdb_plan* plan, int64_t* algorithmic_bytes, double* kernel_ms, int64_t* n_launches, int64_t* rows_scanned) {
  if (!plan) return FDB_ERR_INVALID;
  return guard(plan, [&] {
    plan->plan.settle();  // queued small records count once they are scanned
    if (plan->plan.timing) plan->plan.sync();  // (event pairs are read once their kernels have run: a rank whose merge emitted no record has not waited yet)
    if (algorithmic_bytes) *algorithmic_bytes = plan->plan.stat_bytes;
    if (kernel_ms) *kernel_ms = plan->plan.stat_ms;
    if (n_launches) *n_launches = plan->plan.stat_launches;
    if (rows_scanned) *rows_scanned = plan->plan.stat_rows;
  });
}

int fdb_regex_match(const char* pattern, int64_t pattern_len, const uint8_t* value, int64_t value_len, int32_t* matched) {
  return guard(nullptr, [&] {
    if (pattern == nullptr || pattern_len < 0 || value_len < 0 || (value == nullptr && value_len > 0) || matched == nullptr) throw fdb::Error(FDB_ERR_INVALID, "null argument");
    std::string why;
    std::shared_ptr<const fdb::Regex> re = fdb::Regex::compile(std::string(pattern, (size_t)pattern_len), &why);
    if (!re) throw fdb::Error(FDB_ERR_INVALID, why);
    *matched = re->match((const char*)value, (size_t)value_len) ? 1 : 0;
  });
}

int fdb_parquet_stats(int64_t* calls, double* host_ms, double* device_ms, int64_t* file_bytes, int64_t* out_bytes) {
  return guard(nullptr, [&] { fdb::parquet_stats(calls, host_ms, device_ms, file_bytes, out_bytes); });
}

int fdb_parquet_device_pages(int codec, int64_t* pages, int64_t* bytes) {
  return guard(nullptr, [&] { fdb::parquet_device_pages(codec, pages, bytes); });
}

int fdb_jit_stats(int64_t* n_compiled, double* compile_ms, int64_t* n_disk_loads) {
  return guard(nullptr, [&] { fdb::jit_stats(n_compiled, compile_ms, n_disk_loads); });
}

int fdb_plan_merge_ms(fdb_plan* plan, double* merge_ms) {
  if (!plan || !merge_ms) return FDB_ERR_INVALID;
  return guard(plan, [&] { if (plan->plan.timing) plan->plan.sync(); *merge_ms = plan->plan.stat_merge_ms; });
}

int fdb_plan_set_timing(fdb_plan* plan, int32_t enabled) {
  if (!plan) return FDB_ERR_INVALID;
  plan->plan.timing = enabled != 0;
  return FDB_OK;
}

int fdb_plan_stream(fdb_plan* plan, void** stream_out) {
  if (!plan) return FDB_ERR_INVALID;
  *stream_out = (void*)plan->plan.stream();
  return FDB_OK;
}

// Tuning knobs used by bench.py's variant sweeps (not part of the Go binding).
int fdb_plan_set_tuning(fdb_plan* plan, int32_t rows_per_thread, int32_t grid_blocks) {
  if (!plan) return FDB_ERR_INVALID;
  if (rows_per_thread == 0 || rows_per_thread == 4 || rows_per_thread == 8) plan->plan.rows_per_thread = rows_per_thread;
  plan->plan.grid_override = grid_blocks & 0xFFFFF;  // (bits 20-23 are reserved)
  plan->plan.use_partials = ((grid_blocks >> 24) & 1) == 0;
  plan->plan.sub_tiles = (grid_blocks >> 25) & 7;
  return FDB_OK;
}

int fdb_plan_set_deterministic(fdb_plan* plan, int32_t enabled) {
  if (!plan) return FDB_ERR_INVALID;
  plan->plan.deterministic = enabled != 0;
  return FDB_OK;
}

int fdb_plan_set_exact_sums(fdb_plan* plan, int32_t enabled) {
  if (!plan) return FDB_ERR_INVALID;
  return guard(plan, [&] {
    if (plan->plan.started() || (plan->dyn && plan->dyn->started()))
      throw fdb::Error(FDB_ERR_STATE, "exact sums can only be switched before the plan's first push, merge or seed");
    plan->plan.set_exact_sums(enabled != 0);
    if (plan->dyn) plan->dyn->exact = enabled != 0;  // (every member plan, made on first sight of its column, inherits it)
  });
}

const char* fdb_plan_last_kernel(fdb_plan* plan) {
  if (!plan) return "";
  (void)guard(plan, [&] { plan->plan.settle(); });
  return plan->plan.last_kernel();
}

// ---- cross-GPU merge ---------------------------------------------------------------------------------------------------------

int fdb_comm_unique_id(uint8_t id[FDB_COMM_ID_BYTES]) {
  return comm_guard(nullptr, [&] {
    if (id == nullptr) throw fdb::Error(FDB_ERR_INVALID, "null id");
    fdb::rccl_unique_id(id);
  });
}

int fdb_comm_init_rank(const uint8_t id[FDB_COMM_ID_BYTES], int32_t n_ranks, int32_t rank, int device, fdb_comm** out) {
  return comm_guard(nullptr, [&] {
    if (id == nullptr || out == nullptr) throw fdb::Error(FDB_ERR_INVALID, "null argument");
    *out = nullptr;
    std::unique_ptr<fdb::Comm> c = fdb::rccl_init_rank(id, n_ranks, rank, device);
    *out = new fdb_comm();
    (*out)->c = std::move(c);
  });
}

int fdb_comm_init_all(const int* devices, int32_t n, fdb_comm** out) {
  return comm_guard(nullptr, [&] {
    if (devices == nullptr || out == nullptr) throw fdb::Error(FDB_ERR_INVALID, "null argument");
    for (int32_t i = 0; i < n && i < FDB_MAX_PARTS; i++) out[i] = nullptr;  // (nothing dangling if creation fails)
    wrap_all(fdb::rccl_init_all(devices, n), out);
  });
}

int fdb_comm_init_local(const int* devices, int32_t n, fdb_comm** out) {
  return comm_guard(nullptr, [&] {
    if (devices == nullptr || out == nullptr) throw fdb::Error(FDB_ERR_INVALID, "null argument");
    for (int32_t i = 0; i < n && i < FDB_MAX_PARTS; i++) out[i] = nullptr;  // (nothing dangling if creation fails)
    wrap_all(fdb::local_init(devices, n), out);
  });
}

int32_t fdb_comm_rank(const fdb_comm* comm) { return comm && comm->c ? comm->c->rank : -1; }
int32_t fdb_comm_size(const fdb_comm* comm) { return comm && comm->c ? comm->c->size : 0; }
int32_t fdb_comm_transport_ranks(fdb_comm* comm) {
  if (comm == nullptr || !comm->c) return -1;
  try { return comm->c->transport_ranks(); } catch (...) { return -1; }
}
const char* fdb_comm_last_error(const fdb_comm* comm) { return comm && comm->c ? comm->c->error.c_str() : g_last_error.c_str(); }
void fdb_comm_destroy(fdb_comm* comm) { delete comm; }

int fdb_plan_allreduce(fdb_plan* plan, fdb_comm* comm, int32_t* aligned) {
  if (!plan) return FDB_ERR_INVALID;
  return guard(plan, [&] {
    if (comm == nullptr || !comm->c || aligned == nullptr) throw fdb::Error(FDB_ERR_INVALID, "null argument");
    single_table_only(plan);
    *aligned = plan->plan.comm_allreduce(*comm->c) ? 1 : 0;
  });
}

int fdb_plan_exchange(fdb_plan* plan, fdb_comm* comm, fdb_plan** shard) {
  if (!plan) return FDB_ERR_INVALID;
  return guard(plan, [&] {
    if (comm == nullptr || !comm->c || shard == nullptr) throw fdb::Error(FDB_ERR_INVALID, "null argument");
    single_table_only(plan);
    *shard = nullptr;
    std::unique_ptr<fdb_plan> s(new fdb_plan(plan->plan));
    plan->plan.comm_exchange(*comm->c, s->plan);
    *shard = s.release();
  });
}

int fdb_live_allocations(int64_t* device_blocks, int64_t* device_bytes, int64_t* pinned_blocks) {
  return guard(nullptr, [&] { fdb::live_allocations(device_blocks, device_bytes, pinned_blocks); });
}

}  // extern "C"
