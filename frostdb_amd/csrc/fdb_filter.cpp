// fdb_filter.cpp — selection / filter-only paths of the plan (see fdb_plan.h): filter() and the selection vector of a host record, of a
// record resident in HBM and of every record of a scan at once.
//
// ≙ filter() (filter.go:276-323): the reference turns the predicate's bitmap into index ranges, slices every column per range
// and concatenates the slices. Here ONE kernel pass evaluates the predicate, gives every selected row its output position
// (decoupled look-back over per-tile totals) and writes the compacted columns — see fdb_launch_compact.
#include "fdb_plan.h"
#include "fdb_jit.h"

#include "fdb_context.h"
#include "fdb_plan_internal.h"

#include <algorithm>
#include <cstring>
#include <functional>

namespace fdb {

namespace {
struct DevBuf {  // scratch from the context's caching allocator; the plan's stream orders every reuse
  Context* ctx;
  void* p = nullptr;
  DevBuf(Context* c, size_t bytes) : ctx(c), p(c->dev_alloc(bytes)) {}
  ~DevBuf() { ctx->dev_free(p); }
  DevBuf(const DevBuf&) = delete;
};

// The result record of filtering `in`, without rows yet: every column's name, format, kind and dictionary.
std::unique_ptr<DeviceBatch> filter_output(const DeviceBatch& in) {
  require_values(in, "filter output");
  return RecordBuilder::schema_of(in);
}

// Algorithmic bytes of compacting column `c` to `total` rows: every selected value read once and written once, validity likewise.
int64_t compaction_bytes(const DevColumn& c, int64_t total) {
  return 2 * (total * (int64_t)value_width(c.kind)) + (c.d_validity != nullptr ? 2 * ((total + 7) / 8) : 0);
}
}  // namespace

// Rows of `b` the filter sub-tree rooted at `node` selects (one launch of the interpreting flags kernel + a wait): only used where
// the reference's lazy AND decides whether an error exists at all (emit_filter).
int64_t Plan::count_subtree(const DeviceBatch& b, int node) {
  if (b.rows == 0) return 0;
  hip_check(hipSetDevice(device_), "hipSetDevice");
  slab_ship();  // (a small pushed record may still sit in the pinned slab: its bytes go first)
  Resolved R;
  resolve_filter_only(b, node, &R);
  ctx_->flush_staging();
  b.note_reader(stream_);
  uint8_t* masks = nullptr;
  uint32_t* offs = nullptr;
  return run_flags(R.args, &masks, &offs);
}

void Plan::resolve_filter_only(const DeviceBatch& b, int root, Resolved* R) {
  resolve_predicate(b, root, R);
  unsigned char* d_blob = R->blob.bytes.empty() ? nullptr : (unsigned char*)upload(R->blob.bytes.data(), R->blob.bytes.size());
  R->args.lds_lut_bytes = (uint32_t)place_luts(R->luts, d_blob, 0, &R->args);
}

// Steps 1 + 2 of filter(): selection bitmap and per-tile output offsets on the device (scratch of this plan until its next
// sync()), number of selected rows on the host.
int64_t Plan::run_flags(const FdbScanArgs& a, uint8_t** d_masks, uint32_t** d_offsets) {
  const int64_t n_tiles = (a.n_rows + FDB_COMPACT_TILE - 1) / FDB_COMPACT_TILE;
  uint8_t* masks = (uint8_t*)ctx_->dev_alloc((size_t)n_tiles * (FDB_COMPACT_TILE / 8) + 64);
  uint32_t* offs = (uint32_t*)ctx_->dev_alloc((size_t)(n_tiles + 4 + n_tiles / 1024 + 8) * 4 + 64);  // (+ the scan's per-1024 sums)
  unsigned long long* d_total = (unsigned long long*)ctx_->dev_alloc(64);
  scratch_.push_back(masks); scratch_.push_back(offs); scratch_.push_back(d_total);
  hip_check(hipMemsetAsync(offs, 0, (size_t)(n_tiles + 4) * 4, stream_), "hipMemsetAsync(tile counts)");
  timed([&] {
    hip_check(fdb_launch_filter_flags(a, masks, offs, device_, stream_), "filter flags launch");
    hip_check(fdb_launch_exclusive_scan(offs, n_tiles, offs + n_tiles + 4, d_total, stream_), "tile offsets launch");
  });
  unsigned long long total = 0;
  hip_check(hipMemcpyAsync(&total, d_total, 8, hipMemcpyDeviceToHost, stream_), "hipMemcpyAsync(total)");
  hip_check(hipStreamSynchronize(stream_), "hipStreamSynchronize");
  *d_masks = masks; *d_offsets = offs;
  stat_launches += 1;
  return (int64_t)total;
}

int64_t Plan::select_batch(const DeviceBatch& in, uint32_t* d_indices, int64_t capacity) {
  if (filter_root_ < 0) throw Error(FDB_ERR_STATE, "plan has no filter");
  if (in.device != device_) throw Error(FDB_ERR_INVALID, "batch lives on a different device than the plan");
  if (capacity < in.rows) throw Error(FDB_ERR_INVALID, "indices capacity smaller than the record");
  hip_check(hipSetDevice(device_), "hipSetDevice");
  if (in.rows == 0) return 0;
  Resolved R;
  resolve_filter_only(in, filter_root_, &R);
  uint8_t* masks = nullptr;
  uint32_t* offs = nullptr;
  const int64_t n = run_flags(R.args, &masks, &offs);
  if (n > 0)
    timed([&] { hip_check(fdb_launch_compact_col(0, nullptr, nullptr, d_indices, nullptr, masks, offs, in.rows, nullptr, device_, stream_), "compact launch"); });
  last_kernel_ = "compact_col_kernel";
  sync();
  stat_bytes += R.bytes + n * 4;
  stat_rows += in.rows;
  return n;
}

std::unique_ptr<DeviceBatch> Plan::filter_batch(const DeviceBatch& in, int64_t* n_selected) {
  const DeviceBatch* p = &in;
  std::vector<std::unique_ptr<DeviceBatch>> out = filter_batches(&p, 1, n_selected);  // (falls back to filter_batch_interp by itself)
  return std::move(out[0]);
}

// The per-record path: interpreting flags kernel, one compaction launch per column (what runs when the predicate cannot be
// specialised at run time, and the parity reference of the generated kernels).
// filter_batches_impl has checked the plan and the record.
std::unique_ptr<DeviceBatch> Plan::filter_batch_interp(const DeviceBatch& in, int64_t* n_selected) {
  hip_check(hipSetDevice(device_), "hipSetDevice");
  DrainOnUnwind drain{stream_};  // (`in`, which the caller may release, outlives the queued kernels)
  require_values(in, "filter output");
  *n_selected = 0;
  if (in.rows == 0) return RecordBuilder::schema_of(in);
  Resolved R;
  resolve_filter_only(in, filter_root_, &R);
  uint8_t* masks = nullptr;
  uint32_t* offs = nullptr;
  const int64_t total = run_flags(R.args, &masks, &offs);  // (one host round trip: the output is allocated at its exact size)
  *n_selected = total;
  stat_bytes += R.bytes;
  stat_rows += in.rows;
  RecordBuilder out(device_, total);
  DrainOnUnwind drain_out{stream_};  // (after `out`: its arena outlives the queued kernels)
  for (const DevColumn& c : in.cols) out.add(c.name, c.format, c.kind, c.dict, c.d_validity != nullptr);
  if (total == 0) { sync(); return out.finish(nullptr); }
  out.allocate();
  const size_t n_cols = in.cols.size();
  unsigned long long* d_nulls = (unsigned long long*)ctx_->dev_alloc(128 * 64 * 8);  // 64 partial counts per column
  scratch_.push_back(d_nulls);
  hip_check(hipMemsetAsync(d_nulls, 0, n_cols * 64 * 8, stream_), "hipMemsetAsync(null counts)");
  timed([&] {
    for (size_t k = 0; k < n_cols; k++) {  // one streaming pass per column (fdb_launch_compact_col)
      const DevColumn& c = in.cols[k];
      uint8_t* dst_valid = out.validity(k);
      if (dst_valid != nullptr) hip_check(hipMemsetAsync(dst_valid, 0, out.bitmap_slot_bytes(), stream_), "hipMemsetAsync(validity)");  // the output bitmap is OR-ed into: zero it first
      hip_check(fdb_launch_compact_col((int)value_width(c.kind), c.d_values, c.d_validity, out.values(k), dst_valid, masks, offs, in.rows, d_nulls + k * 64, device_, stream_), "compact launch");
    }
  });
  last_kernel_ = "compact_col_kernel";
  std::vector<unsigned long long> h_parts(n_cols * 64), h_nulls(n_cols, 0);
  hip_check(hipMemcpyAsync(h_parts.data(), d_nulls, n_cols * 64 * 8, hipMemcpyDeviceToHost, stream_), "hipMemcpyAsync(null counts)");
  hip_check(hipStreamSynchronize(stream_), "hipStreamSynchronize");
  for (size_t k = 0; k < n_cols; k++) {
    for (int i = 0; i < 64; i++) h_nulls[k] += h_parts[k * 64 + (size_t)i];
    stat_bytes += compaction_bytes(in.cols[k], total);
  }
  sync();
  return out.finish(h_nulls.data());
}

// ≙ PredicateFilter.Callback for every record of a scan at once (filter.go:255-323). Four launches whatever the number of records
// (five above ≈130 M rows): selection bitmap + per-tile counts by a kernel generated for the predicate (fdb_flags_kernel) →
// prefix sums (sel_scan_kernel) → [host: the records' row counts, outputs allocated at their exact sizes] → zero the output
// bitmaps → every column of every record compacted (compact_multi_kernel). Two host round trips in total. Falls back to the
// per-record path (interpreting flags kernel, one compaction launch per column) when the predicate cannot be specialised.
// The one-pass select kernel's workers and its scanner wait for each other with BOUNDED polls (2^22 of them, ≈ 1–2 s): on a GPU shared
// with long kernels of other processes, or with a queue that is preempted or debugged, a valid filter() can run into the bound. That is
// not the caller's error: the batch is filtered again through the three-launch path (flags → prefix sums → compaction), which waits for
// nothing on the device. ($FDB_TEST_SELECT_STALL: pretends the bound was hit — the test of this road)
std::vector<std::unique_ptr<DeviceBatch>> Plan::filter_batches(const DeviceBatch* const* in, int n, int64_t* n_selected) {
  try {
    return filter_batches_impl(in, n, n_selected, /*force_two_pass=*/false);
  } catch (const SelectStall&) {
    return filter_batches_impl(in, n, n_selected, /*force_two_pass=*/true);
  }
}

// Launch state of one filter_batches_impl call over the records that have rows (`live`). Its members are the steps of the launch
// sequence, called in this order.
struct Plan::FilterRun {
  Plan& P;
  const DeviceBatch* const* in;
  const std::vector<int>& live;
  std::vector<std::unique_ptr<DeviceBatch>>& out;
  const size_t nl, n_cols;
  // a column is compacted as nullable if ANY record of the launch has a bitmap for it (the kernel is specialised per column, not
  // per record); the records that have none read an all-ones bitmap
  std::vector<char> nullable;

  // resolve(): every record's predicate program, LUTs and slots, one argument block per record
  std::vector<Resolved> Rs;
  size_t lut_lds_max = 0;
  JitShape shape;
  int row_bytes = 0;
  std::vector<FdbScanArgs> parts;
  std::vector<FdbCompactRec> recs;
  const FdbScanArgs* d_parts = nullptr;
  const FdbCompactRec* d_recs = nullptr;
  int64_t total_tiles = 0, total_super = 0;

  // choose_kernel(): the generated kernel, and the filter columns the one-pass kernel writes itself
  struct FusedCol { bool wide; int slot; int col; };
  std::vector<FusedCol> fused;
  std::vector<int> fused_of;  // column → index in `fused`, -1
  std::vector<int> rest;      // the columns compact_multi_kernel writes: all of them, minus what the one-pass kernel has written already
  std::vector<int> rest_of;   // column → index in `rest`, -1
  hipFunction_t select_fn = nullptr, flags_fn = nullptr;
  bool one_pass() const { return select_fn != nullptr; }

  // count_rows(): selection bitmap, tile offsets, every record's row count
  uint32_t* d_masks = nullptr;
  uint32_t* d_offsets = nullptr;
  std::vector<int64_t> totals;
  int launches = 0;
  const unsigned long long* d_rec_base_arg = nullptr;  // (one pass: the offsets are relative to their record already)
  std::vector<void*> pre_bits;                         // one pass: the validity bitmaps the select launch zeroed on its way in
  std::vector<size_t> pre_bits_bytes;
  unsigned long long* pre_nulls = nullptr;             // one pass: NULL counters the select launch zeroed
  size_t pre_nulls_words = 0;

  // lay_out(): where every column of every record goes
  struct Placed { void* values = nullptr; uint8_t* valid = nullptr; };
  std::vector<Placed> placed;        // [record][column]
  std::vector<FdbCompactCol> cols;   // [record][rest]
  std::vector<FdbZeroRegion> regions;
  int64_t max_region = 0, any_selected = 0;
  // worst-case blocks whose contents moved into the exact arena (or of records nothing was selected from): back to the pool once the
  // repacking copies have read them — after compact()'s wait, or, when an error unwinds, after a wait of its own
  struct PoolFree {
    int dev; hipStream_t s; std::vector<void*> v; int n = std::uncaught_exceptions();
    ~PoolFree() {
      if (!v.empty() && std::uncaught_exceptions() > n) (void)hipStreamSynchronize(s);
      for (void* p : v) device_pool_free(dev, p);
    }
  } repacked;

  // compact(): NULL counts per record and `rest` column, 64 partial counts each
  std::vector<unsigned long long> h_nulls;

  FilterRun(Plan& plan, const DeviceBatch* const* in_, const std::vector<int>& live_, std::vector<std::unique_ptr<DeviceBatch>>& out_)
      : P(plan), in(in_), live(live_), out(out_), nl(live_.size()), n_cols(in_[live_[0]]->cols.size()), nullable(n_cols, 0), Rs(nl),
        fused_of(n_cols, -1), rest_of(n_cols, -1), totals(nl, 0), pre_bits(nl, nullptr), pre_bits_bytes(nl, 0), placed(nl * n_cols),
        repacked{plan.device_, plan.stream_, {}} {
    for (size_t k = 0; k < nl; k++)
      for (size_t c = 0; c < n_cols; c++) if (in[live[k]]->cols[c].d_validity != nullptr) nullable[c] = 1;
  }
  const DeviceBatch& src(size_t k) const { return *in[live[k]]; }
  DeviceBatch& dst(size_t k) const { return *out[(size_t)live[k]]; }

  bool resolve();
  bool choose_kernel(bool force_two_pass);
  void count_rows();
  void count_rows_one_pass(int64_t grid, size_t first_lds, size_t stage_off, unsigned long long* h_base);
  void count_rows_two_pass(int64_t grid, unsigned long long* h_base);
  void lay_out(int64_t* n_selected);
  void place_record(size_t k, const uint8_t* d_ones);
  void compact();
  void describe();
};

std::vector<std::unique_ptr<DeviceBatch>> Plan::filter_batches_impl(const DeviceBatch* const* in, int n, int64_t* n_selected, bool force_two_pass) {
  if (filter_root_ < 0) throw Error(FDB_ERR_STATE, "plan has no filter");
  std::vector<std::unique_ptr<DeviceBatch>> out;
  auto per_record = [&]() {
    out.clear();
    for (int i = 0; i < n; i++) out.push_back(filter_batch_interp(*in[i], &n_selected[i]));
    return std::move(out);
  };
  std::vector<int> live;
  for (int i = 0; i < n; i++) {
    if (in[i]->device != device_) throw Error(FDB_ERR_INVALID, "batch lives on a different device than the plan");
    if (in[i]->cols.size() > 128) throw Error(FDB_ERR_UNSUPPORTED, "filter output: more than 128 columns");
    if (in[i]->rows > 0) live.push_back(i);
  }
  // one column layout for the whole launch (parts of one table); anything else takes the per-record path
  bool multi = jit_possible() && !live.empty() && !in[live[0]]->cols.empty();
  for (size_t k = 1; k < live.size() && multi; k++) {
    const DeviceBatch& a = *in[live[0]];
    const DeviceBatch& b = *in[live[k]];
    multi = a.cols.size() == b.cols.size();
    for (size_t c = 0; c < a.cols.size() && multi; c++) multi = a.cols[c].kind == b.cols[c].kind && a.cols[c].name == b.cols[c].name;
  }
  if (!multi) return per_record();
  hip_check(hipSetDevice(device_), "hipSetDevice");
  for (int i : live) in[i]->note_reader(stream_);
  for (int i = 0; i < n; i++) {
    out.push_back(filter_output(*in[i]));
    n_selected[i] = 0;
  }
  DrainOnUnwind drain{stream_};  // (declared after `out`: an error waits for the queued kernels before the arenas go back to the pool)
  FilterRun F(*this, in, live, out);
  // (per_record() only once resolve() has returned: the destructor of its StageScope — which ends the deferral and ships what was
  // staged — runs only AFTER a return expression has been evaluated, and the per-record path stages LUTs of its own)
  if (!F.resolve() || !F.choose_kernel(force_two_pass)) return per_record();
  F.count_rows();
  F.lay_out(n_selected);
  F.compact();
  F.describe();
  sync();
  return out;
}

// Every record's predicate: program + LUTs; records with the same LUT set (same_lut_set) share one device copy and one class. false:
// the records cannot share one generated kernel (slots, predicate shapes) — the per-record path takes over.
bool Plan::FilterRun::resolve() {
  LutClasses luts;
  for (size_t k = 0; k < nl; k++) {
    P.resolve_predicate(src(k), P.filter_root_, &Rs[k]);
    luts.add(Rs[k]);
  }
  StageScope stage_scope(P.ctx_);
  unsigned char* d_blob = luts.blob.bytes.empty() ? nullptr : (unsigned char*)P.upload(luts.blob.bytes.data(), luts.blob.bytes.size());
  for (size_t k = 0; k < nl; k++) {
    Resolved& R = Rs[k];
    FdbScanArgs& a = R.args;
    lut_lds_max = std::max(lut_lds_max, luts.place(k, d_blob, R));
    // every filter column in the early pools (the flags kernel has no late phase)
    if (assign_slots(src(k), R, 2, /*relaxed=*/true) == 0) return false;
    if (k == 0) shape = jit_shape(a, true, 512);
    else if (!jit_shape_merge_args(&shape, Rs[0].args, a, true)) return false;  // records of different predicate shapes (schema drift)
    // the flags kernel counts in workgroup shares of four tiles (all of one record), the other kernels in tiles
    const int64_t rec_tiles = (a.n_rows + FDB_COMPACT_TILE - 1) / FDB_COMPACT_TILE;
    a.out_tile_base = total_tiles;
    a.tile_begin = total_super;
    total_super += (rec_tiles + 3) / 4;
    a.tile_end = total_super;
    recs.push_back(FdbCompactRec{total_tiles, a.n_rows});
    total_tiles += rec_tiles;
  }
  for (size_t k = 0; k < nl; k++) { Rs[k].args.lds_lut_bytes = (uint32_t)lut_lds_max; parts.push_back(Rs[k].args); }
  row_bytes = shape.row_bytes();  // (every 4-byte slot at 4: only a dense scan narrows; no late slots)
  d_parts = (const FdbScanArgs*)P.upload(parts.data(), parts.size() * sizeof(FdbScanArgs));
  d_recs = (const FdbCompactRec*)P.upload(recs.data(), recs.size() * sizeof(FdbCompactRec));
  return true;
}

// Which kernel: one pass over the filter columns (fdb_select_kernel), or bitmap → prefix sums → compaction. false: neither can be built.
// One pass: the wave that evaluates a tile also places it (look-back) and writes the compacted values of the filter columns it has
// in registers — columns WITHOUT a validity bitmap in any record, ≤ 8 bytes per row together (their tile is staged in LDS), whose
// slot reads the record's own column (a remapped or widened copy is not the column). Their outputs must exist before the row
// count does: worst-case sized pool blocks (extra_arenas), repacked into the exact arena when less than 40 % of them is used.
bool Plan::FilterRun::choose_kernel(bool force_two_pass) {
  const bool two_pass_env = force_two_pass || std::getenv("FDB_SELECT_TWO_PASS") != nullptr;  // (A/B, tests, fall-back: the three-launch prefix sum; read per call)
  if (!two_pass_env) {
    int budget = 8;
    auto try_slot = [&](bool wide, int slot) {
      const JitSlot& js = wide ? shape.c8[slot] : shape.c4[slot];
      const int w = wide ? 8 : 4;
      if (!js.has_values || js.has_validity != 0 || w > budget || (int)fused.size() >= FDB_SELECT_MAX_FUSED) return;
      int col = -1;
      for (size_t k = 0; k < nl; k++) {
        const DeviceBatch& b = src(k);
        const void* v = wide ? Rs[k].args.c8[slot].values : Rs[k].args.c4[slot].values;
        int found = -1;
        for (size_t c = 0; c < n_cols; c++) if (b.cols[c].d_values == v && v != nullptr) { found = (int)c; break; }
        if (found < 0 || (k > 0 && found != col)) return;
        const DevColumn& dc = b.cols[(size_t)found];
        if (dc.d_validity != nullptr || dc.kind == ColKind::BOOL || (dc.kind == ColKind::DICT) != !wide) return;
        col = found;
      }
      if (col < 0 || fused_of[(size_t)col] >= 0) return;
      fused_of[(size_t)col] = (int)fused.size();
      fused.push_back(FusedCol{wide, slot, col});
      budget -= w;
    };
    for (int i = 0; i < shape.n_c8; i++) try_slot(true, i);
    for (int i = 0; i < shape.n_c4; i++) try_slot(false, i);
    // (the kernel numbers its outputs 8-byte slots first, then 4-byte slots, in slot order — the order they were tried in)
    for (const FusedCol& f : fused) { if (f.wide) shape.fuse8 |= 1 << f.slot; else shape.fuse4 |= 1 << f.slot; }
  }
  // When it pays (MI355X, 100 M rows, 4 columns): `value > x` 0.86 → 0.79 ms of kernels; with a second, unfused filter column the
  // kernel needs 145 registers (one workgroup per CU) and loses what the saved read gains (0.84 → 0.86), cfg 3's three dictionary
  // leaves 0.94 → 1.00. So: every filter column the predicate reads values of is fused, and they are the full 8 bytes per row.
  // ($FDB_SELECT_ONE_PASS: whenever the kernel can be built — tests, A/B)
  bool one_pass_wanted = !two_pass_env;
  if (one_pass_wanted && std::getenv("FDB_SELECT_ONE_PASS") == nullptr) {
    int fused_bytes = 0, value_slots = 0;
    for (const FusedCol& f : fused) fused_bytes += f.wide ? 8 : 4;
    for (int i = 0; i < shape.n_c8; i++) value_slots += shape.c8[i].has_values ? 1 : 0;
    for (int i = 0; i < shape.n_c4; i++) value_slots += shape.c4[i].has_values ? 1 : 0;
    one_pass_wanted = fused_bytes == 8 && value_slots == (int)fused.size();
  }
  if (!one_pass_wanted) { fused.clear(); std::fill(fused_of.begin(), fused_of.end(), -1); shape.fuse4 = shape.fuse8 = 0; }
  select_fn = one_pass_wanted ? jit_select_kernel_get(shape) : nullptr;
  flags_fn = select_fn == nullptr ? jit_flags_get(shape) : nullptr;
  if (select_fn == nullptr) { fused.clear(); std::fill(fused_of.begin(), fused_of.end(), -1); }
  for (size_t c = 0; c < n_cols; c++)
    if (fused_of[c] < 0) { rest_of[c] = (int)rest.size(); rest.push_back((int)c); }
  return select_fn != nullptr || flags_fn != nullptr;
}

// Selection bitmap, tile offsets and every record's row count (the first host round trip).
void Plan::FilterRun::count_rows() {
  d_masks = (uint32_t*)P.ctx_->dev_alloc((size_t)total_tiles * (FDB_COMPACT_TILE / 8) + 256);
  d_offsets = (uint32_t*)P.ctx_->dev_alloc((size_t)total_tiles * 4 + 256);
  P.scratch_.push_back(d_masks); P.scratch_.push_back(d_offsets);
  const size_t stage_off = align_up(lut_lds_max, 16);
  const int first_block = one_pass() ? jit_select_block() : 256;
  const size_t first_lds = one_pass() ? stage_off + (size_t)(first_block / 64) * jit_select_stage_bytes(shape) : lut_lds_max;
  int per_cu = 1;
  {
    // a wave keeps 4 steps × 64 lanes × 4 rows of every filter column in flight: ≈128 KB per CU (twice jit_select's figure: the
    // waves also spend time on words, counts and stores)
    int waves = row_bytes > 0 ? (131072 / (64 * 4 * 4)) / row_bytes : 8;
    waves = std::max(8, std::min(28, waves));
    per_cu = std::max(1, std::min(jit_blocks_per_cu(one_pass() ? select_fn : flags_fn, first_block, first_lds), waves / (first_block / 64)));
  }
  int64_t grid = (int64_t)(fdb_scan_default_grid(P.device_) / 2) * per_cu;
  if (P.grid_override > 0) grid = P.grid_override;
  if (grid > total_super) grid = total_super;
  unsigned long long* h_base = (unsigned long long*)P.ctx_->host_alloc((nl + 1 + FDB_SELECT_CTL_WORDS) * 8);
  struct HostFree { Context* c; void* p; ~HostFree() { c->host_free(p); } } hf{P.ctx_, h_base};
  if (one_pass()) count_rows_one_pass(grid, first_lds, stage_off, h_base);
  else count_rows_two_pass(grid, h_base);
}

void Plan::FilterRun::count_rows_one_pass(int64_t grid, size_t first_lds, size_t stage_off, unsigned long long* h_base) {
  Context* ctx = P.ctx_;
  // outputs of the fused columns: one worst-case block per record, owned by the result from here on
  std::vector<FdbSelectPart> sparts(nl);
  uint32_t epoch = 0;
  unsigned long long ticket_base = 0, arrival_base = 0;
  const size_t status_words = align_up((size_t)total_super, 16);
  unsigned long long* d_ctl = ctx->select_ctl(align_up(nl, 16) + status_words + 16 * (size_t)total_super, &epoch, &ticket_base, &arrival_base);
  for (size_t k = 0; k < nl; k++) {
    DeviceBatch& o = dst(k);
    std::memset(&sparts[k], 0, sizeof(FdbSelectPart));
    sparts[k].total = d_ctl + FDB_SELECT_CTL_WORDS + k;
    if (fused.empty()) continue;
    size_t bytes = 0;
    std::vector<size_t> off(fused.size());
    for (size_t f = 0; f < fused.size(); f++) { off[f] = bytes; bytes += values_slot((size_t)src(k).rows, fused[f].wide ? 8 : 4); }
    void* block = device_pool_alloc(P.device_, bytes);
    o.extra_arenas.push_back(block);
    o.arena_bytes += bytes;
    for (size_t f = 0; f < fused.size(); f++) sparts[k].dst[f] = (unsigned char*)block + off[f];
  }
  // The other columns' validity bitmaps and NULL counters — what the compaction launch ORs / adds into — are zeroed by THIS launch on
  // its way in (FdbSelectArgs::zero) instead of by a launch of their own between the two: they must exist before the row counts do,
  // so a record's bitmaps get a worst-case block of their own (rows / 8 bytes per nullable column; the values still go into an arena
  // of the exact size).
  bool any_nullable_rest = false;
  for (int c : rest) any_nullable_rest = any_nullable_rest || nullable[(size_t)c];
  std::vector<unsigned long long> zero_tab;
  if (any_nullable_rest) {
    for (size_t k = 0; k < nl; k++) {
      DeviceBatch& o = dst(k);
      size_t bytes = 0;
      for (size_t c = 0; c < n_cols; c++) if (nullable[c]) bytes += bitmap_slot((size_t)src(k).rows);
      void* block = device_pool_alloc(P.device_, std::max<size_t>(bytes, 256));
      pre_bits[k] = block;
      pre_bits_bytes[k] = std::max<size_t>(bytes, 256);
      // (in FRONT of the fused columns' block: that one stays extra_arenas.back())
      o.extra_arenas.insert(o.extra_arenas.begin(), block);
      o.arena_bytes += pre_bits_bytes[k];
      zero_tab.push_back((unsigned long long)(uintptr_t)block);
      zero_tab.push_back((unsigned long long)pre_bits_bytes[k]);
    }
    pre_nulls_words = nl * std::max<size_t>(rest.size(), 1) * 64;
    pre_nulls = (unsigned long long*)ctx->dev_alloc(align_up(pre_nulls_words * 8, 256));
    P.scratch_.push_back(pre_nulls);
    zero_tab.push_back((unsigned long long)(uintptr_t)pre_nulls);
    zero_tab.push_back((unsigned long long)align_up(pre_nulls_words * 8, 256));
  }
  FdbSelectArgs sa;
  std::memset(&sa, 0, sizeof(sa));
  sa.ctl = d_ctl;
  sa.ticket_base = ticket_base;
  sa.epoch = epoch;
  sa.stage_off = (uint32_t)stage_off;
  sa.arrival_base = arrival_base;
  sa.status_off = (uint32_t)(FDB_SELECT_CTL_WORDS + align_up(nl, 16));
  sa.place_off = (uint32_t)(sa.status_off + status_words);
  {
    StageScope stage_scope(ctx);
    sa.sparts = (const FdbSelectPart*)P.upload(sparts.data(), sparts.size() * sizeof(FdbSelectPart));
    if (!zero_tab.empty()) { sa.zero = (const unsigned long long*)P.upload(zero_tab.data(), zero_tab.size() * 8); sa.n_zero = (int32_t)(zero_tab.size() / 2); }
  }
  P.timed([&] { hip_check(jit_select_launch(select_fn, d_parts, (int)parts.size(), total_super, parts[0], (int)grid + 1, first_lds, d_masks, d_offsets, sa, P.stream_), "select launch"); });
  // (one workgroup more than workers: the scanner; every worker draws exactly one ticket past the end)
  ctx->select_ctl_drawn((unsigned long long)total_super + (unsigned long long)grid, (unsigned long long)grid + 1);
  launches = 1;
  hip_check(hipMemcpyAsync(h_base, d_ctl + 1, (FDB_SELECT_CTL_WORDS - 1 + nl) * 8, hipMemcpyDeviceToHost, P.stream_), "hipMemcpyAsync(row counts)");
  hip_check(hipStreamSynchronize(P.stream_), "hipStreamSynchronize");  // (first host round trip: the other columns' outputs are allocated at their exact sizes)
  if (h_base[0] != 0ull || std::getenv("FDB_TEST_SELECT_STALL") != nullptr) {  // a wait ran into its bound: nothing of this attempt is kept
    ctx->select_ctl_reset();
    hip_check(hipStreamSynchronize(P.stream_), "hipStreamSynchronize");
    throw SelectStall();
  }
  for (size_t k = 0; k < nl; k++) totals[k] = (int64_t)h_base[FDB_SELECT_CTL_WORDS - 1 + k];
}

void Plan::FilterRun::count_rows_two_pass(int64_t grid, unsigned long long* h_base) {
  const hipStream_t stream = P.stream_;
  const int64_t n_blocks = (total_tiles + 1023) / 1024;
  const size_t counts_bytes = align_up((size_t)n_blocks * 8 + (size_t)total_tiles * 4, 256);
  unsigned char* d_counts = (unsigned char*)P.ctx_->dev_alloc(counts_bytes);
  unsigned long long* d_rec_base = (unsigned long long*)P.ctx_->dev_alloc((nl + 1) * 8 + 64);
  P.scratch_.push_back(d_counts); P.scratch_.push_back(d_rec_base);
  unsigned long long* d_block_sums = (unsigned long long*)d_counts;
  uint32_t* d_tile_counts = (uint32_t*)(d_counts + (size_t)n_blocks * 8);
  const bool two_level = fdb_sel_scan_two_level(total_tiles);  // (below that every scan workgroup adds up the counts in front of its block itself)
  P.timed([&] {
    hip_check(jit_flags_launch(flags_fn, d_parts, (int)parts.size(), total_super, parts[0], (int)grid, lut_lds_max, d_masks, d_tile_counts, stream), "flags launch");
    if (two_level) hip_check(fdb_launch_sel_block_sums(d_tile_counts, total_tiles, d_block_sums, stream), "block sums launch");
    hip_check(fdb_launch_sel_scan(d_tile_counts, two_level ? d_block_sums : nullptr, total_tiles, d_offsets, d_recs, (int)nl, d_rec_base, stream), "prefix sums launch");
  });
  launches = two_level ? 3 : 2;
  hip_check(hipMemcpyAsync(h_base, d_rec_base, (nl + 1) * 8, hipMemcpyDeviceToHost, stream), "hipMemcpyAsync(row counts)");
  hip_check(hipStreamSynchronize(stream), "hipStreamSynchronize");  // (first host round trip: outputs are allocated at their exact sizes)
  for (size_t k = 0; k < nl; k++) totals[k] = (int64_t)(h_base[k + 1] - h_base[k]);
  d_rec_base_arg = d_rec_base;  // (offsets are global here: compact_multi_kernel subtracts the record's base)
}

// Outputs: [values of every column | validity bitmaps of every column] per record, at their exact sizes.
void Plan::FilterRun::lay_out(int64_t* n_selected) {
  cols.resize(nl * std::max<size_t>(rest.size(), 1));
  int64_t ones_rows = 0;
  for (size_t k = 0; k < nl; k++)
    for (size_t c = 0; c < n_cols; c++) if (nullable[c] && src(k).cols[c].d_validity == nullptr) ones_rows = std::max(ones_rows, src(k).rows);
  uint8_t* d_ones = nullptr;
  if (ones_rows > 0) {
    const size_t ones_bytes = bitmap_slot((size_t)ones_rows);
    d_ones = (uint8_t*)P.ctx_->dev_alloc(ones_bytes);
    P.scratch_.push_back(d_ones);
    hip_check(hipMemsetAsync(d_ones, 0xFF, ones_bytes, P.stream_), "hipMemsetAsync(all-valid bitmap)");
  }
  for (size_t k = 0; k < nl; k++) {
    const int64_t total = totals[k];
    if (total < 0 || total > src(k).rows) throw Error(FDB_ERR_DEVICE, "internal: selection counts out of range");
    n_selected[live[k]] = total;
    dst(k).rows = total;
    any_selected += total;
    P.stat_bytes += Rs[k].bytes;
    P.stat_rows += src(k).rows;
    place_record(k, d_ones);
  }
}

void Plan::FilterRun::place_record(size_t k, const uint8_t* d_ones) {
  const DeviceBatch& s = src(k);
  DeviceBatch& o = dst(k);
  const int64_t total = totals[k];
  // the fused columns stay where the kernel put them unless most of the block is unused
  const bool repack = !fused.empty() && total > 0 && (double)total < 0.4 * (double)s.rows;
  size_t bytes = 0, bits_at = 0;
  std::vector<size_t> val_off(n_cols, 0), bit_off(n_cols, 0);
  for (size_t c = 0; c < n_cols; c++) {
    if (fused_of[c] >= 0 && !repack) continue;
    val_off[c] = bytes;
    bytes += values_slot((size_t)total, value_width(s.cols[c].kind));
  }
  bits_at = bytes;
  uint8_t* const bits_block = (uint8_t*)pre_bits[k];  // (one pass with nullable columns: zeroed by the select launch, worst-case sized)
  if (bits_block != nullptr) {
    size_t at = 0;
    for (size_t c = 0; c < n_cols; c++) if (nullable[c]) { bit_off[c] = at; at += bitmap_slot((size_t)s.rows); }
  } else {
    for (size_t c = 0; c < n_cols; c++)
      if (nullable[c]) { bit_off[c] = bytes; bytes += bitmap_slot((size_t)total); }
  }
  if (total > 0 && bytes > 0) {
    o.arena = device_pool_alloc(P.device_, std::max<size_t>(bytes, 256));
    o.arena_bytes += std::max<size_t>(bytes, 256);
    if (bytes > bits_at) { regions.push_back(FdbZeroRegion{(unsigned char*)o.arena + bits_at, (int64_t)(bytes - bits_at)}); max_region = std::max<int64_t>(max_region, (int64_t)(bytes - bits_at)); }
  }
  if (bits_block != nullptr && total == 0) {  // nothing selected: the record's result has no buffers at all
    o.extra_arenas.erase(o.extra_arenas.begin());
    o.arena_bytes -= pre_bits_bytes[k];
    repacked.v.push_back(bits_block);
  }
  if (!fused.empty() && (total == 0 || repack)) {  // the worst-case block is not part of the result
    void* block = o.extra_arenas.back();
    o.extra_arenas.pop_back();
    size_t worst = 0;
    for (size_t f = 0; f < fused.size(); f++) {
      const int w = fused[f].wide ? 8 : 4;
      if (repack) hip_check(hipMemcpyAsync((unsigned char*)o.arena + val_off[(size_t)fused[f].col], (unsigned char*)block + worst, (size_t)total * w, hipMemcpyDeviceToDevice, P.stream_), "hipMemcpyAsync(repack)");
      worst += values_slot((size_t)s.rows, (size_t)w);
    }
    o.arena_bytes -= worst;
    repacked.v.push_back(block);
  }
  for (size_t c = 0; c < n_cols; c++) {
    Placed& Q = placed[k * n_cols + c];
    if (fused_of[c] >= 0 && !repack) {
      // (fused columns sit in the block in `fused` order)
      size_t at = 0;
      for (int f = 0; f < fused_of[c]; f++) at += values_slot((size_t)s.rows, fused[(size_t)f].wide ? 8 : 4);
      Q.values = total > 0 ? (unsigned char*)o.extra_arenas.back() + at : nullptr;
    } else {
      Q.values = total > 0 ? (unsigned char*)o.arena + val_off[c] : nullptr;
    }
    Q.valid = total > 0 && nullable[c] ? (bits_block != nullptr ? bits_block : (uint8_t*)o.arena) + bit_off[c] : nullptr;
  }
  for (size_t r = 0; r < rest.size(); r++) {
    const size_t c = (size_t)rest[r];
    FdbCompactCol& C = cols[k * rest.size() + r];
    C.src = s.cols[c].d_values;
    C.width = (int)value_width(s.cols[c].kind);
    C.nullable = nullable[c];
    C.src_valid = nullable[c] ? (s.cols[c].d_validity != nullptr ? s.cols[c].d_validity : d_ones) : nullptr;
    C.dst = placed[k * n_cols + c].values;
    C.dst_valid = placed[k * n_cols + c].valid;
  }
}

// Zero the output bitmaps and NULL counters that still need it, compact the `rest` columns of every record (compact_multi_kernel),
// read the NULL counts back (the second host round trip).
void Plan::FilterRun::compact() {
  const size_t n_rest = rest.size();
  const hipStream_t stream = P.stream_;
  h_nulls.assign(nl * std::max<size_t>(n_rest, 1) * 64, 0);
  int any_nullable = 0;
  for (size_t r = 0; r < n_rest; r++) any_nullable |= nullable[(size_t)rest[r]] ? 1 : 0;
  if (any_selected > 0 && n_rest > 0) {
    // NULL counts and validity bitmaps exist only when some column has a bitmap: without one there is nothing to zero, count or copy back
    unsigned long long* d_nulls = nullptr;
    if (any_nullable && pre_nulls != nullptr && pre_nulls_words >= h_nulls.size()) {
      d_nulls = pre_nulls;  // (zeroed by the select launch)
    } else if (any_nullable) {
      d_nulls = (unsigned long long*)P.ctx_->dev_alloc(h_nulls.size() * 8);
      P.scratch_.push_back(d_nulls);
      regions.push_back(FdbZeroRegion{d_nulls, (int64_t)(h_nulls.size() * 8)});
      max_region = std::max<int64_t>(max_region, (int64_t)(h_nulls.size() * 8));
    }
    const FdbCompactCol* d_cols = (const FdbCompactCol*)P.upload(cols.data(), cols.size() * sizeof(FdbCompactCol));
    const FdbZeroRegion* d_regions = regions.empty() ? nullptr : (const FdbZeroRegion*)P.upload(regions.data(), regions.size() * sizeof(FdbZeroRegion));
    // waves are dealt to the columns in proportion to their bytes per row (a wave stays on its column for the whole launch):
    // 1.5 × the workgroups of 4 waves that are resident at once (a wave's share of tiles is fixed at launch: smaller shares even out
    // the waves that finish late — measured 8 % faster than exactly-resident; handing tiles out dynamically, one ticket per tile or per
    // 8 tiles on a per-column counter, was slower: 2.5 ms and 1.08 ms against 0.90), at least one wave per column, never more waves
    // than a column has tiles
    const int64_t budget = (int64_t)(fdb_scan_default_grid(P.device_) / 2) * ((fdb_compact_multi_blocks_per_cu(any_nullable) * 3 + 1) / 2) * 4;
    int64_t weight_sum = 0;
    for (size_t r = 0; r < n_rest; r++) weight_sum += cols[r].width;
    std::vector<int32_t> wave_begin(n_rest + 1, 0);
    for (size_t r = 0; r < n_rest; r++) {
      int64_t share = std::max<int64_t>(1, budget * cols[r].width / std::max<int64_t>(weight_sum, 1));
      share = std::min<int64_t>(share, total_tiles);
      wave_begin[r + 1] = wave_begin[r] + (int32_t)share;
    }
    const int32_t* d_wave_begin = (const int32_t*)P.upload(wave_begin.data(), wave_begin.size() * 4);
    P.timed([&] {
      if (!regions.empty()) hip_check(fdb_launch_zero_regions(d_regions, (int)regions.size(), max_region, stream), "zero launch");
      hip_check(fdb_launch_compact_multi(d_recs, (int)nl, d_cols, (int)n_rest, any_nullable, d_wave_begin, wave_begin[n_rest], d_masks, d_offsets, d_rec_base_arg, total_tiles, d_nulls, stream),
                "compact launch");
    });
    launches += regions.empty() ? 1 : 2;
    if (any_nullable) hip_check(hipMemcpyAsync(h_nulls.data(), d_nulls, h_nulls.size() * 8, hipMemcpyDeviceToHost, stream), "hipMemcpyAsync(null counts)");
  }
  hip_check(hipStreamSynchronize(stream), "hipStreamSynchronize");
  for (void* p : repacked.v) device_pool_free(P.device_, p);
  repacked.v.clear();
}

// Column descriptors of every result record, and the plan's counters.
void Plan::FilterRun::describe() {
  P.last_kernel_ = one_pass() ? (!rest.empty() ? "fdb_select_kernel + compact_multi_kernel" : "fdb_select_kernel") : "fdb_flags_kernel + compact_multi_kernel";
  P.stat_launches += launches;
  for (size_t k = 0; k < nl; k++) {
    DeviceBatch& o = dst(k);
    for (size_t c = 0; c < n_cols; c++) {
      const Placed& Q = placed[k * n_cols + c];
      unsigned long long nulls = 0;
      if (rest_of[c] >= 0) for (int q = 0; q < 64; q++) nulls += h_nulls[(k * rest.size() + (size_t)rest_of[c]) * 64 + (size_t)q];
      finish_column(&o, c, (int64_t)nulls, Q.values, Q.valid);
      P.stat_bytes += compaction_bytes(src(k).cols[c], o.rows);
    }
  }
}

// The record of a resident batch as Arrow in host memory (one device→host copy per buffer).
void export_batch(const DeviceBatch& b, ArrowArray* out, ArrowSchema* out_schema) {
  hip_check(hipSetDevice(b.device), "hipSetDevice");
  const int64_t n = b.rows;
  std::vector<OutColumn> cols;
  for (const DevColumn& c : b.cols) {
    if (c.d_values == nullptr && n > 0)
      throw Error(FDB_ERR_UNSUPPORTED, "export: column type " + c.format + " (" + c.name + ") is not held on the device");
    OutColumn o;
    o.name = c.name;
    o.length = n;
    const int w = c.kind == ColKind::DICT ? 4 : 8;
    o.format = c.kind == ColKind::DICT ? "I" : c.format;
    o.values.resize((size_t)n * w);
    if (n > 0) hip_check(hipMemcpy(o.values.data(), c.d_values, (size_t)n * w, hipMemcpyDeviceToHost), "hipMemcpy(export values)");
    if (c.d_validity != nullptr && n > 0) {
      o.validity.assign((size_t)((n + 63) / 64) * 8, 0);
      hip_check(hipMemcpy(o.validity.data(), c.d_validity, (size_t)(n + 7) / 8, hipMemcpyDeviceToHost), "hipMemcpy(export validity)");
      o.null_count = count_nulls(o.validity.data(), 0, n);
    }
    if (c.kind == ColKind::DICT && c.dict && c.dict->plain) {  // a plain string / binary column leaves as one
      const std::vector<uint8_t> idx_bytes = std::move(o.values);
      set_plain_strings(&o, (const uint32_t*)idx_bytes.data(), o.validity.empty() ? nullptr : o.validity.data(), n, c.dict->values, c.dict->value_format);
    } else if (c.kind == ColKind::DICT) {
      if (!c.dict) throw Error(FDB_ERR_INVALID, "export: dictionary column without its dictionary: " + c.name);
      set_dictionary(&o, c.dict->values, c.dict->value_format);
    } else if (c.kind == ColKind::BOOL) {  // held as int64 1 / 2, Arrow wants bits
      std::vector<uint8_t> bits((size_t)(n + 7) / 8 + 8, 0);
      for (int64_t i = 0; i < n; i++) { int64_t v; std::memcpy(&v, o.values.data() + (size_t)i * 8, 8); if (v >= 2) bits[(size_t)(i >> 3)] |= (uint8_t)(1u << (i & 7)); }
      o.values = std::move(bits);
    }
    cols.push_back(std::move(o));
  }
  export_record(std::move(cols), n, out, out_schema);
}

void Plan::select(const ArrowArray* array, const ArrowSchema* schema, uint32_t* indices, int64_t capacity, int64_t* n_selected) {
  if (filter_root_ < 0) throw Error(FDB_ERR_STATE, "plan has no filter");
  HostRecordView view;
  view_record(array, schema, &view);
  if (capacity < view.rows) throw Error(FDB_ERR_INVALID, "indices capacity smaller than the record");
  std::function<bool(const std::string&)> want = [this](const std::string& n) {
    for (const ExprNode& e : filter_) if (is_leaf_op(e.op) && e.column == n) return true;
    return false;
  };
  std::unique_ptr<DeviceBatch> b = import_batch(view, device_, &want, stream_);
  *n_selected = 0;
  if (b->rows == 0) return;
  DevBuf d_idx(ctx_, (size_t)b->rows * 4);
  const int64_t n = select_batch(*b, (uint32_t*)d_idx.p, b->rows);
  *n_selected = n;
  if (n) hip_check(hipMemcpy(indices, d_idx.p, (size_t)n * 4, hipMemcpyDeviceToHost), "hipMemcpy(indices)");
}

void Plan::filter(const ArrowArray* array, const ArrowSchema* schema, ArrowArray* out, ArrowSchema* out_schema, int64_t* n_selected) {
  if (filter_root_ < 0) throw Error(FDB_ERR_STATE, "plan has no filter");
  HostRecordView view;
  view_record(array, schema, &view);
  std::unique_ptr<DeviceBatch> b = import_batch(view, device_, nullptr, stream_);
  std::unique_ptr<DeviceBatch> f = filter_batch(*b, n_selected);
  if (*n_selected == 0) return;  // filter.go:264-266
  export_batch(*f, out, out_schema);
}

}  // namespace fdb
