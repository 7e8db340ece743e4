// fdb_plan_internal.h — per-record resolution state shared by fdb_plan.cpp, fdb_dense.cpp, fdb_filter.cpp, fdb_project.cpp and fdb_hash.cpp (not part of
// any API): Resolved, the LUT blob and its classes (LutClasses), staging scope, phase timer. The stages of a dense scan launch that use them
// — bind_group_columns, stage_luts, assign_all_slots, plan_lds, narrow_slots, choose_kernel, launch — are Plan::DenseLaunch in fdb_dense.cpp.
#pragma once

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <functional>
#include <memory>
#include <string>
#include <vector>

#include "fdb_context.h"
#include "fdb_plan.h"

namespace fdb {

bool is_leaf_op(int32_t op);  // a comparison / regex / contains leaf of a filter expression

struct PhaseTimer {  // FDB_PROFILE=1: per-phase host microseconds on stderr (tuning aid)
  bool on;
  std::chrono::steady_clock::time_point t;
  PhaseTimer() : on(std::getenv("FDB_PROFILE") != nullptr), t(std::chrono::steady_clock::now()) {}
  void mark(const char* what) {
    if (!on) return;
    auto n = std::chrono::steady_clock::now();
    std::fprintf(stderr, "[fdb] %-20s %8.1f us\n", what, std::chrono::duration<double, std::micro>(n - t).count());
    t = n;
  }
};

// FDB_PROFILE=1: one line per dense scan launch with every decision behind it (tuning aid) — no pointers and no times, so that two
// builds that decide alike print alike. `shape_key`: JitShape::key(true) of a specialised kernel, empty otherwise. `folded`: per part
// (empty: none) the slots that read a null-folded narrow-index cache without their bitmap, early slot k as bit k, late slot k as bit
// 16 + k; such a slot's width (H / T: the packed forms of 4 / 12 bits) is followed by `n`. A narrow slot without the mark whose shape has no bitmap is a column without NULLs.
// `ptab_words`: words per record of the packed part table the kernel reads (JitShape::part_table), 0: it reads the argument blocks.
inline void print_dense_launch(const char* kernel, const std::string& shape_key, const FdbScanArgs* const* parts, size_t n_parts, int64_t total_tiles, int grid, int block,
                               size_t lds_bytes, int two_phase, int lds_acc, int cache_slots, size_t lut_lds_max, int per_cu, int tile_rows, bool fill_rides, bool partials,
                               const std::vector<uint32_t>& folded = std::vector<uint32_t>(), int ptab_words = 0) {
  std::string s;
  auto form = [](int w) { const ScanFormRow* f = scan_form_row(w); return f != nullptr ? std::string(f->name) : std::to_string(w); };  // (0: the argument blocks' 4)
  for (size_t p = 0; p < n_parts; p++) {
    const FdbScanArgs& a = *parts[p];
    s += " " + std::to_string(a.lut_class) + ":";
    const uint32_t f = p < folded.size() ? folded[p] : 0u;
    for (int k = 0; k < a.n_c4; k++) s += form((int)a.w4[k]) + ((f >> k) & 1u ? "n" : "");
    s += "/";
    for (int k = 0; k < a.n_l4; k++) s += form((int)a.wl4[k]) + ((f >> (16 + k)) & 1u ? "n" : "");
  }
  std::fprintf(stderr, "[fdb] dense launch %s shape=%s parts=%zu total_tiles=%lld grid=%d block=%d lds_bytes=%zu two_phase=%d lds_acc=%d cache_slots=%d lut_lds_max=%zu "
               "per_cu=%d tile_rows=%d fill=%d partials=%d ptab=%d class:w4/wl4=%s\n", kernel, shape_key.empty() ? "-" : shape_key.c_str(), n_parts, (long long)total_tiles, grid, block,
               lds_bytes, two_phase, lds_acc, cache_slots, lut_lds_max, per_cu, tile_rows, (int)fill_rides, (int)partials, ptab_words, s.c_str());
}

struct Blob {  // LUTs of one batch, shipped with one copy
  std::vector<uint8_t> bytes;
  size_t add(const void* p, size_t n) {
    const size_t off = align_up(bytes.size(), 16);
    bytes.resize(off + std::max<size_t>(n, 1), 0);
    if (n) std::memcpy(bytes.data() + off, p, n);
    return off;
  }
};

struct PendingLut { int kind; int index; size_t blob_off; size_t len_bytes; };  // kind 0: leaf, 1: group col

// LDS plan of a record's LUTs, from `lds_off` on: a LUT of at most 16 KiB is copied into LDS while the LUTs placed there stay within
// 32 KiB (16-byte aligned), the others are read from global memory (FDB_NO_LDS). `d_blob`: the device copy of the record's blob.
// Sets lut / lut_lds of the leaves (kind 0) and dense group columns (kind 1); returns the aligned end of the LDS region.
inline size_t place_luts(const std::vector<PendingLut>& luts, unsigned char* d_blob, size_t lds_off, FdbScanArgs* a) {
  for (const PendingLut& p : luts) {
    const bool in_lds = p.len_bytes <= 16384 && lds_off + p.len_bytes <= 32768;
    uint32_t lds = FDB_NO_LDS;
    if (in_lds) { lds = (uint32_t)lds_off; lds_off = align_up(lds_off + p.len_bytes, 16); }
    unsigned char* at = d_blob + p.blob_off;
    if (p.kind == 0) { a->leaves[p.index].lut = at; a->leaves[p.index].lut_lds = lds; }
    else { a->gcols[p.index].lut = (const uint32_t*)at; a->gcols[p.index].lut_lds = lds; }
  }
  return align_up(lds_off, 16);
}

// Several tables that feed ONE launch are staged between construction and destruction and shipped with one copy command.
struct StageScope {
  Context* c;
  explicit StageScope(Context* ctx) : c(ctx) { c->defer_staging(true); }
  ~StageScope() { try { c->defer_staging(false); } catch (...) {} }
};

template <class F>
void Plan::timed(F&& launch, bool merge) {
  hipEvent_t e0 = nullptr, e1 = nullptr;
  if (timing) { e0 = ctx_->get_event(); e1 = ctx_->get_event(); hip_check(hipEventRecord(e0, stream_), "hipEventRecord"); }
  launch();
  if (timing) { hip_check(hipEventRecord(e1, stream_), "hipEventRecord"); (merge ? merge_events_ : pending_events_).emplace_back(e0, e1); }
}


struct GroupRes {
  int gi, ci, kind;      // kind 2: computed int64 key (ci = -1, expr_root = root node in the record's args.expr)
  int expr_root = -1;
  std::shared_ptr<const std::vector<uint32_t>> lut;
};

struct Plan::Resolved {
  TruthCache* truths = nullptr;           // the plan's cache
  int cur_node = -1;                      // filter node being resolved
  FdbScanArgs args;
  Blob blob;
  std::vector<PendingLut> luts;
  // Where each entry of `luts` came from — the truth cache's table, a group column's key-id LUT — held for the length of the push, so that
  // equal addresses mean one object: records whose LUTs have the same sources share a LUT set without a byte copied or compared.
  std::vector<std::shared_ptr<const void>> lut_src;
  int lut_like = -1;          // dense launch: the earlier record of the push whose LUT set this one shares (its own blob lacks the group LUTs then)
  std::vector<char> counted;  // per batch column: bit 0 values, bit 1 validity already counted in algorithmic bytes
  int64_t bytes = 0;
  int leaf_col[FDB_MAX_LEAVES];           // batch column behind each leaf (-1: constant leaf)
  int gcol_col[FDB_MAX_DENSE_GCOLS];
  int agg_col[FDB_MAX_AGGS];
  int expr_col[FDB_MAX_EXPR_NODES];       // batch column behind each expression column node
  int c4_col[FDB_ARG_C4], l4_col[FDB_ARG_L4];  // batch column behind each 4-byte slot (assign_slots)
  std::vector<GroupRes> groups;           // group-by columns of this record (plan-level index, record column, kind, key-id LUT)
  // AndExpr.Eval is lazy (filter.go:172-190): when the left side of an AND selects no row of the record the right side is not
  // evaluated — so a right side that cannot be evaluated on this record (an operator its column type does not support) only is
  // an error if the left side selects something. Set by the plan: rows of this record the sub-tree rooted at `node` selects.
  std::function<int64_t(int node)> count_selected;
  Resolved() {
    for (int& v : leaf_col) v = -1;
    for (int& v : gcol_col) v = -1;
    for (int& v : agg_col) v = -1;
    for (int& v : expr_col) v = -1;
    for (int& v : c4_col) v = -1;
    for (int& v : l4_col) v = -1;
  }
  // Algorithmic bytes: each referenced buffer once per row, whatever the number of references.
  void count(const DeviceBatch& b, int ci, bool values = true) {
    if (counted.empty()) counted.assign(b.cols.size(), 0);
    char& c = counted[(size_t)ci];
    if (values && !(c & 1)) { c |= 1; bytes += b.cols[(size_t)ci].value_bytes; }
    if (!(c & 2)) { c |= 2; bytes += b.cols[(size_t)ci].validity_bytes; }
  }
};

// Records whose LUT sets are byte-identical (the usual case: parts of one table share dictionaries) share one device copy and one
// class id, so a kernel re-stages LUTs in LDS only when the class changes.
inline bool same_lut_set(const Plan::Resolved& q, const Plan::Resolved& r) {
  if (q.blob.bytes != r.blob.bytes || q.luts.size() != r.luts.size()) return false;
  for (size_t k = 0; k < r.luts.size(); k++)
    if (q.luts[k].kind != r.luts[k].kind || q.luts[k].index != r.luts[k].index || q.luts[k].blob_off != r.luts[k].blob_off ||
        q.luts[k].len_bytes != r.luts[k].len_bytes)
      return false;
  return true;
}

// The LUT sets of the records of ONE launch: add() every record in launch order, upload `blob` once, then place() every record.
struct LutClasses {
  Blob blob;                      // one copy of each distinct set, 16-byte aligned
  std::vector<size_t> blob_base;  // [record] where its set starts in `blob`
  std::vector<int> cls;           // [record] class, numbered in first-seen order
  // record `k` of the launch is known to carry the LUT set of the earlier record `like` (by the identity of its sources)
  void add_like(size_t like) { blob_base.push_back(blob_base[like]); cls.push_back(cls[like]); }
  void add(const Plan::Resolved& R) {
    size_t found = 0;
    while (found < reps_.size() && !same_lut_set(*reps_[found].first, R)) found++;
    if (found == reps_.size()) reps_.emplace_back(&R, R.blob.bytes.empty() ? 0 : blob.add(R.blob.bytes.data(), R.blob.bytes.size()));  // (no LUT: nothing to ship)
    blob_base.push_back(reps_[found].second);
    cls.push_back((int)found);
  }
  // record k of the launch (`d_blob`: the device copy of `blob`): lut / lut_lds of its leaves and group columns, its class; returns the end of its LDS region
  size_t place(size_t k, unsigned char* d_blob, Plan::Resolved& R) const {
    R.args.lut_class = cls[k];
    return place_luts(R.luts, d_blob + blob_base[k], 0, &R.args);
  }
 private:
  std::vector<std::pair<const Plan::Resolved*, size_t>> reps_;  // first record of each class (the caller keeps its records where they are until the last add), its blob_base
};

// Column slots of the load-hoisting kernel for a record (fdb_plan.cpp); 0 when they do not fit.
int assign_slots(const DeviceBatch& b, Plan::Resolved& R, int first_layout = 1, bool relaxed = false, bool* interp_ok = nullptr);


}  // namespace fdb
