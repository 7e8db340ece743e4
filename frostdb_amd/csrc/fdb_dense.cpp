// fdb_dense.cpp — one launch of the dense (mixed-radix table) filter + group-by scan over the resident records of a push:
// Plan::DenseLaunch, the stages Plan::push_batches (fdb_plan.cpp) calls once it has resolved the records and chosen the dense table.
// What needs nothing but numbers (LDS plan, tile ranges, fold table) is in fdb_launch_plan.h, the LUT classes in fdb_plan_internal.h.
#include "fdb_plan.h"
#include "fdb_jit.h"

#include "fdb_context.h"
#include "fdb_launch_plan.h"
#include "fdb_plan_internal.h"

#include <optional>

namespace fdb {

// Launch state of one dense push_batches call over the records that have rows (`live`). Its members are the stages of the launch, called
// in this order; every field is written by the one stage it is listed under and only read by the later ones.
struct Plan::DenseLaunch {
  Plan& P;
  const DeviceBatch* const* bs;
  std::vector<Resolved>& Rs;                   // [record of the push]
  std::vector<std::vector<int>>& part_gcols;   // [record] plan-level index of each of its group columns
  const std::vector<int>& live;
  const bool fixed_order;                      // reproducible float sums: per-wave tables, the specialised kernel or nothing
  PhaseTimer& pt;
  const bool jit_possible;
  const int sub;                               // kernel variant mode (0 = default; sub_tiles 4 = interpreting kernel only)
  FdbScanArgs& args(int i) { return Rs[(size_t)i].args; }

  // stage_luts(): one blob for every LUT of every record; it and the argument blocks go to the device with ONE copy command, issued
  // right before the launch
  std::optional<StageScope> stage_scope;
  LutClasses luts;
  size_t lut_lds_max = 0;

  // assign_all_slots()
  bool slots_ok = false;     // every record fits the slot kernels' pools
  bool interp_ok = true;     // … and the interpreting slot kernel's limits
  int two_phase = 0;

  // plan_lds()
  LdsPlan lds;
  FoldFuncs funcs;

  // narrow_slots() / widen_slots()
  // a slot switched to its record's narrow-index cache; `validity`: the bitmap it read before a null-folded buffer made it needless
  // (prev_of_part: the record's previous entry, SIZE_MAX: none — a record's few slots are found without a walk over the launch's)
  struct Narrowed { int part, k, col; bool late; const void* wide; int64_t saved; const uint8_t* validity; bool folded; size_t prev_of_part; };
  std::vector<Narrowed> narrowed;
  std::vector<size_t> narrowed_by_part;  // [record] its last entry in `narrowed`

  // choose_kernel()
  hipFunction_t jit_fn = nullptr;
  std::string shape_key;     // (FDB_PROFILE)
  int jit_block = 0;         // 0: picked by occupancy
  bool slot_kernel = false;  // a slot kernel (specialised or interpreting) serves the launch; otherwise the sequential kernel
  int per_cu = 1;            // slot kernels: workgroups per CU …
  int tile_rows = 0;         // … and rows per tile (specialised: jit_block × 4, × 16 for a quad shape, JitShape::quad)
  // The packed part table (JitShape::part_table): a specialised quad launch whose records' fields — ptab_words per record — fit the cap
  // ships and reads those words only. 0 words: the argument blocks.
  JitShape shape;
  int ptab_words = 0;
  std::vector<PartField> part_fields;  // jit_part_fields(shape), made once per launch

  DenseLaunch(Plan& p, const DeviceBatch* const* b, std::vector<Resolved>& rs, std::vector<std::vector<int>>& gc, const std::vector<int>& lv, bool fixed, PhaseTimer& t)
      : P(p), bs(b), Rs(rs), part_gcols(gc), live(lv), fixed_order(fixed), pt(t), jit_possible(p.jit_possible()), sub(p.sub_tiles == 4 ? 0 : p.sub_tiles) {}

  void bind_group_columns();
  void stage_luts();
  void assign_all_slots();
  void plan_lds();
  bool specialisable() const { return slots_ok && P.sub_tiles != 4 && lds.lds_bytes <= 150 * 1024; }  // (gfx950: up to 160 KiB of LDS per workgroup)
  void narrow_slots();
  void narrow_pool(bool late);
  void widen_slots();
  bool choose_kernel();
  bool split_by_shape();
  void launch();
  void launch_slots();
  void launch_sequential();
  unsigned long long* alloc_partials(int grid);
  void fold_partials(unsigned long long* partials, int grid);
};

// group columns → mixed-radix digits through per-dictionary LUTs; the table re-laid for the dictionaries as they are now. A column whose
// narrow-index cache is null-folded gets one more entry, lut[entries] = 0, the digit of NULL: narrow_pool may take the slot's bitmap away,
// and then a NULL row arrives as that index. (Here, in front of stage_luts and plan_lds, which size the LUTs' copies; the 4 bytes are
// never read by a launch that keeps the bitmap.)
// The parts of a table mostly share their dictionaries, so their LUTs are the same objects (GroupColState::lut_for, the truth cache): a record
// whose sources are those of an earlier one (`firsts`) takes that record's LUT list and copies nothing into its blob.
void Plan::DenseLaunch::bind_group_columns() {
  struct Src {  // one LUT's source: the object, and for a group LUT whether the entry for NULL follows it (part of the set)
    const void* lut; bool null_entry;
    bool operator==(const Src& o) const { return lut == o.lut && null_entry == o.null_entry; }
  };
  struct First { int rec; size_t n_leaf_luts; std::vector<Src> src; };
  std::vector<First> firsts;
  std::vector<Src> src;
  for (int i : live) {
    Resolved& R = Rs[(size_t)i];
    FdbScanArgs& a = R.args;
    src.clear();
    for (const auto& p : R.lut_src) src.push_back(Src{p.get(), false});
    // whether a group column's LUT gets the entry for NULL (an empty dictionary's LUT is the one entry 0 already)
    auto null_entry_of = [&](const GroupRes& gr) {
      return scan_cache_may_fold(*bs[i], (size_t)gr.ci) && gr.lut->size() <= bs[i]->cols[(size_t)gr.ci].dict->values.size();
    };
    for (const GroupRes& gr : R.groups) src.push_back(Src{gr.lut.get(), null_entry_of(gr)});
    const First* like = nullptr;
    for (const First& f : firsts) {
      const Resolved& Q = Rs[(size_t)f.rec];
      if (f.src != src || f.n_leaf_luts != R.luts.size()) continue;
      bool same = true;
      for (size_t k = 0; same && k < R.luts.size(); k++)
        same = Q.luts[k].kind == R.luts[k].kind && Q.luts[k].index == R.luts[k].index && Q.luts[k].blob_off == R.luts[k].blob_off && Q.luts[k].len_bytes == R.luts[k].len_bytes;
      if (same) { like = &f; break; }
    }
    if (like == nullptr) firsts.push_back(First{i, R.luts.size(), src});
    for (const GroupRes& gr : R.groups) {
      FdbGroupCol& G = a.gcols[a.n_gcols];
      const DevColumn& c = bs[i]->cols[(size_t)gr.ci];
      G.idx = (const uint32_t*)c.d_values;
      G.validity = c.d_validity;
      const size_t null_entry = null_entry_of(gr) ? 1 : 0;
      G.lut_len = (uint32_t)(gr.lut->size() + null_entry);
      G.lut_lds = FDB_NO_LDS;
      G.slot = -1;
      R.gcol_col[a.n_gcols] = gr.ci;
      if (like == nullptr) {
        const size_t off = R.blob.add(gr.lut->data(), gr.lut->size() * 4);
        R.blob.bytes.resize(R.blob.bytes.size() + null_entry * 4, 0);
        R.luts.push_back(PendingLut{1, a.n_gcols, off, (gr.lut->size() + null_entry) * 4});
        R.lut_src.push_back(gr.lut);
      }
      part_gcols[(size_t)i].push_back(gr.gi);
      a.n_gcols++;
    }
    if (like != nullptr) { R.lut_like = like->rec; R.luts = Rs[(size_t)like->rec].luts; }
  }
  std::vector<uint32_t> caps;
  for (const GroupColState& g : P.gcols_) caps.push_back((uint32_t)g.values.size() + 1);
  P.ensure_layout(caps);
  pt.mark("layout");
}

void Plan::DenseLaunch::stage_luts() {
  std::vector<size_t> at(Rs.size(), 0);  // [record] its place among the launch's
  size_t n_added = 0;
  for (int i : live) {
    const Resolved& R = Rs[(size_t)i];
    if (R.lut_like >= 0) luts.add_like(at[(size_t)R.lut_like]); else luts.add(R);
    at[(size_t)i] = n_added++;
  }
  stage_scope.emplace(P.ctx_);
  unsigned char* d_blob = luts.blob.bytes.empty() ? nullptr : (unsigned char*)P.upload(luts.blob.bytes.data(), luts.blob.bytes.size());
  size_t k = 0;
  for (int i : live) lut_lds_max = std::max(lut_lds_max, luts.place(k++, d_blob, Rs[(size_t)i]));
}

// the table's strides and accumulators into every argument block, then column slots: the single-phase layout where a record fits it,
// else the two-phase one — records that fit the single-phase layout also fit the two-phase one and are re-assigned if the launch is mixed
void Plan::DenseLaunch::assign_all_slots() {
  slots_ok = P.rows_per_thread == 0;
  std::vector<int> layouts;
  for (int i : live) {
    Resolved& R = Rs[(size_t)i];
    FdbScanArgs& a = R.args;
    for (int g = 0; g < a.n_gcols; g++) a.gcols[g].stride = P.gcols_[(size_t)part_gcols[(size_t)i][(size_t)g]].stride;
    for (size_t j = 0; j < P.aggs_.size(); j++) a.aggs[j].acc = P.aggs_[j].d_acc;
    a.cnt = P.d_cnt_;
    a.n_slots = P.n_slots_;
    a.need_count = 0;
    for (size_t j = 0; j < P.aggs_.size(); j++) if (a.aggs[j].func == FDB_AGG_COUNT) a.need_count = 1;
    if (slots_ok) {
      bool strict = true;
      const int layout = assign_slots(*bs[i], R, 1, jit_possible, &strict);
      if (layout == 0) slots_ok = false;
      interp_ok = interp_ok && strict;
      layouts.push_back(layout);
    }
  }
  if (!slots_ok) return;
  for (int l : layouts) if (l == 2) two_phase = 1;
  if (two_phase) {
    size_t k = 0;
    for (int i : live)
      if (layouts[k++] == 1 && assign_slots(*bs[i], Rs[(size_t)i], 2, jit_possible) != 2) throw Error(FDB_ERR_INVALID, "internal: slot re-assignment failed");
  }
}

void Plan::DenseLaunch::plan_lds() {
  const size_t acc_bytes = align_up((size_t)P.n_slots_ * 4, 16) + (size_t)P.n_slots_ * 8 * P.aggs_.size();
  lds = fdb::plan_lds(lut_lds_max, acc_bytes, P.aggs_.size(), jit_possible, slots_ok, fixed_order, P.use_partials, P.grid_override,
                      P.grid_override > 0 ? P.grid_override : fdb_scan_default_grid(P.device_));
  if (!lds.refusal.empty()) throw Error(FDB_ERR_UNSUPPORTED, lds.refusal);
  int32_t func[FDB_MAX_AGGS], type[FDB_MAX_AGGS];
  for (size_t j = 0; j < P.aggs_.size(); j++) { func[j] = args(live[0]).aggs[j].func; type[j] = P.aggs_[j].type; }
  funcs = fold_funcs(func, type, P.aggs_.size());
  for (int i : live) { args(i).lds_lut_bytes = (uint32_t)lut_lds_max; args(i).lds_acc = lds.lds_acc; args(i).cache_slots = lds.cache_slots; }
  pt.mark("lut upload");
}

// Narrow index reads (fdb_record.h, ScanForm): a 4-byte slot is scanned at the narrowest form that EVERY part of the launch offers for the
// slot's column (scan_form_common) — its buffers built here, by the first scan that wants them; failing a common narrow form the whole
// launch reads the slot's uint32 columns, which every record has. Slots without values (IS NULL leaves) have nothing to narrow. The
// algorithmic bytes count the form that is scanned. (Before the shape is taken: jit_shape reads the forms.)
// A slot narrowed to a null-folded buffer (scan_cache_folded) also loses its bitmap pointer: the buffer holds NULL as the index one past
// the dictionary, which a leaf's truth table answers last and the group LUT maps to digit 0 (bind_group_columns), so the shape is that of
// a column without NULLs (has_validity 0, or 2 when another record of the launch keeps a bitmap). The exception is a slot an IS (NOT) NULL
// leaf reads: FDB_LEAF_VALIDITY is the one consumer of a 4-byte slot's nibble (<reg>_m in fdb_jitgen.cpp) besides leaf_bits / leaf_lut
// and the group digit, which the folded index serves. The algorithmic bytes keep counting the bitmap: they are what the query reads
// of the record, not what this launch fetches.
void Plan::DenseLaunch::narrow_slots() {
  if (!specialisable() || !jit_possible) return;
  narrowed_by_part.assign(Rs.size(), SIZE_MAX);
  narrow_pool(false);
  if (two_phase) narrow_pool(true);
}
// whether an IS (NOT) NULL leaf reads early 4-byte slot `k` (leaves sit in the early pools only, assign_slots)
static bool validity_leaf_reads(const FdbScanArgs& a, int k) {
  for (int l = 0; l < a.n_leaves; l++)
    if (a.leaves[l].kind == FDB_LEAF_VALIDITY && !a.leaves[l].wide && a.leaves[l].slot == k) return true;
  return false;
}
void Plan::DenseLaunch::narrow_pool(bool late) {
  const FdbScanArgs& a0 = args(live[0]);
  const int n4 = late ? a0.n_l4 : a0.n_c4;
  for (int i : live) if ((late ? args(i).n_l4 : args(i).n_c4) != n4) return;  // (records of different shapes: the launch is split, choose_kernel)
  std::vector<ScanForms> offers;
  for (int k = 0; k < n4; k++) {
    offers.clear();
    for (int i : live) {
      const Resolved& R = Rs[(size_t)i];
      const int ci = late ? R.l4_col[k] : R.c4_col[k];
      const bool none = (late ? R.args.l4[k] : R.args.c4[k]).values == nullptr || ci < 0;
      offers.push_back(none ? ScanForms() : scan_cache_forms(*bs[i], (size_t)ci));
    }
    const ScanForm w = scan_form_common(offers.data(), offers.size());
    if (w == kScanForm4) continue;
    for (int i : live) {
      Resolved& R = Rs[(size_t)i];
      const int ci = late ? R.l4_col[k] : R.c4_col[k];
      FdbColSlot& sl = late ? R.args.l4[k] : R.args.c4[k];
      bool counted = false;  // (a column the filter and the group-by both read sits in two slots and counts once)
      for (size_t at = narrowed_by_part[(size_t)i]; at != SIZE_MAX; at = narrowed[at].prev_of_part) if (narrowed[at].col == ci) counted = true;
      const int64_t saved = counted ? 0 : bs[i]->rows * 4 - scan_form_bytes(bs[i]->rows, w);
      const bool fold = sl.validity != nullptr && scan_cache_folded(*bs[i], (size_t)ci, w) && !(!late && validity_leaf_reads(R.args, k));
      narrowed.push_back(Narrowed{i, k, ci, late, sl.values, saved, sl.validity, fold, narrowed_by_part[(size_t)i]});
      narrowed_by_part[(size_t)i] = narrowed.size() - 1;
      sl.values = scan_cache_get(*bs[i], (size_t)ci, w, P.stream_);
      if (fold) sl.validity = nullptr;
      (late ? R.args.wl4 : R.args.w4)[k] = (uint8_t)w;
      R.bytes -= saved;
    }
  }
}
// … and back, when no specialised kernel came: the interpreting kernels read the uint32 columns
void Plan::DenseLaunch::widen_slots() {
  for (const Narrowed& nw : narrowed) {
    Resolved& R = Rs[(size_t)nw.part];
    (nw.late ? R.args.l4 : R.args.c4)[nw.k].values = nw.wide;
    (nw.late ? R.args.l4 : R.args.c4)[nw.k].validity = nw.validity;
    (nw.late ? R.args.wl4 : R.args.w4)[nw.k] = 0;
    R.bytes += nw.saved;
  }
  narrowed.clear();
}

// The scan kernel: run-time specialised (fdb_jit.cpp: written by fdb_jitgen.cpp for this plan shape, compiled and cached) when every record
// of the launch has the same shape → interpreting slot kernel → sequential kernel. false: the launch was split by shape, each part
// has been pushed on its own and nothing is left to launch.
bool Plan::DenseLaunch::choose_kernel() {
  jit_block = fixed_order ? 256 : sub == 1 ? 512 : sub == 2 ? 256 : sub == 3 ? 1024 : 0;
  if (specialisable()) {
    bool same = true, first = true;
    const FdbScanArgs& args0 = args(live[0]);
    for (int i : live) {
      if (first) { shape = jit_shape(args0, two_phase != 0, jit_block ? jit_block : 256); first = false; }
      else if (!jit_shape_merge_args(&shape, args0, args(i), two_phase != 0)) { same = false; break; }
    }
    if (!same && live.size() > 1 && jit_possible && split_by_shape()) return false;
    {
      // tiny tables live in registers (JitShape::reg_slots): ≤ 8 slots and ≤ 48 accumulator registers per lane
      int regs_per_slot = 2;
      for (const AggState& A : P.aggs_) if (A.func != FDB_AGG_COUNT || P.final_stage_) regs_per_slot += 2;
      if (P.n_slots_ >= 1 && P.n_slots_ <= 8 && (int)P.n_slots_ * regs_per_slot <= 48) shape.reg_slots = (int)P.n_slots_;
    }
    shape.wave_tables = fixed_order;
    shape.uniform_fold = !P.knobs_.no_uniform_fold;
    // (a launch over ONE record has no boundary to cross and its one argument block is the by-value copy already: the table would only
    // add its packing — one 25 M-row record measured 2 µs per step slower with it, profiles/part_table_ab.json)
    if (same && shape.quad && live.size() > 1) {
      part_fields = jit_part_fields(shape);
      const int words = jit_part_words(part_fields);
      if (live.size() * (size_t)words * 8 <= (size_t)P.knobs_.part_table_cap) { shape.part_table = true; ptab_words = words; }
    }
    if (same) {
      // ($FDB_JIT_ASYNC=1: a shape whose kernel still has to be built is scanned by the interpreting kernel meanwhile — when that one can)
      JitDeferScope defer(interp_ok && !fixed_order);
      if (jit_block != 0) { jit_fn = jit_get(shape); if (jit_fn != nullptr) per_cu = jit_blocks_per_cu(jit_fn, jit_block, lds.lds_bytes); }
      else jit_fn = jit_select(shape, lds.lds_bytes, shape.row_bytes(), P.ordered_, &jit_block, &per_cu);
      if (jit_fn != nullptr) tile_rows = jit_block * (shape.quad ? 16 : 4);
      if (pt.on && jit_fn != nullptr) shape_key = shape.key(true);
    }
  }
  if (jit_fn == nullptr) ptab_words = 0;
  if (slots_ok && jit_fn == nullptr) widen_slots();
  // a launch only the specialised kernel could serve (more leaves / aggregates than the interpreting kernel's register-resident
  // plan holds, computed columns) falls back to the sequential kernel when specialisation is unavailable
  slot_kernel = slots_ok && (jit_fn != nullptr || interp_ok);
  if (fixed_order && jit_fn == nullptr) throw Error(FDB_ERR_UNSUPPORTED, "deterministic float sums need the run-time specialised dense kernel (records of one shape, hiprtc available)");
  pt.mark("kernel select");
  if (slot_kernel && jit_fn == nullptr) fdb_slot_geometry(two_phase, sub, lds.lds_acc, lds.lds_bytes, P.device_, &tile_rows, &per_cu);
  return true;
}

// Records of different shapes (schema drift: a filter column missing here, a predicate value absent from that part's dictionary
// there) cannot share one specialised kernel: the launch is split into one launch per shape, so that a few odd parts do not push the
// whole scan onto the interpreting kernel. false: one shape after all (they differ in validity only), nothing was pushed.
// Two quirks are kept as they were: slots already narrowed stay narrowed in this launch's argument blocks (the recursion resolves
// its records afresh and never reads them), and the deferral of staging is ended by hand while stage_scope is still alive (each
// group stages its own tables; what this launch staged goes out with that call).
bool Plan::DenseLaunch::split_by_shape() {
  std::vector<std::string> keys;
  std::vector<std::vector<const DeviceBatch*>> groups;
  for (int i : live) {
    const std::string k = jit_shape(args(i), two_phase != 0, 256).key(false);
    size_t g = 0;
    for (; g < keys.size(); g++) if (keys[g] == k) break;
    if (g == keys.size()) { keys.push_back(k); groups.emplace_back(); }
    groups[g].push_back(bs[i]);
  }
  if (groups.size() <= 1) return false;
  P.ctx_->defer_staging(false);
  for (auto& g : groups) P.push_batches(g.data(), (int)g.size());
  return true;
}

unsigned long long* Plan::DenseLaunch::alloc_partials(int grid) {
  if (!lds.lds_acc || !P.use_partials || grid <= 0) return nullptr;
  void* p = P.ctx_->dev_alloc((size_t)grid * (1 + P.aggs_.size()) * P.n_slots_ * 8);
  P.scratch_.push_back(p);
  return (unsigned long long*)p;
}

// the workgroups' partial tables into the plan's table (and its pinned host mirror, when the table is small enough for one)
void Plan::DenseLaunch::fold_partials(unsigned long long* partials, int grid) {
  if (partials == nullptr) return;
  unsigned long long* host_out = P.mirror_target();
  hip_check(fdb_launch_reduce_partials(partials, grid, (int)(1 + P.aggs_.size()), P.n_slots_, P.d_state_, P.slots_alloc_, funcs.f, host_out, P.stream_), "reduce partials");
  P.mirror_valid_ = host_out != nullptr;
}

void Plan::DenseLaunch::launch() {
  if (slot_kernel) launch_slots(); else launch_sequential();
  pt.mark("reduce launch");
}

// one launch of the slot kernel (specialised or interpreting) over every record
void Plan::DenseLaunch::launch_slots() {
  int grid = P.grid_override > 0 ? P.grid_override : (fdb_scan_default_grid(P.device_) / 2) * per_cu;
  // the records' argument blocks (3 KB apiece) go to the device as they are — or, for a part-table launch, stay where they are: the
  // table is packed straight from them, a few words per record
  const bool ptab = ptab_words > 0;
  std::vector<FdbScanArgs> parts;
  std::vector<FdbScanArgs*> recs;
  int64_t total_tiles = 0;
  if (ptab) {
    for (int i : live) recs.push_back(&args(i));
    total_tiles = assign_tiles(recs.data(), recs.size(), tile_rows);
  } else {
    parts.reserve(live.size());  // (no re-growing copies)
    for (int i : live) parts.push_back(args(i));
    total_tiles = assign_tiles(parts.data(), parts.size(), tile_rows);
  }
  const int n_parts = (int)live.size();
  if (grid > total_tiles) grid = (int)total_tiles;
  unsigned long long* partials = alloc_partials(grid);
  if (ptab) recs[0]->partials = partials;  // (the kernel reads the by-value copy's)
  else for (FdbScanArgs& a : parts) a.partials = partials;
  FdbScanArgs& a0 = ptab ? *recs[0] : parts[0];
  bool fill_rides = false;
  if (P.state_virgin_ && jit_fn != nullptr && partials != nullptr && (uint64_t)P.slots_alloc_ * (1 + P.aggs_.size()) < (1ull << 32)) {
    // nothing accumulates into the table before reduce_partials (the next kernel on the stream): the scan fills it on its way in
    a0.fill_state = P.d_state_;
    a0.fill_words = (uint32_t)(P.slots_alloc_ * (1 + P.aggs_.size()));
    a0.fill_alloc = (uint32_t)P.slots_alloc_;
    P.state_idents(a0.fill_idents);
    fill_rides = true;
  } else {
    P.materialize_state();
  }
  P.trace("before scan");
  pt.mark("parts build");
  const void* d_parts = nullptr;
  if (ptab) {
    std::vector<unsigned long long> table((size_t)n_parts * (size_t)ptab_words);
    jit_pack_parts(part_fields, ptab_words, recs.data(), recs.size(), table.data());
    d_parts = P.upload(table.data(), table.size() * 8);
  } else {
    d_parts = P.upload(parts.data(), parts.size() * sizeof(FdbScanArgs));
  }
  P.ctx_->flush_staging();
  pt.mark("parts upload");
  P.trace("after upload");
  if (pt.on) {
    if (!ptab) for (FdbScanArgs& a : parts) recs.push_back(&a);  // (printed through pointers: no copy of the blocks inside a timed phase)
    std::vector<uint32_t> folded(recs.size(), 0u);
    for (const Narrowed& nw : narrowed)
      if (nw.folded) folded[(size_t)(std::find(live.begin(), live.end(), nw.part) - live.begin())] |= 1u << ((nw.late ? 16 : 0) + nw.k);
    print_dense_launch(jit_fn != nullptr ? "fdb_plan_kernel" : "scan_slots_kernel", shape_key, recs.data(), recs.size(), total_tiles, grid, jit_fn != nullptr ? jit_block : 0, lds.lds_bytes,
                       two_phase, lds.lds_acc, lds.cache_slots, lut_lds_max, per_cu, tile_rows, fill_rides, partials != nullptr, folded, ptab_words);
  }
  P.timed([&] {
    if (ptab) hip_check(jit_launch_ptab(jit_fn, (const unsigned long long*)d_parts, n_parts, total_tiles, a0, grid, jit_block, lds.lds_bytes, P.stream_), "scan launch");
    else if (jit_fn != nullptr) hip_check(jit_launch(jit_fn, (const FdbScanArgs*)d_parts, n_parts, total_tiles, a0, grid, jit_block, lds.lds_bytes, P.stream_), "scan launch");
    else hip_check(fdb_launch_scan_slots((const FdbScanArgs*)d_parts, n_parts, a0, total_tiles, grid, lds.lds_bytes, two_phase, sub, P.stream_), "scan launch");
  });
  if (fill_rides) P.state_virgin_ = false;  // (only once the launch that carries the fill was accepted: a throw above leaves the table marked unfilled)
  P.last_kernel_ = jit_fn != nullptr ? "fdb_plan_kernel" : "scan_slots_kernel";
  pt.mark("scan launch");
  P.trace("after scan");
  fold_partials(partials, grid);
  P.trace("after reduce");
  P.stat_launches += 1;
}

// sequential kernel, one launch per record
void Plan::DenseLaunch::launch_sequential() {
  const int rpt = P.rows_per_thread == 8 ? 8 : 4;
  P.materialize_state();
  P.ctx_->flush_staging();
  for (int i : live) {
    FdbScanArgs& a = args(i);
    if (a.n_expr > 0) throw Error(FDB_ERR_UNSUPPORTED, "computed (projected) columns are not supported by the sequential kernel (too many referenced columns)");
    a.n_c4 = a.n_c8 = 0;
    const int grid = fdb_scan_grid(a, lds.base_grid, rpt);
    a.partials = alloc_partials(grid);
    const FdbScanArgs* one = &a;
    if (pt.on) print_dense_launch("scan_dense_kernel", "", &one, 1, 0, grid, 0, lds.lds_bytes, 0, lds.lds_acc, lds.cache_slots, lut_lds_max, 0, rpt, false, a.partials != nullptr);
    P.timed([&] { hip_check(fdb_launch_scan_dense(a, grid, lds.lds_bytes, rpt, P.stream_), "scan launch"); });
    P.last_kernel_ = "scan_dense_kernel";
    P.mirror_valid_ = false;  // (a launch that flushes with atomics leaves the host copy behind)
    fold_partials(a.partials, grid);
    P.stat_launches += 1;
  }
}

// The dense path of push_batches: the stages in their order. false: the launch was split by shape (choose_kernel).
bool Plan::push_dense(const DeviceBatch* const* bs, std::vector<Resolved>& Rs, std::vector<std::vector<int>>& part_gcols, const std::vector<int>& live, bool fixed_order,
                      PhaseTimer& pt) {
  DenseLaunch D(*this, bs, Rs, part_gcols, live, fixed_order, pt);
  D.bind_group_columns();
  D.stage_luts();
  D.assign_all_slots();
  D.plan_lds();
  D.narrow_slots();
  if (!D.choose_kernel()) return false;
  D.launch();
  return true;
}

}  // namespace fdb
