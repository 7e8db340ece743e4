// fdb_project.cpp — the Projection operator of the plan (see fdb_plan.h): selected and computed columns of a record resident in HBM,
// of every record of a scan at once, and of a host record.
//
// ≙ Projection.Project (project.go:906-943): every item of the output list is expanded against the record's fields — plainProjection
// (:481-491, the first field of that name; a record without it contributes nothing), dynamicProjection (:742-755, every field under
// the prefix, in field order), allProjection, and the computed ones (binaryExprProjection :73-161, boolExprProjection :401-470,
// convertProjection :493-556, isNullProjection :558-601, ifExprProjection :603-702, literalProjection :716-728, aliasProjection
// :40-56), which are the plan's projections[]. Pass-through fields are copied device to device into the output's own arena; ALL
// computed fields of ALL records of the call are evaluated by ONE launch of a kernel generated for the expressions' shape
// (fdb_project_kernel, fdb_jitgen.cpp). Not carried over: boolExprProjection's shortcut for a result column a table scan pre-computed
// (:411-432) — no scan on this path produces one.
#include "fdb_plan.h"
#include "fdb_jit.h"

#include "fdb_context.h"
#include "fdb_plan_internal.h"

#include <algorithm>
#include <cstring>
#include <functional>

namespace fdb {

namespace {
struct Field { int src = -1; const Projection* proj = nullptr; };  // one output field: a column of the record, or a computed one

// The output list of one record (project.go:906-943).
template <typename F>
std::vector<Field> expand_items(const fdb_project_col* cols, int n_cols, const DeviceBatch& b, F find_proj) {
  std::vector<Field> out;
  for (int i = 0; i < n_cols; i++) {
    const fdb_project_col& it = cols[i];
    if (it.kind != 3 && it.name == nullptr) throw Error(FDB_ERR_INVALID, "projection item without a name");
    if (it.kind == 0) {
      for (size_t c = 0; c < b.cols.size(); c++) if (b.cols[c].name == it.name) { out.push_back(Field{(int)c, nullptr}); break; }
    } else if (it.kind == 1) {
      const std::string prefix = std::string(it.name) + ".";
      for (size_t c = 0; c < b.cols.size(); c++) if (b.cols[c].name.compare(0, prefix.size(), prefix) == 0) out.push_back(Field{(int)c, nullptr});
    } else if (it.kind == 2) {
      const Projection* p = find_proj(it.name);
      if (p == nullptr) throw Error(FDB_ERR_INVALID, std::string("projection item names no projection of the plan: ") + it.name);
      out.push_back(Field{-1, p});
    } else if (it.kind == 3) {
      for (size_t c = 0; c < b.cols.size(); c++) out.push_back(Field{(int)c, nullptr});
    } else {
      throw Error(FDB_ERR_INVALID, "unknown projection item kind");
    }
  }
  return out;
}
}  // namespace

// ≙ Projection.Callback for `n` resident records at once. Three steps: (1) per record, the output list, the expressions' argument
// block (resolve_projection: types, slots, truth tables) and the output arena; (2) pass-through copies and ONE launch for every
// computed field of every record; (3) one wait, the NULL counts, the column descriptors. All or nothing.
std::vector<std::unique_ptr<DeviceBatch>> Plan::project_batches(const fdb_project_col* cols, int n_cols, const DeviceBatch* const* in, int n) {
  if (n_cols < 0 || (n_cols > 0 && cols == nullptr)) throw Error(FDB_ERR_INVALID, "projection items missing");
  for (int i = 0; i < n; i++)
    if (in[i]->device != device_) throw Error(FDB_ERR_INVALID, "batch lives on a different device than the plan");
  hip_check(hipSetDevice(device_), "hipSetDevice");
  std::vector<std::unique_ptr<DeviceBatch>> out;
  std::vector<RecordBuilder> outs;  // one per record, finished into `out` in step (3)
  DrainOnUnwind drain{stream_};  // (after `out` and `outs`: their arenas, and the inputs the caller may release, outlive the queued copies and the kernel)
  auto find_proj = [this](const std::string& name) { return find_projection(name); };

  struct Rec {
    std::vector<Field> fields;
    std::vector<int> computed;      // indices into `fields`
    std::vector<int> roots;         // root node of each computed field (in R.args.expr)
    Resolved R;
    int64_t rows = 0;               // of the output: a record that contributes no field contributes no row
    int part = -1;                  // index among the launch's argument blocks
  };
  std::vector<Rec> recs((size_t)n);
  bool any_computed = false;
  for (int i = 0; i < n; i++) {
    const DeviceBatch& b = *in[i];
    Rec& r = recs[(size_t)i];
    r.fields = expand_items(cols, n_cols, b, find_proj);
    resolve_predicate(b, -1, &r.R);  // (fresh arguments, no filter program)
    std::vector<std::pair<const Projection*, int>> done;  // an expression named twice is evaluated once per output field, resolved once
    for (size_t f = 0; f < r.fields.size(); f++) {
      const Field& F = r.fields[f];
      if (F.proj == nullptr) {
        const DevColumn& c = b.cols[(size_t)F.src];
        if (c.d_values == nullptr && b.rows > 0)
          throw Error(FDB_ERR_UNSUPPORTED, "projection: column type " + c.format + " (" + c.name + ") is not supported on the device path");
        continue;
      }
      int root = -1;
      for (const auto& d : done) if (d.first == F.proj) root = d.second;
      if (root < 0) { root = resolve_projection(*F.proj, b, &r.R); done.emplace_back(F.proj, root); }
      const int32_t kind = r.R.args.expr[root].kind;
      if (kind == 8) throw Error(FDB_ERR_UNSUPPORTED, "projection " + F.proj->name + ": not a value");
      r.computed.push_back((int)f);
      r.roots.push_back(root);
    }
    if (r.computed.size() > FDB_PROJECT_MAX_OUT) throw Error(FDB_ERR_UNSUPPORTED, "projection: more than " + std::to_string(FDB_PROJECT_MAX_OUT) + " computed columns in one call");
    any_computed = any_computed || !r.computed.empty();
  }
  if (any_computed && !jit_possible())
    throw Error(FDB_ERR_UNSUPPORTED, "computed (projected) columns need the run-time specialised kernel (hiprtc unavailable or disabled)");

  // (1) outputs: [values of every field | bitmaps], sized exactly, padded like every resident column (tail lanes over-read / over-write)
  auto may_null = [](const Rec& r, const DeviceBatch& b, size_t k) {  // computed field k of the record can carry NULLs
    const FdbExprNode& e = r.R.args.expr[r.roots[k]];
    if (e.kind == 0) return b.cols[(size_t)r.R.expr_col[r.roots[k]]].d_validity != nullptr;  // an aliased column keeps its NULLs
    return e.kind == 2 && e.op == FDB_OP_DIV;
  };
  for (int i = 0; i < n; i++) {
    const DeviceBatch& b = *in[i];
    Rec& r = recs[(size_t)i];
    r.rows = r.fields.empty() ? 0 : b.rows;
    RecordBuilder o(device_, r.rows);
    size_t k = 0;
    for (const Field& F : r.fields) {
      if (F.proj == nullptr) {
        const DevColumn& c = b.cols[(size_t)F.src];
        o.add(c.name, c.format, c.kind, c.dict, c.d_validity != nullptr);
      } else {
        const int32_t t = r.R.args.expr[r.roots[k]].type;
        o.add(F.proj->name, t == FDB_T_I64 ? "l" : t == FDB_T_U64 ? "L" : t == FDB_T_F64 ? "g" : "b",
              t == FDB_T_I64 ? ColKind::I64 : t == FDB_T_U64 ? ColKind::U64 : t == FDB_T_F64 ? ColKind::F64 : ColKind::BOOL, nullptr, may_null(r, b, k));
        k++;
      }
    }
    o.allocate();
    outs.push_back(std::move(o));
  }

  // (2) pass-through fields: bit for bit, into the output's own arena (its lifetime does not depend on the input's)
  for (int i = 0; i < n; i++) in[i]->note_reader(stream_);
  int64_t copied = 0;
  for (int i = 0; i < n; i++) {
    const DeviceBatch& b = *in[i];
    Rec& r = recs[(size_t)i];
    const RecordBuilder& o = outs[(size_t)i];
    if (r.rows == 0) continue;
    for (size_t f = 0; f < r.fields.size(); f++) {
      if (r.fields[f].proj != nullptr) continue;
      const DevColumn& c = b.cols[(size_t)r.fields[f].src];
      const size_t vb = (size_t)r.rows * value_width(c.kind), bb = ((size_t)r.rows + 7) / 8;
      hip_check(hipMemcpyAsync(o.values(f), c.d_values, vb, hipMemcpyDeviceToDevice, stream_), "hipMemcpyAsync(projected column)");
      if (c.d_validity != nullptr) hip_check(hipMemcpyAsync(o.validity(f), c.d_validity, bb, hipMemcpyDeviceToDevice, stream_), "hipMemcpyAsync(projected validity)");
      copied += 2 * (int64_t)(vb + (c.d_validity != nullptr ? bb : 0));
    }
  }

  // computed fields: one argument block per record that has rows, one launch
  std::vector<int> live;
  for (int i = 0; i < n; i++) if (recs[(size_t)i].rows > 0 && !recs[(size_t)i].computed.empty()) live.push_back(i);
  std::vector<unsigned long long> h_nulls;
  if (!live.empty()) {
    std::vector<FdbScanArgs> parts;
    std::vector<FdbProjectPart> oparts;
    LutClasses luts;
    for (int i : live) luts.add(recs[(size_t)i].R);
    JitShape shape;
    size_t lut_lds_max = 0;
    int64_t total_tiles = 0;
    const FdbScanArgs* d_parts = nullptr;
    const FdbProjectPart* d_oparts = nullptr;
    {
      StageScope stage_scope(ctx_);
      unsigned char* d_blob = luts.blob.bytes.empty() ? nullptr : (unsigned char*)upload(luts.blob.bytes.data(), luts.blob.bytes.size());
      for (size_t k = 0; k < live.size(); k++) {
        const DeviceBatch& b = *in[live[k]];
        Rec& r = recs[(size_t)live[k]];
        FdbScanArgs& a = r.R.args;
        lut_lds_max = std::max(lut_lds_max, luts.place(k, d_blob, r.R));
        // leaves of string comparisons in the early pools, the expressions' columns in the late 8-byte pool: a column several
        // expressions reference has ONE slot and is loaded once
        if (assign_slots(b, r.R, 2, /*relaxed=*/true) != 2) throw Error(FDB_ERR_UNSUPPORTED, "projection: the expressions reference more columns than the kernel has slots");
        if (k == 0) { shape = jit_shape(a, true, 256); shape.proj_roots = r.roots; }
        else if (r.roots != shape.proj_roots || !jit_shape_merge_args(&shape, recs[(size_t)live[0]].R.args, a, true))
          throw Error(FDB_ERR_UNSUPPORTED, "projection: the records of one call must share their expressions' column types");
        a.tile_begin = total_tiles;
        total_tiles += (a.n_rows + FDB_PROJECT_TILE - 1) / FDB_PROJECT_TILE;
        a.tile_end = total_tiles;
        r.part = (int)k;
        FdbProjectPart op;
        std::memset(&op, 0, sizeof(op));
        const RecordBuilder& o = outs[(size_t)live[k]];
        for (size_t c = 0; c < r.computed.size(); c++) {
          op.out[c].values = o.values((size_t)r.computed[c]);
          op.out[c].validity = o.validity((size_t)r.computed[c]);
        }
        oparts.push_back(op);
      }
      for (size_t k = 0; k < live.size(); k++) { recs[(size_t)live[k]].R.args.lds_lut_bytes = (uint32_t)lut_lds_max; parts.push_back(recs[(size_t)live[k]].R.args); }
      d_parts = (const FdbScanArgs*)upload(parts.data(), parts.size() * sizeof(FdbScanArgs));
      d_oparts = (const FdbProjectPart*)upload(oparts.data(), oparts.size() * sizeof(FdbProjectPart));
    }
    hipFunction_t fn = jit_project_get(shape);
    if (fn == nullptr) throw Error(FDB_ERR_UNSUPPORTED, "computed (projected) columns need the run-time specialised kernel (hiprtc unavailable or disabled)");
    h_nulls.assign(live.size() * FDB_PROJECT_MAX_OUT, 0);
    unsigned long long* d_nulls = (unsigned long long*)ctx_->dev_alloc(h_nulls.size() * 8);
    scratch_.push_back(d_nulls);
    hip_check(hipMemsetAsync(d_nulls, 0, h_nulls.size() * 8, stream_), "hipMemsetAsync(null counts)");
    // ≈64 KB of loads in flight per CU (jit_select's figure): a lane requests 4 rows of every referenced column per tile
    int row_bytes = 0;
    for (int k = 0; k < shape.n_c4; k++) row_bytes += shape.c4[k].has_values ? 4 : 0;
    for (int k = 0; k < shape.n_c8; k++) row_bytes += shape.c8[k].has_values ? 8 : 0;
    for (int k = 0; k < shape.n_l8; k++) row_bytes += shape.l8[k].has_values ? 8 : 0;
    const int waves = std::max(8, std::min(32, row_bytes > 0 ? 256 / row_bytes : 16));
    const int per_cu = std::max(1, std::min(jit_blocks_per_cu(fn, 256, lut_lds_max), waves / 4));
    int64_t grid = (int64_t)(fdb_scan_default_grid(device_) / 2) * per_cu;
    if (grid_override > 0) grid = grid_override;
    grid = std::max<int64_t>(1, std::min(grid, total_tiles));
    timed([&] { hip_check(jit_project_launch(fn, d_parts, (int)parts.size(), total_tiles, (int)grid, lut_lds_max, d_oparts, d_nulls, stream_), "project launch"); });
    hip_check(hipMemcpyAsync(h_nulls.data(), d_nulls, h_nulls.size() * 8, hipMemcpyDeviceToHost, stream_), "hipMemcpyAsync(null counts)");
    last_kernel_ = "fdb_project_kernel";
    stat_launches += 1;
  }

  // (3) one wait (timing events read, scratch back to the context); a field without NULLs is emitted without a bitmap
  sync();
  for (int i = 0; i < n; i++) {
    const DeviceBatch& b = *in[i];
    Rec& r = recs[(size_t)i];
    if (!r.fields.empty()) { stat_rows += b.rows; stat_bytes += r.R.bytes; }
    std::vector<unsigned long long> nulls;
    size_t k = 0;
    for (const Field& F : r.fields) {
      if (F.proj == nullptr) nulls.push_back((unsigned long long)b.cols[(size_t)F.src].null_count);
      else { nulls.push_back(r.part >= 0 ? h_nulls[(size_t)r.part * FDB_PROJECT_MAX_OUT + k] : 0); k++; }
    }
    out.push_back(outs[(size_t)i].finish(nulls.data()));
    for (int f : r.computed) stat_bytes += r.rows * 8 + out.back()->cols[(size_t)f].validity_bytes;
  }
  stat_bytes += copied;
  return out;
}

std::unique_ptr<DeviceBatch> Plan::project_batch(const fdb_project_col* cols, int n_cols, const DeviceBatch& in) {
  const DeviceBatch* p = &in;
  std::vector<std::unique_ptr<DeviceBatch>> out = project_batches(cols, n_cols, &p, 1);
  return std::move(out[0]);
}

// Host record in, host record out: the columns the items pass through or the plan's projections read are staged (the caller's buffers
// are only borrowed), then the resident path, then the export.
void Plan::project(const fdb_project_col* cols, int n_cols, const ArrowArray* array, const ArrowSchema* schema, ArrowArray* out, ArrowSchema* out_schema) {
  if (n_cols < 0 || (n_cols > 0 && cols == nullptr)) throw Error(FDB_ERR_INVALID, "projection items missing");
  HostRecordView view;
  view_record(array, schema, &view);
  std::function<bool(const std::string&)> want = [&](const std::string& name) {
    for (int i = 0; i < n_cols; i++) {
      const fdb_project_col& it = cols[i];
      if (it.kind == 3) return true;
      if (it.name == nullptr) continue;
      if (it.kind == 0 && name == it.name) return true;
      if (it.kind == 1 && name.compare(0, std::strlen(it.name) + 1, std::string(it.name) + ".") == 0) return true;
      if (it.kind == 2)
        if (const Projection* p = find_projection(it.name))
          for (const ProjNode& nd : p->nodes) if (nd.kind == 0 && nd.column == name) return true;
    }
    return false;
  };
  std::unique_ptr<DeviceBatch> b = import_batch(view, device_, &want, stream_);
  std::unique_ptr<DeviceBatch> p = project_batch(cols, n_cols, *b);
  export_batch(*p, out, out_schema);
}

}  // namespace fdb
