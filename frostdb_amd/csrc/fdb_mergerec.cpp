// fdb_mergerec.cpp — MergeRecords over records resident in HBM (see fdb_mergerec.h for the semantics and the deviations from the reference).
//
// ≙ arrowutils.MergeRecords. The reference keeps a heap of K cursors on the host and appends row by row through builders; here the
// sorting columns of every input become the Sort's radix keys (fdb_sortkey.h: W unsigned words whose lexicographic order IS the
// comparison), laid word-major with the inputs one after the other — an input's first position rounded up to a multiple of 4 rows, so
// that the key kernel's 16-byte stores stay aligned; word w of position g is at keys[w][g] — with the position as uint32 payload. A
// device pass checks every input's order; then ceil(log2 K) rounds of pairwise merge-path merges (fdb_mergepath.hip) ping-pong the
// (key, position) pairs between two buffers, (r0, r1) → r01, (r2, r3) → r23, …, ties to the left run, so the tree is stable. A run
// without a partner stays where it is for the round; it is copied across (device to device) only if, when its partner comes, the two
// sit in different buffers. With a limit every run — an input's too — is cut to `limit` rows, so no round moves more than K / 2 × limit
// rows. One gather launch then copies every column of the result out of the K inputs through the merged positions: no concatenated copy
// of the inputs is made, neither the keys nor the permutation leaves HBM. What the host does is the plan — the field layout
// (pack_sort_fields, once for all inputs: a column gets a NULL bit if ANY input has a NULL in it, a dictionary column's width comes from
// the union's distinct count), the dictionary unions with their translation and rank tables — and the run bookkeeping of the rounds.
// merge_batches_named is the same plan over a unified field list (unify_merge_schema, fdb_mergerec.h) with a per-input column map: a
// column an input lacks becomes FDB_SORT_ABSENT in that input's key fields and a null FdbMergeSrc::values in the gather — no stand-in
// buffer exists anywhere. OrderedSync (the end of this file) calls it once per round of inputs.
// Like Take and Sort the call borrows a pooled context, runs on its one stream and ends synchronised; all temporaries are the context's.
#include "fdb_mergerec.h"

#include <algorithm>
#include <cstring>

#include "fdb_context.h"
#include "fdb_mergepath.h"
#include "fdb_plan_internal.h"
#include "fdb_sortkey.h"
#include "fdb_take.h"

namespace fdb {

namespace {

struct MergeJob {
  int device = 0;
  uint64_t limit = 0;
  std::vector<const DevColumn*> schema;  // per output column: the field where the call first shows it (name, format, kind; its record may have no rows)
  std::vector<const DeviceBatch*> recs;  // the inputs that have rows, in call order
  std::vector<std::vector<const DevColumn*>> cols;  // [input][output column]; nullptr: the input lacks the column (merge_batches_named)
  std::vector<int32_t> call_index;       // … and their places in the call (error texts)
  std::vector<int64_t> start;            // first position of each, a multiple of 4
  int64_t positions = 0;                 // end of the last one
  std::vector<int> bits;                 // per key word
  std::vector<std::vector<std::vector<FdbSortField>>> fields;  // [input][word][field]; ranks = an OFFSET into `ranks` + 1 until they are on the device
  std::vector<uint32_t> ranks;           // the rank tables of the dictionary sorting columns, back to back
  std::vector<MergeDictPlan> dicts;      // per column of the schema (used for dictionary columns only)
  int words() const { return (int)bits.size(); }
};

void check_devices(const DeviceBatch* const* in, int32_t n) {
  for (int32_t r = 1; r < n; r++)
    if (in[r]->device != in[0]->device) throw Error(FDB_ERR_INVALID, "merge: record " + std::to_string(r) + " lives on a different device than record 0");
}

// The plan over the unified field list `schema`: map[r][c] = where column c sits in record r (-1: the record lacks it), cols[k].index a
// position in `schema`. Everything that is left to refuse before a launch is refused here.
MergeJob plan_merge_columns(const DeviceBatch* const* in, int32_t n, std::vector<const DevColumn*> schema, const std::vector<std::vector<int32_t>>& map, const fdb_sort_col* cols,
                            int32_t n_cols, uint64_t limit) {
  const size_t C = schema.size();
  int64_t total = 0;
  for (int32_t r = 0; r < n; r++) {
    total += in[r]->rows;
    if (total > 0x7FFFFFFFll) throw Error(FDB_ERR_INVALID, "merge: more than 2^31 - 1 rows in total");
  }
  for (int32_t k = 0; k < n_cols; k++) {
    const DevColumn& c = *schema[(size_t)cols[k].index];
    if (c.kind != ColKind::I64 && c.kind != ColKind::U64 && c.kind != ColKind::F64 && c.kind != ColKind::DICT)
      throw Error(FDB_ERR_UNSUPPORTED, "unsupported column type for merging " + c.format + " for column " + c.name);
  }
  MergeJob job;
  job.device = in[0]->device;
  job.limit = limit;
  job.schema = std::move(schema);
  for (int32_t r = 0; r < n; r++) {
    const DeviceBatch& b = *in[r];
    require_values(b, "merge");
    if (b.rows == 0) continue;
    std::vector<const DevColumn*> at(C, nullptr);
    for (size_t c = 0; c < C; c++)
      if (map[(size_t)r][c] >= 0) at[c] = &b.cols[(size_t)map[(size_t)r][c]];
    for (int32_t k = 0; k < n_cols; k++) {
      if (at[(size_t)cols[k].index] == nullptr) continue;
      const DevColumn& c = *at[(size_t)cols[k].index];
      if (c.d_values == nullptr || (c.kind == ColKind::DICT && !c.dict)) throw Error(FDB_ERR_UNSUPPORTED, "unsupported column type for merging " + c.format + " for column " + c.name);
      if (((uintptr_t)c.d_values & 15u) != 0) throw Error(FDB_ERR_UNSUPPORTED, "merge: the values of column " + c.name + " are not 16-byte aligned");
    }
    for (const DevColumn& c : b.cols)
      if (c.kind == ColKind::DICT && !c.dict) throw Error(FDB_ERR_INVALID, "merge: dictionary column without its dictionary: " + c.name);
    job.start.push_back(job.positions);
    job.positions = (int64_t)align_up((size_t)(job.positions + b.rows), 4);
    job.recs.push_back(&b);
    job.cols.push_back(std::move(at));
    job.call_index.push_back(r);
  }
  const size_t R = job.recs.size();
  if (R == 0) return job;
  // the dictionaries: one plan per dictionary column over the inputs that have it; a sorting column's carries the ranks
  std::vector<char> sorts(C, 0);
  for (int32_t k = 0; k < n_cols; k++) sorts[(size_t)cols[k].index] = 1;
  job.dicts.resize(C);
  for (size_t c = 0; c < C; c++) {
    if (job.schema[c]->kind != ColKind::DICT) continue;
    std::vector<std::shared_ptr<HostDict>> ds(R);
    bool any = false;
    for (size_t r = 0; r < R; r++)
      if (job.cols[r][c] != nullptr) { ds[r] = job.cols[r][c]->dict; any = true; }
    if (any) { job.dicts[c] = plan_merge_dict(ds, job.schema[c]->name, sorts[c] != 0); continue; }
    // only records without rows carry the column: it comes out all NULL, with such a record's dictionary
    MergeDictPlan& p = job.dicts[c];
    p.out = job.schema[c]->dict ? job.schema[c]->dict : make_dictionary({}, "z");
    p.tables.assign(R, nullptr);
    if (sorts[c] != 0) p.out_ranks = dense_ranks(*p.out, &p.distinct);
  }
  // the key layout, once for all inputs: a column has its NULL bit when some input has a NULL in it, or lacks it
  std::vector<SortColBits> col_bits((size_t)n_cols);
  for (int32_t k = 0; k < n_cols; k++) {
    const size_t c = (size_t)cols[k].index;
    bool any_null = false;
    for (size_t r = 0; r < R; r++) any_null = any_null || job.cols[r][c] == nullptr || (job.cols[r][c]->null_count != 0 && job.cols[r][c]->d_validity != nullptr);
    col_bits[(size_t)k] = SortColBits{job.schema[c]->kind == ColKind::DICT ? bits_for(job.dicts[c].distinct) : 64, any_null};
  }
  const std::vector<SortPart> parts = pack_sort_fields(col_bits, &job.bits);
  // rank tables: one per (dictionary sorting column, input that has it) — one for all inputs where they share the dictionary
  std::vector<std::vector<size_t>> rank_off((size_t)n_cols, std::vector<size_t>(R, 0)), rank_len = rank_off;
  for (int32_t k = 0; k < n_cols; k++) {
    const size_t c = (size_t)cols[k].index;
    if (job.schema[c]->kind != ColKind::DICT || col_bits[(size_t)k].value_bits == 0) continue;
    const MergeDictPlan& dp = job.dicts[c];
    size_t shared_from = R;  // the input whose table a shared dictionary's other inputs reuse
    for (size_t r = 0; r < R; r++) {
      if (job.cols[r][c] == nullptr) continue;
      if (dp.shared && shared_from < R) { rank_off[(size_t)k][r] = rank_off[(size_t)k][shared_from]; rank_len[(size_t)k][r] = rank_len[(size_t)k][shared_from]; continue; }
      const std::vector<uint32_t> t = dp.ranks_of(r);
      rank_off[(size_t)k][r] = job.ranks.size();
      rank_len[(size_t)k][r] = t.size();
      job.ranks.insert(job.ranks.end(), t.begin(), t.end());
      if (dp.shared) shared_from = r;
    }
  }
  job.fields.assign(R, std::vector<std::vector<FdbSortField>>(job.bits.size()));
  for (size_t r = 0; r < R; r++)
    for (const SortPart& p : parts) {
      const fdb_sort_col& sc = cols[p.col];
      const DevColumn* c = job.cols[r][(size_t)sc.index];
      FdbSortField f;
      std::memset(&f, 0, sizeof(f));
      f.kind = (int32_t)job.schema[(size_t)sc.index]->kind;
      f.width = p.width; f.shift = p.shift; f.null_shift = p.null_shift;
      f.flags = (sc.direction == 1u ? FDB_SORT_DESC : 0u) | (sc.nulls_first != 0u ? FDB_SORT_NULLS_FIRST : 0u);
      if (c == nullptr) {
        f.flags |= FDB_SORT_ABSENT;  // (every row NULL; the kernel loads nothing for this field)
      } else {
        f.values = c->d_values;
        f.validity = col_bits[(size_t)p.col].has_null_bit && c->null_count != 0 ? c->d_validity : nullptr;  // (no NULL in THIS input: every row valid)
        if (c->kind == ColKind::DICT && p.width > 0) {
          f.ranks = (const uint32_t*)(uintptr_t)(rank_off[(size_t)p.col][r] + 1);
          f.rank_len = (uint32_t)std::min<size_t>(rank_len[(size_t)p.col][r], 0xFFFFFFFFu);
        }
      }
      job.fields[r][(size_t)p.word].push_back(f);
    }
  return job;
}

// Everything that can refuse the call before a launch, and the plan. `in` has n >= 1 non-null records.
MergeJob plan_merge(const DeviceBatch* const* in, int32_t n, const fdb_sort_col* cols, int32_t n_cols, uint64_t limit) {
  const DeviceBatch& first = *in[0];
  check_devices(in, n);
  if (n_cols == 0) throw Error(FDB_ERR_INVALID, "merge: at least one column is needed for sorting");
  if (n_cols < 0 || cols == nullptr) throw Error(FDB_ERR_INVALID, "merge: bad column list");
  for (int32_t k = 0; k < n_cols; k++) {
    if (cols[k].index < 0 || (size_t)cols[k].index >= first.cols.size())
      throw Error(FDB_ERR_INVALID, "merge: column index " + std::to_string(cols[k].index) + " outside the record's " + std::to_string(first.cols.size()) + " columns");
    if (cols[k].direction > 1u) throw Error(FDB_ERR_INVALID, "merge: unexpected direction value " + std::to_string(cols[k].direction) + ", only 0 (ascending) and 1 (descending) are allowed");
  }
  for (int32_t r = 0; r < n; r++) {
    const DeviceBatch& b = *in[r];
    if (b.cols.size() != first.cols.size())
      throw Error(FDB_ERR_INVALID, "merge: record " + std::to_string(r) + " has " + std::to_string(b.cols.size()) + " fields, record 0 has " + std::to_string(first.cols.size()));
    for (size_t c = 0; c < b.cols.size(); c++)
      if (b.cols[c].name != first.cols[c].name || b.cols[c].kind != first.cols[c].kind)
        throw Error(FDB_ERR_INVALID, "merge: field " + std::to_string(c) + " of record " + std::to_string(r) + " (" + b.cols[c].name + ", " + b.cols[c].format + ") is not record 0's (" +
                                         first.cols[c].name + ", " + first.cols[c].format + ")");
  }
  std::vector<const DevColumn*> schema;
  std::vector<int32_t> identity;
  for (size_t c = 0; c < first.cols.size(); c++) { schema.push_back(&first.cols[c]); identity.push_back((int32_t)c); }
  return plan_merge_columns(in, n, std::move(schema), std::vector<std::vector<int32_t>>((size_t)n, identity), cols, n_cols, limit);
}

struct Merged { const uint32_t* perm = nullptr; int64_t n = 0; uint32_t* d_error = nullptr; };

// Keys, order check (one host round trip) and the rounds, queued on the scope's stream. `marks` (measurement): an event after the order
// check and one after every round. Takes `job` by value: staging turns its rank offsets into device pointers.
Merged merge_on_device(MergeJob job, CallScope* cs, std::vector<hipEvent_t>* marks) {
  Context* ctx = cs->ctx;
  hipStream_t stream = ctx->stream;
  const size_t R = job.recs.size();
  const int W = job.words();
  const int64_t stride = (int64_t)align_up((size_t)job.positions + 4, 4);
  auto mark = [&] {
    if (marks == nullptr) return;
    hipEvent_t e = ctx->get_event();
    marks->push_back(e);
    hip_check(hipEventRecord(e, stream), "hipEventRecord");
  };
  unsigned long long* keys[2] = {nullptr, nullptr};
  uint32_t* pay[2];
  for (int b = 0; b < 2; b++) {
    if (W > 0) keys[b] = (unsigned long long*)cs->alloc((size_t)W * (size_t)stride * 8 + kTailPad);
    pay[b] = (uint32_t*)cs->alloc((size_t)stride * 4 + kTailPad);
  }
  Merged m;
  m.d_error = (uint32_t*)cs->alloc(256);
  hip_check(hipMemsetAsync(m.d_error, 0, 4, stream), "hipMemsetAsync(merge error word)");
  for (const DeviceBatch* b : job.recs) b->note_reader(stream);
  hip_check(fdb_launch_sort_iota(pay[0], job.positions, stream), "merge iota launch");
  if (W > 0) {
    const uint32_t* d_ranks = nullptr;
    if (!job.ranks.empty()) {
      uint32_t* r = (uint32_t*)cs->alloc(job.ranks.size() * 4 + kTailPad);
      ctx->copy_in(r, job.ranks.data(), job.ranks.size() * 4);
      d_ranks = r;
    }
    std::vector<std::vector<const FdbSortField*>> d_fields(R, std::vector<const FdbSortField*>((size_t)W, nullptr));
    {
      StageScope stage_scope(ctx);  // the descriptors of all inputs and words leave with one copy
      for (size_t r = 0; r < R; r++)
        for (int w = 0; w < W; w++) {
          for (FdbSortField& f : job.fields[r][(size_t)w])
            if (f.ranks != nullptr) f.ranks = d_ranks + ((size_t)(uintptr_t)f.ranks - 1);
          d_fields[r][(size_t)w] = (const FdbSortField*)ctx->stage(job.fields[r][(size_t)w].data(), job.fields[r][(size_t)w].size() * sizeof(FdbSortField));
        }
    }
    uint32_t* d_bad = (uint32_t*)cs->alloc(R * 4 + kTailPad);
    hip_check(hipMemsetAsync(d_bad, 0xFF, R * 4, stream), "hipMemsetAsync(merge order words)");
    for (size_t r = 0; r < R; r++) {
      for (int w = 0; w < W; w++)
        hip_check(fdb_launch_sort_keys(d_fields[r][(size_t)w], (int)job.fields[r][(size_t)w].size(), nullptr, job.recs[r]->rows, keys[0] + (int64_t)w * stride + job.start[r], nullptr, stream),
                  "merge keys launch");
      hip_check(fdb_launch_merge_order(keys[0], stride, W, job.start[r], job.recs[r]->rows, d_bad + r, stream), "merge order launch");
    }
    std::vector<uint32_t> bad(R, 0xFFFFFFFFu);
    hip_check(hipMemcpyAsync(bad.data(), d_bad, R * 4, hipMemcpyDeviceToHost, stream), "hipMemcpyAsync(merge order words)");
    hip_check(hipStreamSynchronize(stream), "hipStreamSynchronize");
    for (size_t r = 0; r < R; r++)
      if (bad[r] != 0xFFFFFFFFu)
        throw Error(FDB_ERR_INVALID, "merge: record " + std::to_string(job.call_index[r]) + " is not ordered by the sorting columns: row " + std::to_string(bad[r]) +
                                         " sorts before row " + std::to_string(bad[r] - 1));
  }
  mark();
  // the rounds
  struct Run { int buf; int64_t off, len; };
  std::vector<Run> runs;
  for (size_t r = 0; r < R; r++) {
    const int64_t rows = job.recs[r]->rows;
    runs.push_back(Run{0, job.start[r], job.limit > 0 && (uint64_t)rows > job.limit ? (int64_t)job.limit : rows});
  }
  const int64_t T = fdb_merge_tile(W);
  uint32_t* splits = runs.size() > 1 ? (uint32_t*)cs->alloc((size_t)(job.positions / T + 2 * (int64_t)R + 4) * 4) : nullptr;
  int cur = 0;
  auto bring = [&](Run& x) {  // a run that sat out a round, into the buffer its partner is in (its positions are free there)
    if (x.buf == cur) return;
    for (int w = 0; w < W; w++)
      hip_check(hipMemcpyAsync(keys[cur] + (int64_t)w * stride + x.off, keys[x.buf] + (int64_t)w * stride + x.off, (size_t)x.len * 8, hipMemcpyDeviceToDevice, stream), "hipMemcpyAsync(merge run)");
    hip_check(hipMemcpyAsync(pay[cur] + x.off, pay[x.buf] + x.off, (size_t)x.len * 4, hipMemcpyDeviceToDevice, stream), "hipMemcpyAsync(merge run)");
    x.buf = cur;
  };
  while (runs.size() > 1) {
    std::vector<FdbMergePair> pairs;
    std::vector<Run> next;
    int64_t tiles = 0;
    for (size_t i = 0; i + 1 < runs.size(); i += 2) {
      bring(runs[i]);
      bring(runs[i + 1]);
      const Run &A = runs[i], &B = runs[i + 1];
      int64_t n_out = A.len + B.len;
      if (job.limit > 0 && (uint64_t)n_out > job.limit) n_out = (int64_t)job.limit;
      pairs.push_back(FdbMergePair{A.off, A.len, B.off, B.len, A.off, n_out, tiles});
      tiles += (n_out + T - 1) / T;
      next.push_back(Run{cur ^ 1, A.off, n_out});
    }
    if (runs.size() & 1) next.push_back(runs.back());
    FdbMergeArgs a;
    std::memset(&a, 0, sizeof(a));
    a.src_keys = keys[cur]; a.dst_keys = keys[cur ^ 1];
    a.src_pay = pay[cur]; a.dst_pay = pay[cur ^ 1];
    a.stride = stride;
    a.pairs = (const FdbMergePair*)ctx->stage(pairs.data(), pairs.size() * sizeof(FdbMergePair));
    a.splits = splits;
    a.error = m.d_error;
    a.n_tiles = tiles;
    a.n_pairs = (int32_t)pairs.size();
    a.words = W;
    hip_check(fdb_launch_merge_round(&a, stream), "merge round launch");
    cur ^= 1;
    runs.swap(next);
    mark();
  }
  m.perm = pay[runs[0].buf] + runs[0].off;
  m.n = runs[0].len;
  return m;
}

// Row perm[i] of the concatenated inputs → row i of a new record of `n` > 0 rows: one launch, one wait.
// A column gets a bitmap when some input has one for it or lacks the column; one that ends without a NULL is emitted without it.
std::unique_ptr<DeviceBatch> gather_merged(const MergeJob& job, CallScope* cs, const Merged& m, hipEvent_t done) {
  Context* ctx = cs->ctx;
  hipStream_t stream = ctx->stream;
  const size_t C = job.schema.size(), R = job.recs.size();
  const int64_t n = m.n;
  RecordBuilder out(job.device, n);
  DrainOnUnwind drain{stream};  // (after `out`: its arena outlives the queued kernel)
  for (size_t c = 0; c < C; c++) {
    const DevColumn& src = *job.schema[c];
    bool any_validity = false;
    for (size_t r = 0; r < R; r++) any_validity = any_validity || job.cols[r][c] == nullptr || job.cols[r][c]->d_validity != nullptr;
    out.add(src.name, src.format, src.kind, src.kind == ColKind::DICT ? job.dicts[c].out : src.dict, any_validity);
  }
  out.allocate();
  std::vector<FdbMergeCol> mc(C);
  std::vector<FdbMergeSrc> ms(C * R);
  std::vector<FdbMergeInput> mi(R);
  for (size_t r = 0; r < R; r++) mi[r] = FdbMergeInput{(uint32_t)job.start[r], (uint32_t)job.recs[r]->rows};
  std::vector<unsigned long long> h_nulls(C, 0);
  uint32_t h_error = 0;
  if (C > 0) {
    unsigned long long* d_nulls = (unsigned long long*)cs->alloc(C * 8 + kTailPad);
    hip_check(hipMemsetAsync(d_nulls, 0, C * 8, stream), "hipMemsetAsync(null counts)");
    const FdbMergeCol* d_cols;
    const FdbMergeSrc* d_srcs;
    const FdbMergeInput* d_inputs;
    {
      StageScope stage_scope(ctx);  // the translation tables and the descriptors leave with one copy
      for (size_t c = 0; c < C; c++) {
        std::memset(&mc[c], 0, sizeof(FdbMergeCol));
        mc[c].dst = out.values(c);
        mc[c].dst_valid = out.validity(c);
        mc[c].width = (int32_t)value_width(job.schema[c]->kind);
        for (size_t r = 0; r < R; r++) {
          FdbMergeSrc& s = ms[c * R + r];
          std::memset(&s, 0, sizeof(s));
          if (job.cols[r][c] == nullptr) { mc[c].lacking = 1; continue; }  // values == nullptr, the gather's ABSENT marker: its rows leave as NULL, nothing is read
          const DevColumn& col = *job.cols[r][c];
          s.values = col.d_values;
          s.validity = col.d_validity;
          if (col.kind == ColKind::DICT && !job.dicts[c].shared && job.dicts[c].tables[r] && !job.dicts[c].tables[r]->empty()) {  // (an empty dictionary: every row NULL)
            const std::vector<uint32_t>& t = *job.dicts[c].tables[r];
            s.table = (const uint32_t*)ctx->stage(t.data(), t.size() * 4);
            s.table_len = (uint32_t)std::min<size_t>(t.size(), 0xFFFFFFFFu);
          }
        }
      }
      d_cols = (const FdbMergeCol*)ctx->stage(mc.data(), mc.size() * sizeof(FdbMergeCol));
      d_srcs = (const FdbMergeSrc*)ctx->stage(ms.data(), ms.size() * sizeof(FdbMergeSrc));
      d_inputs = (const FdbMergeInput*)ctx->stage(mi.data(), mi.size() * sizeof(FdbMergeInput));
    }
    hip_check(fdb_launch_merge_gather(d_cols, (int)C, d_srcs, d_inputs, (int)R, m.perm, n, d_nulls, stream), "merge gather launch");
    if (done != nullptr) hip_check(hipEventRecord(done, stream), "hipEventRecord");
    hip_check(hipMemcpyAsync(h_nulls.data(), d_nulls, C * 8, hipMemcpyDeviceToHost, stream), "hipMemcpyAsync(null counts)");
  }
  hip_check(hipMemcpyAsync(&h_error, m.d_error, 4, hipMemcpyDeviceToHost, stream), "hipMemcpyAsync(merge error word)");
  hip_check(hipStreamSynchronize(stream), "hipStreamSynchronize");
  if (h_error != 0) throw Error(FDB_ERR_STATE, "merge: a tile's split points crossed (the inputs passed the order check: this is a bug)");
  return out.finish(h_nulls.data());
}

void check_records(const DeviceBatch* const* in, int32_t n) {
  if (n <= 0 || in == nullptr) throw Error(FDB_ERR_INVALID, "merge: at least one record is needed");
  for (int32_t r = 0; r < n; r++)
    if (in[r] == nullptr) throw Error(FDB_ERR_INVALID, "merge: record " + std::to_string(r) + " is null");
}

std::vector<MergeOrder> check_order(const fdb_order_col* order, int32_t n_order) {
  if (order == nullptr || n_order <= 0) throw Error(FDB_ERR_INVALID, "merge: at least one order expression is needed");
  std::vector<MergeOrder> exprs;
  for (int32_t k = 0; k < n_order; k++) {
    if (order[k].name == nullptr) throw Error(FDB_ERR_INVALID, "merge: order expression " + std::to_string(k) + " has no name");
    if (order[k].direction > 1u) throw Error(FDB_ERR_INVALID, "merge: unexpected direction value " + std::to_string(order[k].direction) + ", only 0 (ascending) and 1 (descending) are allowed");
    exprs.push_back(MergeOrder{order[k].name, order[k].dynamic != 0});
  }
  return exprs;
}

}  // namespace

std::unique_ptr<DeviceBatch> merge_batches(const DeviceBatch* const* in, int32_t n, const fdb_sort_col* cols, int32_t n_cols, uint64_t limit) {
  check_records(in, n);
  MergeJob job = plan_merge(in, n, cols, n_cols, limit);
  if (job.recs.empty()) return limit_batch(*in[0], 0);                   // no rows at all: the schema
  if (n == 1) return limit_batch(*in[0], limit > 0 ? limit : ~0ull);     // nothing to merge with
  CallScope cs(job.device);
  DrainOnUnwind drain{cs.ctx->stream};
  const Merged m = merge_on_device(job, &cs, nullptr);
  return gather_merged(job, &cs, m, nullptr);
}

std::unique_ptr<DeviceBatch> merge_batches_named(const DeviceBatch* const* in, int32_t n, const fdb_order_col* order, int32_t n_order, uint64_t limit) {
  check_records(in, n);
  check_devices(in, n);
  const std::vector<MergeOrder> exprs = check_order(order, n_order);
  std::vector<std::vector<MergeField>> lists((size_t)n);
  for (int32_t r = 0; r < n; r++)
    for (const DevColumn& c : in[r]->cols) lists[(size_t)r].push_back(MergeField{c.name, (int32_t)c.kind});
  const MergeSchema u = unify_merge_schema(lists, exprs);
  std::vector<const DevColumn*> schema;
  for (const MergeSchema::At& at : u.first) schema.push_back(&in[at.record]->cols[(size_t)at.field]);
  std::vector<fdb_sort_col> cols;
  if (n > 1)  // (a single record's order is not looked at: no key)
    for (size_t k = 0; k < u.sort_expr.size(); k++) cols.push_back(fdb_sort_col{(int32_t)k, order[u.sort_expr[k]].direction, order[u.sort_expr[k]].nulls_first});
  MergeJob job = plan_merge_columns(in, n, schema, u.map, cols.data(), (int32_t)cols.size(), limit);
  if (job.recs.empty()) {  // no rows at all: the unified schema
    RecordBuilder out(job.device, 0);
    for (const DevColumn* c : schema) out.add(c->name, c->format, c->kind, c->kind == ColKind::DICT && !c->dict ? make_dictionary({}, "z") : c->dict, false);
    return out.finish(nullptr);
  }
  CallScope cs(job.device);
  DrainOnUnwind drain{cs.ctx->stream};
  const Merged m = merge_on_device(job, &cs, nullptr);
  return gather_merged(job, &cs, m, nullptr);
}

// ---- OrderedSync -----------------------------------------------------------------------------------------------------------------------------
OrderedSync::OrderedSync(int32_t inputs, const fdb_order_col* order, int32_t n_order) {
  if (inputs <= 0) throw Error(FDB_ERR_INVALID, "ordered synchronizer: at least one input is needed");
  for (const MergeOrder& o : check_order(order, n_order)) names_.push_back(o.name);
  order_.assign(order, order + n_order);
  for (size_t k = 0; k < order_.size(); k++) order_[k].name = names_[k].c_str();  // (names_ is not touched again)
  parked_.assign((size_t)inputs, nullptr);
  finished_.assign((size_t)inputs, 0);
  running_ = inputs;
}

void OrderedSync::check_input(int32_t input) const {
  if (input < 0 || (size_t)input >= parked_.size()) throw Error(FDB_ERR_INVALID, "ordered synchronizer: input " + std::to_string(input) + " outside the " + std::to_string(parked_.size()) + " inputs");
}

std::unique_ptr<DeviceBatch> OrderedSync::merge_round() {
  std::vector<const DeviceBatch*> recs;
  for (const DeviceBatch* b : parked_)
    if (b != nullptr) recs.push_back(b);
  std::fill(parked_.begin(), parked_.end(), nullptr);  // (whatever the merge answers: the round is over)
  waiting_ = 0;
  return merge_batches_named(recs.data(), (int32_t)recs.size(), order_.data(), (int32_t)order_.size(), 0);
}

std::unique_ptr<DeviceBatch> OrderedSync::push(int32_t input, const DeviceBatch* batch) {
  if (batch == nullptr) throw Error(FDB_ERR_INVALID, "null argument");
  std::lock_guard<std::mutex> lock(mu_);
  check_input(input);
  if (finished_[(size_t)input]) throw Error(FDB_ERR_STATE, "ordered synchronizer: input " + std::to_string(input) + " has finished");
  if (parked_[(size_t)input] != nullptr) throw Error(FDB_ERR_STATE, "ordered synchronizer: input " + std::to_string(input) + " already waits in this round");
  parked_[(size_t)input] = batch;
  waiting_++;
  if (waiting_ != running_) return nullptr;
  return merge_round();  // this is the last input of the round (ordered_synchronizer.go:76-88)
}

std::unique_ptr<DeviceBatch> OrderedSync::finish(int32_t input, bool* done) {
  std::lock_guard<std::mutex> lock(mu_);
  if (done != nullptr) *done = false;
  check_input(input);
  if (running_ == 0) throw Error(FDB_ERR_STATE, "too many OrderedSynchronizer Finish calls");
  if (finished_[(size_t)input]) throw Error(FDB_ERR_STATE, "ordered synchronizer: input " + std::to_string(input) + " has already finished");
  if (parked_[(size_t)input] != nullptr) throw Error(FDB_ERR_STATE, "ordered synchronizer: input " + std::to_string(input) + " waits in this round and cannot finish before it is merged");
  finished_[(size_t)input] = 1;
  running_--;
  if (done != nullptr) *done = running_ == 0;
  if (running_ > 0 && running_ == waiting_) return merge_round();  // everyone else waits (:96-104)
  return nullptr;
}

void merge_bench(const DeviceBatch* const* in, int32_t n, const fdb_sort_col* cols, int32_t n_cols, int32_t reps, int32_t warmup, double* merge_ms, double* gather_ms,
                 double* round_ms, int32_t round_cap, int32_t* n_rounds, int32_t* words) {
  check_records(in, n);
  if (reps < 1 || warmup < 0 || merge_ms == nullptr || gather_ms == nullptr || round_cap < 0 || (round_cap > 0 && round_ms == nullptr)) throw Error(FDB_ERR_INVALID, "merge bench: bad arguments");
  const MergeJob job = plan_merge(in, n, cols, n_cols, 0);
  if (job.recs.size() < 2) throw Error(FDB_ERR_INVALID, "merge bench: at least two records with rows are needed");
  if (words != nullptr) *words = job.words();
  auto median = [](std::vector<float> v) { std::sort(v.begin(), v.end()); return (double)v[v.size() / 2]; };
  std::vector<float> t_merge, t_gather;
  std::vector<std::vector<float>> t_round;
  for (int32_t r = 0; r < warmup + reps; r++) {
    CallScope cs(job.device);
    Context* ctx = cs.ctx;
    std::vector<hipEvent_t> marks;
    struct PutBack { Context* c; std::vector<hipEvent_t>* v; ~PutBack() { for (hipEvent_t e : *v) c->put_event(e); } } put_back{ctx, &marks};
    DrainOnUnwind drain{ctx->stream};
    hipEvent_t e0 = ctx->get_event();
    marks.push_back(e0);
    hip_check(hipEventRecord(e0, ctx->stream), "hipEventRecord");
    const Merged m = merge_on_device(job, &cs, &marks);
    hipEvent_t e_done = ctx->get_event();
    marks.push_back(e_done);
    std::unique_ptr<DeviceBatch> out = gather_merged(job, &cs, m, e_done);  // (ends synchronised)
    // marks: [start, after the order check, after round 0, …, after the gather]
    const size_t rounds = marks.size() - 3;
    float t = 0;
    if (r < warmup) continue;
    hip_check(hipEventElapsedTime(&t, marks[0], marks[marks.size() - 2]), "hipEventElapsedTime");
    t_merge.push_back(t);
    hip_check(hipEventElapsedTime(&t, marks[marks.size() - 2], marks[marks.size() - 1]), "hipEventElapsedTime");
    t_gather.push_back(t);
    t_round.resize(rounds);
    for (size_t k = 0; k < rounds; k++) {
      hip_check(hipEventElapsedTime(&t, marks[1 + k], marks[2 + k]), "hipEventElapsedTime");
      t_round[k].push_back(t);
    }
  }
  *merge_ms = median(t_merge);
  *gather_ms = median(t_gather);
  if (n_rounds != nullptr) *n_rounds = (int32_t)t_round.size();
  for (size_t k = 0; k < t_round.size() && k < (size_t)round_cap; k++) round_ms[k] = median(t_round[k]);
}

}  // namespace fdb
