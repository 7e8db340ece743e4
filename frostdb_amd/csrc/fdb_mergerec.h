// fdb_mergerec.h — MergeRecords over records resident in HBM (fdb_mergerec.cpp; kernels in fdb_mergepath.hip, merge-path arithmetic in
// fdb_mergepath.h, key encoding in fdb_sortkey.h).
//
// ≙ arrowutils.MergeRecords (pqarrow/arrowutils/merge.go:23-68), what OrderedSynchronizer.mergeRecordsLocked and OrderedAggregate run
// wherever several ordered streams meet: K >= 1 records of one schema, each already ordered by the same sorting columns, become ONE new
// resident record holding all their rows in that order, cut to `limit` rows when limit > 0. The result is the STABLE sort of the
// concatenation records[0] ‖ records[1] ‖ … under the Sort's comparison (fdb_sort.h): rows equal on every sorting column come out in
// record order, inside a record in row order — container/heap promises no order of ties, so this is one of the legal orders, always the
// same one. Where this differs from the reference:
//   both rows NULL in a column   cursorHeap.Less returns false without a look at the later columns (merge.go:91-98); here the next column
//                                decides, as in the Sort.
//   float64 sorting columns      the reference panics (merge.go:169-171); here they compare as Go's cmp.Compare (the Sort's encoding).
//   descending order             the reference's comment says "only ascending", its own TestMerge vectors merge descending and mixed
//                                orders; both directions are supported.
//   dictionaries                 may differ between the inputs: entries compare by their bytes (rank tables over the union of the
//                                entries), the output column carries the union in first-seen order; when every input shares one
//                                dictionary's content nothing is translated and that dictionary is the output's.
//   unordered inputs             the reference does not look; here a device pass over each input's keys checks key[i - 1] <= key[i]
//                                before any merge launch, and an unordered input is FDB_ERR_INVALID naming the record and the first
//                                offending row (a merge-path partition over unordered keys could return crossing splits).
// merge_batches wants equal field lists. merge_batches_named takes records whose field lists differ (≙ OrderedSynchronizer.ensureSameSchema,
// ordered_synchronizer.go:143-241): the sorting columns are named by order expressions, the output has the union of the fields
// (unify_merge_schema below), and where the reference hands MergeRecords a virtual NULL column for a field a record lacks, here the key
// kernel and the gather get an ABSENT marker for that (input, column) — nothing is allocated, filled or read for it. OrderedSync is the
// operator on top (≙ OrderedSynchronizer.Callback / Finish, :59-137, without the blocking): one merge per round of inputs.
//
// The first half of this header is host-only (no device, no HIP): the dictionary plan of one column across the inputs with the per-input
// rank tables, and the schema union with the per-input column map. tools/asan_merge.sh runs it under AddressSanitizer with
// FDB_MERGEREC_HOST_ONLY defined.
#pragma once

#include <algorithm>
#include <memory>
#include <string>
#include <vector>

#include "fdb_reservoir.h"
#include "fdb_sortplan.h"

namespace fdb {

// One dictionary column across the inputs. dicts[r] == nullptr: input r takes no part (it has no rows).
struct MergeDictPlan {
  std::shared_ptr<HostDict> out;  // the output column's dictionary: the shared one, or the union in first-seen order
  bool shared = true;             // every input's dictionary has the same content: no translation
  std::vector<std::shared_ptr<const std::vector<uint32_t>>> tables;  // [input] entry → entry of `out`; all null when shared
  std::vector<uint32_t> out_ranks;  // dense byte-order rank of every entry of `out`
  uint32_t distinct = 0;
  // entry of input r → rank: what the key kernel reads
  std::vector<uint32_t> ranks_of(size_t r) const {
    if (shared || !tables[r]) return out_ranks;
    std::vector<uint32_t> v(tables[r]->size());
    for (size_t i = 0; i < v.size(); i++) v[i] = (*tables[r])[i] < out_ranks.size() ? out_ranks[(*tables[r])[i]] : 0u;
    return v;
  }
};

// Throws FDB_ERR_UNSUPPORTED when the field is utf8 in one input and binary in another, or plain in one and a dictionary in another
// (DictUnion::check_type); FDB_ERR_INVALID when no input takes part.
inline MergeDictPlan plan_merge_dict(const std::vector<std::shared_ptr<HostDict>>& dicts, const std::string& field, bool want_ranks) {
  MergeDictPlan p;
  p.tables.assign(dicts.size(), nullptr);
  std::shared_ptr<HostDict> first;
  for (const auto& d : dicts) {
    if (!d) continue;
    if (!first) { first = d; continue; }
    if (d.get() != first.get() && !first->same_content(*d)) p.shared = false;
    if (first->utf8() != d->utf8() || first->plain != d->plain) p.shared = false;  // (refused below, by the union)
  }
  if (!first) throw Error(FDB_ERR_INVALID, "merge: dictionary column without its dictionary: " + field);
  if (p.shared) {
    p.out = first;
  } else {
    DictUnion u;
    for (size_t r = 0; r < dicts.size(); r++)
      if (dicts[r]) p.tables[r] = u.table_for(dicts[r], field);
    std::vector<std::string> values = u.values();
    p.out = u.plain() ? make_plain_dictionary(std::move(values), u.value_format()) : make_dictionary(std::move(values), u.utf8() ? "u" : "z");
  }
  if (want_ranks) p.out_ranks = dense_ranks(*p.out, &p.distinct);
  return p;
}

// ---- the unified schema of records whose field lists differ (≙ ensureSameSchema, ordered_synchronizer.go:155-208) ----------------------
struct MergeField { std::string name; int32_t kind; };
struct MergeOrder { std::string name; bool dynamic; };  // the vocabulary of fdb_group_expr / GroupMatcher
struct MergeSchema {
  struct At { int32_t record, field; };
  std::vector<At> first;                  // per output column: where the field is first seen (record order, then field order)
  std::vector<int32_t> sort_expr;         // per SORTING column (the leading sort_expr.size() output columns): the order expression it matched
  std::vector<std::vector<int32_t>> map;  // [record][output column] = the field's position inside the record, -1: the record lacks it
};

inline bool merge_order_matches(const MergeOrder& o, const std::string& field) {  // = match_group (fdb_plan.cpp): expr.go:353-355, :564-566
  if (o.dynamic) return field.size() > o.name.size() && field.compare(0, o.name.size(), o.name) == 0 && field[o.name.size()] == '.';
  return field == o.name;
}

// For each order expression in turn the fields that match it in any record (records without rows included), in byte order of their
// names, become sorting columns; an expression that matches nothing is skipped; then every remaining field once, in first-seen order
// (the reference iterates a Go map there). A field is emitted once: one that an earlier expression took is not matched again, and no
// sorting column reappears among the rest (the reference's leftoverCols duplicates them when there are two or more expressions).
// FDB_ERR_INVALID: a record with two fields of one name (:219-227), a name whose kind differs between two records.
inline MergeSchema unify_merge_schema(const std::vector<std::vector<MergeField>>& records, const std::vector<MergeOrder>& order) {
  struct Seen { std::string name; int32_t kind; MergeSchema::At at; bool taken; };
  std::vector<Seen> seen;  // every distinct name, first seen first
  auto find = [&](const std::string& name) -> Seen* {
    for (Seen& s : seen) if (s.name == name) return &s;
    return nullptr;
  };
  for (size_t r = 0; r < records.size(); r++)
    for (size_t f = 0; f < records[r].size(); f++) {
      const MergeField& fld = records[r][f];
      for (size_t g = 0; g < f; g++)
        if (records[r][g].name == fld.name)
          throw Error(FDB_ERR_INVALID, "merge: found multiple fields (" + std::to_string(g) + ", " + std::to_string(f) + ") for name " + fld.name + " in record " + std::to_string(r));
      if (Seen* s = find(fld.name)) {
        if (s->kind != fld.kind)
          throw Error(FDB_ERR_INVALID, "merge: field " + fld.name + " has column kind " + std::to_string(s->kind) + " in record " + std::to_string(s->at.record) + " and column kind " +
                                           std::to_string(fld.kind) + " in record " + std::to_string(r));
        continue;
      }
      seen.push_back(Seen{fld.name, fld.kind, MergeSchema::At{(int32_t)r, (int32_t)f}, false});
    }
  MergeSchema out;
  std::vector<const Seen*> cols;
  for (size_t e = 0; e < order.size(); e++) {
    std::vector<Seen*> found;
    for (Seen& s : seen)
      if (!s.taken && merge_order_matches(order[e], s.name)) found.push_back(&s);
    std::sort(found.begin(), found.end(), [](const Seen* a, const Seen* b) { return a->name < b->name; });  // (sort.Strings: bytewise)
    for (Seen* s : found) { s->taken = true; cols.push_back(s); out.sort_expr.push_back((int32_t)e); }
  }
  for (const Seen& s : seen)
    if (!s.taken) cols.push_back(&s);
  out.map.assign(records.size(), std::vector<int32_t>(cols.size(), -1));
  for (size_t c = 0; c < cols.size(); c++) {
    out.first.push_back(cols[c]->at);
    for (size_t r = 0; r < records.size(); r++)
      for (size_t f = 0; f < records[r].size(); f++)
        if (records[r][f].name == cols[c]->name) { out.map[r][c] = (int32_t)f; break; }
  }
  return out;
}

}  // namespace fdb

#ifndef FDB_MERGEREC_HOST_ONLY
#include <mutex>

#include "fdb_plan.h"

namespace fdb {

// Everything that can refuse the call is checked before anything is launched, and an unordered input before any MERGE launch.
// FDB_ERR_INVALID: n == 0, a null record, records on different devices, no sorting columns, a column index or direction out of range,
// field lists that differ in length, names, order or kind, more than 2^31 - 1 rows in total, an unordered input. FDB_ERR_UNSUPPORTED: a
// bool sorting column, a column the resident record cannot hold, a field that is utf8 in one record and binary in another.
// n == 1 is limit_batch of the record (its order is not looked at); a total of 0 rows gives a zero-row record of the schema.
std::unique_ptr<DeviceBatch> merge_batches(const DeviceBatch* const* in, int32_t n, const fdb_sort_col* cols, int32_t n_cols, uint64_t limit);

// ≙ ensureSameSchema + MergeRecords: records whose field lists may differ, the sorting columns named by `order` (unify_merge_schema; an
// expression's direction / nulls_first hold for every column it matches). A record's rows are NULL in a column it lacks. The output
// always has the unified column order; n == 1: the record's columns in that order, cut to `limit`, its order not looked at. No
// expression matches any field: the key is empty and the result is the concatenation in call order. A dictionary column that only
// records without rows carry keeps such a record's dictionary (an empty binary one if it has none).
// FDB_ERR_INVALID: n == 0, a null record, records on different devices, order == nullptr, n_order <= 0, a null name, a direction above
// 1, what unify_merge_schema refuses, more than 2^31 - 1 rows in total, an unordered input. FDB_ERR_UNSUPPORTED: as merge_batches.
std::unique_ptr<DeviceBatch> merge_batches_named(const DeviceBatch* const* in, int32_t n, const fdb_order_col* order, int32_t n_order, uint64_t limit);

// ≙ OrderedSynchronizer (ordered_synchronizer.go:59-137) without the blocking: a push parks the record as its input's contribution to
// the current round (borrowed until the round is merged); the call that makes "inputs waiting == inputs still running" — a push, or
// the finish that retires the last input the round waited for — merges the parked records with merge_batches_named (limit 0, in INPUT
// order: ties between inputs do not depend on who arrived first), returns the result and empties the round. A round whose merge throws
// is discarded and the error leaves through the completing call; the synchronizer stays usable. One mutex guards everything, the merge
// included (the reference holds its mutex there too). FDB_ERR_STATE: a push from an input that has finished or already waits in this
// round, a finish from such an input, one more finish than inputs ("too many OrderedSynchronizer Finish calls").
class OrderedSync {
 public:
  OrderedSync(int32_t inputs, const fdb_order_col* order, int32_t n_order);
  std::unique_ptr<DeviceBatch> push(int32_t input, const DeviceBatch* batch);  // nullptr unless this call completed the round
  std::unique_ptr<DeviceBatch> finish(int32_t input, bool* done);              // *done: the last input has finished

 private:
  std::unique_ptr<DeviceBatch> merge_round();  // (mu_ held)
  void check_input(int32_t input) const;
  std::mutex mu_;
  std::vector<std::string> names_;
  std::vector<fdb_order_col> order_;
  std::vector<const DeviceBatch*> parked_;  // [input]; nullptr: not waiting
  std::vector<char> finished_;
  int32_t running_ = 0, waiting_ = 0;
};

// Measurement aid (fdb_merge_bench, tools/merge_bench.py): device time between HIP events on the call's stream, medians over `reps`
// calls after `warmup` calls — *merge_ms: keys + order check + rounds; *gather_ms: the gather; round_ms[k] (up to round_cap): round k.
void merge_bench(const DeviceBatch* const* in, int32_t n, const fdb_sort_col* cols, int32_t n_cols, int32_t reps, int32_t warmup, double* merge_ms, double* gather_ms,
                 double* round_ms, int32_t round_cap, int32_t* n_rounds, int32_t* words);

}  // namespace fdb
#endif
