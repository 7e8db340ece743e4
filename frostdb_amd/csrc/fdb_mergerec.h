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
// ensureSameSchema's virtual NULL columns (ordered_synchronizer.go:143-241) are not built: the field lists must agree.
//
// The first half of this header is host-only (no device, no HIP): the dictionary plan of one column across the inputs and the per-input
// rank tables. tools/asan_merge.sh runs it under AddressSanitizer with FDB_MERGEREC_HOST_ONLY defined.
#pragma once

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

}  // namespace fdb

#ifndef FDB_MERGEREC_HOST_ONLY
#include "fdb_plan.h"

namespace fdb {

// Everything that can refuse the call is checked before anything is launched, and an unordered input before any MERGE launch.
// FDB_ERR_INVALID: n == 0, a null record, records on different devices, no sorting columns, a column index or direction out of range,
// field lists that differ in length, names, order or kind, more than 2^31 - 1 rows in total, an unordered input. FDB_ERR_UNSUPPORTED: a
// bool sorting column, a column the resident record cannot hold, a field that is utf8 in one record and binary in another.
// n == 1 is limit_batch of the record (its order is not looked at); a total of 0 rows gives a zero-row record of the schema.
std::unique_ptr<DeviceBatch> merge_batches(const DeviceBatch* const* in, int32_t n, const fdb_sort_col* cols, int32_t n_cols, uint64_t limit);

// Measurement aid (fdb_merge_bench, tools/merge_bench.py): device time between HIP events on the call's stream, medians over `reps`
// calls after `warmup` calls — *merge_ms: keys + order check + rounds; *gather_ms: the gather; round_ms[k] (up to round_cap): round k.
void merge_bench(const DeviceBatch* const* in, int32_t n, const fdb_sort_col* cols, int32_t n_cols, int32_t reps, int32_t warmup, double* merge_ms, double* gather_ms,
                 double* round_ms, int32_t round_cap, int32_t* n_rounds, int32_t* words);

}  // namespace fdb
#endif
