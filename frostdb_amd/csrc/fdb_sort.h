// fdb_sort.h — Sort of a record resident in HBM (fdb_sort.cpp; key kernel in fdb_sortkeys.hip, key encoding in fdb_sortkey.h).
#pragma once

#include <memory>
#include <string>
#include <vector>

#include "fdb_plan.h"

namespace fdb {

// ≙ arrowutils.SortRecord (pqarrow/arrowutils/sort.go:48-65, multiColSorter :400-564): indices_out[i] = the row of `in` that is row i of
// the sorted record. Columns are compared left to right, the first on which two rows differ decides; with nulls_first a column's NULLs
// come before all its values, else after them, whatever the direction; int64 signed, uint64 unsigned, float64 as Go's cmp.Compare (every
// NaN equal, below -Inf; -0.0 == +0.0), dictionary / string columns by the bytes of the entry. STABLE — rows equal on every sorting column
// keep their input order; the reference's sort.Sort is not stable, so any tie order is legal there and ours is one of them, always the same.
// Everything that can refuse the call is checked before anything is launched: no columns FDB_ERR_INVALID (first); a record of 0 or 1 rows
// is answered without looking at the columns (sort.go:412-417); index outside the record / direction other than 0, 1 / more than
// 2^31 - 1 rows FDB_ERR_INVALID; a bool column or one the resident record cannot hold FDB_ERR_UNSUPPORTED.
void sort_batch_indices(const DeviceBatch& in, const fdb_sort_col* cols, int32_t n_cols, int32_t* indices_out);
// = SortRecord + Take, the permutation never leaving HBM: a new resident record, independent of `in`.
std::unique_ptr<DeviceBatch> sort_batch(const DeviceBatch& in, const fdb_sort_col* cols, int32_t n_cols);

// Measurement aid (fdb_sort_bench): see fdb_sort.cpp.
void sort_bench(const DeviceBatch& in, const fdb_sort_col* cols, int32_t n_cols, int32_t reps, int32_t warmup, double* sort_ms, double* bare_ms, int32_t* n_passes);

}  // namespace fdb
