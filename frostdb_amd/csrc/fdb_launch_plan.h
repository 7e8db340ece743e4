// fdb_launch_plan.h — the decisions of a dense scan launch (Plan::DenseLaunch, fdb_dense.cpp) that need nothing but numbers: pure
// functions, no device call, checked without a GPU by tools/launch_plan_dump.cpp (tests/test_launch_plan_cpu.py).
#pragma once

#include <cstddef>
#include <cstdint>
#include <string>

#include "../../include/frostdb_amd.h"
#include "fdb_kernels.h"

namespace fdb {

// Dynamic LDS of a launch: [LUT copies][cnt u32 × n_slots][acc u64 × n_slots × n_aggs]. `refusal` non-empty: the scan cannot run
// (FDB_ERR_UNSUPPORTED with that text), the other fields mean nothing.
struct LdsPlan {
  int lds_acc = 0;        // the table is staged in LDS
  size_t lds_bytes = 0;
  int cache_slots = 0;    // table too big for LDS: entries of the specialised kernel's combining cache (JitShape::cache), ≤ 48 KiB per workgroup
  int base_grid = 0;      // workgroups of the sequential kernel
  std::string refusal;
};
// `acc_bytes`: one table. `base_grid`: grid_override when > 0, else the device's default grid. `slots_ok`: every record of the launch fits
// the slot kernels (fixed_order has no other kernel).
inline LdsPlan plan_lds(size_t lut_lds_max, size_t acc_bytes, size_t n_aggs, bool jit_possible, bool slots_ok, bool fixed_order, bool use_partials, int grid_override, int base_grid) {
  LdsPlan p;
  p.lds_bytes = lut_lds_max;
  p.base_grid = base_grid;
  if (fixed_order) {
    // a table per wave, 4 waves (256-thread workgroups); no combining cache, no interpreting or sequential kernel
    if (!jit_possible || !slots_ok || !use_partials) { p.refusal = "deterministic float sums need the run-time specialised dense kernel"; return p; }
    if (lut_lds_max + 4 * acc_bytes > 150 * 1024) { p.refusal = "deterministic float sums: four per-wave tables of " + std::to_string(acc_bytes) + " bytes do not fit LDS"; return p; }
    p.lds_acc = 1; p.lds_bytes += 4 * acc_bytes;
  }
  else if (lut_lds_max + acc_bytes <= FDB_LDS_BUDGET) { p.lds_acc = 1; p.lds_bytes += acc_bytes; }
  else if (lut_lds_max + acc_bytes <= 150 * 1024) { p.lds_acc = 1; p.lds_bytes += acc_bytes; if (grid_override <= 0) p.base_grid /= 2; }
  if (!p.lds_acc && jit_possible) {
    const size_t entry = 8 + 8 * n_aggs;
    p.cache_slots = 1;
    while ((size_t)p.cache_slots * 2 * entry <= 48 * 1024) p.cache_slots *= 2;
    p.lds_bytes = lut_lds_max + (size_t)p.cache_slots * entry;
  }
  return p;
}

// The records of one launch own consecutive tile ranges: parts[k] gets [tile_begin, tile_end) for its n_rows; returns total_tiles.
inline int64_t assign_tiles(FdbScanArgs* parts, size_t n, int64_t tile_rows) {
  int64_t total_tiles = 0;
  for (size_t k = 0; k < n; k++) {
    parts[k].tile_begin = total_tiles;
    total_tiles += (parts[k].n_rows + tile_rows - 1) / tile_rows;
    parts[k].tile_end = total_tiles;
  }
  return total_tiles;
}

// The same on the records' own argument blocks, in place (a launch that ships the packed part table makes no copy of them).
inline int64_t assign_tiles(FdbScanArgs* const* parts, size_t n, int64_t tile_rows) {
  int64_t total_tiles = 0;
  for (size_t k = 0; k < n; k++) {
    parts[k]->tile_begin = total_tiles;
    total_tiles += (parts[k]->n_rows + tile_rows - 1) / tile_rows;
    parts[k]->tile_end = total_tiles;
  }
  return total_tiles;
}

// How fdb_launch_reduce_partials folds each table array: [0] the row counts, [1 + j] aggregation j — 0 none (COUNT reads the counts), 1 integer
// sum, 2 float64 sum, 3 min, 4 max. `func`: the aggregation's function in the argument block, `type`: the plan's accumulator type.
struct FoldFuncs { int32_t f[1 + FDB_MAX_AGGS]; };
inline FoldFuncs fold_funcs(const int32_t* func, const int32_t* type, size_t n_aggs) {
  FoldFuncs F = {{0}};
  F.f[0] = 1;
  for (size_t j = 0; j < n_aggs; j++)
    F.f[1 + j] = func[j] == FDB_AGG_COUNT ? 0 : func[j] == FDB_AGG_SUM ? (type[j] == FDB_T_F64 ? 2 : 1) : func[j] == FDB_AGG_MIN ? 3 : 4;
  return F;
}

}  // namespace fdb
