// fdb_pqstats.hip — the min / max pass of the Parquet writer (host side: fdb_pqwrite.cpp; keys and table: fdb_pqstats.h). It runs after the
// survey of fdb_pqwrite.hip when the caller asked for statistics (fdb_batch_to_parquet_indexed), and its table comes back in the survey's wait.
//
// pqx_minmax_kernel: one workgroup per (column, page, tile) — tile-parallel, unlike the survey, which walks a page's tiles in order for
//   the running count: bounds need no scan. Every lane folds the smallest and largest KEY of its rows, 16 bytes of values at a load (two
//   8-byte values or four indices, the index keys gathered from the column's rank table), NULL rows and values that do not count left
//   out; the wave reduces by shuffles, the four waves through LDS, and thread 0 issues ONE atomicMin and ONE atomicMax on the (column,
//   page) slot of the table, which the caller set to empty on the same stream. A tile that found nothing issues none. Min and max
//   commute, so the table is the same whatever order the tiles ran in.
// The grid is capped at FDB_PQW_MAX_GRID workgroups and strided.
#include "fdb_pqstats.h"

namespace {

__device__ __forceinline__ uint64_t wave_min_u64(uint64_t v) {
  for (int d = 32; d > 0; d >>= 1) { const uint64_t o = (uint64_t)__shfl_down((unsigned long long)v, d, 64); v = o < v ? o : v; }
  return v;
}
__device__ __forceinline__ uint64_t wave_max_u64(uint64_t v) {
  for (int d = 32; d > 0; d >>= 1) { const uint64_t o = (uint64_t)__shfl_down((unsigned long long)v, d, 64); v = o > v ? o : v; }
  return v;
}

__global__ __launch_bounds__(FDB_PQW_BLOCK) void pqx_minmax_kernel(const FdbPqxCol* __restrict__ cols, FdbPqwGeom g, unsigned long long* __restrict__ table) {
  __shared__ uint64_t s_mn[FDB_PQW_BLOCK / 64], s_mx[FDB_PQW_BLOCK / 64];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int64_t slots = (int64_t)g.n_cols * g.n_pages, items = slots * g.tiles_per_page;
  for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
    const int64_t cp = item / g.tiles_per_page, page = cp % g.n_pages;
    const int32_t t = (int32_t)(item % g.tiles_per_page);
    int64_t first, end;
    fdb_pqw_tile_rows(g, page, t, &first, &end);
    if (first >= end) continue;  // (the whole workgroup)
    const FdbPqxCol c = cols[cp / g.n_pages];
    const uint32_t n = (uint32_t)(end - first);
    uint64_t mn = FDB_PQX_EMPTY_MIN, mx = FDB_PQX_EMPTY_MAX, key;
    if (c.mode == FDB_PQX_INDEX) {
      const uint32_t* idx = (const uint32_t*)c.values + first;
      for (uint32_t u = tid; u * FDB_PQX_UNIT_INDEX < n && c.rank_len > 0; u += FDB_PQW_BLOCK) {
        const uint32_t bits = fdb_pqx_unit_bits(c.validity, first, end, u, FDB_PQX_UNIT_INDEX), lr = u * FDB_PQX_UNIT_INDEX;
        if (bits == 0) continue;
        uint32_t v0 = 0, v1 = 0, v2 = 0, v3 = 0;
        if (lr + FDB_PQX_UNIT_INDEX <= n) { const uint4 q = *reinterpret_cast<const uint4*>(idx + lr); v0 = q.x; v1 = q.y; v2 = q.z; v3 = q.w; }
        else { v0 = idx[lr]; if (bits & 2) v1 = idx[lr + 1]; if (bits & 4) v2 = idx[lr + 2]; }  // (a short last unit: bit 0 is set or a later one is, and bit 3 is not)
        if ((bits & 1) && fdb_pqx_index_key(c.ranks, c.rank_len, v0, &key)) fdb_pqx_fold(key, &mn, &mx);
        if ((bits & 2) && fdb_pqx_index_key(c.ranks, c.rank_len, v1, &key)) fdb_pqx_fold(key, &mn, &mx);
        if ((bits & 4) && fdb_pqx_index_key(c.ranks, c.rank_len, v2, &key)) fdb_pqx_fold(key, &mn, &mx);
        if ((bits & 8) && fdb_pqx_index_key(c.ranks, c.rank_len, v3, &key)) fdb_pqx_fold(key, &mn, &mx);
      }
    } else {
      const uint64_t* val = (const uint64_t*)c.values + first;
      for (uint32_t u = tid; u * FDB_PQX_UNIT_V64 < n; u += FDB_PQW_BLOCK) {
        const uint32_t bits = fdb_pqx_unit_bits(c.validity, first, end, u, FDB_PQX_UNIT_V64), lr = u * FDB_PQX_UNIT_V64;
        if (bits == 0) continue;
        uint64_t v0, v1 = 0;
        if (lr + FDB_PQX_UNIT_V64 <= n) { const ulonglong2 q = *reinterpret_cast<const ulonglong2*>(val + lr); v0 = q.x; v1 = q.y; }
        else v0 = val[lr];
        if ((bits & 1) && fdb_pqx_key(c.mode, v0, &key)) fdb_pqx_fold(key, &mn, &mx);
        if ((bits & 2) && fdb_pqx_key(c.mode, v1, &key)) fdb_pqx_fold(key, &mn, &mx);
      }
    }
    mn = wave_min_u64(mn); mx = wave_max_u64(mx);
    if (lane == 0) { s_mn[wave] = mn; s_mx[wave] = mx; }
    __syncthreads();
    if (tid == 0) {
      for (int q = 1; q < FDB_PQW_BLOCK / 64; q++) { mn = s_mn[q] < mn ? s_mn[q] : mn; mx = s_mx[q] > mx ? s_mx[q] : mx; }
      if (mn <= mx) { atomicMin(&table[cp], (unsigned long long)mn); atomicMax(&table[slots + cp], (unsigned long long)mx); }
    }
    __syncthreads();  // (the two arrays are the next tile's)
  }
}

}  // namespace

hipError_t fdb_launch_pqx_minmax(const FdbPqxCol* cols, FdbPqwGeom g, unsigned long long* table, hipStream_t stream) {
  const int64_t items = (int64_t)g.n_cols * g.n_pages * g.tiles_per_page;
  hipLaunchKernelGGL(pqx_minmax_kernel, dim3((int)(items < FDB_PQW_MAX_GRID ? (items < 1 ? 1 : items) : FDB_PQW_MAX_GRID)), dim3(FDB_PQW_BLOCK), 0, stream, cols, g, table);
  return hipGetLastError();
}
