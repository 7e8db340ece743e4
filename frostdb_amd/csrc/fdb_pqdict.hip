// fdb_pqdict.hip — the two passes behind used-entry dictionaries of the Parquet writer (host side: fdb_pqwrite.cpp; the bitmap and the
// rank: fdb_pqdict.h), run when the caller asked for them (fdb_batch_to_parquet_grouped, dictionaries = 1). Both have the geometry of
// the min / max and the bloom pass (fdb_pqstats.hip, fdb_pqbloom.hip): one workgroup per (pruned column, page, tile), every lane 16
// bytes of indices — four rows, which never cross a validity word — at a load, the grid capped at FDB_PQW_MAX_GRID and strided.
//
// pqg_present_kernel, behind the survey: every non-NULL row's index sets its bit in the column's presence bitmap. An index at or past
//   `entries` is skipped (the survey's to refuse after the wait, never a subscript here). An index equal to the row before it (of the
//   lane's own unit, or the last row of the lane before, by one shuffle) is not looked at again: label columns are runs. Otherwise the
//   word is read first — a relaxed atomic load at agent scope, for the reason fdb_pqbloom.hip gives: the ORs are done at the memory
//   side — and a 64-bit atomic OR is issued only for a bit that is missing, so an entry seen before costs a load. A dictionary of at
//   most FDB_PQG_LDS_ENTRIES entries (fdb_pqdict.h) — every label column of the bench's record — goes through an LDS copy of its
//   bitmap instead: 1 KiB of the CU's 160 KiB, zeroed per tile, a bit set by a 32-bit LDS atomic OR where a read of the word finds it
//   missing, and after the tile one lane per non-zero 64-bit word reads the global word and ORs what it lacks — at most 128 global
//   loads a tile instead of one a row. Above that bound the copy's zeroing and flush, which cost the whole bitmap per tile whatever
//   the tile holds (at most 4 096 distinct indices), are not paid: the global words are L2-resident (8 KiB for 65 537 entries).
//   OR commutes: the bitmap does not depend on launch order or on which path set a bit.
// pqg_remap_kernel, after the wait: the host has counted the used entries in front of every word (`before`); a lane loads its four
//   indices, replaces each by fdb_pqg_rank and stores the unit with one 16-byte store into the re-keyed copy. A NULL row and an index
//   at or past `entries` are written as 0, nothing looked up. Bitmap and counts are read from global memory (12 KiB for 65 537 entries).
#include "fdb_pqdict.h"

namespace {

__device__ __forceinline__ void pqg_set(unsigned long long* __restrict__ bits, uint32_t v) {
  unsigned long long* w = bits + (v >> 6);
  const unsigned long long m = fdb_pqg_bit(v);
  if ((__hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & m) == 0) (void)atomicOr(w, m);
}

// The unit of lane-unit `u` of the tile [first, first + n): its validity bits and, as far as those or the tile's end allow, its indices.
__device__ __forceinline__ uint32_t pqg_unit(const FdbPqgCol& c, int64_t first, int64_t end, uint32_t n, uint32_t u, uint32_t* v) {
  const uint32_t lr = u * FDB_PQX_UNIT_INDEX;
  const uint32_t bits = lr < n ? fdb_pqx_unit_bits(c.validity, first, end, u, FDB_PQX_UNIT_INDEX) : 0;
  v[0] = 0; v[1] = 0; v[2] = 0; v[3] = 0;
  if (bits != 0) {
    const uint32_t* idx = c.values + first;
    if (lr + FDB_PQX_UNIT_INDEX <= n) { const uint4 q = *reinterpret_cast<const uint4*>(idx + lr); v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w; }
    else { v[0] = idx[lr]; if (bits & 2) v[1] = idx[lr + 1]; if (bits & 4) v[2] = idx[lr + 2]; }  // (a short last unit: bit 3 is not set)
  }
  return bits;
}

__device__ __forceinline__ void pqg_set_staged(uint32_t* s_bits, uint32_t v) {
  const uint32_t m = 1u << (v & 31);
  if ((__hip_atomic_load(s_bits + (v >> 5), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) & m) == 0) (void)atomicOr(s_bits + (v >> 5), m);
}

__global__ __launch_bounds__(FDB_PQW_BLOCK) void pqg_present_kernel(const FdbPqgCol* __restrict__ cols, int32_t n_cols, FdbPqwGeom g) {
  __shared__ uint32_t s_bits[2 * FDB_PQG_LDS_WORDS];  // the tile's copy of a small bitmap: word i of it is s_bits[2i] | s_bits[2i + 1] << 32
  const int tid = threadIdx.x, lane = tid & 63;
  const int64_t items = (int64_t)n_cols * g.n_pages * g.tiles_per_page;
  for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
    const int64_t cp = item / g.tiles_per_page, page = cp % g.n_pages;
    const int32_t t = (int32_t)(item % g.tiles_per_page);
    int64_t first, end;
    fdb_pqw_tile_rows(g, page, t, &first, &end);
    if (first >= end) continue;  // (the whole workgroup)
    const FdbPqgCol c = cols[cp / g.n_pages];
    const uint32_t n = (uint32_t)(end - first), words = (uint32_t)fdb_pqg_words(c.entries);
    const bool staged = c.entries <= FDB_PQG_LDS_ENTRIES;  // (the whole workgroup's)
    if (staged) {
      for (uint32_t i = tid; i < 2 * words; i += FDB_PQW_BLOCK) s_bits[i] = 0;
      __syncthreads();
    }
    for (uint32_t base = 0; base * FDB_PQX_UNIT_INDEX < n; base += FDB_PQW_BLOCK) {  // (the same trips for every lane: the shuffle below is the whole wave's)
      uint32_t v[4];
      const uint32_t bits = pqg_unit(c, first, end, n, base + tid, v);
      const uint32_t pv = __shfl_up(v[3], 1, 64);
      const uint32_t pb = lane == 0 ? 0 : __shfl_up(bits >> 3, 1, 64);  // (a wave's first lane knows no row before it: it looks)
      const bool on0 = (bits & 1) && !(pb && pv == v[0]) && v[0] < c.entries, on1 = (bits & 2) && !((bits & 1) && v[0] == v[1]) && v[1] < c.entries;
      const bool on2 = (bits & 4) && !((bits & 2) && v[1] == v[2]) && v[2] < c.entries, on3 = (bits & 8) && !((bits & 4) && v[2] == v[3]) && v[3] < c.entries;
      if (staged) {
        if (on0) pqg_set_staged(s_bits, v[0]);
        if (on1) pqg_set_staged(s_bits, v[1]);
        if (on2) pqg_set_staged(s_bits, v[2]);
        if (on3) pqg_set_staged(s_bits, v[3]);
      } else {
        if (on0) pqg_set(c.bits, v[0]);
        if (on1) pqg_set(c.bits, v[1]);
        if (on2) pqg_set(c.bits, v[2]);
        if (on3) pqg_set(c.bits, v[3]);
      }
    }
    if (staged) {  // the tile's bits to the column's bitmap: a lane per 64-bit word, only what the word lacks
      __syncthreads();
      for (uint32_t i = tid; i < words; i += FDB_PQW_BLOCK) {
        const unsigned long long m = (unsigned long long)s_bits[2 * i] | ((unsigned long long)s_bits[2 * i + 1] << 32);
        if (m != 0 && (__hip_atomic_load(c.bits + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & m) != m) (void)atomicOr(c.bits + i, m);
      }
      __syncthreads();  // (before the next item zeroes the copy)
    }
  }
}

__device__ __forceinline__ uint32_t pqg_new(const FdbPqgCol& c, uint32_t on, uint32_t v) {
  return on != 0 && v < c.entries ? fdb_pqg_rank(c.bits, c.before, v) : 0;
}

__global__ __launch_bounds__(FDB_PQW_BLOCK) void pqg_remap_kernel(const FdbPqgCol* __restrict__ cols, int32_t n_cols, FdbPqwGeom g) {
  const int tid = threadIdx.x;
  const int64_t items = (int64_t)n_cols * g.n_pages * g.tiles_per_page;
  for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
    const int64_t cp = item / g.tiles_per_page, page = cp % g.n_pages;
    const int32_t t = (int32_t)(item % g.tiles_per_page);
    int64_t first, end;
    fdb_pqw_tile_rows(g, page, t, &first, &end);
    if (first >= end) continue;
    const FdbPqgCol c = cols[cp / g.n_pages];
    const uint32_t n = (uint32_t)(end - first);
    for (uint32_t u = tid; u * FDB_PQX_UNIT_INDEX < n; u += FDB_PQW_BLOCK) {
      uint32_t v[4];
      const uint32_t bits = pqg_unit(c, first, end, n, u, v);
      uint4 q;
      q.x = pqg_new(c, bits & 1, v[0]); q.y = pqg_new(c, bits & 2, v[1]); q.z = pqg_new(c, bits & 4, v[2]); q.w = pqg_new(c, bits & 8, v[3]);
      *reinterpret_cast<uint4*>(c.out + first + u * FDB_PQX_UNIT_INDEX) = q;  // (the whole unit: the copy is padded to one)
    }
  }
}

int pqg_grid(int32_t n_cols, const FdbPqwGeom& g) {
  const int64_t items = (int64_t)n_cols * g.n_pages * g.tiles_per_page;
  return (int)(items < FDB_PQW_MAX_GRID ? (items < 1 ? 1 : items) : FDB_PQW_MAX_GRID);
}

}  // namespace

hipError_t fdb_launch_pqg_present(const FdbPqgCol* cols, int32_t n_cols, FdbPqwGeom g, hipStream_t stream) {
  hipLaunchKernelGGL(pqg_present_kernel, dim3(pqg_grid(n_cols, g)), dim3(FDB_PQW_BLOCK), 0, stream, cols, n_cols, g);
  return hipGetLastError();
}

hipError_t fdb_launch_pqg_remap(const FdbPqgCol* cols, int32_t n_cols, FdbPqwGeom g, hipStream_t stream) {
  hipLaunchKernelGGL(pqg_remap_kernel, dim3(pqg_grid(n_cols, g)), dim3(FDB_PQW_BLOCK), 0, stream, cols, n_cols, g);
  return hipGetLastError();
}
