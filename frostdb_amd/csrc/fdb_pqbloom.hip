// fdb_pqbloom.hip — the bloom filter pass of the Parquet writer (host side: fdb_pqwrite.cpp; hash, block, bits and size: fdb_pqbloom.h). It
// runs once the survey's table has sized the filters, when the caller asked for some (fdb_batch_to_parquet_filtered), on the call's
// stream beside the encode pass; the bitsets come back after the image.
//
// pqb_insert_kernel: one workgroup per (filtered column, page, tile), the geometry of the min / max pass (fdb_pqstats.hip): every lane
//   takes 16 bytes of values at a load — two 8-byte values, hashed in registers, or four indices, whose hashes are gathered from the
//   column's table of entry hashes — NULL rows left out, and an index at or past the table as well (the survey's to refuse, never a
//   subscript here). A value equal to the row before it (of the lane's own unit, or the last row of the lane before, by one shuffle) is
//   not inserted again: sorted and label columns are runs. An insert reads the value's block — four 64-bit words, each a pair of the
//   block's 32-bit words — and issues a 64-bit atomic OR only for the pairs that lack a bit, so a value seen before costs its loads. The
//   loads are relaxed atomic loads at agent scope: the ORs are done at the memory side, and a plain load could be answered by a line
//   another XCD's L2 does not have — which would only cost ORs that set nothing, never a bit, but those are what the loads are there
//   to save. OR commutes, so the bitsets are the same whatever order the tiles ran in.
// The grid is capped at FDB_PQW_MAX_GRID workgroups and strided.
#include "fdb_pqbloom.h"

namespace {

__device__ __forceinline__ void pqb_insert(unsigned long long* __restrict__ bits, uint32_t n_blocks, uint64_t h) {
  unsigned long long* blk = bits + (size_t)fdb_pqb_block(h, n_blocks) * (FDB_PQB_BLOCK_BYTES / 8);
  unsigned long long cur[4];
#pragma unroll
  for (int p = 0; p < 4; p++) cur[p] = __hip_atomic_load(blk + p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
  for (int p = 0; p < 4; p++) {
    const unsigned long long m = fdb_pqb_pair_mask(h, p);
    if ((cur[p] & m) != m) (void)atomicOr(blk + p, m);
  }
}

__global__ __launch_bounds__(FDB_PQW_BLOCK) void pqb_insert_kernel(const FdbPqbCol* __restrict__ cols, int32_t n_cols, FdbPqwGeom g) {
  const int tid = threadIdx.x, lane = tid & 63;
  const int64_t items = (int64_t)n_cols * g.n_pages * g.tiles_per_page;
  for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
    const int64_t cp = item / g.tiles_per_page, page = cp % g.n_pages;
    const int32_t t = (int32_t)(item % g.tiles_per_page);
    int64_t first, end;
    fdb_pqw_tile_rows(g, page, t, &first, &end);
    if (first >= end) continue;  // (the whole workgroup)
    const FdbPqbCol c = cols[cp / g.n_pages];
    const uint32_t n = (uint32_t)(end - first);
    if (c.index != 0) {
      const uint32_t* idx = (const uint32_t*)c.values + first;
      for (uint32_t base = 0; base * FDB_PQX_UNIT_INDEX < n; base += FDB_PQW_BLOCK) {  // (the same trips for every lane: the shuffle below is the whole wave's)
        const uint32_t u = base + tid, lr = u * FDB_PQX_UNIT_INDEX;
        const uint32_t bits = lr < n ? fdb_pqx_unit_bits(c.validity, first, end, u, FDB_PQX_UNIT_INDEX) : 0;
        uint32_t v0 = 0, v1 = 0, v2 = 0, v3 = 0;
        if (bits != 0) {
          if (lr + FDB_PQX_UNIT_INDEX <= n) { const uint4 q = *reinterpret_cast<const uint4*>(idx + lr); v0 = q.x; v1 = q.y; v2 = q.z; v3 = q.w; }
          else { v0 = idx[lr]; if (bits & 2) v1 = idx[lr + 1]; if (bits & 4) v2 = idx[lr + 2]; }  // (a short last unit: bit 3 is not set)
        }
        const uint32_t pv = __shfl_up(v3, 1, 64);
        const uint32_t pb = lane == 0 ? 0 : __shfl_up(bits >> 3, 1, 64);  // (a wave's first lane knows no row before it: it inserts)
        if ((bits & 1) && !(pb && pv == v0) && v0 < c.hash_len) pqb_insert(c.bits, c.n_blocks, c.hashes[v0]);
        if ((bits & 2) && !((bits & 1) && v0 == v1) && v1 < c.hash_len) pqb_insert(c.bits, c.n_blocks, c.hashes[v1]);
        if ((bits & 4) && !((bits & 2) && v1 == v2) && v2 < c.hash_len) pqb_insert(c.bits, c.n_blocks, c.hashes[v2]);
        if ((bits & 8) && !((bits & 4) && v2 == v3) && v3 < c.hash_len) pqb_insert(c.bits, c.n_blocks, c.hashes[v3]);
      }
    } else {
      const uint64_t* val = (const uint64_t*)c.values + first;
      for (uint32_t base = 0; base * FDB_PQX_UNIT_V64 < n; base += FDB_PQW_BLOCK) {
        const uint32_t u = base + tid, lr = u * FDB_PQX_UNIT_V64;
        const uint32_t bits = lr < n ? fdb_pqx_unit_bits(c.validity, first, end, u, FDB_PQX_UNIT_V64) : 0;
        uint64_t v0 = 0, v1 = 0;
        if (bits != 0) {
          if (lr + FDB_PQX_UNIT_V64 <= n) { const ulonglong2 q = *reinterpret_cast<const ulonglong2*>(val + lr); v0 = q.x; v1 = q.y; }
          else v0 = val[lr];  // (a short last unit: bit 1 is not set)
        }
        const uint64_t pv = (uint64_t)__shfl_up((unsigned long long)v1, 1, 64);
        const uint32_t pb = lane == 0 ? 0 : __shfl_up(bits >> 1, 1, 64);
        if ((bits & 1) && !(pb && pv == v0)) pqb_insert(c.bits, c.n_blocks, fdb_pqb_hash8(v0));
        if ((bits & 2) && !((bits & 1) && v0 == v1)) pqb_insert(c.bits, c.n_blocks, fdb_pqb_hash8(v1));
      }
    }
  }
}

}  // namespace

hipError_t fdb_launch_pqb_insert(const FdbPqbCol* cols, int32_t n_cols, FdbPqwGeom g, hipStream_t stream) {
  const int64_t items = (int64_t)n_cols * g.n_pages * g.tiles_per_page;
  hipLaunchKernelGGL(pqb_insert_kernel, dim3((int)(items < FDB_PQW_MAX_GRID ? (items < 1 ? 1 : items) : FDB_PQW_MAX_GRID)), dim3(FDB_PQW_BLOCK), 0, stream, cols, n_cols, g);
  return hipGetLastError();
}
