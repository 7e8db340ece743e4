// fdb_pqwrite.hip — the two passes of the Parquet writer over a record resident in HBM (host side: fdb_pqwrite.cpp; arithmetic: fdb_pqwrite.h).
//
// pqw_survey_kernel: one workgroup per (column, page) walks the page's tiles in order — popcounts of the validity words give the non-NULL
//   rows, of INDEX columns the smallest and largest non-NULL index are folded along — and leaves the page's totals and, per tile, the rank
//   of its first value (the running count: the exclusive scan pass 2 needs, made in place). Reads the bitmaps and the indices once.
// pqw_encode_kernel: one workgroup per (column, page, tile) writes the tile's share of the page's payloads to their final place in the
//   file image: definition-level bytes (the validity bits of the page's rows), 8-byte values compacted by rank, and BOOLEAN bits / dictionary
//   indices bit-packed at the column's width. The packer stages the tile's compacted values in LDS, then every lane puts whole 32-bit
//   image words together from the values that overlap them (fdb_pqw_assemble_word) and stores them side by side. A run's payload starts
//   at any byte and a tile at any bit, so the first and last word of a tile are shared — with the neighbouring tiles, which may run
//   anywhere at any time, and with bytes the host fills in later: those two words are OR-ed into the zeroed image with atomicOr, the
//   words between belong to the tile alone and are stored. In a packed column the level bytes take the same route (atomicOr of one byte),
//   so a word is either stored by its one owner or only ever OR-ed; a V64 column is written with plain stores of disjoint bytes throughout.
#include "fdb_pqwrite.h"

namespace {

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
  for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d, 64);
  return v;
}
__device__ __forceinline__ uint32_t wave_min(uint32_t v) {
  for (int d = 32; d > 0; d >>= 1) { const uint32_t o = __shfl_down(v, d, 64); v = o < v ? o : v; }
  return v;
}
__device__ __forceinline__ uint32_t wave_max(uint32_t v) {
  for (int d = 32; d > 0; d >>= 1) { const uint32_t o = __shfl_down(v, d, 64); v = o > v ? o : v; }
  return v;
}

__global__ __launch_bounds__(FDB_PQW_BLOCK) void pqw_survey_kernel(const FdbPqwCol* __restrict__ cols, FdbPqwGeom g, FdbPqwPageStat* __restrict__ stats,
                                                                   uint32_t* __restrict__ tile_base) {
  __shared__ uint32_t s_cnt[FDB_PQW_BLOCK / 64], s_mn[FDB_PQW_BLOCK / 64], s_mx[FDB_PQW_BLOCK / 64];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int64_t items = (int64_t)g.n_cols * g.n_pages;
  for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
    const int64_t page = item % g.n_pages;
    const FdbPqwCol c = cols[item / g.n_pages];
    const bool index = c.kind == FDB_PQW_INDEX;
    const uint32_t* idx = (const uint32_t*)c.values;
    uint32_t run = 0, pmn = 0xFFFFFFFFu, pmx = 0;  // (thread 0's)
    for (int32_t t = 0; t < g.tiles_per_page; t++) {
      int64_t first, end;
      fdb_pqw_tile_rows(g, page, t, &first, &end);
      uint32_t cnt = 0, mn = 0xFFFFFFFFu, mx = 0;
      if (first < end) {
        if (tid < FDB_PQW_TILE_WORDS) cnt = (uint32_t)fdb_pqw_popc(fdb_pqw_valid_word(c.validity, first, tid, end));
        if (index) {
          for (int64_t r = first + tid; r < end; r += FDB_PQW_BLOCK) {
            const bool valid = c.validity == nullptr || ((c.validity[r >> 3] >> (r & 7)) & 1);
            if (valid) { const uint32_t v = idx[r]; mn = v < mn ? v : mn; mx = v > mx ? v : mx; }
          }
        }
      }
      cnt = wave_sum(cnt); mn = wave_min(mn); mx = wave_max(mx);
      if (lane == 0) { s_cnt[wave] = cnt; s_mn[wave] = mn; s_mx[wave] = mx; }
      __syncthreads();
      if (tid == 0) {
        tile_base[item * g.tiles_per_page + t] = run;
        for (int q = 0; q < FDB_PQW_BLOCK / 64; q++) { run += s_cnt[q]; pmn = s_mn[q] < pmn ? s_mn[q] : pmn; pmx = s_mx[q] > pmx ? s_mx[q] : pmx; }
      }
      __syncthreads();
    }
    if (tid == 0) { FdbPqwPageStat s; s.count = run; s.mn = pmn; s.mx = pmx; s.pad = 0; stats[item] = s; }
  }
}

__global__ __launch_bounds__(FDB_PQW_BLOCK) void pqw_encode_kernel(const FdbPqwCol* __restrict__ cols, FdbPqwGeom g, const FdbPqwPageOut* __restrict__ out,
                                                                   const uint32_t* __restrict__ tile_base, unsigned char* __restrict__ image) {
  __shared__ uint64_t s_word[FDB_PQW_TILE_WORDS];   // the tile's validity words, rows past its end cleared
  __shared__ uint32_t s_before[FDB_PQW_TILE_WORDS]; // non-NULL rows of the tile before each word
  __shared__ uint32_t s_total;
  __shared__ uint32_t s_vals[FDB_PQW_STAGE_WORDS];  // the tile's values by rank (fdb_pqw_slot)
  const int tid = threadIdx.x;
  uint32_t* image32 = (uint32_t*)image;
  const int64_t per_col = g.n_pages * g.tiles_per_page, items = (int64_t)g.n_cols * per_col;
  for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
    const int64_t cp = item / g.tiles_per_page, page = cp % g.n_pages;
    const int32_t t = (int32_t)(item % g.tiles_per_page);
    int64_t first, end;
    fdb_pqw_tile_rows(g, page, t, &first, &end);
    if (first >= end) continue;  // (the whole workgroup)
    const FdbPqwCol c = cols[cp / g.n_pages];
    const FdbPqwPageOut po = out[cp];
    if (po.levels_off == FDB_PQW_NONE && po.values_off == FDB_PQW_NONE) continue;
    const uint32_t n = (uint32_t)(end - first);
    if (tid < 64) {  // (wave 0: FDB_PQW_TILE_WORDS == 64)
      const uint64_t w = fdb_pqw_valid_word(c.validity, first, tid, end);
      const uint32_t pc = (uint32_t)fdb_pqw_popc(w);
      uint32_t inc = pc;
      for (int d = 1; d < 64; d <<= 1) { const uint32_t o = __shfl_up(inc, d, 64); if (tid >= d) inc += o; }
      s_word[tid] = w;
      s_before[tid] = inc - pc;
      if (tid == 63) s_total = inc;
    }
    __syncthreads();
    const uint32_t count = s_total;
    const uint64_t base = tile_base[item];
    const bool packed = c.kind != FDB_PQW_V64;
    if (po.levels_off != FDB_PQW_NONE) {
      const uint64_t at = po.levels_off + (uint64_t)((first - fdb_pqw_page_first(g, page)) >> 3);
      const unsigned char* bytes = (const unsigned char*)s_word;
      for (uint32_t i = tid; i < fdb_pqw_level_bytes(n); i += FDB_PQW_BLOCK) {
        if (packed) { if (bytes[i] != 0) atomicOr(&image32[(at + i) >> 2], (uint32_t)bytes[i] << (8 * (uint32_t)((at + i) & 3))); }
        else image[at + i] = bytes[i];
      }
    }
    if (po.values_off != FDB_PQW_NONE && count > 0) {
      if (!packed) {
        const uint64_t* src = (const uint64_t*)c.values;
        for (uint32_t lr = tid; lr < n; lr += FDB_PQW_BLOCK) {
          const uint64_t w = s_word[lr >> 6];
          if ((w >> (lr & 63)) & 1) {
            const uint64_t rank = base + s_before[lr >> 6] + (uint32_t)fdb_pqw_popc(w & ((1ull << (lr & 63)) - 1));
            const uint64_t v = src[first + lr];
            __builtin_memcpy(image + po.values_off + rank * 8, &v, 8);  // (a page's values start at any byte of the file)
          }
        }
      } else if (c.width > 0) {
        const uint32_t w_bits = (uint32_t)c.width, mask = w_bits >= 32 ? 0xFFFFFFFFu : ((1u << w_bits) - 1);
        for (uint32_t lr = tid; lr < n; lr += FDB_PQW_BLOCK) {
          const uint64_t w = s_word[lr >> 6];
          if ((w >> (lr & 63)) & 1) {  // NULL rows stage nothing: their index never reaches the payload
            const uint32_t j = s_before[lr >> 6] + (uint32_t)fdb_pqw_popc(w & ((1ull << (lr & 63)) - 1));
            const uint32_t v = c.kind == FDB_PQW_BOOL ? (uint32_t)(((const int64_t*)c.values)[first + lr] >= 2) : ((const uint32_t*)c.values)[first + lr];
            s_vals[fdb_pqw_slot(j)] = v & mask;
          }
        }
        __syncthreads();
        const uint64_t payload_bit = po.values_off * 8;
        const uint64_t k0 = fdb_pqw_first_word(payload_bit, base, w_bits), k1 = fdb_pqw_last_word(payload_bit, base, count, w_bits);
        for (uint64_t k = k0 + tid; k <= k1; k += FDB_PQW_BLOCK) {
          const uint32_t word = fdb_pqw_assemble_word(s_vals, base, count, payload_bit, w_bits, k);
          if (k == k0 || k == k1) { if (word != 0) atomicOr(&image32[k], word); }
          else image32[k] = word;
        }
      }
    }
    __syncthreads();  // (the staging arrays are the next tile's)
  }
}

int grid_for(int64_t items) { return (int)(items < FDB_PQW_MAX_GRID ? (items < 1 ? 1 : items) : FDB_PQW_MAX_GRID); }

}  // namespace

hipError_t fdb_launch_pqw_survey(const FdbPqwCol* cols, FdbPqwGeom g, FdbPqwPageStat* stats, uint32_t* tile_base, hipStream_t stream) {
  hipLaunchKernelGGL(pqw_survey_kernel, dim3(grid_for((int64_t)g.n_cols * g.n_pages)), dim3(FDB_PQW_BLOCK), 0, stream, cols, g, stats, tile_base);
  return hipGetLastError();
}

hipError_t fdb_launch_pqw_encode(const FdbPqwCol* cols, FdbPqwGeom g, const FdbPqwPageOut* out, const uint32_t* tile_base, unsigned char* image, hipStream_t stream) {
  hipLaunchKernelGGL(pqw_encode_kernel, dim3(grid_for((int64_t)g.n_cols * g.n_pages * g.tiles_per_page)), dim3(FDB_PQW_BLOCK), 0, stream, cols, g, out, tile_base, image);
  return hipGetLastError();
}
