// fdb_pqdelta.hip — the DELTA_BINARY_PACKED passes of the Parquet writer (host side: fdb_pqwrite.cpp; arithmetic: fdb_pqdelta.h). They run
// beside the two passes of fdb_pqwrite.hip, over the int64 / uint64 columns the caller asked to be written DELTA:
//
// pqd_compact_kernel: one workgroup per (column, page, tile) of a column WITH a bitmap copies the tile's non-NULL values to their rank in
//   the page (the survey's tile_base + the rank inside the tile, as the V64 branch of pqw_encode_kernel finds it) in scratch; a column
//   without a bitmap is read where it is. From here on a page is a dense run of `count` values.
// pqd_block_survey_kernel: one WAVE per block of 128 deltas, two deltas per lane (lane l: delta l and delta 64 + l, so the two 32-lane
//   halves of the wave hold miniblocks 0 | 1 and 2 | 3): signed minimum over the wave, unsigned maximum of delta − min over each half,
//   the four widths, the block's byte count.
// pqd_page_walk_kernel: one wave per (column, page) walks the page's blocks in order, 64 at a step: the running sum of their sizes is
//   each block's offset inside the page, the total with the page header the page's value bytes — what the host lays the file out with.
// pqd_encode_kernel: one wave per block stages the block's 128 delta − min in LDS, then every lane puts whole 32-bit words of the
//   miniblocks together (a miniblock at width w is exactly w words: fdb_pqd_assemble_word) and stores them at their final file bytes.
//   A block starts at any byte: the words go out as unaligned 4-byte stores, the block head and the page header byte by byte, one lane
//   a byte. Every byte has one writer, so there is nothing to OR and no atomics.
// All grids are capped at FDB_PQW_MAX_GRID workgroups and strided.
#include "fdb_pqdelta.h"

namespace {

__device__ __forceinline__ int64_t wave_min_i64(int64_t v) {  // (every lane gets it)
  for (int d = 32; d > 0; d >>= 1) { const int64_t o = (int64_t)__shfl_xor((long long)v, d, 64); v = o < v ? o : v; }
  return v;
}
__device__ __forceinline__ uint64_t half_max_u64(uint64_t v) {  // over the lane's 32-lane half
  for (int d = 16; d > 0; d >>= 1) { const uint64_t o = (uint64_t)__shfl_xor((unsigned long long)v, d, 64); v = o > v ? o : v; }
  return v;
}

// Block b of a page whose dense values start at `v`: this lane's two deltas of the block's n (0 where the block has none there).
__device__ __forceinline__ void load_deltas(const uint64_t* v, uint32_t b, uint32_t n, int lane, uint64_t* d0, uint64_t* d1) {
  const uint64_t at = (uint64_t)b * FDB_PQD_BLOCK;
  *d0 = (uint32_t)lane < n ? fdb_pqd_delta(v, at + lane) : 0;
  *d1 = (uint32_t)lane + 64 < n ? fdb_pqd_delta(v, at + 64 + lane) : 0;
}

__global__ __launch_bounds__(FDB_PQD_THREADS) void pqd_compact_kernel(const FdbPqdCol* __restrict__ dcols, int32_t n_dcols, FdbPqwGeom g, const uint32_t* __restrict__ tile_base) {
  __shared__ uint64_t s_word[FDB_PQW_TILE_WORDS];
  __shared__ uint32_t s_before[FDB_PQW_TILE_WORDS];
  const int tid = threadIdx.x;
  const int64_t per_col = g.n_pages * g.tiles_per_page, items = (int64_t)n_dcols * per_col;
  for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
    const FdbPqdCol c = dcols[item / per_col];
    if (c.validity == nullptr) continue;  // (the whole workgroup)
    const int64_t page = (item % per_col) / g.tiles_per_page;
    const int32_t t = (int32_t)(item % g.tiles_per_page);
    int64_t first, end;
    fdb_pqw_tile_rows(g, page, t, &first, &end);
    if (first >= end) continue;
    if (tid < 64) {  // (wave 0: FDB_PQW_TILE_WORDS == 64)
      const uint64_t w = fdb_pqw_valid_word(c.validity, first, tid, end);
      const uint32_t pc = (uint32_t)fdb_pqw_popc(w);
      uint32_t inc = pc;
      for (int d = 1; d < 64; d <<= 1) { const uint32_t o = __shfl_up(inc, d, 64); if (tid >= d) inc += o; }
      s_word[tid] = w;
      s_before[tid] = inc - pc;
    }
    __syncthreads();
    const uint32_t n = (uint32_t)(end - first);
    uint64_t* dst = c.dense + fdb_pqw_page_first(g, page) + tile_base[((int64_t)c.col * g.n_pages + page) * g.tiles_per_page + t];
    for (uint32_t lr = tid; lr < n; lr += FDB_PQD_THREADS) {
      const uint64_t w = s_word[lr >> 6];
      if ((w >> (lr & 63)) & 1) dst[s_before[lr >> 6] + (uint32_t)fdb_pqw_popc(w & ((1ull << (lr & 63)) - 1))] = c.values[first + lr];
    }
    __syncthreads();  // (the staging arrays are the next tile's)
  }
}

__global__ __launch_bounds__(FDB_PQD_THREADS) void pqd_block_survey_kernel(const FdbPqdCol* __restrict__ dcols, int32_t n_dcols, FdbPqwGeom g, const FdbPqwPageStat* __restrict__ stats,
                                                                            FdbPqdBlock* __restrict__ blocks) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int32_t bpp = fdb_pqd_blocks_per_page(g.page_rows);
  const int64_t items = (int64_t)n_dcols * g.n_pages * bpp;
  for (int64_t item = (int64_t)blockIdx.x * FDB_PQD_WAVES + wave; item < items; item += (int64_t)gridDim.x * FDB_PQD_WAVES) {
    const int64_t cp = item / bpp, page = cp % g.n_pages;
    const uint32_t b = (uint32_t)(item % bpp);
    const FdbPqdCol c = dcols[cp / g.n_pages];
    const uint32_t n = fdb_pqd_block_deltas(fdb_pqd_deltas(stats[(int64_t)c.col * g.n_pages + page].count), b);
    if (n == 0) continue;  // (the whole wave; the page walk and the encoder do not look at a block that holds nothing)
    uint64_t d0, d1;
    load_deltas(c.dense + fdb_pqw_page_first(g, page), b, n, lane, &d0, &d1);
    const int64_t a0 = (uint32_t)lane < n ? (int64_t)d0 : INT64_MAX, a1 = (uint32_t)lane + 64 < n ? (int64_t)d1 : INT64_MAX;  // padding is not a delta
    const int64_t mn = wave_min_i64(a0 < a1 ? a0 : a1);
    const uint32_t w_lo = fdb_pqd_bit_length(half_max_u64((uint32_t)lane < n ? fdb_pqd_rel(d0, mn) : 0));
    const uint32_t w_hi = fdb_pqd_bit_length(half_max_u64((uint32_t)lane + 64 < n ? fdb_pqd_rel(d1, mn) : 0));
    const uint32_t widths = (uint32_t)__shfl((int)w_lo, 0, 64) | (uint32_t)__shfl((int)w_lo, 32, 64) << 8 | (uint32_t)__shfl((int)w_hi, 0, 64) << 16 | (uint32_t)__shfl((int)w_hi, 32, 64) << 24;
    if (lane == 0) {
      FdbPqdBlock r;
      r.min = mn; r.widths = widths; r.bytes = fdb_pqd_block_bytes(mn, widths, fdb_pqd_minis(n)); r.off = 0; r.pad = 0;
      blocks[item] = r;
    }
  }
}

__global__ __launch_bounds__(FDB_PQD_THREADS) void pqd_page_walk_kernel(const FdbPqdCol* __restrict__ dcols, int32_t n_dcols, FdbPqwGeom g, const FdbPqwPageStat* __restrict__ stats,
                                                                         FdbPqdBlock* __restrict__ blocks, uint32_t* __restrict__ page_bytes) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int32_t bpp = fdb_pqd_blocks_per_page(g.page_rows);
  const int64_t items = (int64_t)n_dcols * g.n_pages;
  for (int64_t item = (int64_t)blockIdx.x * FDB_PQD_WAVES + wave; item < items; item += (int64_t)gridDim.x * FDB_PQD_WAVES) {
    const int64_t page = item % g.n_pages;
    const FdbPqdCol c = dcols[item / g.n_pages];
    const uint32_t count = stats[(int64_t)c.col * g.n_pages + page].count, nb = fdb_pqd_blocks(fdb_pqd_deltas(count));
    uint32_t run = fdb_pqd_header_len(count, count > 0 ? c.dense[fdb_pqw_page_first(g, page)] : 0);
    FdbPqdBlock* pb = blocks + item * bpp;
    for (uint32_t b0 = 0; b0 < nb; b0 += 64) {
      const uint32_t i = b0 + (uint32_t)lane, bytes = i < nb ? pb[i].bytes : 0;
      uint32_t inc = bytes;
      for (int d = 1; d < 64; d <<= 1) { const uint32_t o = __shfl_up(inc, d, 64); if (lane >= d) inc += o; }
      if (i < nb) pb[i].off = run + inc - bytes;
      run += (uint32_t)__shfl((int)inc, 63, 64);
    }
    if (lane == 0) page_bytes[item] = run;
  }
}

__global__ __launch_bounds__(FDB_PQD_THREADS) void pqd_encode_kernel(const FdbPqdCol* __restrict__ dcols, int32_t n_dcols, FdbPqwGeom g, const FdbPqwPageStat* __restrict__ stats,
                                                                      const FdbPqdBlock* __restrict__ blocks, const uint64_t* __restrict__ values_off, unsigned char* __restrict__ image) {
  __shared__ uint64_t s_rel[FDB_PQD_WAVES][FDB_PQD_BLOCK];  // per wave: the block's delta − min, padding zero
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int32_t bpp = fdb_pqd_blocks_per_page(g.page_rows);
  const int64_t items = (int64_t)n_dcols * g.n_pages * bpp;
  for (int64_t base = (int64_t)blockIdx.x * FDB_PQD_WAVES; base < items; base += (int64_t)gridDim.x * FDB_PQD_WAVES) {  // (the whole workgroup goes round together)
    const int64_t item = base + wave;
    uint32_t b = 0, n = 0, count = 0;
    int64_t cp = 0;
    const uint64_t* v = nullptr;
    FdbPqdBlock r;
    r.min = 0; r.widths = 0; r.bytes = 0; r.off = 0; r.pad = 0;
    if (item < items) {
      cp = item / bpp;
      b = (uint32_t)(item % bpp);
      const int64_t page = cp % g.n_pages;
      const FdbPqdCol c = dcols[cp / g.n_pages];
      count = stats[(int64_t)c.col * g.n_pages + page].count;
      n = fdb_pqd_block_deltas(fdb_pqd_deltas(count), b);
      v = c.dense + fdb_pqw_page_first(g, page);
      if (n > 0) {
        r = blocks[item];
        uint64_t d0, d1;
        load_deltas(v, b, n, lane, &d0, &d1);
        s_rel[wave][lane] = (uint32_t)lane < n ? fdb_pqd_rel(d0, r.min) : 0;
        s_rel[wave][64 + lane] = (uint32_t)lane + 64 < n ? fdb_pqd_rel(d1, r.min) : 0;
      }
    }
    __syncthreads();
    if (item < items && (n > 0 || b == 0)) {
      unsigned char* out = image + values_off[cp];
      if (b == 0) {  // the page header goes with the page's first block — which a page of one value or none does not have
        const uint64_t first = count > 0 ? v[0] : 0;
        if ((uint32_t)lane < fdb_pqd_header_len(count, first)) out[lane] = fdb_pqd_header_byte(count, first, (uint32_t)lane);
      }
      if (n > 0) {
        unsigned char* p = out + r.off;
        const uint32_t head = fdb_pqd_block_head_len(r.min), words = fdb_pqd_block_words(r.widths, fdb_pqd_minis(n));
        if ((uint32_t)lane < head) p[lane] = fdb_pqd_block_head_byte(r.min, r.widths, (uint32_t)lane);
        for (uint32_t k = (uint32_t)lane; k < words; k += 64) {
          uint32_t m = 0, kk = k;
          while (kk >= fdb_pqd_width(r.widths, m)) { kk -= fdb_pqd_width(r.widths, m); m++; }  // (k < words: m stays below the block's miniblocks)
          const uint32_t word = fdb_pqd_assemble_word(&s_rel[wave][m * FDB_PQD_MINI], fdb_pqd_width(r.widths, m), kk);
          __builtin_memcpy(p + head + (uint64_t)k * 4, &word, 4);  // (a block starts at any byte of the file)
        }
      }
    }
    __syncthreads();  // (the staging array is the next block's)
  }
}

int grid_for(int64_t items) { return (int)(items < FDB_PQW_MAX_GRID ? (items < 1 ? 1 : items) : FDB_PQW_MAX_GRID); }
int64_t wave_groups(int64_t items) { return (items + FDB_PQD_WAVES - 1) / FDB_PQD_WAVES; }

}  // namespace

hipError_t fdb_launch_pqd_compact(const FdbPqdCol* dcols, int32_t n_dcols, FdbPqwGeom g, const uint32_t* tile_base, hipStream_t stream) {
  hipLaunchKernelGGL(pqd_compact_kernel, dim3(grid_for((int64_t)n_dcols * g.n_pages * g.tiles_per_page)), dim3(FDB_PQD_THREADS), 0, stream, dcols, n_dcols, g, tile_base);
  return hipGetLastError();
}

hipError_t fdb_launch_pqd_survey(const FdbPqdCol* dcols, int32_t n_dcols, FdbPqwGeom g, const FdbPqwPageStat* stats, FdbPqdBlock* blocks, uint32_t* page_bytes, hipStream_t stream) {
  const int64_t pages = (int64_t)n_dcols * g.n_pages;
  hipLaunchKernelGGL(pqd_block_survey_kernel, dim3(grid_for(wave_groups(pages * fdb_pqd_blocks_per_page(g.page_rows)))), dim3(FDB_PQD_THREADS), 0, stream, dcols, n_dcols, g, stats, blocks);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(pqd_page_walk_kernel, dim3(grid_for(wave_groups(pages))), dim3(FDB_PQD_THREADS), 0, stream, dcols, n_dcols, g, stats, blocks, page_bytes);
  return hipGetLastError();
}

hipError_t fdb_launch_pqd_encode(const FdbPqdCol* dcols, int32_t n_dcols, FdbPqwGeom g, const FdbPqwPageStat* stats, const FdbPqdBlock* blocks, const uint64_t* values_off,
                                 unsigned char* image, hipStream_t stream) {
  hipLaunchKernelGGL(pqd_encode_kernel, dim3(grid_for(wave_groups((int64_t)n_dcols * g.n_pages * fdb_pqd_blocks_per_page(g.page_rows)))), dim3(FDB_PQD_THREADS), 0, stream, dcols, n_dcols,
                     g, stats, blocks, values_off, image);
  return hipGetLastError();
}
