// fdb_pqbytes.hip — the two passes behind PLAIN and DELTA_LENGTH_BYTE_ARRAY value pages of the Parquet writer (host side: fdb_pqwrite.cpp;
// the rule: fdb_pqbytes.h), run for the dictionary / string / binary columns the caller gave a form (fdb_batch_to_parquet_strings). Both
// have the geometry of the encode pass: one workgroup per (column, page, tile), at most FDB_PQW_MAX_GRID of them, strided.
//
// pqy_survey_kernel: sums what the tile's non-NULL rows add to the page's byte stream (the entry's length, with PLAIN four bytes more) into
//   one 64-bit sum per tile — the table the host scans into page sizes and per-tile byte bases — and, of a DELTA_LENGTH column, writes the
//   rows' lengths in rank order into the scratch 64-bit column the DELTA passes then survey and pack like any other.
// pqy_encode_kernel: stages the entry index and the byte cost of the tile's <= 4 096 values by rank in LDS, scans the costs into exclusive
//   byte offsets (16 values a thread, a wave scan of the threads' sums, the four waves' sums through LDS), and then writes the tile's
//   output range word by word: lane after lane owns consecutive aligned 32-bit words of the image, finds the value its first byte belongs
//   to by bisection of the offsets (fdb_pqy_word) and reads the entry table from there. A wave's stores are 256 consecutive bytes whatever
//   the lengths are; a range longer than one pass of the workgroup is looped over. A word the tile owns whole is stored; the first and the
//   last word of the range, where shared with a neighbouring tile, the page's DELTA lengths or bytes of the host, is OR-ed into the zeroed
//   image with atomicOr — no byte is written by two workgroups.
#include "fdb_pqbytes.h"

namespace {

__device__ __forceinline__ uint64_t wave_sum_u64(uint64_t v) {
  for (int d = 32; d > 0; d >>= 1) v += (uint64_t)__shfl_down((unsigned long long)v, d, 64);
  return v;
}

// The tile's validity words and the non-NULL rows before each (wave 0), as the encode pass stages them.
__device__ __forceinline__ void stage_validity(const unsigned char* validity, int64_t first, int64_t end, int tid, uint64_t* s_word, uint32_t* s_before, uint32_t* s_total) {
  if (tid < 64) {  // (FDB_PQW_TILE_WORDS == 64)
    const uint64_t w = fdb_pqw_valid_word(validity, first, tid, end);
    const uint32_t pc = (uint32_t)fdb_pqw_popc(w);
    uint32_t inc = pc;
    for (int d = 1; d < 64; d <<= 1) { const uint32_t o = __shfl_up(inc, d, 64); if (tid >= d) inc += o; }
    s_word[tid] = w;
    s_before[tid] = inc - pc;
    if (tid == 63) *s_total = inc;
  }
}

__global__ __launch_bounds__(FDB_PQY_THREADS) void pqy_survey_kernel(const FdbPqyCol* __restrict__ ycols, int32_t n_ycols, FdbPqwGeom g, const uint32_t* __restrict__ tile_base,
                                                                     uint64_t* __restrict__ tile_bytes) {
  __shared__ uint64_t s_word[FDB_PQW_TILE_WORDS];
  __shared__ uint32_t s_before[FDB_PQW_TILE_WORDS];
  __shared__ uint32_t s_total;
  __shared__ uint64_t s_sum[FDB_PQY_THREADS / 64];
  const int tid = threadIdx.x;
  const int64_t per_col = g.n_pages * g.tiles_per_page, items = (int64_t)n_ycols * per_col;
  for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
    const FdbPqyCol c = ycols[item / per_col];
    const int64_t page = (item % per_col) / g.tiles_per_page;
    const int32_t t = (int32_t)(item % g.tiles_per_page);
    int64_t first, end;
    fdb_pqw_tile_rows(g, page, t, &first, &end);
    if (first >= end) { if (tid == 0) tile_bytes[item] = 0; continue; }  // (the whole workgroup)
    stage_validity(c.validity, first, end, tid, s_word, s_before, &s_total);
    __syncthreads();
    const uint32_t n = (uint32_t)(end - first);
    uint64_t* dst = c.lengths != nullptr ? c.lengths + fdb_pqw_page_first(g, page) + tile_base[((int64_t)c.col * g.n_pages + page) * g.tiles_per_page + t] : nullptr;
    uint64_t sum = 0;
    for (uint32_t lr = tid; lr < n; lr += FDB_PQY_THREADS) {
      const uint64_t w = s_word[lr >> 6];
      if ((w >> (lr & 63)) & 1) {
        const uint32_t len = fdb_pqy_entry_len(c.entry_off, c.entries, c.values[first + lr]);
        sum += fdb_pqy_value_bytes(len, c.plain != 0);
        if (dst != nullptr) dst[s_before[lr >> 6] + (uint32_t)fdb_pqw_popc(w & ((1ull << (lr & 63)) - 1))] = len;
      }
    }
    sum = wave_sum_u64(sum);
    if ((tid & 63) == 0) s_sum[tid >> 6] = sum;
    __syncthreads();
    if (tid == 0) { uint64_t all = 0; for (int q = 0; q < FDB_PQY_THREADS / 64; q++) all += s_sum[q]; tile_bytes[item] = all; }
    __syncthreads();  // (the staging arrays are the next tile's)
  }
}

__global__ __launch_bounds__(FDB_PQY_THREADS) void pqy_encode_kernel(const FdbPqyCol* __restrict__ ycols, int32_t n_ycols, FdbPqwGeom g, const uint64_t* __restrict__ bytes_out,
                                                                     const uint64_t* __restrict__ byte_base, unsigned char* __restrict__ image) {
  __shared__ uint64_t s_word[FDB_PQW_TILE_WORDS];
  __shared__ uint32_t s_before[FDB_PQW_TILE_WORDS];
  __shared__ uint32_t s_total;
  __shared__ uint32_t s_wave[FDB_PQY_THREADS / 64];
  __shared__ uint32_t s_idx[FDB_PQW_TILE];      // the tile's values by rank: the entry …
  __shared__ uint32_t s_off[FDB_PQW_TILE + 1];  // … and its cost, scanned into its exclusive byte offset; s_off[count]: the tile's bytes
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  uint32_t* image32 = (uint32_t*)image;
  const int64_t per_col = g.n_pages * g.tiles_per_page, items = (int64_t)n_ycols * per_col;
  for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
    const int64_t cp = item / g.tiles_per_page, page = cp % g.n_pages;
    const int32_t t = (int32_t)(item % g.tiles_per_page);
    int64_t first, end;
    fdb_pqw_tile_rows(g, page, t, &first, &end);
    if (first >= end) continue;  // (the whole workgroup)
    const uint64_t page_out = bytes_out[cp];
    if (page_out == FDB_PQW_NONE) continue;
    const FdbPqyCol c = ycols[cp / g.n_pages];
    const bool plain = c.plain != 0;
    stage_validity(c.validity, first, end, tid, s_word, s_before, &s_total);
    __syncthreads();
    const uint32_t n = (uint32_t)(end - first), count = s_total;
    if (count == 0) { __syncthreads(); continue; }  // (the whole workgroup)
    for (uint32_t lr = tid; lr < n; lr += FDB_PQY_THREADS) {
      const uint64_t w = s_word[lr >> 6];
      if ((w >> (lr & 63)) & 1) {
        const uint32_t j = s_before[lr >> 6] + (uint32_t)fdb_pqw_popc(w & ((1ull << (lr & 63)) - 1)), e = c.values[first + lr];
        s_idx[j] = e < c.entries ? e : 0u;  // (an index past the dictionary never gets here: the layout has refused it)
        s_off[j] = fdb_pqy_value_bytes(fdb_pqy_entry_len(c.entry_off, c.entries, e), plain);
      }
    }
    __syncthreads();
    // the costs into exclusive offsets: every thread its FDB_PQY_PER_THREAD ranks, ranks at and past `count` costing nothing
    const uint32_t j0 = (uint32_t)tid * FDB_PQY_PER_THREAD;
    uint32_t mine = 0;
    for (uint32_t i = 0; i < FDB_PQY_PER_THREAD; i++) mine += j0 + i < count ? s_off[j0 + i] : 0u;
    uint32_t inc = mine;
    for (int d = 1; d < 64; d <<= 1) { const uint32_t o = __shfl_up(inc, d, 64); if (lane >= d) inc += o; }
    if (lane == 63) s_wave[wave] = inc;
    __syncthreads();
    uint32_t run = inc - mine;
    for (int q = 0; q < wave; q++) run += s_wave[q];
    for (uint32_t i = 0; i < FDB_PQY_PER_THREAD; i++) {
      const uint32_t cost = j0 + i < count ? s_off[j0 + i] : 0u;
      s_off[j0 + i] = run;
      run += cost;
    }
    if (tid == FDB_PQY_THREADS - 1) s_off[FDB_PQW_TILE] = run;  // (ranks below: s_off[count] is the total by the loop above)
    __syncthreads();
    const uint32_t total = s_off[count];
    if (total > 0) {
      const uint64_t dst = page_out + byte_base[item];
      const uint64_t k1 = fdb_pqy_last_word(dst, total);
      for (uint64_t k = fdb_pqy_first_word(dst) + (uint64_t)tid; k <= k1; k += FDB_PQY_THREADS) {
        uint32_t mask;
        const uint32_t word = fdb_pqy_word(s_off, s_idx, count, plain, c.entry_off, c.entry_bytes, dst, total, k, &mask);
        if (mask == 0xFFFFFFFFu) image32[k] = word;
        else if (word != 0) atomicOr(&image32[k], word);
      }
    }
    __syncthreads();  // (the staging arrays are the next tile's)
  }
}

int grid_for(int64_t items) { return (int)(items < FDB_PQW_MAX_GRID ? (items < 1 ? 1 : items) : FDB_PQW_MAX_GRID); }

}  // namespace

hipError_t fdb_launch_pqy_survey(const FdbPqyCol* ycols, int32_t n_ycols, FdbPqwGeom g, const uint32_t* tile_base, uint64_t* tile_bytes, hipStream_t stream) {
  hipLaunchKernelGGL(pqy_survey_kernel, dim3(grid_for((int64_t)n_ycols * g.n_pages * g.tiles_per_page)), dim3(FDB_PQY_THREADS), 0, stream, ycols, n_ycols, g, tile_base, tile_bytes);
  return hipGetLastError();
}

hipError_t fdb_launch_pqy_encode(const FdbPqyCol* ycols, int32_t n_ycols, FdbPqwGeom g, const uint64_t* bytes_out, const uint64_t* byte_base, unsigned char* image, hipStream_t stream) {
  hipLaunchKernelGGL(pqy_encode_kernel, dim3(grid_for((int64_t)n_ycols * g.n_pages * g.tiles_per_page)), dim3(FDB_PQY_THREADS), 0, stream, ycols, n_ycols, g, bytes_out, byte_base, image);
  return hipGetLastError();
}
