// fdb_pqsnappy.hip — the SNAPPY passes of the Parquet writer (host side: fdb_pqwrite.cpp; the rule: fdb_pqsnappy.h). They run after the
// encode passes have written the uncompressed file body into a staging image in HBM, over the pages of the columns asked to be SNAPPY:
//
// pqs_place_kernel: the few bytes per page the host contributes inside a page body (level length and run header, index width byte, run
//   header or RLE run) go from an uploaded blob into the staging image, one thread a piece — a body has to be whole before it is compressed.
// pqs_compress_kernel: one WAVE per fragment (FDB_PQS_FRAGMENT bytes of one page body), with a table of its own in LDS. The fragment is
//   walked in windows of 64 positions, a lane a position: each lane looks its 4 bytes up in the table (positions before the window) and,
//   by shuffles, in the FDB_PQS_NEAR lanes below it (positions inside the window — runs and values repeated with a short period, which
//   the table cannot see yet); a ballot finds the lowest lane with a candidate, and the wave does the rest together: the pending literal goes out,
//   the match is extended 64 bytes at a compare + ballot, the copy goes out as elements, the table is filled up to the new cursor with
//   atomicMax of the position — the largest position wins whatever lane comes first, and the wave waits before it looks anything up.
//   The elements go to the fragment's slot of scratch (Snappy's bound), the byte count to frag_bytes.
// pqs_scan_kernel: one wave per page sums its fragments' sizes 64 at a step: each fragment's offset inside the page's block, the page's
//   size — which is all the host reads back to lay the final file out.
// pqs_gather_kernel: one workgroup per fragment moves its elements to their final file bytes, and one per piece of an uncompressed
//   column's chunk moves that from the staging image as it is. One launch fills the final image.
// All grids are capped and strided: at FDB_PQW_MAX_GRID workgroups, the compress kernel's — whose waves spend their time waiting for one
// load after the other — at FDB_PQS_COMPRESS_GRID, as many as the LDS lets a chip of 256 CUs hold.
#include "fdb_pqsnappy.h"

namespace {

// The lanes of one wave have written LDS and are about to read what the others wrote (or the other way round).
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ uint32_t lowest_lane(unsigned long long mask) { return mask != 0ull ? (uint32_t)__builtin_ctzll(mask) : 64u; }

// `len` bytes src → dst at any alignment, by the 64 lanes of a wave (or the `threads` threads of a workgroup).
__device__ __forceinline__ void copy_bytes(const unsigned char* __restrict__ src, unsigned char* __restrict__ dst, uint32_t len, uint32_t tid, uint32_t threads) {
  for (uint32_t i = tid * 4; i + 4 <= len; i += threads * 4) { const uint32_t x = fdb_pqs_load32(src + i); __builtin_memcpy(dst + i, &x, 4); }
  const uint32_t r = len & ~3u;
  if (r + tid < len) dst[r + tid] = src[r + tid];
}

__device__ __forceinline__ uint32_t emit_literal(const unsigned char* __restrict__ src, uint32_t from, uint32_t to, unsigned char* __restrict__ out, uint32_t o, uint32_t lane) {
  const uint32_t L = to - from;
  if (L == 0) return o;
  const uint32_t tl = fdb_pqs_literal_tag_len(L);
  if (lane < tl) out[o + lane] = fdb_pqs_literal_tag_byte(L, lane);
  copy_bytes(src + from, out + o + tl, L, lane, 64);
  return o + tl + L;
}

__device__ __forceinline__ uint32_t emit_copy(uint32_t len, uint32_t off, unsigned char* __restrict__ out, uint32_t o, uint32_t lane) {
  const uint32_t full = fdb_pqs_copy_full(len), mid = fdb_pqs_copy_mid(len), rest = fdb_pqs_copy_rest(len);
  for (uint32_t k = lane; k < full; k += 64)
    for (uint32_t i = 0; i < 3; i++) out[o + 3 * k + i] = fdb_pqs_copy_elem_byte(64, off, i);
  o += 3 * full;
  if (mid != 0) {
    if (lane < 3) out[o + lane] = fdb_pqs_copy_elem_byte(mid, off, lane);
    o += 3;
  }
  const uint32_t el = fdb_pqs_copy_elem_len(rest, off);
  if (lane < el) out[o + lane] = fdb_pqs_copy_elem_byte(rest, off, lane);
  return o + el;
}

__global__ __launch_bounds__(256) void pqs_place_kernel(const FdbPqsRange* __restrict__ ranges, int32_t n_ranges, const unsigned char* __restrict__ blob, unsigned char* __restrict__ image) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_ranges; i += (int64_t)gridDim.x * blockDim.x) {
    const FdbPqsRange r = ranges[i];
    for (uint32_t b = 0; b < r.len; b++) image[r.dst_off + b] = blob[r.src_off + b];
  }
}

__global__ __launch_bounds__(FDB_PQS_THREADS) void pqs_compress_kernel(const FdbPqsFrag* __restrict__ frags, int32_t n_frags, const unsigned char* __restrict__ staging,
                                                                        unsigned char* __restrict__ scratch, uint32_t* __restrict__ frag_bytes) {
  __shared__ uint32_t s_table[FDB_PQS_WAVES][FDB_PQS_TABLE];
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t* table = s_table[wave];
  for (int64_t item = (int64_t)blockIdx.x * FDB_PQS_WAVES + wave; item < n_frags; item += (int64_t)gridDim.x * FDB_PQS_WAVES) {
    const FdbPqsFrag f = frags[item];
    const unsigned char* src = staging + f.src_off;
    unsigned char* out = scratch + (uint64_t)item * fdb_pqs_slot_bytes();
    const uint32_t n = f.len;
    wave_sync();  // (the last fragment's lookups are done)
    for (uint32_t i = lane; i < FDB_PQS_TABLE; i += 64) table[i] = 0;
    wave_sync();
    uint32_t cursor = 0, lit = 0, filled = 0, o = 0;
    uint32_t ahead = 0, ahead_at = ~0u;  // the 4 bytes of the position 64 further, loaded while this window is searched: the next window's, if nothing matches here
    while (cursor + 4 <= n) {
      const uint32_t p = cursor + lane;
      const bool valid = p + 4 <= n;
      uint32_t x;
      if (ahead_at == cursor) x = ahead;
      else x = valid ? fdb_pqs_load32(src + p) : 0;
      const uint32_t t = valid ? table[fdb_pqs_hash(x)] : 0;
      const bool t_hit = t != 0 && fdb_pqs_load32(src + t - 1) == x;  // (t − 1 < cursor: 4 bytes are left there)
      ahead = p + FDB_PQS_WINDOW + 4 <= n ? fdb_pqs_load32(src + p + FDB_PQS_WINDOW) : 0;
      ahead_at = cursor + FDB_PQS_WINDOW;
      const unsigned long long t_mask = __ballot(t_hit);
      unsigned long long w_mask = 0;  // the lanes with a candidate inside the window, best_d back
      uint32_t best_d = 0, w = lowest_lane(t_mask);
      // the lanes up to the lowest one with a candidate try every distance up to FDB_PQS_NEAR, down to the window's first position:
      // a lane l has tried them all once d reaches l, so when d passes w no lane below w can turn up any more, and w's own nearest
      // is found. Eight distances at a step, so that the shuffles do not wait for each other's ballot (a distance past w finds
      // nothing below w).
      static_assert(FDB_PQS_NEAR % 8 == 0 && FDB_PQS_NEAR < FDB_PQS_WINDOW, "the distances are tried eight at a step");
      for (uint32_t d0 = 1; d0 <= FDB_PQS_NEAR && d0 <= w; d0 += 8) {
#pragma unroll
        for (uint32_t k = 0; k < 8; k++) {
          const uint32_t d = d0 + k;  // (FDB_PQS_NEAR at the most)
          const uint32_t y = (uint32_t)__shfl_up((int)x, d, 64);
          if (valid && lane >= d && y == x && best_d == 0) best_d = d;
        }
        w_mask = __ballot(best_d != 0);
        w = lowest_lane(w_mask | t_mask);
      }
      if (w < 64) {
        const uint32_t win = cursor + w, wd = (uint32_t)__shfl((int)best_d, (int)w, 64), wt = (uint32_t)__shfl((int)t, (int)w, 64);
        const uint32_t cand = wd != 0 ? win - wd : wt - 1;
        uint32_t len = 4;
        for (;;) {
          const uint32_t i = len + lane;
          const bool same = win + i < n && src[cand + i] == src[win + i];
          const unsigned long long mask = __ballot(same);
          if (mask != ~0ull) { len += (uint32_t)__builtin_ctzll(~mask); break; }
          len += 64;
        }
        o = emit_literal(src, lit, win, out, o, lane);
        o = emit_copy(len, win - cand, out, o, lane);
        cursor = lit = win + len;
      } else {  // the window's own positions go into the table with the bytes the lanes hold (filled == cursor at a window's start)
        wave_sync();
        if (valid) atomicMax(&table[fdb_pqs_hash(x)], p + 1);
        cursor += FDB_PQS_WINDOW;
        filled = cursor;
        wave_sync();
        continue;
      }
      wave_sync();  // (every lane has looked up what it wanted)
      for (uint32_t base = filled; base < cursor; base += 64) {
        const uint32_t q = base + lane;
        if (q < cursor && q + 4 <= n) atomicMax(&table[fdb_pqs_hash(fdb_pqs_load32(src + q))], q + 1);
      }
      filled = cursor;
      wave_sync();
    }
    o = emit_literal(src, lit, n, out, o, lane);
    if (lane == 0) frag_bytes[item] = o;
  }
}

__global__ __launch_bounds__(FDB_PQS_THREADS) void pqs_scan_kernel(const FdbPqsPage* __restrict__ pages, int32_t n_pages, const uint32_t* __restrict__ frag_bytes,
                                                                    uint32_t* __restrict__ frag_off, uint32_t* __restrict__ page_bytes) {
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int64_t item = (int64_t)blockIdx.x * FDB_PQS_WAVES + wave; item < n_pages; item += (int64_t)gridDim.x * FDB_PQS_WAVES) {
    const FdbPqsPage pg = pages[item];
    uint32_t run = 0;
    for (uint32_t f0 = 0; f0 < pg.n_frags; f0 += 64) {
      const uint32_t i = f0 + lane, bytes = i < pg.n_frags ? frag_bytes[pg.first_frag + i] : 0;
      uint32_t inc = bytes;
      for (int d = 1; d < 64; d <<= 1) { const uint32_t v = (uint32_t)__shfl_up((int)inc, d, 64); if (lane >= (uint32_t)d) inc += v; }
      if (i < pg.n_frags) frag_off[pg.first_frag + i] = run + inc - bytes;
      run += (uint32_t)__shfl((int)inc, 63, 64);
    }
    if (lane == 0) page_bytes[item] = run;
  }
}

__global__ __launch_bounds__(FDB_PQW_BLOCK) void pqs_gather_kernel(const FdbPqsFrag* __restrict__ frags, int32_t n_frags, const uint32_t* __restrict__ frag_bytes,
                                                                    const uint32_t* __restrict__ frag_off, const uint64_t* __restrict__ page_dst, const unsigned char* __restrict__ scratch,
                                                                    const FdbPqsRange* __restrict__ ranges, int32_t n_ranges, const unsigned char* __restrict__ staging,
                                                                    unsigned char* __restrict__ final_image) {
  const int64_t items = (int64_t)n_frags + n_ranges;
  for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
    if (item < n_frags) {
      copy_bytes(scratch + (uint64_t)item * fdb_pqs_slot_bytes(), final_image + page_dst[frags[item].page] + frag_off[item], frag_bytes[item], threadIdx.x, FDB_PQW_BLOCK);
    } else {
      const FdbPqsRange r = ranges[item - n_frags];
      copy_bytes(staging + r.src_off, final_image + r.dst_off, r.len, threadIdx.x, FDB_PQW_BLOCK);
    }
  }
}

int grid_for(int64_t items, int64_t cap = FDB_PQW_MAX_GRID) { return (int)(items < cap ? (items < 1 ? 1 : items) : cap); }
int64_t wave_groups(int64_t items) { return (items + FDB_PQS_WAVES - 1) / FDB_PQS_WAVES; }

}  // namespace

hipError_t fdb_launch_pqs_place(const FdbPqsRange* ranges, int32_t n_ranges, const unsigned char* blob, unsigned char* image, hipStream_t stream) {
  if (n_ranges <= 0) return hipSuccess;
  hipLaunchKernelGGL(pqs_place_kernel, dim3(grid_for(((int64_t)n_ranges + 255) / 256)), dim3(256), 0, stream, ranges, n_ranges, blob, image);
  return hipGetLastError();
}

hipError_t fdb_launch_pqs_compress(const FdbPqsFrag* frags, int32_t n_frags, const unsigned char* staging, unsigned char* scratch, uint32_t* frag_bytes, hipStream_t stream) {
  if (n_frags <= 0) return hipSuccess;
  hipLaunchKernelGGL(pqs_compress_kernel, dim3(grid_for(wave_groups(n_frags), FDB_PQS_COMPRESS_GRID)), dim3(FDB_PQS_THREADS), 0, stream, frags, n_frags, staging, scratch, frag_bytes);
  return hipGetLastError();
}

hipError_t fdb_launch_pqs_scan(const FdbPqsPage* pages, int32_t n_pages, const uint32_t* frag_bytes, uint32_t* frag_off, uint32_t* page_bytes, hipStream_t stream) {
  if (n_pages <= 0) return hipSuccess;
  hipLaunchKernelGGL(pqs_scan_kernel, dim3(grid_for(wave_groups(n_pages))), dim3(FDB_PQS_THREADS), 0, stream, pages, n_pages, frag_bytes, frag_off, page_bytes);
  return hipGetLastError();
}

hipError_t fdb_launch_pqs_gather(const FdbPqsFrag* frags, int32_t n_frags, const uint32_t* frag_bytes, const uint32_t* frag_off, const uint64_t* page_dst, const unsigned char* scratch,
                                 const FdbPqsRange* ranges, int32_t n_ranges, const unsigned char* staging, unsigned char* final_image, hipStream_t stream) {
  if ((int64_t)n_frags + n_ranges <= 0) return hipSuccess;
  hipLaunchKernelGGL(pqs_gather_kernel, dim3(grid_for((int64_t)n_frags + n_ranges)), dim3(FDB_PQW_BLOCK), 0, stream, frags, n_frags, frag_bytes, frag_off, page_dst, scratch, ranges,
                     n_ranges, staging, final_image);
  return hipGetLastError();
}
