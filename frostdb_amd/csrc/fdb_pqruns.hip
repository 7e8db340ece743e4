// fdb_pqruns.hip — the run passes of the Parquet writer (host side: fdb_pqwrite.cpp; the rule: fdb_pqruns.h). They run beside the passes
// of fdb_pqwrite.hip over the streams — an INDEX column's page values, a column's definition levels — the caller asked to be cut into
// the runs of the RLE / bit-packed hybrid:
//
// pqr_compact_kernel: one workgroup per (value stream, page, tile) of a column WITH a bitmap copies the tile's non-NULL indices to
//   their rank in the page in scratch, as pqd_compact_kernel does for DELTA; a column without a bitmap is read where it is. Levels
//   need none: a group is a byte of the bitmap.
// pqr_survey_kernel / pqr_encode_kernel: one workgroup per (stream, page) walks the page's groups in chunks of FDB_PQR_CHUNK, one
//   group per lane, FROM THE PAGE'S END TOWARDS ITS START, with carried state. Walking backwards, a run's end is met before its start,
//   so at the run's first group its length — which its header's size depends on — is known, and so is the size of everything behind
//   it: every byte's place follows from the stream's total, which the survey leaves and the encoder takes. Per chunk: the keys of the
//   chunk's groups and of FDB_PQR_HALO to either side into LDS; every group's class from that window (fdb_pqr_class); where the class
//   changes a run ends or starts; a max-scan of the run ends gives every group the end of its run, hence at a run's start its length
//   and size; an exclusive sum of the sizes at the starts gives every group the bytes that lie behind its run. The carry is the two
//   scans' last values. The survey stops there. The encoder then has every group of a bit-packed run write its w bytes, and a run's
//   first group the run's header (and an RLE run's value): whole bytes, each with one writer, stored byte by byte.
// Both kernels are one walk (pqr_walk<WRITE>), so what the survey sizes is what the encoder fills. All grids are capped at
// FDB_PQW_MAX_GRID workgroups and strided.
#include "fdb_pqruns.h"

namespace {

#define PQR_WAVES (FDB_PQR_CHUNK / 64)
#define PQR_SYM_STRIDE 9  // a lane's 8 staged symbols + 1: lanes a group apart do not share an LDS bank

// The walk holds more workgroup-wide values than there are scalar registers. The ones that only ever meet per-lane values in
// arithmetic are kept in vector registers instead, and a lane number passed through here is looked at afresh where it is used, so
// that its comparisons are not all kept, as lane masks in scalar registers, for the length of the kernel: nothing is spilled. (An
// empty statement: it emits no instruction.)
template <typename V> __device__ __forceinline__ void in_vgpr(V& v) { asm volatile("" : "+v"(v)); }

// Inclusive scans over the workgroup's FDB_PQR_CHUNK lanes; `s_part`: PQR_WAVES words of LDS. Every lane calls them.
__device__ __forceinline__ uint32_t block_scan_sum(uint32_t v, uint32_t* s_part, uint32_t* total) {
  int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  in_vgpr(lane); in_vgpr(wave);
  for (int d = 1; d < 64; d <<= 1) { const uint32_t o = __shfl_up(v, d, 64); if (lane >= d) v += o; }
  __syncthreads();  // (s_part is free again)
  if (lane == 63) s_part[wave] = v;
  __syncthreads();
  uint32_t before = 0, all = 0;
  for (int q = 0; q < PQR_WAVES; q++) { const uint32_t p = s_part[q]; if (q < wave) before += p; all += p; }
  *total = all;
  return v + before;
}
__device__ __forceinline__ int32_t block_scan_max(int32_t v, int32_t* s_part) {
  int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  in_vgpr(lane); in_vgpr(wave);
  for (int d = 1; d < 64; d <<= 1) { const int32_t o = __shfl_up(v, d, 64); if (lane >= d) v = o > v ? o : v; }
  __syncthreads();
  if (lane == 63) s_part[wave] = v;
  __syncthreads();
  for (int q = 0; q < wave; q++) { const int32_t p = s_part[q]; v = p > v ? p : v; }
  return v;
}

__global__ __launch_bounds__(FDB_PQW_BLOCK) void pqr_compact_kernel(const FdbPqrStream* __restrict__ streams, int32_t n_streams, FdbPqwGeom g, const uint32_t* __restrict__ tile_base) {
  __shared__ uint64_t s_word[FDB_PQW_TILE_WORDS];
  __shared__ uint32_t s_before[FDB_PQW_TILE_WORDS];
  const int tid = threadIdx.x;
  const int64_t per_col = g.n_pages * g.tiles_per_page, items = (int64_t)n_streams * per_col;
  for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
    const FdbPqrStream c = streams[item / per_col];
    if (c.levels != 0 || c.validity == nullptr) continue;  // (the whole workgroup)
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
    uint32_t* dst = c.dense + fdb_pqw_page_first(g, page) + tile_base[((int64_t)c.col * g.n_pages + page) * g.tiles_per_page + t];
    for (uint32_t lr = tid; lr < n; lr += FDB_PQW_BLOCK) {
      const uint64_t w = s_word[lr >> 6];
      if ((w >> (lr & 63)) & 1) dst[s_before[lr >> 6] + (uint32_t)fdb_pqw_popc(w & ((1ull << (lr & 63)) - 1))] = c.values[first + lr];
    }
    __syncthreads();  // (the staging arrays are the next tile's)
  }
}

// The key of group j counted from the page's END (j = 0: the last group, which is the tail when there is one) of a stream of G full
// groups and `tail` more symbols; FDB_PQR_MIXED outside the page and for the tail, whose own key goes to *tail_key. `sym` != nullptr:
// the group's 8 symbols are left there, cut to `mask`, padding zero (value streams); *level_byte: the group's byte (level streams).
__device__ __forceinline__ uint32_t load_key(const FdbPqrStream& c, const uint32_t* __restrict__ dense, const unsigned char* __restrict__ bits, int32_t j, int32_t GG, uint32_t G,
                                             uint32_t tail, uint32_t mask, uint32_t* sym, uint32_t* level_byte, uint32_t* tail_key) {
  if (j < 0 || j >= GG) return FDB_PQR_MIXED;
  const uint32_t i = (uint32_t)(GG - 1 - j), k = i < G ? 8u : tail;
  if (c.levels != 0) {
    const uint32_t byte = (uint32_t)bits[i] & ((1u << k) - 1);
    if (level_byte != nullptr) *level_byte = byte;
    const uint32_t key = fdb_pqr_level_key(byte, k);
    if (i < G) return key;
    *tail_key = key;
    return FDB_PQR_MIXED;
  }
  const uint32_t* src = dense + (uint64_t)i * 8;
  uint32_t first = 0;
  bool same = true;
  for (uint32_t q = 0; q < 8; q++) {
    const uint32_t v = q < k ? src[q] & mask : 0;
    if (q == 0) first = v;
    same = same && (q >= k || v == first);
    if (sym != nullptr) sym[q] = v;
  }
  const uint32_t key = same ? first : FDB_PQR_MIXED;
  if (i < G) return key;
  *tail_key = key;
  return FDB_PQR_MIXED;
}

template <bool WRITE>
__device__ __forceinline__ void pqr_walk(const FdbPqrStream* __restrict__ streams, int32_t n_streams, const FdbPqwGeom& g, const FdbPqwPageStat* __restrict__ stats,
                                         uint32_t* __restrict__ page_bytes, const uint64_t* __restrict__ out, unsigned char* __restrict__ image) {
  __shared__ uint32_t s_key[FDB_PQR_CHUNK + 2 * FDB_PQR_HALO];  // entry x: group j = chunk's first − FDB_PQR_HALO + x
  __shared__ uint32_t s_cls[FDB_PQR_CHUNK + 2];                 // entry y: group j = chunk's first − 1 + y
  __shared__ uint32_t s_sym[WRITE ? FDB_PQR_CHUNK * PQR_SYM_STRIDE : 1];
  __shared__ uint32_t s_part[PQR_WAVES];
  __shared__ uint32_t s_tail_key;
  __shared__ int32_t s_carry_end;
  const int tid = threadIdx.x;
  const int64_t items = (int64_t)n_streams * g.n_pages;
  if (items <= 0) return;
  // (item = which × n_pages + page, kept in step by hand: a 64-bit division inside the loop costs more scalar registers than there are)
  int64_t which = (int64_t)blockIdx.x / g.n_pages, page = (int64_t)blockIdx.x % g.n_pages - gridDim.x;
  for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
    page += gridDim.x;
    while (page >= g.n_pages) { page -= g.n_pages; which++; }
    const FdbPqrStream c = streams[which];
    const FdbPqwPageStat st = stats[(int64_t)c.col * g.n_pages + page];
    const bool levels = c.levels != 0;
    const uint32_t rows = (uint32_t)(fdb_pqw_page_end(g, page) - fdb_pqw_page_first(g, page));
    const bool active = fdb_pqr_active(levels, st.count, rows, st.mn, st.mx);
    uint64_t payload_end = 0;
    if (WRITE) {
      if (!active || out[item] == FDB_PQW_NONE) continue;  // (the whole workgroup)
      payload_end = out[item] + page_bytes[item];
    } else if (!active) {
      if (tid == 0) page_bytes[item] = 0;
      continue;
    }
    const uint32_t n = fdb_pqr_symbols(levels, st.count, rows), w = (uint32_t)c.width, T = fdb_pqr_threshold(w);
    const uint32_t G = n / 8, tail = n % 8, mask = w >= 32 ? 0xFFFFFFFFu : ((1u << w) - 1);
    const int32_t GG = (int32_t)fdb_pqw_groups(n);
    const uint32_t* dense = levels ? nullptr : c.dense + fdb_pqw_page_first(g, page);
    const unsigned char* bits = levels ? c.validity + (fdb_pqw_page_first(g, page) >> 3) : nullptr;
    if (tid == 0) { s_tail_key = FDB_PQR_MIXED; s_carry_end = -1; }
    uint32_t behind = 0;  // the bytes of the runs that lie wholly behind the chunk's
    in_vgpr(payload_end); in_vgpr(dense); in_vgpr(bits); in_vgpr(behind);
    __syncthreads();
    for (int32_t j0 = 0; j0 < GG; j0 += FDB_PQR_CHUNK) {
      int tid = threadIdx.x;
      in_vgpr(tid);
      const int32_t j = j0 + tid;
      const bool valid = j < GG;
      uint32_t level_byte = 0, tk = FDB_PQR_MIXED;
      s_key[FDB_PQR_HALO + tid] = load_key(c, dense, bits, j, GG, G, tail, mask, WRITE && !levels ? &s_sym[tid * PQR_SYM_STRIDE] : nullptr, &level_byte, &tk);
      if (j == 0 && tail > 0) s_tail_key = tk;
      if (tid < 2 * FDB_PQR_HALO) {
        const int x = tid < FDB_PQR_HALO ? tid : FDB_PQR_CHUNK + tid;
        uint32_t unused = FDB_PQR_MIXED;
        s_key[x] = load_key(c, dense, bits, j0 - FDB_PQR_HALO + x, GG, G, tail, mask, nullptr, nullptr, &unused);
      }
      __syncthreads();
      for (int y = tid; y < FDB_PQR_CHUNK + 2; y += FDB_PQR_CHUNK) {
        const int32_t jy = j0 - 1 + y, x = y + FDB_PQR_HALO - 1;
        uint32_t cls = FDB_PQR_MIXED;
        if (jy >= 0 && jy < GG) {
          if (jy == 0 && tail > 0) cls = fdb_pqr_tail_class(s_tail_key, GG >= 2, GG >= 2 ? fdb_pqr_class(s_key, x + 1, 0, FDB_PQR_CHUNK + 2 * FDB_PQR_HALO, T) : FDB_PQR_MIXED);
          else cls = fdb_pqr_class(s_key, x, 0, FDB_PQR_CHUNK + 2 * FDB_PQR_HALO, T);
        }
        s_cls[y] = cls;
      }
      __syncthreads();
      const uint32_t cls = s_cls[tid + 1];
      const bool ends = valid && (j == 0 || s_cls[tid] != cls);           // the last group of its run
      const bool starts = valid && (j == GG - 1 || s_cls[tid + 2] != cls);  // the first
      int32_t run_end = block_scan_max(ends ? j : -1, (int32_t*)s_part);
      const int32_t carried = s_carry_end;
      run_end = carried > run_end ? carried : run_end;
      const uint32_t len = valid ? (uint32_t)(j - run_end + 1) : 0;       // groups of the run from this one to its end
      const uint32_t symbols = len * 8 - (run_end == 0 && tail > 0 ? 8 - tail : 0);
      const uint32_t size = !starts ? 0 : cls == FDB_PQR_MIXED ? fdb_pqr_packed_bytes(len, w) : fdb_pqr_rle_bytes(symbols, w);
      uint32_t total;
      const uint32_t inc = block_scan_sum(size, s_part, &total);
      if (WRITE && valid) {
        const uint64_t run_stop = payload_end - (behind + inc - size);     // where the run's bytes end
        if (cls == FDB_PQR_MIXED) {
          unsigned char* p = image + run_stop - (uint64_t)len * w;
          if (levels) p[0] = (unsigned char)level_byte;
          else for (uint32_t b = 0; b < w; b++) p[b] = fdb_pqr_group_byte(&s_sym[tid * PQR_SYM_STRIDE], w, b);
        }
        if (starts) {
          unsigned char* p = image + run_stop - size;
          const uint32_t head = cls == FDB_PQR_MIXED ? fdb_pqr_packed_header(len) : fdb_pqr_rle_header(symbols), hl = fdb_pqr_varint_len(head);
          for (uint32_t b = 0; b < hl; b++) p[b] = fdb_pqr_varint_byte(head, b);
          if (cls != FDB_PQR_MIXED)
            for (uint32_t b = 0; b < fdb_pqr_value_bytes(w); b++) p[hl + b] = (unsigned char)(cls >> (8 * b));
        }
      }
      behind += total;
      __syncthreads();  // (everyone has read s_carry_end, s_key, s_cls and s_sym)
      if (tid == FDB_PQR_CHUNK - 1) s_carry_end = run_end;
    }
    __syncthreads();
    if (!WRITE && tid == 0) page_bytes[item] = behind;
  }
}

__global__ __launch_bounds__(FDB_PQR_CHUNK) void pqr_survey_kernel(const FdbPqrStream* __restrict__ streams, int32_t n_streams, FdbPqwGeom g, const FdbPqwPageStat* __restrict__ stats,
                                                                   uint32_t* __restrict__ page_bytes) {
  pqr_walk<false>(streams, n_streams, g, stats, page_bytes, nullptr, nullptr);
}

__global__ __launch_bounds__(FDB_PQR_CHUNK) void pqr_encode_kernel(const FdbPqrStream* __restrict__ streams, int32_t n_streams, FdbPqwGeom g, const FdbPqwPageStat* __restrict__ stats,
                                                                   const uint32_t* __restrict__ page_bytes, const uint64_t* __restrict__ out, unsigned char* __restrict__ image) {
  pqr_walk<true>(streams, n_streams, g, stats, const_cast<uint32_t*>(page_bytes), out, image);
}

int grid_for(int64_t items) { return (int)(items < FDB_PQW_MAX_GRID ? (items < 1 ? 1 : items) : FDB_PQW_MAX_GRID); }

}  // namespace

hipError_t fdb_launch_pqr_compact(const FdbPqrStream* streams, int32_t n_streams, FdbPqwGeom g, const uint32_t* tile_base, hipStream_t stream) {
  hipLaunchKernelGGL(pqr_compact_kernel, dim3(grid_for((int64_t)n_streams * g.n_pages * g.tiles_per_page)), dim3(FDB_PQW_BLOCK), 0, stream, streams, n_streams, g, tile_base);
  return hipGetLastError();
}

hipError_t fdb_launch_pqr_survey(const FdbPqrStream* streams, int32_t n_streams, FdbPqwGeom g, const FdbPqwPageStat* stats, uint32_t* page_bytes, hipStream_t stream) {
  hipLaunchKernelGGL(pqr_survey_kernel, dim3(grid_for((int64_t)n_streams * g.n_pages)), dim3(FDB_PQR_CHUNK), 0, stream, streams, n_streams, g, stats, page_bytes);
  return hipGetLastError();
}

hipError_t fdb_launch_pqr_encode(const FdbPqrStream* streams, int32_t n_streams, FdbPqwGeom g, const FdbPqwPageStat* stats, const uint32_t* page_bytes, const uint64_t* out,
                                 unsigned char* image, hipStream_t stream) {
  hipLaunchKernelGGL(pqr_encode_kernel, dim3(grid_for((int64_t)n_streams * g.n_pages)), dim3(FDB_PQR_CHUNK), 0, stream, streams, n_streams, g, stats, page_bytes, out, image);
  return hipGetLastError();
}
