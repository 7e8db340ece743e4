// fdb_pqlz4.hip — the LZ4_RAW passes of the Parquet writer (host side: fdb_pqwrite.cpp; the rule: fdb_pqlz4.h). They run beside the
// SNAPPY passes over the same staging image, over the pages of the columns asked to be LZ4_RAW; the host's bytes inside those bodies
// have been placed by pqs_place_kernel, and the chunks of uncompressed columns keep moving through pqs_gather_kernel's ranges.
//
// pql_compress_kernel: one WAVE per fragment, with a table of its own in LDS, searching as pqs_compress_kernel does (fdb_pqs_find /
//   _extend / _fill of fdb_pqsnappy.h) within the fragment's `stop` and `reach`. A fragment cannot know how many literals its first
//   sequence holds, so it leaves head, tail and the first match's length in outs[f] and, in its slot of scratch, the middle: the first
//   match's offset and extension, then every later sequence whole.
// pql_scan_kernel: one wave per page, lane 0 walking the page's fragments in order with the carry — a reset-or-add scan, done serially
//   so that it is the host walk's loop whatever the number of fragments: each fragment's offset in the block and its joined run, the
//   closing sequence's, and the page's size, which is all the host reads back.
// pql_gather_kernel: one workgroup per fragment with a match writes token, extension and the joined run of literals — read from the
//   staging image starting `carry` bytes in front of the fragment — then the middle; one per page writes the closing sequence.
// All grids are capped and strided as the SNAPPY ones are.
#include "fdb_pqlz4.h"

namespace {

// The extension bytes of the length v, by the lanes of a wave (or the threads of a workgroup).
__device__ __forceinline__ uint32_t emit_ext(uint32_t v, unsigned char* __restrict__ out, uint32_t tid, uint32_t threads) {
  const uint32_t el = fdb_pql_ext_len(v);
  for (uint32_t i = tid; i < el; i += threads) out[i] = fdb_pql_ext_byte(v, i);
  return el;
}

// A sequence's front — token, literal extension, the literals src[0 … literals) — to out[0 …]; returns its bytes.
__device__ __forceinline__ uint32_t emit_run(const unsigned char* __restrict__ src, uint32_t literals, uint32_t match_len, unsigned char* __restrict__ out, uint32_t tid, uint32_t threads) {
  if (tid == 0) out[0] = fdb_pql_token(literals, match_len);
  const uint32_t el = emit_ext(literals, out + 1, tid, threads);
  fdb_pqs_copy_bytes(src, out + 1 + el, literals, tid, threads);
  return 1 + el + literals;
}

__global__ __launch_bounds__(FDB_PQS_THREADS) void pql_compress_kernel(const FdbPqlFrag* __restrict__ frags, int32_t n_frags, const unsigned char* __restrict__ staging,
                                                                        unsigned char* __restrict__ scratch, FdbPqlOut* __restrict__ outs) {
  __shared__ uint32_t s_table[FDB_PQS_WAVES][FDB_PQS_TABLE];
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t* table = s_table[wave];
  for (int64_t item = (int64_t)blockIdx.x * FDB_PQS_WAVES + wave; item < n_frags; item += (int64_t)gridDim.x * FDB_PQS_WAVES) {
    const FdbPqlFrag f = frags[item];
    const unsigned char* src = staging + f.src_off;
    unsigned char* mid = scratch + (uint64_t)item * fdb_pql_slot_bytes();
    const uint32_t n = f.len, stop = f.stop, reach = f.reach;
    fdb_pqs_wave_sync();  // (the last fragment's lookups are done)
    for (uint32_t i = lane; i < FDB_PQS_TABLE; i += 64) table[i] = 0;
    fdb_pqs_wave_sync();
    uint32_t cursor = 0, lit = 0, filled = 0, o = 0, head = n, first_len = 0;
    FdbPqsAhead ahead;
    while (cursor < stop) {
      uint32_t win, cand;
      if (!fdb_pqs_find(src, cursor, stop, table, lane, &ahead, &win, &cand)) {  // (the window's own positions are in the table)
        cursor += FDB_PQS_WINDOW;
        filled = cursor;
        continue;
      }
      const uint32_t len = fdb_pqs_extend(src, win, cand, reach, lane), off = win - cand;
      if (first_len == 0) { head = win; first_len = len; }
      else o += emit_run(src + lit, win - lit, len, mid + o, lane, 64);
      if (lane < 2) mid[o + lane] = (unsigned char)(off >> (8 * lane));
      o += 2 + emit_ext(len - 4, mid + o + 2, lane, 64);
      cursor = lit = win + len;
      fdb_pqs_fill(src, table, filled, cursor, stop, lane);
      filled = cursor;
    }
    if (lane == 0) outs[item] = first_len != 0 ? FdbPqlOut{head, n - lit, first_len, o} : FdbPqlOut{n, 0, 0, 0};
  }
}

__global__ __launch_bounds__(FDB_PQS_THREADS) void pql_scan_kernel(const FdbPqlPage* __restrict__ pages, int32_t n_pages, const FdbPqlOut* __restrict__ outs,
                                                                    FdbPqlPlace* __restrict__ places, FdbPqlPlace* __restrict__ closes, uint32_t* __restrict__ page_bytes) {
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int64_t item = (int64_t)blockIdx.x * FDB_PQS_WAVES + wave; item < n_pages; item += (int64_t)gridDim.x * FDB_PQS_WAVES) {
    if (lane != 0) continue;
    const FdbPqlPage pg = pages[item];
    uint32_t at = 0, carry = 0;
    for (uint32_t i = 0; i < pg.n_frags; i++) {
      const FdbPqlOut r = outs[pg.first_frag + i];
      if (r.first_len == 0) { carry += r.head; continue; }
      const uint32_t run = carry + r.head;
      places[pg.first_frag + i] = FdbPqlPlace{at, run};
      at += 1 + fdb_pql_ext_len(run) + run + r.mid_bytes;
      carry = r.tail;
    }
    closes[item] = FdbPqlPlace{at, carry};
    page_bytes[item] = at + 1 + fdb_pql_ext_len(carry) + carry;
  }
}

__global__ __launch_bounds__(FDB_PQW_BLOCK) void pql_gather_kernel(const FdbPqlFrag* __restrict__ frags, int32_t n_frags, const FdbPqlPage* __restrict__ pages, int32_t n_pages,
                                                                    const FdbPqlOut* __restrict__ outs, const FdbPqlPlace* __restrict__ places, const FdbPqlPlace* __restrict__ closes,
                                                                    const uint64_t* __restrict__ page_dst, const unsigned char* __restrict__ scratch,
                                                                    const unsigned char* __restrict__ staging, unsigned char* __restrict__ final_image) {
  const int64_t items = (int64_t)n_frags + n_pages;
  for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
    if (item < n_frags) {
      const FdbPqlOut r = outs[item];
      if (r.first_len == 0) continue;  // (its bytes are literals of a later fragment's run, or of the closing sequence)
      const FdbPqlFrag f = frags[item];
      const FdbPqlPlace pl = places[item];
      unsigned char* dst = final_image + page_dst[f.page] + pl.off;
      const uint32_t front = emit_run(staging + f.src_off - (pl.run - r.head), pl.run, r.first_len, dst, threadIdx.x, FDB_PQW_BLOCK);
      fdb_pqs_copy_bytes(scratch + (uint64_t)item * fdb_pql_slot_bytes(), dst + front, r.mid_bytes, threadIdx.x, FDB_PQW_BLOCK);
    } else {
      const int64_t page = item - n_frags;
      const FdbPqlPlace cl = closes[page];
      emit_run(staging + pages[page].src_end - cl.run, cl.run, 0, final_image + page_dst[page] + cl.off, threadIdx.x, FDB_PQW_BLOCK);
    }
  }
}

int grid_for(int64_t items, int64_t cap = FDB_PQW_MAX_GRID) { return (int)(items < cap ? (items < 1 ? 1 : items) : cap); }
int64_t wave_groups(int64_t items) { return (items + FDB_PQS_WAVES - 1) / FDB_PQS_WAVES; }

}  // namespace

hipError_t fdb_launch_pql_compress(const FdbPqlFrag* frags, int32_t n_frags, const unsigned char* staging, unsigned char* scratch, FdbPqlOut* outs, hipStream_t stream) {
  if (n_frags <= 0) return hipSuccess;
  hipLaunchKernelGGL(pql_compress_kernel, dim3(grid_for(wave_groups(n_frags), FDB_PQS_COMPRESS_GRID)), dim3(FDB_PQS_THREADS), 0, stream, frags, n_frags, staging, scratch, outs);
  return hipGetLastError();
}

hipError_t fdb_launch_pql_scan(const FdbPqlPage* pages, int32_t n_pages, const FdbPqlOut* outs, FdbPqlPlace* places, FdbPqlPlace* closes, uint32_t* page_bytes, hipStream_t stream) {
  if (n_pages <= 0) return hipSuccess;
  hipLaunchKernelGGL(pql_scan_kernel, dim3(grid_for(wave_groups(n_pages))), dim3(FDB_PQS_THREADS), 0, stream, pages, n_pages, outs, places, closes, page_bytes);
  return hipGetLastError();
}

hipError_t fdb_launch_pql_gather(const FdbPqlFrag* frags, int32_t n_frags, const FdbPqlPage* pages, int32_t n_pages, const FdbPqlOut* outs, const FdbPqlPlace* places,
                                 const FdbPqlPlace* closes, const uint64_t* page_dst, const unsigned char* scratch, const unsigned char* staging, unsigned char* final_image,
                                 hipStream_t stream) {
  if ((int64_t)n_frags + n_pages <= 0) return hipSuccess;
  hipLaunchKernelGGL(pql_gather_kernel, dim3(grid_for((int64_t)n_frags + n_pages)), dim3(FDB_PQW_BLOCK), 0, stream, frags, n_frags, pages, n_pages, outs, places, closes, page_dst,
                     scratch, staging, final_image);
  return hipGetLastError();
}
