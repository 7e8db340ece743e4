// frostdb_amd — the kernels of the device MergeRecords (fdb_mergerec.cpp; the merge-path arithmetic is fdb_mergepath.h): the order check
// of one input's keys, the partition and merge kernels of one round of the pairwise merge tree, and the gather that copies every column of
// the result out of the K inputs. In a translation unit of its own, like fdb_sortkeys.hip.
//
// One round merges neighbouring runs pairwise, all pairs in one launch. Keys are W 64-bit words per row held word-major (word w of
// position g at keys[w * stride + g]), the payload is the row's position among the concatenated inputs (uint32). A pair's output is cut
// into tiles of fdb_merge_tile(W) rows; merge_partition_kernel gives one lane to every tile boundary and binary-searches its diagonal in
// global memory; merge_tile_kernel<W> gives one workgroup to a tile: it stages the tile's A range and B range (keys and payloads) into
// LDS with 16-byte loads, every lane finds its own diagonal in LDS and merges fdb_merge_items(W) consecutive outputs serially, and keys
// and payloads leave through LDS as 16-byte stores in output order. LDS image: tile × (8 W + 4) bytes — 24 KiB at W = 1 (six workgroups
// on a CU's 160 KiB), 40 KiB at W = 2, 28 / 36 KiB at W = 3 / 4. The serial phase reads LDS at a stride of `items` keys between
// neighbouring lanes (8 keys = 16 banks at W <= 2: up to 4 lanes of a 32-lane group meet on a bank when a tile's lanes advance evenly
// through one run); measured cost and what would remove it are in DESIGN §4. Keys of more than FDB_MERGE_LDS_WORDS words (and the key of
// no words at all: everything ties) take merge_tile_kernel_any, which has W at run time and merges straight out of global memory.
//
// Every kernel checks what it indexes with: a tile whose splits cross, leave the runs or do not add up to the tile is not merged (the
// error word is set instead — the host has checked the inputs' order before the first round, so this does not happen), and the gather
// leaves a row whose position lies in no input NULL instead of reading it.
#include <hip/hip_runtime.h>

#include "fdb_mergepath.h"

namespace {

#define FDB_GLOBAL __attribute__((address_space(1)))

typedef unsigned long long u64;
typedef u64 u64x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// ---- order check ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(FDB_MERGE_BLOCK) void merge_order_kernel(const u64* __restrict__ keys, const int64_t stride, const int words, const int64_t off,
                                                                      const int64_t len, uint32_t* __restrict__ first_bad) {
  const int64_t i = (int64_t)blockIdx.x * FDB_MERGE_BLOCK + threadIdx.x + 1;
  if (i >= len) return;
  const uint64_t* k = (const uint64_t*)keys;
  if (!fdb_mp_le(k, stride, off + i - 1, k, stride, off + i, words)) atomicMin(first_bad, (uint32_t)i);
}

// ---- one round -----------------------------------------------------------------------------------------------------------------------------
// the pair whose tiles (by_boundary: whose tile boundaries) hold `q`: the last one that starts at or before it
__device__ __forceinline__ int pair_of(const FdbMergePair* __restrict__ pairs, const int n_pairs, const int64_t q, const bool by_boundary) {
  int lo = 0, hi = n_pairs - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (pairs[mid].tile_first + (by_boundary ? mid : 0) <= q) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

__global__ __launch_bounds__(FDB_MERGE_BLOCK) void merge_partition_kernel(const FdbMergeArgs a) {
  const int64_t q = (int64_t)blockIdx.x * FDB_MERGE_BLOCK + threadIdx.x;
  if (q >= a.n_tiles + a.n_pairs) return;
  const int p = pair_of(a.pairs, a.n_pairs, q, true);
  const FdbMergePair P = a.pairs[p];
  const int64_t t = q - (P.tile_first + p), T = fdb_merge_tile(a.words);
  const int64_t d = t * T < P.n_out ? t * T : P.n_out;
  const uint64_t* k = (const uint64_t*)a.src_keys;
  a.splits[q] = (uint32_t)fdb_mp_diagonal(k + P.a_off, a.stride, P.na, k + P.b_off, a.stride, P.nb, d, a.words);
}

struct Tile { int64_t a0, b0, out0; int ta, tb; bool ok; };

// the ranges of tile `b` (a workgroup's), checked: ok == false leaves nothing to index with
__device__ __forceinline__ Tile tile_of(const FdbMergeArgs& a, const int64_t b, const int T) {
  const int p = pair_of(a.pairs, a.n_pairs, b, false);
  const FdbMergePair P = a.pairs[p];
  const int64_t t = b - P.tile_first, q = P.tile_first + p + t;
  const int64_t s0 = a.splits[q], s1 = a.splits[q + 1];
  const int64_t d0 = t * T, d1 = d0 + T < P.n_out ? d0 + T : P.n_out;
  Tile r;
  r.a0 = P.a_off + s0; r.b0 = P.b_off + (d0 - s0); r.out0 = P.out_off + d0;
  const int64_t ta = s1 - s0, tb = (d1 - s1) - (d0 - s0);
  r.ta = (int)ta; r.tb = (int)tb;
  r.ok = d1 > d0 && ta >= 0 && tb >= 0 && s0 <= d0 && s1 <= P.na && d1 - s1 <= P.nb && ta + tb == d1 - d0;
  return r;
}

// `count` elements from src[start …) to LDS, 16 bytes per load (src's base is 16-byte aligned; its allocation is readable a chunk past
// any element)
__device__ __forceinline__ void stage_u64(u64* dst, const u64* __restrict__ src, const int64_t start, const int count) {
  const int64_t g0 = start & ~(int64_t)1;
  const int chunks = (int)((start + count - g0 + 1) >> 1);
  for (int c = threadIdx.x; c < chunks; c += FDB_MERGE_BLOCK) {
    const u64x2 v = *(const FDB_GLOBAL u64x2*)(src + g0 + 2 * c);
    const int i = (int)(g0 + 2 * c - start);
    if (i >= 0 && i < count) dst[i] = v.x;
    if (i + 1 < count) dst[i + 1] = v.y;
  }
}

__device__ __forceinline__ void stage_u32(uint32_t* dst, const uint32_t* __restrict__ src, const int64_t start, const int count) {
  const int64_t g0 = start & ~(int64_t)3;
  const int chunks = (int)((start + count - g0 + 3) >> 2);
  for (int c = threadIdx.x; c < chunks; c += FDB_MERGE_BLOCK) {
    const u32x4 v = *(const FDB_GLOBAL u32x4*)(src + g0 + 4 * c);
    const int i = (int)(g0 + 4 * c - start);
    if (i >= 0 && i < count) dst[i] = v.x;
    if (i + 1 >= 0 && i + 1 < count) dst[i + 1] = v.y;
    if (i + 2 >= 0 && i + 2 < count) dst[i + 2] = v.z;
    if (i + 3 < count) dst[i + 3] = v.w;
  }
}

// `count` elements from LDS to dst[start …): whole 16-byte chunks with one store, the ragged ends element by element
__device__ __forceinline__ void unstage_u64(u64* __restrict__ dst, const int64_t start, const int count, const u64* src) {
  const int64_t g0 = start & ~(int64_t)1;
  const int chunks = (int)((start + count - g0 + 1) >> 1);
  for (int c = threadIdx.x; c < chunks; c += FDB_MERGE_BLOCK) {
    const int i = (int)(g0 + 2 * c - start);
    if (i >= 0 && i + 1 < count) {
      u64x2 v;
      v.x = src[i]; v.y = src[i + 1];
      *(FDB_GLOBAL u64x2*)(dst + start + i) = v;
    } else {
      if (i >= 0 && i < count) dst[start + i] = src[i];
      if (i + 1 >= 0 && i + 1 < count) dst[start + i + 1] = src[i + 1];
    }
  }
}

__device__ __forceinline__ void unstage_u32(uint32_t* __restrict__ dst, const int64_t start, const int count, const uint32_t* src) {
  const int64_t g0 = start & ~(int64_t)3;
  const int chunks = (int)((start + count - g0 + 3) >> 2);
  for (int c = threadIdx.x; c < chunks; c += FDB_MERGE_BLOCK) {
    const int i = (int)(g0 + 4 * c - start);
    if (i >= 0 && i + 3 < count) {
      u32x4 v;
      v.x = src[i]; v.y = src[i + 1]; v.z = src[i + 2]; v.w = src[i + 3];
      *(FDB_GLOBAL u32x4*)(dst + start + i) = v;
    } else {
      for (int k = 0; k < 4; k++)
        if (i + k >= 0 && i + k < count) dst[start + i + k] = src[i + k];
    }
  }
}

template <int W>
__global__ __launch_bounds__(FDB_MERGE_BLOCK) void merge_tile_kernel(const FdbMergeArgs a) {
  constexpr int ITEMS = W <= 2 ? 8 : 4, T = FDB_MERGE_BLOCK * ITEMS;
  static_assert(W >= 1 && W <= FDB_MERGE_LDS_WORDS, "the LDS image is sized for keys of 1 … FDB_MERGE_LDS_WORDS words");
  __shared__ __attribute__((aligned(16))) u64 lk[W * T];
  __shared__ __attribute__((aligned(16))) uint32_t lp[T];
  const Tile t = tile_of(a, blockIdx.x, T);  // (workgroup-uniform)
  if (!t.ok) {
    if (threadIdx.x == 0) atomicOr(a.error, 1u);
    return;
  }
  const int n = t.ta + t.tb;
#pragma unroll
  for (int w = 0; w < W; w++) {
    stage_u64(lk + w * T, a.src_keys + (int64_t)w * a.stride, t.a0, t.ta);
    stage_u64(lk + w * T + t.ta, a.src_keys + (int64_t)w * a.stride, t.b0, t.tb);
  }
  stage_u32(lp, a.src_pay, t.a0, t.ta);
  stage_u32(lp + t.ta, a.src_pay, t.b0, t.tb);
  __syncthreads();
  const int d = (int)threadIdx.x * ITEMS < n ? (int)threadIdx.x * ITEMS : n;
  const uint64_t* ka = (const uint64_t*)lk;
  const uint64_t* kb = (const uint64_t*)lk + t.ta;
  const int ai = (int)fdb_mp_diagonal(ka, T, t.ta, kb, T, t.tb, d, W);
  uint32_t src[ITEMS];
  // (always ITEMS steps, so that src[] is indexed statically; a step past the tile's end compares nothing and is dropped below)
  const int ta = t.ta;
  fdb_mp_serial(ka, T, t.ta, kb, T, t.tb, ai, d - ai, ITEMS, W, [&](int k, bool from_b, int64_t idx) { src[k] = (uint32_t)(from_b ? ta + idx : idx); });
  u64 ok[ITEMS][W];
  uint32_t op[ITEMS];
#pragma unroll
  for (int k = 0; k < ITEMS; k++) {
    const bool live = d + k < n;
    const uint32_t s = live ? src[k] : 0u;
#pragma unroll
    for (int w = 0; w < W; w++) ok[k][w] = lk[w * T + s];
    op[k] = lp[s];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < ITEMS; k++) {
    if (d + k < n) {
#pragma unroll
      for (int w = 0; w < W; w++) lk[w * T + d + k] = ok[k][w];
      lp[d + k] = op[k];
    }
  }
  __syncthreads();
#pragma unroll
  for (int w = 0; w < W; w++) unstage_u64(a.dst_keys + (int64_t)w * a.stride, t.out0, n, lk + w * T);
  unstage_u32(a.dst_pay, t.out0, n, lp);
}

// W at run time, no LDS: a lane finds its diagonal among the tile's ranges in global memory and writes its outputs where they go.
__global__ __launch_bounds__(FDB_MERGE_BLOCK) void merge_tile_kernel_any(const FdbMergeArgs a) {
  const int W = a.words, ITEMS = fdb_merge_items(W), T = FDB_MERGE_BLOCK * ITEMS;
  const Tile t = tile_of(a, blockIdx.x, T);
  if (!t.ok) {
    if (threadIdx.x == 0) atomicOr(a.error, 1u);
    return;
  }
  const int n = t.ta + t.tb;
  const int d = (int)threadIdx.x * ITEMS;
  if (d >= n) return;
  const int count = n - d < ITEMS ? n - d : ITEMS;
  const uint64_t* ka = (const uint64_t*)a.src_keys + t.a0;
  const uint64_t* kb = (const uint64_t*)a.src_keys + t.b0;
  const int64_t stride = a.stride;
  const int ai = (int)fdb_mp_diagonal(ka, stride, t.ta, kb, stride, t.tb, d, W);
  u64* __restrict__ out_keys = a.dst_keys + t.out0 + d;
  uint32_t* __restrict__ out_pay = a.dst_pay + t.out0 + d;
  const uint32_t* pa = a.src_pay + t.a0;
  const uint32_t* pb = a.src_pay + t.b0;
  fdb_mp_serial(ka, stride, t.ta, kb, stride, t.tb, ai, d - ai, count, W, [&](int k, bool from_b, int64_t idx) {
    const uint64_t* from = from_b ? kb : ka;
    for (int w = 0; w < W; w++) out_keys[(int64_t)w * stride + k] = from[(int64_t)w * stride + idx];
    out_pay[k] = (from_b ? pb : pa)[idx];
  });
}

// ---- gather --------------------------------------------------------------------------------------------------------------------------------
// Row i of the result = the row at position rows[i] of the concatenated inputs: blockIdx.y = column, the lane's input is the last one
// that starts at or before its position. Modelled on take_kernel (fdb_take.hip): validity leaves as one ballot per wave, NULLs are
// counted per column. A NULL row's dictionary index is never translated: it leaves as 0. A row of an input that lacks the column
// (FdbMergeSrc::values == nullptr) is NULL with value 0; the marker is tested before any load from that source — and only in the columns
// that some input lacks (FdbMergeCol::lacking, block-uniform): every other column runs the code it ran before the marker existed.
template <bool LACKING>
__device__ __forceinline__ bool merge_gather_row(const FdbMergeCol& c, const FdbMergeSrc& s, const bool inside, const uint64_t j, const int64_t i) {
  const bool have = LACKING ? inside && s.values != nullptr : inside;  // (values == nullptr: the input lacks the column — NULL, value 0, no load)
  const bool ok = have && (s.validity == nullptr || ((s.validity[j >> 3] >> (j & 7)) & 1) != 0);
  if (c.width == 4) {
    uint32_t v = 0u;
    if (ok) {
      v = ((const uint32_t*)s.values)[j];
      if (s.table != nullptr) v = v < s.table_len ? s.table[v] : 0u;
    }
    ((uint32_t*)c.dst)[i] = v;
  } else {
    ((unsigned long long*)c.dst)[i] = have ? ((const unsigned long long*)s.values)[j] : 0ull;
  }
  return ok;
}

__global__ __launch_bounds__(FDB_MERGE_BLOCK) void merge_gather_kernel(const FdbMergeCol* __restrict__ cols, const FdbMergeSrc* __restrict__ srcs,
                                                                       const FdbMergeInput* __restrict__ inputs, const int n_inputs, const uint32_t* __restrict__ rows,
                                                                       const int64_t n, unsigned long long* __restrict__ nulls) {
  __shared__ uint32_t wave_nulls[FDB_MERGE_BLOCK / 64];
  const FdbMergeCol c = cols[blockIdx.y];  // (block-uniform)
  const int64_t i = (int64_t)blockIdx.x * FDB_MERGE_BLOCK + threadIdx.x;
  const bool live = i < n;
  bool ok = false;
  if (live) {
    const uint32_t g = rows[i];
    int lo = 0, hi = n_inputs - 1;
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (inputs[mid].start <= g) lo = mid;
      else hi = mid - 1;
    }
    const FdbMergeInput in = inputs[lo];
    const uint64_t j = (uint64_t)g - in.start;
    const bool inside = g >= in.start && j < in.rows;
    const FdbMergeSrc s = srcs[(size_t)blockIdx.y * (size_t)n_inputs + (size_t)lo];
    ok = c.lacking != 0 ? merge_gather_row<true>(c, s, inside, j, i) : merge_gather_row<false>(c, s, inside, j, i);  // (block-uniform choice)
  }
  if (c.dst_valid == nullptr) return;  // (block-uniform: no input has a NULL in this column)
  const unsigned long long valid = __ballot(ok), present = __ballot(live);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
    if (present != 0ull) ((unsigned long long*)c.dst_valid)[i >> 6] = valid;
    wave_nulls[wave] = (uint32_t)__popcll(present & ~valid);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t t = 0;
    for (int w = 0; w < FDB_MERGE_BLOCK / 64; w++) t += wave_nulls[w];
    if (t != 0) atomicAdd(&nulls[blockIdx.y], (unsigned long long)t);
  }
}

}  // namespace

hipError_t fdb_launch_merge_order(const unsigned long long* keys, int64_t stride, int words, int64_t off, int64_t len, uint32_t* first_bad, hipStream_t stream) {
  if (len <= 1 || words <= 0) return hipSuccess;
  const int64_t blocks = (len - 1 + FDB_MERGE_BLOCK - 1) / FDB_MERGE_BLOCK;
  if (keys == nullptr || first_bad == nullptr || off < 0 || off + len > stride || blocks > 0x7FFFFFFFll) return hipErrorInvalidValue;
  merge_order_kernel<<<dim3((unsigned)blocks), FDB_MERGE_BLOCK, 0, stream>>>(keys, stride, words, off, len, first_bad);
  return hipGetLastError();
}

hipError_t fdb_launch_merge_round(const FdbMergeArgs* args, hipStream_t stream) {
  const FdbMergeArgs& a = *args;
  if (a.n_pairs <= 0 || a.n_tiles <= 0) return hipSuccess;
  const int64_t bounds = a.n_tiles + a.n_pairs, pblocks = (bounds + FDB_MERGE_BLOCK - 1) / FDB_MERGE_BLOCK;
  if (a.words < 0 || a.src_pay == nullptr || a.dst_pay == nullptr || a.pairs == nullptr || a.splits == nullptr || a.error == nullptr || (a.words > 0 && (a.src_keys == nullptr || a.dst_keys == nullptr)) ||
      (a.stride & 3) != 0 || a.n_tiles > 0x7FFFFFFFll || pblocks > 0x7FFFFFFFll)
    return hipErrorInvalidValue;
  merge_partition_kernel<<<dim3((unsigned)pblocks), FDB_MERGE_BLOCK, 0, stream>>>(a);
  const dim3 grid((unsigned)a.n_tiles);
  switch (a.words) {
    case 1: merge_tile_kernel<1><<<grid, FDB_MERGE_BLOCK, 0, stream>>>(a); break;
    case 2: merge_tile_kernel<2><<<grid, FDB_MERGE_BLOCK, 0, stream>>>(a); break;
    case 3: merge_tile_kernel<3><<<grid, FDB_MERGE_BLOCK, 0, stream>>>(a); break;
    case 4: merge_tile_kernel<4><<<grid, FDB_MERGE_BLOCK, 0, stream>>>(a); break;
    default: merge_tile_kernel_any<<<grid, FDB_MERGE_BLOCK, 0, stream>>>(a); break;
  }
  return hipGetLastError();
}

hipError_t fdb_launch_merge_gather(const FdbMergeCol* d_cols, int n_cols, const FdbMergeSrc* d_srcs, const FdbMergeInput* d_inputs, int n_inputs, const uint32_t* d_rows,
                                   int64_t n, unsigned long long* d_nulls, hipStream_t stream) {
  if (n_cols <= 0 || n <= 0) return hipSuccess;
  const int64_t blocks = (n + FDB_MERGE_BLOCK - 1) / FDB_MERGE_BLOCK;
  if (n_cols > 65535 || n_inputs <= 0 || d_cols == nullptr || d_srcs == nullptr || d_inputs == nullptr || d_rows == nullptr || d_nulls == nullptr || blocks > 0x7FFFFFFFll)
    return hipErrorInvalidValue;
  merge_gather_kernel<<<dim3((unsigned)blocks, (unsigned)n_cols), FDB_MERGE_BLOCK, 0, stream>>>(d_cols, d_srcs, d_inputs, n_inputs, d_rows, n, d_nulls);
  return hipGetLastError();
}
