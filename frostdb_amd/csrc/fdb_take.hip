// frostdb_amd — row gather and row scatter over the columns of a resident record (see fdb_kernels.h, "row gather / scatter"):
// take_kernel places row rows[i] of a record at row i of another (Take, Limit's prefix, the Sampler's Finish), scatter_kernel places row
// r of a record at slot s of the Sampler's reservoir. Both copy every column in one launch (blockIdx.y = column) and re-key dictionary
// indices through an optional translation table while they copy. Random reads by nature: the writes are coalesced (gather) or as sparse
// as the replacements are (scatter); a row costs 4 or 8 bytes in and out per column, plus its validity.
#include <hip/hip_runtime.h>

#include "fdb_kernels.h"

namespace {

__device__ __forceinline__ bool row_valid(const FdbTakeCol& c, const uint64_t j) {
  if (c.absent) return false;
  if (c.src_valid == nullptr) return true;
  return c.valid_bytes ? c.src_valid[j] != 0 : ((c.src_valid[j >> 3] >> (j & 7)) & 1) != 0;
}

// row j of the source to row k of the destination (the column is not `absent`)
__device__ __forceinline__ void copy_value(const FdbTakeCol& c, const uint64_t j, const uint64_t k) {
  if (c.width == 4) {
    uint32_t v = ((const uint32_t*)c.src)[j];
    if (c.table != nullptr) v = v < c.table_len ? c.table[v] : 0u;
    ((uint32_t*)c.dst)[k] = v;
  } else {
    ((unsigned long long*)c.dst)[k] = ((const unsigned long long*)c.src)[j];
  }
}

__global__ __launch_bounds__(FDB_TAKE_BLOCK) void take_kernel(const FdbTakeCol* __restrict__ cols, const uint32_t* __restrict__ rows, const int64_t n,
                                                              unsigned long long* __restrict__ nulls) {
  __shared__ uint32_t wave_nulls[FDB_TAKE_BLOCK / 64];
  const FdbTakeCol c = cols[blockIdx.y];  // (block-uniform)
  const int64_t i = (int64_t)blockIdx.x * FDB_TAKE_BLOCK + threadIdx.x;
  const bool live = i < n;
  bool ok = false;
  if (live) {
    const uint64_t j = rows != nullptr ? (uint64_t)rows[i] : (uint64_t)i;
    ok = row_valid(c, j);
    copy_value(c, j, (uint64_t)i);
  }
  if (c.dst_valid == nullptr) return;  // (block-uniform: a source without NULLs has none to count either)
  const unsigned long long valid = __ballot(ok), present = __ballot(live);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
    if (present != 0ull) ((unsigned long long*)c.dst_valid)[i >> 6] = valid;
    wave_nulls[wave] = (uint32_t)__popcll(present & ~valid);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t t = 0;
    for (int w = 0; w < FDB_TAKE_BLOCK / 64; w++) t += wave_nulls[w];
    if (t != 0) atomicAdd(&nulls[blockIdx.y], (unsigned long long)t);
  }
}

__global__ __launch_bounds__(FDB_TAKE_BLOCK) void scatter_kernel(const FdbTakeCol* __restrict__ cols, const uint32_t* __restrict__ pairs, const int64_t m) {
  const FdbTakeCol c = cols[blockIdx.y];
  const int64_t i = (int64_t)blockIdx.x * FDB_TAKE_BLOCK + threadIdx.x;
  if (i >= m) return;
  const uint64_t j = pairs[2 * i], k = pairs[2 * i + 1];
  const bool ok = row_valid(c, j);
  if (!c.absent) copy_value(c, j, k);
  else if (c.width == 4) ((uint32_t*)c.dst)[k] = 0u;
  else ((unsigned long long*)c.dst)[k] = 0ull;
  ((uint8_t*)c.dst_valid)[k] = ok ? 1 : 0;
}

}  // namespace

hipError_t fdb_launch_take(const FdbTakeCol* d_cols, int n_cols, const uint32_t* d_rows, int64_t n, unsigned long long* d_nulls, hipStream_t stream) {
  if (n_cols <= 0 || n <= 0) return hipSuccess;
  const int64_t blocks = (n + FDB_TAKE_BLOCK - 1) / FDB_TAKE_BLOCK;
  if (n_cols > FDB_TAKE_MAX_COLS || blocks > 0x7FFFFFFFll) return hipErrorInvalidValue;
  take_kernel<<<dim3((unsigned)blocks, (unsigned)n_cols), FDB_TAKE_BLOCK, 0, stream>>>(d_cols, d_rows, n, d_nulls);
  return hipGetLastError();
}

hipError_t fdb_launch_scatter(const FdbTakeCol* d_cols, int n_cols, const uint32_t* d_pairs, int64_t m, hipStream_t stream) {
  if (n_cols <= 0 || m <= 0) return hipSuccess;
  const int64_t blocks = (m + FDB_TAKE_BLOCK - 1) / FDB_TAKE_BLOCK;
  if (n_cols > FDB_TAKE_MAX_COLS || blocks > 0x7FFFFFFFll) return hipErrorInvalidValue;
  scatter_kernel<<<dim3((unsigned)blocks, (unsigned)n_cols), FDB_TAKE_BLOCK, 0, stream>>>(d_cols, d_pairs, m);
  return hipGetLastError();
}
