// frostdb_amd — radix keys of the device Sort (fdb_sort.cpp; the encoding is fdb_sortkey.h): sort_keys_kernel turns the sorting columns of a
// resident record into one 64-bit key word per row, in row order (the first pass of the LSD sort) or through the current permutation (every
// later pass). In a translation unit of its own: fdb_kernels.hip is not compiled for it.
//
// Geometry: the scans' — a lane owns FDB_SORT_ROWS = 4 consecutive rows, so in row order an 8-byte column is read with two 16-byte loads, a
// 4-byte index column with one, and the 4 validity bits of the lane sit in one byte (the row number is a multiple of 4); through a permutation
// the loads are gathers by nature and only the permutation itself (one 16-byte load) and the keys (two 16-byte stores) are contiguous. The
// field descriptors are wave-uniform and read through the constant address space (scalar loads); rank tables are read from global memory,
// where a dictionary's table stays hot in L2. A NULL row's raw slot is never used: not as a value, not as an index into a rank table. A field
// marked FDB_SORT_ABSENT (the merge of records with differing field lists) has no column behind it: its rows are NULL and nothing is loaded.
#include <hip/hip_runtime.h>

#include "fdb_sortkey.h"

namespace {

#define FDB_CONST __attribute__((address_space(4)))
#define FDB_GLOBAL __attribute__((address_space(1)))

typedef unsigned long long u64;
typedef u64 u64x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

template <bool PERM>
__global__ __launch_bounds__(FDB_SORT_BLOCK) void sort_keys_kernel(const FdbSortField* __restrict__ fields_in, const int n_fields, const uint32_t* __restrict__ perm,
                                                                   const int64_t n, u64* __restrict__ keys, uint32_t* __restrict__ iota) {
  const int64_t i0 = ((int64_t)blockIdx.x * FDB_SORT_BLOCK + threadIdx.x) * FDB_SORT_ROWS;
  if (i0 >= n) return;
  const bool full = i0 + FDB_SORT_ROWS <= n;  // (only the last live lane of a launch is not)
  bool live[FDB_SORT_ROWS];
  u64 row[FDB_SORT_ROWS];
#pragma unroll
  for (int k = 0; k < FDB_SORT_ROWS; k++) { live[k] = i0 + k < n; row[k] = (u64)(i0 + k); }
  if (PERM) {
    if (full) {
      const u32x4 p = *(const FDB_GLOBAL u32x4*)(perm + i0);
      row[0] = p.x; row[1] = p.y; row[2] = p.z; row[3] = p.w;
    } else {
#pragma unroll
      for (int k = 0; k < FDB_SORT_ROWS; k++) row[k] = live[k] ? (u64)perm[i0 + k] : 0ull;
    }
  }
  u64 key[FDB_SORT_ROWS] = {0ull, 0ull, 0ull, 0ull};
  const FDB_CONST FdbSortField* fields = (const FDB_CONST FdbSortField*)fields_in;
  for (int f = 0; f < n_fields; f++) {
    const FDB_GLOBAL unsigned char* values = (const FDB_GLOBAL unsigned char*)fields[f].values;
    const FDB_GLOBAL uint8_t* validity = (const FDB_GLOBAL uint8_t*)fields[f].validity;
    const FDB_GLOBAL uint32_t* ranks = (const FDB_GLOBAL uint32_t*)fields[f].ranks;
    const uint32_t rank_len = fields[f].rank_len, flags = fields[f].flags;
    const int32_t kind = fields[f].kind, width = fields[f].width, shift = fields[f].shift, null_shift = fields[f].null_shift;
    const bool absent = (flags & FDB_SORT_ABSENT) != 0u;  // (wave-uniform) every row NULL, nothing of the column is loaded
    bool valid[FDB_SORT_ROWS];
    if (absent) {
#pragma unroll
      for (int k = 0; k < FDB_SORT_ROWS; k++) valid[k] = false;
    } else if (validity == nullptr) {
#pragma unroll
      for (int k = 0; k < FDB_SORT_ROWS; k++) valid[k] = true;
    } else if (!PERM) {
      const uint32_t bits = (uint32_t)validity[i0 >> 3] >> (uint32_t)(i0 & 4);  // rows i0 … i0 + 3 of one byte (i0 < n: inside the bitmap)
#pragma unroll
      for (int k = 0; k < FDB_SORT_ROWS; k++) valid[k] = ((bits >> k) & 1u) != 0u;
    } else {
#pragma unroll
      for (int k = 0; k < FDB_SORT_ROWS; k++) valid[k] = live[k] && (((uint32_t)validity[row[k] >> 3] >> (uint32_t)(row[k] & 7)) & 1u) != 0u;
    }
    if (width > 0 && !absent) {  // (wave-uniform; an absent column's value field stays 0, as under every NULL)
      u64 v[FDB_SORT_ROWS];
      if (kind == FDB_SORT_DICT) {
        uint32_t idx[FDB_SORT_ROWS];
        if (!PERM && full) {
          const u32x4 q = *(const FDB_GLOBAL u32x4*)(values + i0 * 4);
          idx[0] = q.x; idx[1] = q.y; idx[2] = q.z; idx[3] = q.w;
        } else {
#pragma unroll
          for (int k = 0; k < FDB_SORT_ROWS; k++) idx[k] = live[k] ? ((const FDB_GLOBAL uint32_t*)values)[row[k]] : 0u;
        }
#pragma unroll
        for (int k = 0; k < FDB_SORT_ROWS; k++) v[k] = live[k] && valid[k] && idx[k] < rank_len ? (u64)ranks[idx[k]] : 0ull;
      } else {
        u64 raw[FDB_SORT_ROWS];
        if (!PERM && full) {
          const u64x2 a = *(const FDB_GLOBAL u64x2*)(values + i0 * 8), b = *(const FDB_GLOBAL u64x2*)(values + i0 * 8 + 16);
          raw[0] = a.x; raw[1] = a.y; raw[2] = b.x; raw[3] = b.y;
        } else {
#pragma unroll
          for (int k = 0; k < FDB_SORT_ROWS; k++) raw[k] = live[k] ? ((const FDB_GLOBAL u64*)values)[row[k]] : 0ull;
        }
#pragma unroll
        for (int k = 0; k < FDB_SORT_ROWS; k++) v[k] = fdb_sortkey_value(kind, raw[k]);
      }
#pragma unroll
      for (int k = 0; k < FDB_SORT_ROWS; k++) key[k] |= (valid[k] ? fdb_sortkey_directed(v[k], flags, width) : 0ull) << shift;
    }
    if (null_shift >= 0) {
#pragma unroll
      for (int k = 0; k < FDB_SORT_ROWS; k++) key[k] |= fdb_sortkey_null_bit(valid[k], flags) << null_shift;
    }
  }
  if (full) {
    u64x2 a, b;
    a.x = key[0]; a.y = key[1]; b.x = key[2]; b.y = key[3];
    *(FDB_GLOBAL u64x2*)(keys + i0) = a;
    *(FDB_GLOBAL u64x2*)(keys + i0 + 2) = b;
    if (!PERM && iota != nullptr) {
      u32x4 r;
      r.x = (uint32_t)i0; r.y = (uint32_t)i0 + 1u; r.z = (uint32_t)i0 + 2u; r.w = (uint32_t)i0 + 3u;
      *(FDB_GLOBAL u32x4*)(iota + i0) = r;
    }
  } else {
#pragma unroll
    for (int k = 0; k < FDB_SORT_ROWS; k++)
      if (live[k]) {
        keys[i0 + k] = key[k];
        if (!PERM && iota != nullptr) iota[i0 + k] = (uint32_t)(i0 + k);
      }
  }
}

__global__ __launch_bounds__(FDB_SORT_BLOCK) void sort_iota_kernel(uint32_t* __restrict__ p, const int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * FDB_SORT_BLOCK + threadIdx.x;
  if (i < n) p[i] = (uint32_t)i;
}

}  // namespace

hipError_t fdb_launch_sort_keys(const FdbSortField* d_fields, int n_fields, const uint32_t* perm, int64_t n, unsigned long long* keys, uint32_t* iota, hipStream_t stream) {
  if (n <= 0) return hipSuccess;
  const int64_t per_block = (int64_t)FDB_SORT_BLOCK * FDB_SORT_ROWS, blocks = (n + per_block - 1) / per_block;
  if (n_fields < 0 || d_fields == nullptr || keys == nullptr || blocks > 0x7FFFFFFFll || (perm != nullptr && iota != nullptr)) return hipErrorInvalidValue;
  if (perm != nullptr) sort_keys_kernel<true><<<dim3((unsigned)blocks), FDB_SORT_BLOCK, 0, stream>>>(d_fields, n_fields, perm, n, keys, nullptr);
  else sort_keys_kernel<false><<<dim3((unsigned)blocks), FDB_SORT_BLOCK, 0, stream>>>(d_fields, n_fields, nullptr, n, keys, iota);
  return hipGetLastError();
}

hipError_t fdb_launch_sort_iota(uint32_t* p, int64_t n, hipStream_t stream) {
  if (n <= 0) return hipSuccess;
  const int64_t blocks = (n + FDB_SORT_BLOCK - 1) / FDB_SORT_BLOCK;
  if (p == nullptr || blocks > 0x7FFFFFFFll) return hipErrorInvalidValue;
  sort_iota_kernel<<<dim3((unsigned)blocks), FDB_SORT_BLOCK, 0, stream>>>(p, n);
  return hipGetLastError();
}
