// fdb_sortkey.h — the radix-key encoding of the device Sort (fdb_sort.cpp; kernel in fdb_sortkeys.hip): ONE definition for the kernel and
// for the host self-check (fdb_selftest_sort_key). ≙ multiColSorter.compare / Less (pqarrow/arrowutils/sort.go:517-564).
//
// Every sorting column becomes one or two unsigned FIELDS whose ascending unsigned order is the wanted order:
//   value field   int64: v ^ 1<<63 · uint64: v · float64: Go's cmp.Compare — 0 for every NaN (all NaNs are equal and sort below -Inf), else
//                 the usual order-preserving flip of the value with -0.0 first turned into +0.0 (-Inf still lands above 0) · dictionary /
//                 string: the dense byte-order rank of the entry, in ceil(log2(distinct)) bits. Descending complements the field within
//                 its width. A NULL row's value field is 0 (the raw slot under a NULL is never used).
//   NULL field    1 bit immediately above the value field, only when the column has NULLs: nulls_first ? (NULL = 0, valid = 1) : (NULL = 1,
//                 valid = 0) — whatever the direction; never complemented.
// Fields are packed greedily into 64-bit key words from the most significant column down; a field never straddles two words (a nullable
// int64 has its NULL bit in one word and its 64 value bits in the next). The sort is a stable LSD radix sort over the words, last word
// first. STABLE: rows equal on every sorting column keep their input order — the reference's sort.Sort is not stable, so any order of
// ties is legal there; stability makes ours deterministic.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) || defined(__HIP__)
#include <hip/hip_runtime.h>
#define FDB_SORTKEY_HD __host__ __device__ __forceinline__
#else
#define FDB_SORTKEY_HD inline
#endif

// column kinds of a field (the values of fdb::ColKind for the kinds that sort)
#define FDB_SORT_I64 1
#define FDB_SORT_U64 2
#define FDB_SORT_F64 3
#define FDB_SORT_DICT 6

#define FDB_SORT_DESC 1u         // FdbSortField::flags
#define FDB_SORT_NULLS_FIRST 2u
#define FDB_SORT_ABSENT 4u       // the record has no such column (a merge of records with differing field lists): every row is NULL and
                                 // neither values, validity nor ranks are read — they may be nullptr

FDB_SORTKEY_HD uint64_t fdb_sortkey_i64(uint64_t raw) { return raw ^ (1ull << 63); }

FDB_SORTKEY_HD uint64_t fdb_sortkey_f64(uint64_t raw) {
  const uint64_t mag = raw & ~(1ull << 63);
  if (mag > 0x7FF0000000000000ull) return 0ull;  // NaN, any sign or payload
  if (mag == 0ull) raw = 0ull;                   // -0.0 == +0.0
  return (raw >> 63) != 0ull ? ~raw : raw | (1ull << 63);
}

// The 64-bit ascending value field of one non-NULL value of an int64 / uint64 / float64 column (`raw` = its bits).
FDB_SORTKEY_HD uint64_t fdb_sortkey_value(int32_t kind, uint64_t raw) {
  return kind == FDB_SORT_I64 ? fdb_sortkey_i64(raw) : kind == FDB_SORT_F64 ? fdb_sortkey_f64(raw) : raw;
}

FDB_SORTKEY_HD uint64_t fdb_sortkey_mask(int32_t width) { return width >= 64 ? ~0ull : (1ull << width) - 1ull; }

// … in the column's direction, cut to the field's width.
FDB_SORTKEY_HD uint64_t fdb_sortkey_directed(uint64_t value, uint32_t flags, int32_t width) {
  return ((flags & FDB_SORT_DESC) != 0u ? ~value : value) & fdb_sortkey_mask(width);
}

FDB_SORTKEY_HD uint64_t fdb_sortkey_null_bit(bool valid, uint32_t flags) { return valid == ((flags & FDB_SORT_NULLS_FIRST) != 0u) ? 1ull : 0ull; }

// What one sorting column contributes to ONE key word: its value field, its NULL bit, or both.
struct FdbSortField {
  const void* values;       // 8-byte values, or 4-byte dictionary indices (kind FDB_SORT_DICT)
  const uint8_t* validity;  // bitmap at bit offset 0; nullptr: the column has no NULLs
  const uint32_t* ranks;    // FDB_SORT_DICT: entry → dense byte-order rank; read only for valid rows, an index ≥ rank_len reads nothing
  uint32_t rank_len;
  int32_t kind;
  int32_t width;            // bits of the value field in this word; 0: it is in another word (or the column has a single distinct value)
  int32_t shift;            // its lowest bit
  int32_t null_shift;       // the NULL bit's place in this word; -1: none here
  uint32_t flags;
};

#define FDB_SORT_BLOCK 256
#define FDB_SORT_ROWS 4  // consecutive rows per lane

#if !defined(FDB_SORTKEY_NO_LAUNCHERS) && (defined(__HIPCC__) || defined(__HIP__))
// keys[i] = the key word made of `d_fields` (device memory) for row perm[i] (perm == nullptr: row i), i < n. `iota` (may be nullptr, only
// with perm == nullptr): iota[i] = i on the way. Lanes past n store nothing.
hipError_t fdb_launch_sort_keys(const FdbSortField* d_fields, int n_fields, const uint32_t* perm, int64_t n, unsigned long long* keys, uint32_t* iota, hipStream_t stream);
hipError_t fdb_launch_sort_iota(uint32_t* p, int64_t n, hipStream_t stream);  // p[i] = i
// fdb_sort_pairs_u64 (fdb_kernels.h) with 32-bit values: row numbers, half the payload traffic. Stable, by the low `bits` bits of the key.
hipError_t fdb_sort_pairs_u64_u32(void* temp, size_t* temp_bytes, const unsigned long long* keys_in, unsigned long long* keys_out, const uint32_t* vals_in,
                                  uint32_t* vals_out, int64_t n, int bits, hipStream_t stream);
#endif
