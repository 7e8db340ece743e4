// fdb_mergepath.h — the merge-path arithmetic of the device MergeRecords (fdb_mergerec.cpp; kernels in fdb_mergepath.hip): ONE definition
// for the kernels and for the host self-check (fdb_selftest_merge_path), as fdb_sortkey.h is for the key encoding.
//
// A key is W unsigned 64-bit words, word 0 the most significant, compared lexicographically (the words are the Sort's radix keys: their
// unsigned order IS the reference's comparison). Keys are held as a structure of arrays: word w of element i is at k[w * stride + i].
// Two sorted runs A and B merge STABLY with ties going to A: the first d outputs hold i elements of A and d - i of B, where i is the one
// split with A[i - 1] <= B[d - i] and B[d - i - 1] < A[i] (fdb_mp_diagonal). The output is cut into tiles of fdb_merge_tile(W) rows; a
// partition step finds the split of every tile boundary over the whole runs, a merge step gives each of the FDB_MERGE_BLOCK lanes of a
// tile its own diagonal inside the tile and lets it merge fdb_merge_items(W) consecutive outputs serially (fdb_mp_serial).
//
// Partition bugs are tie-handling bugs: fdb_merge_path_host runs the same three functions over host arrays, tile by tile and lane by
// lane, with these constants, so that a CPU test reaches them.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) || defined(__HIP__)
#include <hip/hip_runtime.h>
#define FDB_MP_HD __host__ __device__ __forceinline__
#else
#define FDB_MP_HD inline
#endif

#define FDB_MERGE_BLOCK 256
// W <= FDB_MERGE_LDS_WORDS: the tile is staged in LDS (tile × (8 W + 4) bytes: 24 KiB at W = 1, at most 40 KiB); more words: the
// run-time-W kernel, which merges straight out of global memory.
#define FDB_MERGE_LDS_WORDS 4

FDB_MP_HD int fdb_merge_items(int words) { return words <= 2 ? 8 : words <= FDB_MERGE_LDS_WORDS ? 4 : 2; }
FDB_MP_HD int fdb_merge_tile(int words) { return FDB_MERGE_BLOCK * fdb_merge_items(words); }

// A[i] <= B[j], lexicographically over the W words.
FDB_MP_HD bool fdb_mp_le(const uint64_t* a, int64_t sa, int64_t i, const uint64_t* b, int64_t sb, int64_t j, int W) {
  for (int w = 0; w < W; w++) {
    const uint64_t x = a[(int64_t)w * sa + i], y = b[(int64_t)w * sb + j];
    if (x != y) return x < y;
  }
  return true;
}

// How many of the first d outputs (0 <= d <= na + nb) of the stable merge come from A. Ties go to A. Always within
// [max(0, d - nb), min(d, na)], whatever the keys hold.
FDB_MP_HD int64_t fdb_mp_diagonal(const uint64_t* a, int64_t sa, int64_t na, const uint64_t* b, int64_t sb, int64_t nb, int64_t d, int W) {
  int64_t lo = d > nb ? d - nb : 0, hi = d < na ? d : na;
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (fdb_mp_le(a, sa, mid, b, sb, d - 1 - mid, W)) lo = mid + 1;  // A[mid] is out before B[d - 1 - mid]: at least mid + 1 of A
    else hi = mid;
  }
  return lo;
}

// The serial merge of one lane: from (ai, bi) on, `count` outputs; emit(k, from_b, index) names output k's source element. An
// exhausted run loses, a tie goes to A.
template <class Emit>
FDB_MP_HD void fdb_mp_serial(const uint64_t* a, int64_t sa, int64_t na, const uint64_t* b, int64_t sb, int64_t nb, int64_t ai, int64_t bi, int count, int W,
                             Emit&& emit) {
  for (int k = 0; k < count; k++) {
    const bool from_a = bi >= nb || (ai < na && fdb_mp_le(a, sa, ai, b, sb, bi, W));
    if (from_a) { emit(k, false, ai); ai++; }
    else { emit(k, true, bi); bi++; }
  }
}

// One pair of a round: runs A = [a_off, a_off + na) and B = [b_off, b_off + nb) of the source buffers merge into [out_off, out_off + n_out)
// of the destination buffers, n_out <= na + nb (a limit cuts it). tile_first = the tiles of the pairs before this one; pair p's tile
// boundaries (one more than its tiles) start at splits[tile_first + p].
struct FdbMergePair { int64_t a_off, na, b_off, nb, out_off, n_out, tile_first; };
struct FdbMergeArgs {
  const unsigned long long* src_keys;  // word w of position g at [w * stride + g]; both buffers 16-byte aligned, stride a multiple of 4
  unsigned long long* dst_keys;
  const uint32_t* src_pay;
  uint32_t* dst_pay;
  int64_t stride;
  const FdbMergePair* pairs;
  uint32_t* splits;                    // n_tiles + n_pairs entries: how many of a boundary's outputs come from A
  uint32_t* error;                     // set when a tile's splits are unusable (nothing is merged there)
  int64_t n_tiles;
  int32_t n_pairs;
  int32_t words;
};
// The gather: one FdbMergeCol per output column, one FdbMergeSrc per (column, input) at [column * n_inputs + input], one FdbMergeInput
// per input in position order (start ascending).
struct FdbMergeCol { void* dst; void* dst_valid; int32_t width; int32_t lacking; };  // lacking != 0: some input lacks the column (then dst_valid is set)
// FdbMergeSrc::values == nullptr is the ABSENT marker (≙ FDB_SORT_ABSENT of the key kernel): the input lacks the column — its rows leave
// as NULL with value 0 and nothing of the source is read. The kernel looks at the marker only in columns whose FdbMergeCol::lacking says
// that some input lacks them, so a column that every input has is gathered by the code that ran before the marker existed.
struct FdbMergeSrc { const void* values; const uint8_t* validity; const uint32_t* table; uint32_t table_len; uint32_t _pad; };
struct FdbMergeInput { uint32_t start, rows; };

#if !defined(FDB_MERGEPATH_NO_LAUNCHERS) && (defined(__HIPCC__) || defined(__HIP__))
// *first_bad = min(*first_bad, i) for every i in [1, len) whose key sorts before its predecessor's (positions off … off + len of `keys`)
hipError_t fdb_launch_merge_order(const unsigned long long* keys, int64_t stride, int words, int64_t off, int64_t len, uint32_t* first_bad, hipStream_t stream);
// partition + merge of every pair of one round (the tile is fdb_merge_tile(args->words))
hipError_t fdb_launch_merge_round(const FdbMergeArgs* args, hipStream_t stream);
hipError_t fdb_launch_merge_gather(const FdbMergeCol* d_cols, int n_cols, const FdbMergeSrc* d_srcs, const FdbMergeInput* d_inputs, int n_inputs, const uint32_t* d_rows,
                                   int64_t n, unsigned long long* d_nulls, hipStream_t stream);
#endif

#ifdef __cplusplus
#include <vector>
// The host walk (fdb_selftest_merge_path). a / b: na / nb keys of W words each, ROW-major (word w of key i at a[i * W + w]), each run
// sorted. src_out[o] (na + nb entries) = the source of output o: i for A[i], na + j for B[j]. Returns 0, or 1 + the first tile whose
// splits cross or leave the runs (cannot happen with sorted runs).
inline int64_t fdb_merge_path_host(const uint64_t* a, int64_t na, const uint64_t* b, int64_t nb, int W, uint32_t* src_out) {
  const int64_t T = fdb_merge_tile(W), n = na + nb, tiles = (n + T - 1) / T;
  const int items = fdb_merge_items(W);
  std::vector<uint64_t> ka((size_t)(na * W) + 1), kb((size_t)(nb * W) + 1);  // the runs as the device holds them: word-major
  for (int64_t i = 0; i < na; i++) for (int w = 0; w < W; w++) ka[(size_t)(w * na + i)] = a[i * W + w];
  for (int64_t j = 0; j < nb; j++) for (int w = 0; w < W; w++) kb[(size_t)(w * nb + j)] = b[j * W + w];
  std::vector<int64_t> split((size_t)tiles + 1);
  for (int64_t t = 0; t <= tiles; t++) split[(size_t)t] = fdb_mp_diagonal(ka.data(), na, na, kb.data(), nb, nb, t * T < n ? t * T : n, W);  // the partition kernel
  std::vector<uint64_t> image((size_t)(T * W));  // the tile as the merge kernel stages it: A's range, then B's, stride T
  for (int64_t t = 0; t < tiles; t++) {
    const int64_t d0 = t * T, d1 = (t + 1) * T < n ? (t + 1) * T : n;
    const int64_t a0 = split[(size_t)t], a1 = split[(size_t)t + 1], b0 = d0 - a0, b1 = d1 - a1;
    const int64_t ta = a1 - a0, tb = b1 - b0;
    if (ta < 0 || tb < 0 || a1 > na || b1 > nb || ta + tb != d1 - d0) return 1 + t;
    for (int w = 0; w < W; w++) {
      for (int64_t i = 0; i < ta; i++) image[(size_t)(w * T + i)] = ka[(size_t)(w * na + a0 + i)];
      for (int64_t j = 0; j < tb; j++) image[(size_t)(w * T + ta + j)] = kb[(size_t)(w * nb + b0 + j)];
    }
    const uint64_t* ia = image.data();
    const uint64_t* ib = image.data() + ta;
    for (int lane = 0; lane < FDB_MERGE_BLOCK; lane++) {
      const int64_t d = (int64_t)lane * items < ta + tb ? (int64_t)lane * items : ta + tb;
      const int64_t left = ta + tb - d, count = left < items ? left : items;
      const int64_t ai = fdb_mp_diagonal(ia, T, ta, ib, T, tb, d, W);
      fdb_mp_serial(ia, T, ta, ib, T, tb, ai, d - ai, (int)count, W,
                    [&](int k, bool from_b, int64_t idx) { src_out[d0 + d + k] = (uint32_t)(from_b ? na + b0 + idx : a0 + idx); });
    }
  }
  return 0;
}
#endif
