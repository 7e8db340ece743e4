// fdb_sortplan.h — the host half of the radix-key plan that the device Sort (fdb_sort.cpp) and the device MergeRecords (fdb_mergerec.cpp)
// share: the dense byte-order ranks of a dictionary and the packing of the key fields into 64-bit words (the encoding itself is
// fdb_sortkey.h). No device, no HIP: tools/asan_merge.sh runs exactly this code under AddressSanitizer.
#pragma once

#include <algorithm>
#include <cstdint>
#include <vector>

#include "fdb_arrow.h"

namespace fdb {

// Dense ranks of a dictionary's entries by their bytes (equal bytes — a dictionary with unique == false — share a rank), and the number of
// distinct entries.
inline std::vector<uint32_t> dense_ranks(const HostDict& d, uint32_t* distinct) {
  const size_t n = d.values.size();
  if (d.unique) {  // positions among the sorted entries are dense already, and computed once per interned dictionary
    *distinct = (uint32_t)n;
    return d.sorted_ranks();
  }
  std::vector<uint32_t> order(n), rank(n);
  for (size_t i = 0; i < n; i++) order[i] = (uint32_t)i;
  std::sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return d.values[x] < d.values[y]; });  // (std::string: bytewise, as bytes.Compare)
  uint32_t r = 0;
  for (size_t k = 0; k < n; k++) {
    if (k > 0 && d.values[order[k]] != d.values[order[k - 1]]) r++;
    rank[order[k]] = r;
  }
  *distinct = n == 0 ? 0u : r + 1u;
  return rank;
}

// A hash of every entry's bytes, entry by entry — the table the Parquet writer's bloom filter pass gathers an index column's hashes
// from (`hash`: fdb_pqb_hash of fdb_pqbloom.h; equal entries get equal hashes, an empty entry the hash of no bytes).
template <class Hash>
inline std::vector<uint64_t> entry_hashes(const HostDict& d, Hash hash) {
  std::vector<uint64_t> h(d.values.size());
  for (size_t i = 0; i < h.size(); i++) h[i] = hash((const unsigned char*)d.values[i].data(), d.values[i].size());
  return h;
}

// The packing of the key fields into words: one SortPart per (word, column) — the column's value field, its NULL bit, or both; bits_out[w]
// = the bits word w uses. Word 0 is the most significant.
struct SortPart { int word; int col; int width; int shift; int null_shift; };
struct SortColBits { int value_bits; bool has_null_bit; };

inline std::vector<SortPart> pack_sort_fields(const std::vector<SortColBits>& cols, std::vector<int>* bits_out) {
  // greedy, most significant column first; `top` = bits of the current word already given away, counted from its top
  struct Piece { int word, col, width, top; bool null_bit; };
  std::vector<Piece> pieces;
  std::vector<int> used;
  auto place = [&](int col, int width, bool null_bit) {
    if (used.empty() || used.back() + width > 64) used.push_back(0);
    pieces.push_back(Piece{(int)used.size() - 1, col, width, used.back(), null_bit});
    used.back() += width;
  };
  for (size_t c = 0; c < cols.size(); c++) {
    if (cols[c].has_null_bit) place((int)c, 1, true);
    if (cols[c].value_bits > 0) place((int)c, cols[c].value_bits, false);
  }
  // a word sorts on its low used[w] bits: the first piece of a word ends at bit used[w] - 1
  std::vector<SortPart> parts;
  for (const Piece& p : pieces) {
    const int low = used[(size_t)p.word] - p.top - p.width;
    if (!parts.empty() && parts.back().word == p.word && parts.back().col == p.col) {  // the value field right under its NULL bit
      parts.back().width = p.width; parts.back().shift = low;
      continue;
    }
    parts.push_back(p.null_bit ? SortPart{p.word, p.col, 0, 0, low} : SortPart{p.word, p.col, p.width, low, -1});
  }
  *bits_out = used;
  return parts;
}

inline int bits_for(uint64_t distinct) {  // ceil(log2(distinct))
  int b = 0;
  while (b < 64 && ((uint64_t)1 << b) < distinct) b++;
  return b;
}

}  // namespace fdb
