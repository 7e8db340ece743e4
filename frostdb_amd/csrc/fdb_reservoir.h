// fdb_reservoir.h — the host-only half of Take and the Sampler (fdb_take.cpp): which rows a reservoir keeps, the union of the dictionaries
// of the records that feed it, and the validation of row numbers. No device, no HIP: tools/asan_sampler.sh runs exactly this code under
// AddressSanitizer, and fdb_selftest_reservoir hands the selection to tests.
#pragma once

#include <cmath>
#include <cstdint>
#include <memory>
#include <string>
#include <unordered_map>
#include <vector>

#include "fdb_arrow.h"

namespace fdb {

// The Sampler's generator (documented in include/frostdb_amd.h so that a test can predict every draw): splitmix64 seeded with the
// caller's seed; a unit draw is ((x >> 11) + 0.5) · 2^-53 — never 0, so its logarithm is finite —, a slot draw (x · size) >> 64.
struct SplitMix64 {
  uint64_t x;
  uint64_t next() {
    x += 0x9E3779B97F4A7C15ull;
    uint64_t z = x;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
  }
  double unit() { return ((double)(next() >> 11) + 0.5) * 0x1p-53; }
  uint64_t below(uint64_t n) { return (uint64_t)(((unsigned __int128)next() * n) >> 64); }
};

// Which rows a reservoir of `size` slots keeps: Algorithm L as ReservoirSampler runs it (sampler.go:128-198) — fill() in order, then
// sample(): the `s.i == 0` sentinel that starts the skipping at row n - 1, the pending index carried into the next record (the
// `else if s.i < n` branch), one slot draw and one update of w per replacement. Where the reference indexes the UNSLICED record with a
// row number counted from the slice fill() cut off (its `ref` still points at the whole record), this indexes the slice, as the
// algorithm means.
class ReservoirSelect {
 public:
  ReservoirSelect(int64_t size, uint64_t seed) : size_(size), rng_{seed} {
    if (size_ > 0) w_ = std::exp(std::log(rng_.unit()) / (double)size_);
  }
  int64_t size() const { return size_; }
  int64_t kept() const { return kept_; }  // slots in use: min(size, rows seen)
  // The next record has `rows` rows: emit(row, slot) for every row that enters the reservoir, in the order the reference replaces
  // (a later pair for the same slot wins).
  template <typename F>
  void push(int64_t rows, F&& emit) {
    if (rows <= 0) return;  // (a zero-row record is no record: in the reference it would use up the sentinel and leave i = n - 1 pending)
    int64_t lo = 0;
    if (n_ < size_) {  // fill (sampler.go:129-156)
      const int64_t t = rows < size_ - n_ ? rows : size_ - n_;
      for (int64_t k = 0; k < t; k++) emit(k, n_ + k);
      n_ += t;
      kept_ = n_;
      lo = t;
      if (lo == rows) return;
    }
    if (size_ == 0) return;
    const int64_t nn = n_ + (rows - lo);  // (rows [lo, rows) are the slice sample() sees; its row r is our row lo + r)
    const double fn = (double)nn;
    if (i_ == 0) {
      i_ = (double)n_ - 1;
    } else if (i_ < fn) {
      emit(lo + ((int64_t)i_ - n_), (int64_t)rng_.below((uint64_t)size_));
      w_ *= std::exp(std::log(rng_.unit()) / (double)size_);
    }
    while (i_ < fn) {
      // (1 - w rounds to 0 when w is within 2^-54 of 1: log gives -inf, the quotient +0, the skip 1)
      i_ += std::floor(std::log(rng_.unit()) / std::log(1 - w_)) + 1;
      if (i_ < fn) {
        emit(lo + ((int64_t)i_ - n_), (int64_t)rng_.below((uint64_t)size_));
        w_ *= std::exp(std::log(rng_.unit()) / (double)size_);
      }
    }
    n_ = nn;
  }

 private:
  int64_t size_;
  SplitMix64 rng_;
  double w_ = 0, i_ = 0;
  int64_t n_ = 0, kept_ = 0;
};

// Keeps the LAST pair per slot (the reference replaces one after the other: the last one stays), in launch order otherwise.
// pairs = (row, slot) × m, in place; returns the number kept. `stamp` is scratch of ≥ `slots` entries the caller keeps zeroed between
// calls (it is zeroed again before this returns).
inline size_t keep_last_per_slot(std::vector<uint32_t>* pairs, std::vector<uint8_t>* stamp) {
  std::vector<uint32_t>& p = *pairs;
  const size_t m = p.size() / 2;
  size_t out = m;
  for (size_t k = m; k-- > 0;) {
    const uint32_t slot = p[2 * k + 1];
    if ((*stamp)[slot]) continue;
    (*stamp)[slot] = 1;
    out--;
    p[2 * out] = p[2 * k];
    p[2 * out + 1] = slot;
  }
  for (size_t k = out; k < m; k++) (*stamp)[p[2 * k + 1]] = 0;
  p.erase(p.begin(), p.begin() + (std::ptrdiff_t)(2 * out));
  return m - out;
}

// ≙ the bounds check of arrowutils.Take: every index in [0, rows), or FDB_ERR_INVALID naming the first offender — before any launch.
inline void check_take_indices(const int32_t* indices, int64_t n, int64_t rows) {
  if (n < 0 || (n > 0 && indices == nullptr)) throw Error(FDB_ERR_INVALID, "take: indices missing");
  for (int64_t i = 0; i < n; i++)
    if (indices[i] < 0 || (int64_t)indices[i] >= rows)
      throw Error(FDB_ERR_INVALID, "take: index " + std::to_string(indices[i]) + " at position " + std::to_string(i) + " is outside the record's " + std::to_string(rows) + " rows");
}

// The output dictionary of one Sampler field: the union of the contributing records' dictionaries in first-seen order, entries compared
// by their bytes (two entries with equal bytes are one). The union only grows, so an index written into the reservoir stays right and a
// translation table (source index → union index), once built for a dictionary, stays right too: one is kept per source dictionary —
// found by address, else by content (HostDict::same_content: hash, then the values) — so a table whose parts repeat their dictionaries
// pays two compares per record, not a rebuild.
class DictUnion {
 public:
  const std::vector<std::string>& values() const { return values_; }
  bool utf8() const { return utf8_; }
  bool plain() const { return plain_; }
  const std::string& value_format() const { return format_; }
  // Throws FDB_ERR_UNSUPPORTED when `d` is binary where the field was utf8 (or the reverse), or a plain column where it was a dictionary.
  void check_type(const HostDict& d, const std::string& field) const {
    if (typed_ && (utf8_ != d.utf8() || plain_ != d.plain))
      throw Error(FDB_ERR_UNSUPPORTED, "sampler: field " + field + " changes its type between records (" + (plain_ ? "plain " : "dictionary of ") + format_ + " against " +
                                           (d.plain ? "plain " : "dictionary of ") + d.value_format + ")");
  }
  std::shared_ptr<const std::vector<uint32_t>> table_for(const std::shared_ptr<HostDict>& d, const std::string& field) {
    if (!d) throw Error(FDB_ERR_INVALID, "sampler: dictionary column without its dictionary: " + field);
    check_type(*d, field);
    if (!typed_) { typed_ = true; utf8_ = d->utf8(); plain_ = d->plain; format_ = d->value_format; }
    for (const Cached& c : cache_) if (c.dict.get() == d.get()) return c.table;
    for (size_t k = 0; k < cache_.size(); k++)
      if (cache_[k].dict->same_content(*d)) { const auto t = cache_[k].table; remember(d, t); return t; }
    auto t = std::make_shared<std::vector<uint32_t>>(d->values.size());
    for (size_t i = 0; i < d->values.size(); i++) {
      auto it = ids_.find(d->values[i]);
      if (it == ids_.end()) {
        if (values_.size() >= 0xFFFFFFFEull) throw Error(FDB_ERR_UNSUPPORTED, "sampler: more than 2^32 distinct values in field " + field);
        it = ids_.emplace(d->values[i], (uint32_t)values_.size()).first;
        values_.push_back(d->values[i]);
      }
      (*t)[i] = it->second;
    }
    remember(d, t);
    return t;
  }

 private:
  struct Cached { std::shared_ptr<HostDict> dict; std::shared_ptr<const std::vector<uint32_t>> table; };
  void remember(const std::shared_ptr<HostDict>& d, const std::shared_ptr<const std::vector<uint32_t>>& t) {
    if (cache_.size() >= 256) cache_.erase(cache_.begin(), cache_.begin() + 128);  // (bounded: parts with ever-changing dictionaries)
    cache_.push_back(Cached{d, t});
  }
  bool typed_ = false, utf8_ = false, plain_ = false;
  std::string format_;
  std::vector<std::string> values_;
  std::unordered_map<std::string, uint32_t> ids_;
  std::vector<Cached> cache_;
};

}  // namespace fdb
