// Stand-alone driver of the host-only half of the device MergeRecords for tools/asan_merge.sh: the key layout across records
// (fdb_sortplan.h), the dictionary plan of a column across the inputs and the schema union with its per-input column map of records
// whose field lists differ (fdb_mergerec.h, host-only part) and the merge-path walk of fdb_selftest_merge_path (fdb_mergepath.h). No GPU, no HIP, no python. Prints "asan merge ok" and exits 0 when every check holds.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "fdb_mergepath.h"
#include "fdb_mergerec.h"

using namespace fdb;

#define CHECK(cond) do { if (!(cond)) { std::fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #cond); std::exit(1); } } while (0)

static uint64_t rnd(uint64_t* s) { SplitMix64 g{*s}; const uint64_t v = g.next(); *s = g.x; return v; }

// the layout of every combination of column widths and NULL bits: no field straddles a word, no two fields overlap, every bit is used
static void layouts() {
  const int widths[] = {0, 1, 4, 17, 63, 64};
  uint64_t seed = 3;
  for (int round = 0; round < 2000; round++) {
    std::vector<SortColBits> cols(1 + rnd(&seed) % 6);
    for (SortColBits& c : cols) c = SortColBits{widths[rnd(&seed) % 6], (rnd(&seed) & 1) != 0};
    std::vector<int> bits;
    const std::vector<SortPart> parts = pack_sort_fields(cols, &bits);
    std::vector<uint64_t> used(bits.size(), 0);
    std::vector<int> seen_value(cols.size(), 0), seen_null(cols.size(), 0);
    int last_word = -1, last_col = -1;
    for (const SortPart& p : parts) {
      CHECK(p.word >= 0 && (size_t)p.word < bits.size() && p.col >= 0 && (size_t)p.col < cols.size());
      CHECK(p.word > last_word || (p.word == last_word && p.col > last_col));  // most significant column first
      last_word = p.word; last_col = p.col;
      if (p.width > 0) {
        CHECK(p.width == cols[(size_t)p.col].value_bits && p.shift >= 0 && p.shift + p.width <= bits[(size_t)p.word]);
        const uint64_t m = (p.width >= 64 ? ~0ull : ((1ull << p.width) - 1)) << p.shift;
        CHECK((used[(size_t)p.word] & m) == 0);
        used[(size_t)p.word] |= m;
        seen_value[(size_t)p.col]++;
      }
      if (p.null_shift >= 0) {
        CHECK(cols[(size_t)p.col].has_null_bit && p.null_shift < bits[(size_t)p.word]);
        CHECK((used[(size_t)p.word] & (1ull << p.null_shift)) == 0);
        used[(size_t)p.word] |= 1ull << p.null_shift;
        if (p.width > 0) CHECK(p.null_shift == p.shift + p.width);  // the NULL bit sits right above its value
        seen_null[(size_t)p.col]++;
      }
    }
    for (size_t c = 0; c < cols.size(); c++) CHECK(seen_value[c] == (cols[c].value_bits > 0) && seen_null[c] == (cols[c].has_null_bit ? 1 : 0));
    for (size_t w = 0; w < bits.size(); w++) CHECK(bits[w] >= 1 && bits[w] <= 64 && used[w] == (bits[w] >= 64 ? ~0ull : (1ull << bits[w]) - 1));
  }
  CHECK(bits_for(0) == 0 && bits_for(1) == 0 && bits_for(2) == 1 && bits_for(3) == 2 && bits_for(1000) == 10 && bits_for(1ull << 40) == 40);
}

static void dictionaries() {
  // different dictionaries: the union in first-seen order, ranks by bytes across the inputs, duplicates share a rank
  std::vector<std::shared_ptr<HostDict>> ds = {make_dictionary({"m", "a", "z"}, "z"), nullptr, make_dictionary({"z", "m", "k", "m"}, "z"), make_dictionary({}, "z")};
  MergeDictPlan p = plan_merge_dict(ds, "f", true);
  CHECK(!p.shared && p.distinct == 4 && (p.out->values == std::vector<std::string>{"m", "a", "z", "k"}));
  CHECK(!p.tables[1] && (*p.tables[0] == std::vector<uint32_t>{0, 1, 2}) && (*p.tables[2] == std::vector<uint32_t>{2, 0, 3, 0}) && p.tables[3]->empty());
  CHECK((p.ranks_of(0) == std::vector<uint32_t>{2, 0, 3}) && (p.ranks_of(2) == std::vector<uint32_t>{3, 2, 1, 2}) && p.ranks_of(3).empty());
  for (size_t r : {0u, 2u})
    for (size_t q : {0u, 2u})
      for (size_t i = 0; i < ds[r]->values.size(); i++)
        for (size_t j = 0; j < ds[q]->values.size(); j++) {
          const int c = ds[r]->values[i].compare(ds[q]->values[j]);
          const uint32_t x = p.ranks_of(r)[i], y = p.ranks_of(q)[j];
          CHECK((c < 0) == (x < y) && (c == 0) == (x == y));
        }
  // one dictionary's content everywhere (another object, same content): shared, nothing translated, duplicates kept
  HostDict copy = *make_dictionary({"b", "a", "b"}, "u");
  std::vector<std::shared_ptr<HostDict>> same = {make_dictionary({"b", "a", "b"}, "u"), std::make_shared<HostDict>(copy), nullptr};
  MergeDictPlan s = plan_merge_dict(same, "g", true);
  CHECK(s.shared && s.out.get() == same[0].get() && !s.tables[0] && !s.tables[1] && s.distinct == 2 && (s.ranks_of(1) == std::vector<uint32_t>{1, 0, 1}));
  MergeDictPlan no_ranks = plan_merge_dict(same, "g", false);
  CHECK(no_ranks.out_ranks.empty());
  // utf8 against binary with the same entries, plain against dictionary: refused; no input at all: invalid
  int refused = 0;
  try { plan_merge_dict({make_dictionary({"x"}, "u"), make_dictionary({"x"}, "z")}, "h", true); } catch (const Error& e) { refused += e.code == FDB_ERR_UNSUPPORTED; }
  try { plan_merge_dict({make_dictionary({"x"}, "z"), make_plain_dictionary({"x"}, "z")}, "h", true); } catch (const Error& e) { refused += e.code == FDB_ERR_UNSUPPORTED; }
  try { plan_merge_dict({nullptr, nullptr}, "h", true); } catch (const Error& e) { refused += e.code == FDB_ERR_INVALID; }
  CHECK(refused == 3);
  // a plain column's union stays plain
  MergeDictPlan pl = plan_merge_dict({make_plain_dictionary({"p", "q"}, "u"), make_plain_dictionary({"q", "r"}, "u")}, "i", true);
  CHECK(!pl.shared && pl.out->plain && pl.out->utf8() && pl.distinct == 3);
}

// the walk against std::stable_sort of the tagged concatenation
static void walk(const std::vector<std::vector<uint64_t>>& a, const std::vector<std::vector<uint64_t>>& b, int W) {
  std::vector<uint64_t> fa, fb;
  for (const auto& k : a) fa.insert(fa.end(), k.begin(), k.end());
  for (const auto& k : b) fb.insert(fb.end(), k.begin(), k.end());
  std::vector<uint32_t> got(a.size() + b.size());  // exactly na + nb entries: a write past the end is the sanitizer's to find
  CHECK(fdb_merge_path_host(fa.data(), (int64_t)a.size(), fb.data(), (int64_t)b.size(), W, got.data()) == 0);
  std::vector<uint32_t> want(got.size());
  for (size_t i = 0; i < want.size(); i++) want[i] = (uint32_t)i;
  auto key = [&](uint32_t s) -> const std::vector<uint64_t>& { return s < a.size() ? a[s] : b[s - a.size()]; };
  std::stable_sort(want.begin(), want.end(), [&](uint32_t x, uint32_t y) { return key(x) < key(y); });
  CHECK(got == want);
}

static void merge_paths() {
  uint64_t seed = 9;
  for (int W : {1, 2, 3, 5, 9}) {
    const int64_t T = fdb_merge_tile(W);
    CHECK(T == (int64_t)FDB_MERGE_BLOCK * fdb_merge_items(W));
    auto run = [&](int64_t n, uint64_t distinct) {
      std::vector<std::vector<uint64_t>> r((size_t)n, std::vector<uint64_t>((size_t)W));
      for (auto& k : r) for (int w = 0; w < W; w++) k[(size_t)w] = w + 1 < W ? rnd(&seed) % 2 : rnd(&seed) % distinct;
      std::sort(r.begin(), r.end());
      return r;
    };
    const int64_t sizes[][2] = {{0, 0}, {0, 1}, {1, 0}, {1, 2 * T}, {2 * T, 1}, {T, T}, {T - 1, T + 2}, {3 * T + 1, 0}, {0, 3 * T + 1}, {T + 1, 2 * T}};
    for (const auto& s : sizes)
      for (uint64_t distinct : {1ull, 3ull, ~0ull}) walk(run(s[0], distinct), run(s[1], distinct), W);
    for (int k = 0; k < 40; k++) walk(run((int64_t)(rnd(&seed) % (uint64_t)(2 * T)), 5), run((int64_t)(rnd(&seed) % (uint64_t)(2 * T)), 5), W);
  }
  // runs that are NOT sorted: the walk reports the tile instead of indexing outside the runs
  const int64_t T = fdb_merge_tile(1);
  std::vector<uint64_t> a((size_t)(2 * T)), b((size_t)(2 * T));
  for (size_t i = 0; i < a.size(); i++) { a[i] = rnd(&seed); b[i] = rnd(&seed); }
  std::vector<uint32_t> out(a.size() + b.size());
  (void)fdb_merge_path_host(a.data(), (int64_t)a.size(), b.data(), (int64_t)b.size(), 1, out.data());
}

// the schema union and the column map over random field lists: dynamic and plain expressions, 0 to 6 records, empty records, and —
// refused — duplicate names and kind conflicts
static void schemas() {
  const char* pool[] = {"labels.a", "labels.b", "labels.c", "labels.", "labels", "labelsx", "pprof.x", "pprof.y", "timestamp", "value", ""};
  const size_t P = sizeof(pool) / sizeof(pool[0]);
  uint64_t seed = 21;
  int refused = 0, accepted = 0;
  for (int round = 0; round < 600; round++) {
    std::vector<std::vector<MergeField>> recs(rnd(&seed) % 7);
    bool duplicate = false, conflict = false;
    std::vector<int32_t> kind_of(P, 0);
    for (auto& r : recs) {
      const size_t n = rnd(&seed) % 9;
      for (size_t f = 0; f < n; f++) {
        const size_t k = rnd(&seed) % P;
        const int32_t kind = rnd(&seed) % 16 == 0 ? 3 : (k < 8 ? 6 : 1);  // now and then another kind than the name's usual one
        for (const MergeField& g : r) duplicate = duplicate || g.name == pool[k];
        r.push_back(MergeField{pool[k], kind});
      }
    }
    for (const auto& r : recs)
      for (const MergeField& f : r)
        for (size_t k = 0; k < P; k++)
          if (f.name == pool[k]) { conflict = conflict || (kind_of[k] != 0 && kind_of[k] != f.kind); kind_of[k] = f.kind; }
    const MergeOrder exprs[] = {{"labels", true}, {"pprof", true}, {"timestamp", false}, {"labels.a", false}, {"missing", true}, {"", false}, {"", true}};
    std::vector<MergeOrder> order;
    for (size_t k = 0, n = 1 + rnd(&seed) % 3; k < n; k++) order.push_back(exprs[rnd(&seed) % 7]);
    MergeSchema u;
    try {
      u = unify_merge_schema(recs, order);
    } catch (const Error& e) {
      CHECK(e.code == FDB_ERR_INVALID && (duplicate || conflict));
      refused++;
      continue;
    }
    CHECK(!duplicate && !conflict);
    accepted++;
    const size_t C = u.first.size(), S = u.sort_expr.size();
    CHECK(S <= C && u.map.size() == recs.size());
    std::vector<std::string> names;
    for (const MergeSchema::At& at : u.first) {
      CHECK(at.record >= 0 && (size_t)at.record < recs.size() && at.field >= 0 && (size_t)at.field < recs[(size_t)at.record].size());
      names.push_back(recs[(size_t)at.record][(size_t)at.field].name);
    }
    for (size_t c = 0; c < C; c++) {
      for (size_t d = 0; d < c; d++) CHECK(names[d] != names[c]);  // a field is emitted once
      for (int32_t r = 0; r < u.first[c].record; r++)              // … named by its first occurrence
        for (const MergeField& f : recs[(size_t)r]) CHECK(f.name != names[c]);
      bool matched = false;  // by an expression up to the column's own (sorting columns), by none at all (the rest)
      for (size_t e = 0; e < order.size(); e++) matched = matched || merge_order_matches(order[e], names[c]);
      CHECK(matched == (c < S));
      if (c < S) {
        CHECK(u.sort_expr[c] >= 0 && (size_t)u.sort_expr[c] < order.size() && merge_order_matches(order[(size_t)u.sort_expr[c]], names[c]));
        for (int32_t e = 0; e < u.sort_expr[c]; e++) CHECK(!merge_order_matches(order[(size_t)e], names[c]));  // the first expression that matches takes it
        if (c > 0) CHECK(u.sort_expr[c - 1] < u.sort_expr[c] || (u.sort_expr[c - 1] == u.sort_expr[c] && names[c - 1] < names[c]));  // expression order, then byte order
      }
    }
    size_t distinct = 0;
    for (size_t r = 0; r < recs.size(); r++) {
      CHECK(u.map[r].size() == C);
      size_t present = 0;
      for (size_t c = 0; c < C; c++) {
        const int32_t f = u.map[r][c];
        CHECK(f >= -1 && f < (int32_t)recs[r].size());
        if (f >= 0) { CHECK(recs[r][(size_t)f].name == names[c]); present++; }
        else for (const MergeField& g : recs[r]) CHECK(g.name != names[c]);
      }
      CHECK(present == recs[r].size());  // every field of every record has its output column
      distinct += present;
    }
    CHECK(distinct >= C || recs.empty());
  }
  CHECK(refused > 50 && accepted > 50);
}

int main() {
  layouts();
  dictionaries();
  schemas();
  merge_paths();
  std::puts("asan merge ok");
  return 0;
}
