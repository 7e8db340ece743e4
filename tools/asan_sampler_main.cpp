// Stand-alone driver of the host-only half of Take and the Sampler (frostdb_amd/csrc/fdb_reservoir.h) for tools/asan_sampler.sh: the
// selection (Algorithm L, the last-pair-per-slot pass), the dictionary union with its translation tables, and the index validation.
// No GPU, no HIP, no python. Prints "asan sampler ok" and exits 0 when every check holds.
#include <cstdio>
#include <cstdlib>
#include <set>
#include <string>
#include <vector>

#include "fdb_reservoir.h"

using namespace fdb;

#define CHECK(cond) do { if (!(cond)) { std::fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #cond); std::exit(1); } } while (0)

static void selection(uint64_t seed, int64_t size, const std::vector<int64_t>& lens) {
  ReservoirSelect sel(size, seed);
  std::vector<int64_t> kept;  // slot → global row: what a reservoir would hold
  std::vector<uint8_t> stamp;
  int64_t base = 0, total = 0;
  for (int64_t rows : lens) {
    std::vector<uint32_t> pairs;
    sel.push(rows, [&](int64_t row, int64_t slot) {
      CHECK(row >= 0 && row < rows && slot >= 0 && slot < size);
      pairs.push_back((uint32_t)row);
      pairs.push_back((uint32_t)slot);
    });
    CHECK(sel.kept() <= size);
    kept.resize((size_t)sel.kept(), -1);
    stamp.resize((size_t)sel.kept(), 0);
    // the sequential replacement and the de-duplicated launch must leave the same reservoir
    std::vector<int64_t> seq = kept;
    for (size_t k = 0; k + 1 < pairs.size(); k += 2) { CHECK(pairs[k + 1] < seq.size()); seq[pairs[k + 1]] = base + pairs[k]; }
    const size_t m = keep_last_per_slot(&pairs, &stamp);
    CHECK(pairs.size() == 2 * m);
    std::set<uint32_t> slots;
    for (size_t k = 0; k < m; k++) { CHECK(slots.insert(pairs[2 * k + 1]).second); kept[pairs[2 * k + 1]] = base + pairs[2 * k]; }
    for (uint8_t s : stamp) CHECK(s == 0);
    CHECK(seq == kept);
    base += rows;
    total += rows;
  }
  CHECK((int64_t)kept.size() == (total < size ? total : size));
  std::set<int64_t> distinct(kept.begin(), kept.end());
  CHECK(distinct.size() == kept.size());
  for (int64_t r : kept) CHECK(r >= 0 && r < total);
}

static void dictionaries() {
  DictUnion u;
  std::shared_ptr<HostDict> a = make_dictionary({"x", "y", "z"}, "u"), b = make_dictionary({"z", "w", "x", "w"}, "u"), a2 = make_dictionary({"x", "y", "z"}, "u");
  auto ta = u.table_for(a, "f");
  CHECK((*ta == std::vector<uint32_t>{0, 1, 2}));
  auto tb = u.table_for(b, "f");
  CHECK((*tb == std::vector<uint32_t>{2, 3, 0, 3}));
  CHECK(u.table_for(a2, "f").get() == ta.get());  // interned or equal by content: the cached table
  HostDict copy = *a;                              // same content, another object
  CHECK(u.table_for(std::make_shared<HostDict>(copy), "f").get() == ta.get());
  CHECK((u.values() == std::vector<std::string>{"x", "y", "z", "w"}));
  CHECK(u.utf8() && !u.plain());
  bool refused = false;
  try { u.table_for(make_dictionary({"x"}, "z"), "f"); } catch (const Error& e) { refused = e.code == FDB_ERR_UNSUPPORTED; }
  CHECK(refused);
  refused = false;
  try { u.table_for(make_plain_dictionary({"x"}, "u"), "f"); } catch (const Error& e) { refused = e.code == FDB_ERR_UNSUPPORTED; }
  CHECK(refused);
  CHECK((u.values() == std::vector<std::string>{"x", "y", "z", "w"}));  // a refused dictionary adds nothing
  // many dictionaries: the cache is bounded, the tables stay right
  DictUnion p;
  for (int k = 0; k < 600; k++) {
    std::shared_ptr<HostDict> d = make_plain_dictionary({"v" + std::to_string(k), "shared", ""}, "z");
    auto t = p.table_for(d, "g");
    CHECK(t->size() == 3 && p.values()[(*t)[0]] == "v" + std::to_string(k) && p.values()[(*t)[1]] == "shared" && p.values()[(*t)[2]].empty());
  }
  CHECK(p.values().size() == 602 && p.plain() && !p.utf8());
  DictUnion e;  // an empty dictionary (a column of NULLs)
  CHECK(e.table_for(make_dictionary({}, "z"), "h")->empty() && e.values().empty());
}

static void indices() {
  const int32_t ok[] = {4, 0, 4, 2}, neg[] = {1, -1}, past[] = {0, 5};
  check_take_indices(ok, 4, 5);
  check_take_indices(nullptr, 0, 0);
  int refused = 0;
  try { check_take_indices(neg, 2, 5); } catch (const Error& e) { refused += e.code == FDB_ERR_INVALID; }
  try { check_take_indices(past, 2, 5); } catch (const Error& e) { refused += e.code == FDB_ERR_INVALID; }
  try { check_take_indices(ok, 1, 0); } catch (const Error& e) { refused += e.code == FDB_ERR_INVALID; }
  try { check_take_indices(nullptr, 3, 5); } catch (const Error& e) { refused += e.code == FDB_ERR_INVALID; }
  try { check_take_indices(ok, -1, 5); } catch (const Error& e) { refused += e.code == FDB_ERR_INVALID; }
  CHECK(refused == 5);
}

int main() {
  const std::vector<std::pair<int64_t, std::vector<int64_t>>> shapes = {
      {5, {7, 1, 12}}, {3, {3, 5000}}, {64, {1, 64, 65, 1000}}, {1, {1, 1, 1, 1, 1, 1}}, {4, {4, 5}}, {10, {4, 5}}, {0, {4, 5}}, {5, {0, 7, 0, 13}},
      {1000, {999, 1, 0, 1, 100000}}, {2, {1, 0, 1, 0, 50}}};
  for (const auto& s : shapes)
    for (uint64_t seed = 0; seed < 200; seed++) selection(seed, s.first, s.second);
  selection(0xFFFFFFFFFFFFFFFFull, 7, {3, 3, 3, 1000000});
  dictionaries();
  indices();
  std::puts("asan sampler ok");
  return 0;
}
