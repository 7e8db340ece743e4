// Stand-alone driver of the host-only half of the resident record's layout contract (frostdb_amd/csrc/fdb_record.h) for
// tools/asan_record.sh: the slot arithmetic, RecordLayout and finish_column. No GPU, no HIP, no python. Prints "asan record ok" and exits
// 0 when every check holds.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "fdb_record.h"

using namespace fdb;

#define CHECK(cond) do { if (!(cond)) { std::fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #cond); std::exit(1); } } while (0)

// A random column list: every slot 256-aligned, in order without overlap, ending at least kTailPad past its payload; the total is their sum.
static void layout(std::mt19937_64& rng) {
  const size_t rows = (size_t)(rng() % 70001), n_cols = (size_t)(rng() % 9);
  RecordLayout L;
  std::vector<size_t> width;
  std::vector<char> nullable;
  for (size_t c = 0; c < n_cols; c++) {
    width.push_back(rng() & 1 ? 4 : 8);
    nullable.push_back((char)(rng() & 1));
    L.add(rows, width[c], nullable[c] != 0);
  }
  CHECK(L.cols.size() == n_cols);
  size_t at = 0;
  for (size_t c = 0; c < n_cols; c++) {
    CHECK(L.cols[c].val_off == at && at % 256 == 0);
    CHECK(values_slot(rows, width[c]) % 256 == 0 && values_slot(rows, width[c]) >= rows * width[c] + kTailPad);
    at += values_slot(rows, width[c]);
    CHECK((L.cols[c].bit_off != kNoSlot) == (nullable[c] != 0));
    if (!nullable[c]) continue;
    CHECK(L.cols[c].bit_off == at && at % 256 == 0);
    CHECK(bitmap_slot(rows) % 256 == 0 && bitmap_slot(rows) >= (rows + 63) / 64 * 8 + kTailPad);
    at += bitmap_slot(rows);
  }
  CHECK(L.total == at);
}

static void finishing() {
  static int64_t values[4], bitmap[4];
  int64_t payload = 0, want = 0;
  for (ColKind kind : {ColKind::I64, ColKind::U64, ColKind::F64, ColKind::BOOL, ColKind::STR, ColKind::DICT})
    for (int64_t rows : {0, 1, 7, 8, 9, 64, 65, 70000})
      for (int64_t nulls : {(int64_t)0, rows / 2, rows}) {
        DevColumn d;
        d.kind = kind;
        payload += finish_column(&d, rows, nulls, values, bitmap);
        CHECK(d.length == rows && d.null_count == nulls && d.d_values == values);
        CHECK(d.value_bytes == (kind == ColKind::BOOL ? (rows + 7) / 8 : rows * (kind == ColKind::DICT || kind == ColKind::STR ? 4 : 8)));
        CHECK((d.d_validity != nullptr) == (nulls > 0) && d.validity_bytes == (nulls > 0 ? (rows + 7) / 8 : 0));
        CHECK(d.d_validity == nullptr || d.d_validity == (uint8_t*)bitmap);
        want += d.value_bytes + d.validity_bytes;
      }
  CHECK(payload == want && payload > 0);
  CHECK(value_width(ColKind::DICT) == 4 && value_width(ColKind::STR) == 4 && value_width(ColKind::BOOL) == 8 && value_width(ColKind::F64) == 8);
}

int main() {
  std::mt19937_64 rng(20240607);
  for (int k = 0; k < 2000; k++) layout(rng);
  // the three ways a bitmap's payload has been written down give one slot
  for (size_t rows = 0; rows <= 70000; rows++) {
    CHECK(bitmap_slot(rows) == align_up((rows + 7) / 8 + kTailPad, 256));
    CHECK(bitmap_slot(rows) == align_up((rows + 31) / 32 * 4 + kTailPad, 256));
  }
  finishing();
  std::printf("asan record ok\n");
  return 0;
}
