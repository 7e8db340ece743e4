// CPU-only: prints what the narrow-index cache of a resident record (frostdb_amd/csrc/fdb_record.h, ScanCache) holds for a dictionary
// column, from numbers on the command line, so that tests/test_null_folded_cache_cpu.py can hold the rules to a hand-worked table.
// Host-only (FDB_RECORD_HOST_ONLY: no device, no HIP), so it also builds and runs as its own program under the sanitizers:
//   g++ -std=c++17 -DFDB_RECORD_HOST_ONLY -I frostdb_amd/csrc -I include tools/scan_cache_dump.cpp -o /tmp/scan_cache_dump
//   (… or with -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=undefined added)
//   fold <entries>:<nulls>:<rows> …   per column: the width it is scanned at (4: the column itself, no buffer), whether its buffer is
//                                     null-folded, and the index a NULL row holds then
//   at <rows> <width> <row> …         scan_cache_position of each row
//   form <entries>:<nulls>:<rows> …   per column: the form it is scanned at (H: 4 bits, T: 12 bits, else the byte width), whether that
//                                     buffer is null-folded, the index of NULL, the buffer's bytes
//   pat <rows> <H|T> <row> …          scan_cache_packed_position of each row: low byte (T), nibble byte, nibble shift
#include <cstdio>
#include <cstdlib>
#include <string>

#include "fdb_record.h"

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "";
  if (mode == "fold" && argc > 2) {
    for (int i = 2; i < argc; i++) {
      unsigned long long entries = 0;
      long long nulls = 0, rows = 0;
      if (std::sscanf(argv[i], "%llu:%lld:%lld", &entries, &nulls, &rows) != 3 || nulls < 0 || rows < 0 || nulls > rows) return 2;
      const int w = fdb::scan_cache_width_of((size_t)entries, rows);
      const bool folded = fdb::scan_cache_folds((size_t)entries, nulls, rows);
      if (folded) std::printf("width=%d folded=1 null_index=%llu\n", w, entries);
      else std::printf("width=%d folded=0 null_index=-\n", w);
    }
    return 0;
  }
  if (mode == "at" && argc > 4) {
    const long long rows = std::atoll(argv[2]);
    const int width = std::atoi(argv[3]);
    if (rows <= 0 || (width != 1 && width != 2)) return 2;
    for (int i = 4; i < argc; i++) {
      const long long row = std::atoll(argv[i]);
      if (row < 0 || row >= rows) return 2;
      std::printf("%lld\n", (long long)fdb::scan_cache_position(row, rows, width));
    }
    return 0;
  }
  // the form a launch over such records reads the column at — the packed form where the rule gives one, else the byte form —, whether
  // that buffer is null-folded, the index of NULL, and the buffer's bytes
  if (mode == "form" && argc > 2) {
    for (int i = 2; i < argc; i++) {
      unsigned long long entries = 0;
      long long nulls = 0, rows = 0;
      if (std::sscanf(argv[i], "%llu:%lld:%lld", &entries, &nulls, &rows) != 3 || nulls < 0 || rows < 0 || nulls > rows) return 2;
      const int p = fdb::scan_cache_packed_of((size_t)entries, nulls, rows), w = fdb::scan_cache_width_of((size_t)entries, rows);
      const bool folded = p != 0 ? nulls > 0 : fdb::scan_cache_folds((size_t)entries, nulls, rows);
      const size_t bytes = p != 0 ? fdb::packed_slot((size_t)rows, p) : w < 4 ? fdb::values_slot((size_t)rows, (size_t)w) : 0;
      std::printf("form=%s folded=%d null_index=%s bytes=%zu\n", p == fdb::kScanFormH ? "H" : p == fdb::kScanFormT ? "T" : std::to_string(w).c_str(), (int)folded,
                  folded ? std::to_string(entries).c_str() : "-", bytes);
    }
    return 0;
  }
  // scan_cache_packed_position of each row: the byte of its low 8 bits (T; - for H), the byte of its nibble and the nibble's shift
  if (mode == "pat" && argc > 4) {
    const long long rows = std::atoll(argv[2]);
    const std::string f = argv[3];
    if (rows <= 0 || (f != "H" && f != "T")) return 2;
    for (int i = 4; i < argc; i++) {
      const long long row = std::atoll(argv[i]);
      if (row < 0 || row >= rows) return 2;
      const fdb::PackedAt at = fdb::scan_cache_packed_position(row, rows, f == "H" ? fdb::kScanFormH : fdb::kScanFormT);
      if (at.byte < 0) std::printf("- %lld %d\n", (long long)at.nibble_byte, at.nibble_shift);
      else std::printf("%lld %lld %d\n", (long long)at.byte, (long long)at.nibble_byte, at.nibble_shift);
    }
    return 0;
  }
  std::fprintf(stderr, "scan_cache_dump: fold <entries>:<nulls>:<rows> … | at <rows> <width> <row> … | form <entries>:<nulls>:<rows> … | pat <rows> <H|T> <row> … (see the head of tools/scan_cache_dump.cpp)\n");
  return 2;
}
