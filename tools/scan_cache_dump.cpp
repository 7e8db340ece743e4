// CPU-only: prints what the narrow-index cache of a resident record (frostdb_amd/csrc/fdb_record.h, ScanForm) holds for a dictionary
// column, from numbers on the command line, so that tests/test_null_folded_cache_cpu.py, tests/test_packed_cache_cpu.py and
// tests/test_scan_form_cpu.py can hold the rules to hand-worked tables.
// Host-only (FDB_RECORD_HOST_ONLY: no device, no HIP), so it also builds and runs as its own program under the sanitizers:
//   g++ -std=c++17 -DFDB_RECORD_HOST_ONLY -I frostdb_amd/csrc -I include tools/scan_cache_dump.cpp -o /tmp/scan_cache_dump
//   (… or with -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=undefined added)
//   fold <entries>:<nulls>:<rows> …   per column: the byte width it is scanned at (4: the column itself, no buffer), whether that buffer is
//                                     null-folded, and the index a NULL row holds then
//   at <rows> <width> <row> …         the element (byte / width) of each row in a buffer at 1 or 2 bytes
//   form <entries>:<nulls>:<rows> …   per column: the narrowest form it is scanned at, whether that buffer is null-folded, the index of
//                                     NULL, the buffer's bytes
//   pat <rows> <H|T> <row> …          scan_cache_at of each row of a packed buffer: low byte (T), nibble byte, nibble shift
//   table [<rows> …]                  the form table, a row per form; with row counts, scan_form_slot of each behind every row
//   common <entries>:<nulls>:<rows> … the form a launch over those parts reads the column at
//   forms <entries>:<nulls>:<rows> …  per column: every candidate form, narrowest first, as <name>:<whether its buffer is null-folded>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "fdb_record.h"

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "";
  auto named = [](const std::string& name) -> const fdb::ScanFormRow* {
    for (const fdb::ScanFormRow& f : fdb::kScanForms) if (name == f.name) return &f;
    return nullptr;
  };
  if ((mode == "fold" || mode == "form" || mode == "forms" || mode == "common") && argc > 2) {
    std::vector<fdb::ScanForms> parts;
    for (int i = 2; i < argc; i++) {
      unsigned long long entries = 0;
      long long nulls = 0, rows = 0;
      if (std::sscanf(argv[i], "%llu:%lld:%lld", &entries, &nulls, &rows) != 3 || nulls < 0 || rows < 0 || nulls > rows) return 2;
      const fdb::ScanForms f = fdb::scan_forms_of((size_t)entries, nulls, rows);
      parts.push_back(f);
      int k = 0;
      while (mode == "fold" && fdb::scan_form(f.form[k]).framed) k++;  // (fold: the first candidate that is no packed form)
      const fdb::ScanForm form = f.form[k];
      const bool folded = fdb::scan_form_folds(form, (size_t)entries, nulls);
      if (mode == "fold" || mode == "form")
        std::printf("%s=%s folded=%d null_index=%s", mode == "form" ? "form" : "width", fdb::scan_form_name(form), (int)folded, folded ? std::to_string(entries).c_str() : "-");
      if (mode == "form") std::printf(" bytes=%zu", form == fdb::kScanForm4 ? (size_t)0 : fdb::scan_form_slot((size_t)rows, form));
      for (k = 0; mode == "forms" && k < f.n; k++) std::printf("%s%s:%d", k > 0 ? " " : "", fdb::scan_form_name(f.form[k]), (int)fdb::scan_form_folds(f.form[k], (size_t)entries, nulls));
      if (mode != "common") std::printf("\n");
    }
    if (mode == "common") std::printf("%s\n", fdb::scan_form_name(fdb::scan_form_common(parts.data(), parts.size())));
    return 0;
  }
  if ((mode == "at" || mode == "pat") && argc > 4) {
    const long long rows = std::atoll(argv[2]);
    const fdb::ScanFormRow* f = named(argv[3]);
    if (rows <= 0 || f == nullptr || f->form == fdb::kScanForm4 || f->framed != (mode == "pat")) return 2;
    for (int i = 4; i < argc; i++) {
      const long long row = std::atoll(argv[i]);
      if (row < 0 || row >= rows) return 2;
      const fdb::ScanCacheAt at = fdb::scan_cache_at(row, rows, f->form);
      if (mode == "at") std::printf("%lld\n", (long long)at.byte / at.n_bytes);
      else if (at.n_bytes == 0) std::printf("- %lld %d\n", (long long)at.nibble_byte, at.nibble_shift);
      else std::printf("%lld %lld %d\n", (long long)at.byte, (long long)at.nibble_byte, at.nibble_shift);
    }
    return 0;
  }
  if (mode == "table") {
    for (const fdb::ScanFormRow& f : fdb::kScanForms) {
      std::printf("code=%d name=%s bits=%d max_index=%u block_bytes=%lld framed=%d min_rows=%lld", (int)f.form, f.name, f.bits, f.max_index, (long long)f.block_bytes, (int)f.framed, (long long)f.min_rows);
      for (int i = 2; i < argc; i++) {
        if (std::atoll(argv[i]) <= 0) return 2;
        std::printf(" %zu", fdb::scan_form_slot((size_t)std::atoll(argv[i]), f.form));
      }
      std::printf("\n");
    }
    return 0;
  }
  std::fprintf(stderr, "scan_cache_dump: fold | form | forms | common <entries>:<nulls>:<rows> … ; at <rows> <width> <row> … ; pat <rows> <H|T> <row> … ; table [<rows> …] (see the head of tools/scan_cache_dump.cpp)\n");
  return 2;
}
