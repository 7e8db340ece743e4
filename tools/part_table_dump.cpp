// Test aid (host only, no GPU and no HIP runtime): the packed part table of a dense scan launch (fdb_jit.h, JitShape::part_table) for
// hand-built argument blocks of three shapes — the field list jit_part_fields gives the shape, W, and the words jit_pack_parts writes
// for each record — so that tests/test_part_table_cpu.py can hold them to hand-worked values, and so that the packer runs under
// sanitizers on its own:
//   g++ -std=c++17 -D__HIP_PLATFORM_AMD__ -I frostdb_amd/csrc -I include -I /opt/rocm/include tools/part_table_dump.cpp \
//       frostdb_amd/csrc/fdb_jitgen.cpp -o /tmp/part_table_dump          (add -fsanitize=address,undefined -fno-sanitize-recover=all)
//   /tmp/part_table_dump            every shape: fields, W, words
//   /tmp/part_table_dump source K   the kernel source of shape K with the part table on (its record entry reads W words per record)
// Pointers are made-up addresses: nothing is dereferenced.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "frostdb_amd.h"
#include "fdb_kernels.h"
#include "fdb_jit.h"

static const void* addr(unsigned long long v) { return (const void*)(uintptr_t)v; }

// Shape 0 — bench.py's headline: `labels.code == X`, SUM(value) GROUP BY labels.path over null-folded narrow-index caches (no bitmaps);
// the filter's truth table rides in a 64-bit word, the group LUT sits in LDS. Two records.
static std::vector<FdbScanArgs> headline() {
  std::vector<FdbScanArgs> v(2);
  for (size_t k = 0; k < v.size(); k++) {
    FdbScanArgs& a = v[k];
    std::memset(&a, 0, sizeof a);
    a.n_rows = k == 0 ? 25000000 : 1048577;
    a.tile_begin = k == 0 ? 0 : 6104; a.tile_end = k == 0 ? 6104 : 6361;
    a.lds_acc = 1; a.n_c4 = 2; a.n_c8 = 1; a.n_leaves = 1; a.n_code = 1; a.n_gcols = 1; a.n_aggs = 1;
    a.c4[0].values = addr(0x7f0000001000ull + k * 0x100000000ull); a.w4[0] = 1;
    a.c4[1].values = addr(0x7f0000002000ull + k * 0x100000000ull); a.w4[1] = 2;
    a.c8[0].values = addr(0x7f0000003000ull + k * 0x100000000ull);
    a.leaves[0].kind = FDB_LEAF_DICT_BITS; a.leaves[0].lit = 0x25; a.leaves[0].lut_len = 7; a.leaves[0].lut_lds = FDB_NO_LDS;
    a.gcols[0].lut = (const uint32_t*)addr(0x7e0000000040ull); a.gcols[0].lut_len = 1025; a.gcols[0].lut_lds = 0; a.gcols[0].stride = 1; a.gcols[0].slot = 1;
    a.aggs[0].func = FDB_AGG_SUM; a.aggs[0].type = FDB_T_F64; a.aggs[0].slot = 0;
    a.lut_class = 0;
  }
  return v;
}

// Shape 1 — two-phase, three records of two LUT classes: a 1-byte filter column with a bitmap in every record, read by a truth table in
// LDS (a LUT leaf) and by an IS NOT NULL leaf; a late 2-byte group column whose bitmap only record 1 has (has_validity 2); two late
// 8-byte columns, COUNT / MIN / SUM.
static std::vector<FdbScanArgs> two_phase() {
  std::vector<FdbScanArgs> v(3);
  for (size_t k = 0; k < v.size(); k++) {
    FdbScanArgs& a = v[k];
    std::memset(&a, 0, sizeof a);
    a.n_rows = 1048576 + (long long)k;
    static const long long ends[4] = {0, 256, 513, 770};  // (4 096-row tiles: 256, 257 and 257 of them)
    a.tile_begin = ends[k]; a.tile_end = ends[k + 1];
    a.lds_acc = 1; a.need_count = 1; a.n_c4 = 1; a.n_l4 = 1; a.n_l8 = 2; a.n_leaves = 2; a.n_code = 3; a.n_gcols = 1; a.n_aggs = 3;
    a.code[0] = 0; a.code[1] = 1; a.code[2] = FDB_CODE_AND;
    a.c4[0].values = addr(0x10000 + k * 0x1000); a.c4[0].validity = (const uint8_t*)addr(0x20000 + k * 0x1000); a.w4[0] = 1;
    a.l4[0].values = addr(0x30000 + k * 0x1000); a.l4[0].validity = k == 1 ? (const uint8_t*)addr(0x40000) : nullptr; a.wl4[0] = 2;
    a.l8[0].values = addr(0x50000 + k * 0x1000); a.l8[1].values = addr(0x60000 + k * 0x1000);
    a.leaves[0].kind = FDB_LEAF_DICT_LUT; a.leaves[0].lut = (const uint8_t*)addr(0x70000 + (k == 2 ? 0x800 : 0)); a.leaves[0].lut_len = 200; a.leaves[0].lut_lds = 0; a.leaves[0].slot = 0;
    a.leaves[1].kind = FDB_LEAF_VALIDITY; a.leaves[1].op = 1; a.leaves[1].lut_lds = FDB_NO_LDS; a.leaves[1].slot = 0;
    a.gcols[0].lut = (const uint32_t*)addr(0x70100 + (k == 2 ? 0x800 : 0)); a.gcols[0].lut_len = 300 + (uint32_t)k; a.gcols[0].lut_lds = 208; a.gcols[0].stride = 1; a.gcols[0].slot = 0;
    a.aggs[0].func = FDB_AGG_COUNT; a.aggs[0].type = FDB_T_I64; a.aggs[0].slot = 1;
    a.aggs[1].func = FDB_AGG_MIN; a.aggs[1].type = FDB_T_I64; a.aggs[1].slot = 0;
    a.aggs[2].func = FDB_AGG_SUM; a.aggs[2].type = FDB_T_F64; a.aggs[2].slot = 1;
    a.lut_class = k == 2 ? 1 : 0;
  }
  return v;
}

// Shape 2 — single-phase with a computed input: `value > T` on the 8-byte column (a literal), SUM(value * L) (an expression literal),
// GROUP BY a 2-byte column whose LUT is too big for LDS (gathered from memory), with a stride. One record.
static std::vector<FdbScanArgs> computed() {
  std::vector<FdbScanArgs> v(1);
  FdbScanArgs& a = v[0];
  std::memset(&a, 0, sizeof a);
  a.n_rows = 5000000; a.tile_begin = 0; a.tile_end = 1221;
  a.lds_acc = 1; a.n_c4 = 1; a.n_c8 = 1; a.n_leaves = 1; a.n_code = 1; a.n_gcols = 1; a.n_aggs = 1; a.n_expr = 3;
  a.c4[0].values = addr(0xA000); a.w4[0] = 2;
  a.c8[0].values = addr(0xB000);
  a.leaves[0].kind = FDB_LEAF_CMP_F64; a.leaves[0].op = 5; a.leaves[0].wide = 1; a.leaves[0].lit = 0x4059000000000000ll; a.leaves[0].lut_len = 1; a.leaves[0].lut_lds = FDB_NO_LDS;
  a.gcols[0].lut = (const uint32_t*)addr(0xC000); a.gcols[0].lut_len = 60000; a.gcols[0].lut_lds = FDB_NO_LDS; a.gcols[0].stride = 7; a.gcols[0].slot = 0;
  a.expr[0].kind = 0; a.expr[0].slot = 0; a.expr[0].type = FDB_T_F64; a.expr[0].left = a.expr[0].right = -1;
  a.expr[1].kind = 1; a.expr[1].lit = 0x3FE0000000000000ll; a.expr[1].type = FDB_T_F64; a.expr[1].slot = -1; a.expr[1].left = a.expr[1].right = -1;
  a.expr[2].kind = 2; a.expr[2].op = FDB_OP_MUL; a.expr[2].left = 0; a.expr[2].right = 1; a.expr[2].type = FDB_T_F64; a.expr[2].slot = -1;
  a.aggs[0].func = FDB_AGG_SUM; a.aggs[0].type = FDB_T_F64; a.aggs[0].slot = -1; a.aggs[0].expr = 3;
  a.lut_class = 0;
  return v;
}

int main(int argc, char** argv) {
  const char* names[3] = {"headline", "two_phase", "computed"};
  std::vector<FdbScanArgs> sets[3] = {headline(), two_phase(), computed()};
  const bool two[3] = {false, true, false};
  const int only = argc > 2 && std::string(argv[1]) == "source" ? std::atoi(argv[2]) : -1;
  for (int k = 0; k < 3; k++) {
    const std::vector<FdbScanArgs>& v = sets[k];
    fdb::JitShape s = fdb::jit_shape(v[0], two[k], 256);
    for (size_t i = 1; i < v.size(); i++)
      if (!fdb::jit_shape_merge_args(&s, v[0], v[i], two[k])) { std::fprintf(stderr, "part_table_dump: records of shape %s do not merge\n", names[k]); return 1; }
    s.part_table = true;
    if (only >= 0) { if (only == k) std::fputs(fdb::jit_source(s).c_str(), stdout); continue; }
    const std::vector<fdb::PartField> fields = fdb::jit_part_fields(s);
    const int W = fdb::jit_part_words(s);
    std::printf("shape %s key=%s records=%zu W=%d\n", names[k], s.key().c_str(), v.size(), W);
    for (const fdb::PartField& f : fields) {
      const char* pools[4] = {"c4", "c8", "l4", "l8"};
      std::string where;
      if (f.what == fdb::PartField::SLOT_VALUES || f.what == fdb::PartField::SLOT_VALIDITY) where = std::string(pools[f.pool]) + "[" + std::to_string(f.index) + "].";
      else if (f.what >= fdb::PartField::LEAF_LIT && f.what <= fdb::PartField::EXPR_LIT) where = "[" + std::to_string(f.index) + "] ";
      std::printf("  field %s%s bits=%d word=%d shift=%d\n", where.c_str(), fdb::jit_part_field_name(f.what), f.bits, f.word, f.shift);
    }
    std::vector<const FdbScanArgs*> ptrs;
    for (const FdbScanArgs& a : v) ptrs.push_back(&a);
    std::vector<unsigned long long> words(v.size() * (size_t)W, 0xDEADBEEFDEADBEEFull);
    fdb::jit_pack_parts(s, ptrs.data(), ptrs.size(), words.data());
    for (size_t i = 0; i < v.size(); i++) {
      std::printf("  record %zu:", i);
      for (int w = 0; w < W; w++) std::printf(" %016llx", words[i * (size_t)W + (size_t)w]);
      std::printf("\n");
    }
  }
  return 0;
}
