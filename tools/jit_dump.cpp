// Tuning aid (CPU-only): prints the source the generators of frostdb_amd/csrc/fdb_jitgen.cpp write for a shape — by default the
// run-time specialised hash-scan kernel for a cfg 5-like shape (N dictionary key columns with validity, SUM(float64) + COUNT) — so
// that it can be compiled offline, and so that its text can be pinned (tests/jit_corpus.py, tests/test_jit_source_identity_cpu.py):
//   g++ -std=c++17 -D__HIP_PLATFORM_AMD__ -I frostdb_amd/csrc -I include -I /opt/rocm/include tools/jit_dump.cpp frostdb_amd/csrc/*.o \
//       -L/opt/rocm/lib -lamdhip64 -lhiprtc -ldl -lpthread -lz -Wl,-rpath,/opt/rocm/lib -o /tmp/jit_dump
//   (the library's objects, fdb_jitgen.cpp.o among them, not the .so: the generators are internals and the .so exports the C ABI only)
//   /tmp/jit_dump 32 > /tmp/k.hip && hipcc --offload-arch=gfx950 -O3 -std=c++17 -munsafe-fp-atomics -DFDB_DEVICE_ONLY=1 \
//       -I frostdb_amd/csrc --cuda-device-only -Rpass-analysis=kernel-resource-usage -c /tmp/k.hip -o /tmp/k.o
#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <string>
#include <vector>

#include "frostdb_amd.h"
#include "fdb_kernels.h"
#include "fdb_jit.h"

// Expressions in postfix, tokens separated by ',', expressions by ';' (the `project` mode's fields, `agg=` / `key=` of the other modes):
//   c<t><slot>[n]  column of type i (int64) / u (uint64) / f (float64) in 8-byte slot <slot>, n: with a validity bitmap
//   l<t>           literal of that type          + - * /   arithmetic (type of the left operand)
//   q1 … q6        comparison (fdb_op EQ … GT_EQ)          and / or   over two booleans
//   cv  nu  if     convert(int64 → float64) / isnull(column) / if(cond, then, else) — operands pushed in that order
//   db<slot>[n]    a dictionary column (4-byte slot) compared with a string literal: truth table in a 64-bit word
//   dl<slot>[n]    … truth table in LDS          u8<slot>  a uint64 column (early 8-byte slot) compared as a filter leaf does
//   e.g.  'ci0,ci1,*'    'ci0n,ci1n,/,ci2,+;ci0n,cv,cf3,*'    'db0n,ci0,li,q5,and'
// Appends the nodes to `exprs` and returns the root of every expression. What a column or a compared column means to the shape is the
// mode's business: `col(slot, nullable)` notes an 8-byte expression column, `leaf(kind, wide, lut_in_lds, slot, nullable)` adds the
// leaf of a compared column and returns its index.
template <typename C, typename L>
static std::vector<int> parse_exprs(const std::string& spec, std::vector<fdb::JitExprNode>& exprs, C col, L leaf) {
  std::vector<int> roots, st;
  auto push = [&](fdb::JitExprNode n) { exprs.push_back(n); st.push_back((int)exprs.size() - 1); };
  auto pop = [&]() { if (st.empty()) { std::fprintf(stderr, "jit_dump: malformed expression\n"); std::exit(2); } const int v = st.back(); st.pop_back(); return v; };
  auto type_of = [](char t) { return t == 'i' ? FDB_T_I64 : t == 'u' ? FDB_T_U64 : FDB_T_F64; };
  size_t at = 0;
  while (at <= spec.size()) {
    size_t end = spec.find_first_of(",;", at);
    if (end == std::string::npos) end = spec.size();
    const std::string t = spec.substr(at, end - at);
    const bool nullable = !t.empty() && t.back() == 'n' && t != "and";
    if (t.size() >= 3 && t[0] == 'c' && (t[1] == 'i' || t[1] == 'u' || t[1] == 'f')) {
      const int slot = t[2] - '0';
      col(slot, nullable);
      push({0, 0, -1, -1, slot, type_of(t[1])});
    } else if (t.size() == 2 && t[0] == 'l') push({1, 0, -1, -1, -1, type_of(t[1])});
    else if (t == "+" || t == "-" || t == "*" || t == "/") {
      const int r = pop(), l = pop();
      push({2, t == "+" ? FDB_OP_ADD : t == "-" ? FDB_OP_SUB : t == "*" ? FDB_OP_MUL : FDB_OP_DIV, l, r, -1, exprs[(size_t)l].type});
    } else if (t.size() == 2 && t[0] == 'q') { const int r = pop(), l = pop(); push({3, t[1] - '0', l, r, -1, FDB_T_BOOL}); }
    else if (t == "and" || t == "or") { const int r = pop(), l = pop(); push({3, t == "and" ? FDB_OP_AND : FDB_OP_OR, l, r, -1, FDB_T_BOOL}); }
    else if (t == "cv") { const int l = pop(); push({4, 0, l, -1, -1, FDB_T_F64}); }
    else if (t == "nu") { const int l = pop(); push({5, 0, l, -1, -1, FDB_T_BOOL}); }
    else if (t == "if") { const int e = pop(), th = pop(), c = pop(); push({6, c, th, e, -1, FDB_T_I64}); }
    else if (t.size() >= 3 && (t.substr(0, 2) == "db" || t.substr(0, 2) == "dl" || t.substr(0, 2) == "u8")) {
      const int slot = t[2] - '0';
      const int l = t[0] == 'u' ? leaf(FDB_LEAF_CMP_U64, 1, false, slot, nullable) : leaf(t[1] == 'b' ? FDB_LEAF_DICT_BITS : FDB_LEAF_DICT_LUT, 0, t[1] == 'l', slot, nullable);
      push({7, 0, -1, -1, l, FDB_T_BOOL});
    } else if (!t.empty()) { std::fprintf(stderr, "jit_dump: unknown token %s\n", t.c_str()); std::exit(2); }
    if (end == spec.size() || spec[end] == ';') { roots.push_back(pop()); st.clear(); }
    at = end + 1;
  }
  return roots;
}

// The dense kernels' shapes: an expression column is an 8-byte slot of the pool the aggregates read (late in the two-phase layout, which
// is also the Projection's), a compared column an early slot.
static std::vector<int> parse_into(fdb::JitShape& s, const std::string& spec) {
  return parse_exprs(spec, s.exprs,
    [&](int slot, bool nullable) {
      fdb::JitSlot* p = s.two_phase ? s.l8 : s.c8;
      int& n = s.two_phase ? s.n_l8 : s.n_c8;
      n = std::max(n, slot + 1); p[slot].has_values = true; if (nullable) p[slot].has_validity = 1;
    },
    [&](int kind, int wide, bool lut_in_lds, int slot, bool nullable) {
      fdb::JitLeaf L;
      L.kind = kind; L.slot = slot; L.wide = wide; L.lut_in_lds = lut_in_lds; if (wide) L.op = 5;
      fdb::JitSlot* p = wide ? s.c8 : s.c4;
      int& n = wide ? s.n_c8 : s.n_c4;
      n = std::max(n, slot + 1); p[slot].has_values = true; if (nullable) p[slot].has_validity = 1;
      s.leaves.push_back(L);
      return (int)s.leaves.size() - 1;
    });
}

// `agg=<func><type>:<expression>` (func sum / min / max, type i / u / f): {func, type} and the expression
static fdb::JitAgg computed_agg(const std::string& a, std::string* spec) {
  const size_t c = a.find(':');
  if (c != 4 || (a.substr(0, 3) != "sum" && a.substr(0, 3) != "min" && a.substr(0, 3) != "max")) { std::fprintf(stderr, "jit_dump: agg=<sum|min|max><i|u|f>:<expression>\n"); std::exit(2); }
  *spec = a.substr(c + 1);
  return {a[0] == 's' ? FDB_AGG_SUM : a[1] == 'i' ? FDB_AGG_MIN : FDB_AGG_MAX, a[3] == 'i' ? FDB_T_I64 : a[3] == 'u' ? FDB_T_U64 : FDB_T_F64, -1, 0};
}
// … in the place of the shape's first SUM
static void replace_sum(std::vector<fdb::JitAgg>& aggs, fdb::JitAgg a, int root) {
  a.expr = root + 1;
  for (fdb::JitAgg& x : aggs) if (x.func == FDB_AGG_SUM) { x = a; return; }
  aggs.push_back(a);
}

int main(int argc0, char** argv0) {
  // keyword arguments, anywhere on the line: agg=<func><type>:<expression> (a computed aggregate input in the place of the shape's first SUM),
  // key=<expression> (hash modes: the last key column computed), nopred (flags / select: no predicate), fuse4 (select: the 4-byte slot fused too),
  // nonull (plan: the dictionary slots without bitmaps), ptab (plan: per-record fields from the packed part table, read from global memory; JitShape::part_table),
  // cfg3 (plan two: bench.py's cfg 3 — three filter columns, `code` and `method` through truth tables, `instance` IS NOT NULL from its bitmap alone)
  std::string agg_arg, key_arg;
  bool nopred = false, fuse4 = false, nonull = false, ptab = false, cfg3 = false;
  std::vector<char*> pos;
  for (int i = 0; i < argc0; i++) {
    const std::string a = argv0[i];
    if (i > 0 && a.rfind("agg=", 0) == 0) agg_arg = a.substr(4);
    else if (i > 0 && a.rfind("key=", 0) == 0) key_arg = a.substr(4);
    else if (i > 0 && a == "nopred") nopred = true;
    else if (i > 0 && a == "fuse4") fuse4 = true;
    else if (i > 0 && a == "nonull") nonull = true;
    else if (i > 0 && a == "ptab") ptab = true;
    else if (i > 0 && a == "cfg3") cfg3 = true;
    else pos.push_back(argv0[i]);
  }
  const int argc = (int)pos.size();
  char** argv = pos.data();
  if (argc > 1 && (std::string(argv[1]) == "flags" || std::string(argv[1]) == "select")) {
    const bool select = std::string(argv[1]) == "select";
    // the selection-bitmap kernel of filter(): `value > T AND labels.code == <one of a few>` (an 8-byte compare + a dictionary truth table)
    fdb::JitShape s;
    s.block = 512; s.two_phase = true; s.lds_acc = false;
    s.n_c8 = 1; s.c8[0].has_values = true; s.c8[0].has_validity = 0;
    s.n_c4 = 1; s.c4[0].has_values = true; s.c4[0].has_validity = 2;
    fdb::JitLeaf a; a.kind = FDB_LEAF_CMP_F64; a.slot = 0; a.wide = 1; a.op = 5;
    fdb::JitLeaf b; b.kind = FDB_LEAF_DICT_BITS; b.slot = 0; b.wide = 0;
    fdb::JitLeaf c; c.kind = FDB_LEAF_DICT_LUT; c.slot = 0; c.wide = 0; c.lut_in_lds = true;
    s.leaves = {a, b, c};
    s.code = {0, 1, FDB_CODE_AND, 2, FDB_CODE_OR};
    if (argc > 2) { s.n_c4 = 0; s.leaves = {a}; s.code = {0}; }  // `value > T` alone (bench.py's select line)
    if (nopred) { s.leaves.clear(); s.code.clear(); }  // every row selected: the slots are still loaded
    if (select) { s.fuse8 = 1; if (argc > 3 || fuse4) s.fuse4 = 1; }  // the one-pass kernel: `value` (and the dictionary column) compacted by the predicate's own wave
    std::fputs((select ? fdb::jit_select_source(s) : fdb::jit_flags_source(s)).c_str(), stdout);
    return 0;
  }
  if (argc > 2 && std::string(argv[1]) == "project") {
    // the Projection kernel (fdb_project_kernel) of one or more expressions (parse_exprs), e.g.
    //   project 'ci0,ci1,*'    project 'ci0n,ci1n,/,ci2,+;ci0n,cv,cf3,*'    project 'db0n,ci0,li,q5,and'
    fdb::JitShape s;
    s.block = 256; s.two_phase = true; s.lds_acc = false;
    s.proj_roots = parse_into(s, argv[2]);
    std::fputs(fdb::jit_project_source(s).c_str(), stdout);
    return 0;
  }
  if (argc > 1 && std::string(argv[1]) == "plan") {
    // the dense scan kernel of a cfg 2-like shape (`labels.code == X` + SUM(float64) [+ MIN / COUNT] GROUP BY labels.path):
    //   plan [variant] [narrow [threads]]   narrow: the dictionary slots read from narrow-index caches (1-byte filter column, 2-byte group column),
    //                                       the quad shape of such a launch; threads: per workgroup (256 / 512 / 1024)
    //   plan [variant] packed [threads]     the same with the slots read from packed index caches: the filter column at 4 bits, the group column at 12
    //   plan [variant] narrow threads sum   the same with SUM(float64) as the only aggregate: the shape bench.py's headline runs
    //   plan … agg=sumf:ci0n,ci1n,/         the shape's SUM over a computed input
    //   plan [variant]   variant: lds (default) | wave (per-wave tables: fdb_plan_set_deterministic) | reg (≤ 8 slots in registers) | cache (table too big for LDS) | two (two-phase layout, 4 aggregates)
    const std::string v = argc > 2 ? argv[2] : "lds";
    fdb::JitShape s;
    s.block = v == "wave" ? 256 : 512;
    s.two_phase = v == "two";
    s.lds_acc = v != "cache"; s.cache = v == "cache"; s.need_count = v == "two";
    s.wave_tables = v == "wave";
    if (v == "reg") s.reg_slots = 6;
    fdb::JitLeaf a; a.kind = FDB_LEAF_DICT_BITS; a.slot = 0; a.wide = 0;
    s.leaves = {a};
    s.code = {0};
    if (s.two_phase) {
      s.n_c4 = 1; s.c4[0].has_values = true; s.c4[0].has_validity = 1;
      s.n_l4 = 1; s.l4[0].has_values = true; s.l4[0].has_validity = 2;
      s.n_l8 = 2; s.l8[0].has_values = true; s.l8[1].has_values = true;
      s.gcols.push_back({0, true});
      s.aggs = {{FDB_AGG_COUNT, FDB_T_I64, 1, 0}, {FDB_AGG_MIN, FDB_T_I64, 0, 0}, {FDB_AGG_MAX, FDB_T_I64, 0, 0}, {FDB_AGG_SUM, FDB_T_F64, 1, 0}};
    } else {
      s.n_c4 = 2; s.c4[0].has_values = true; s.c4[0].has_validity = 1; s.c4[1].has_values = true; s.c4[1].has_validity = 1;
      s.n_c8 = 1; s.c8[0].has_values = true;
      s.gcols.push_back({1, true});
      s.aggs = {{FDB_AGG_SUM, FDB_T_F64, 0, 0}, {FDB_AGG_MIN, FDB_T_F64, 0, 0}};
    }
    if (argc > 3 && std::string(argv[3]) == "narrow") {  // narrow-index caches: the filter column read at 1 byte, the group column at 2
      s.c4[0].form = fdb::kScanForm1;
      (s.two_phase ? s.l4[0] : s.c4[1]).form = fdb::kScanForm2;
      s.quad = true;  // (what jit_shape sets for a launch with a narrow slot)
    }
    if (argc > 3 && std::string(argv[3]) == "packed") {  // packed index caches in the place of `narrow`: the filter column at 4 bits (form H), the group column at 12 (form T)
      s.c4[0].form = fdb::kScanFormH;
      (s.two_phase ? s.l4[0] : s.c4[1]).form = fdb::kScanFormT;
      s.quad = true;
    }
    if (cfg3 && s.two_phase) {  // plan two [narrow …] cfg3: two more early slots and leaves, AND-ed
      s.n_c4 = 3;
      s.c4[1].has_values = true; s.c4[1].has_validity = 1; s.c4[1].form = s.c4[0].form;
      s.c4[2].has_values = false; s.c4[2].has_validity = 1;
      fdb::JitLeaf b; b.kind = FDB_LEAF_DICT_BITS; b.slot = 1; b.wide = 0;
      fdb::JitLeaf c; c.kind = FDB_LEAF_VALIDITY; c.slot = 2; c.wide = 0;
      s.leaves = {a, b, c};
      s.code = {0, 1, FDB_CODE_AND, 2, FDB_CODE_AND};
    }
    if (argc > 4) s.block = std::atoi(argv[4]);  // plan <variant> narrow <threads per workgroup>
    if (argc > 5 && std::string(argv[5]) == "sum" && !s.two_phase) s.aggs.resize(1);  // plan <variant> narrow <threads> sum: SUM(float64) alone, bench.py's headline query
    if (nonull) {  // plan … nonull: no 4-byte slot has a bitmap — columns without NULLs, or null-folded caches (fdb_record.h), the headline's launch
      for (int i = 0; i < s.n_c4; i++) s.c4[i].has_validity = 0;
      for (int i = 0; i < s.n_l4; i++) s.l4[i].has_validity = 0;
    }
    if (!agg_arg.empty()) { std::string spec; const fdb::JitAgg A = computed_agg(agg_arg, &spec); replace_sum(s.aggs, A, parse_into(s, spec).at(0)); }
    s.part_table = ptab;
    std::fputs(fdb::jit_source(s).c_str(), stdout);
    return 0;
  }
  const int n = argc > 1 ? std::atoi(argv[1]) : 32;
  const int kinds = argc > 2 ? std::atoi(argv[2]) : 0;  // 1: make the last column an int64 key; 2: run kernel, narrow records; 3: run kernel, wide records; 4: wide + an int64 key; 5: run kernel, medium records
  // a third argument "exact": exact float64 SUMs (fdb_plan_set_exact_sums; kinds 0 / 1 only)
  fdb::JitHashShape s;
  for (int c = 0; c < n; c++) s.cols.push_back({(kinds == 1 || kinds == 4) && c == n - 1 ? 1 : 0, true, c < 8, -1});
  s.aggs.push_back({FDB_AGG_SUM, FDB_T_F64, -1, 0});
  s.agg_validity.push_back(false);
  if (kinds >= 2) s.runs = kinds == 2 ? 1 : kinds == 5 ? 3 : 2;  // the table-free OrderedAggregate's run kernel (one aggregation); 5: medium records (two bytes per key id)
  else { s.aggs.push_back({FDB_AGG_COUNT, FDB_T_I64, -1, 0}); s.agg_validity.push_back(false); }
  s.need_count = true;
  if (argc > 3 && std::string(argv[3]) == "exact") {
    s.exact = true;
    s.aggs.push_back({FDB_AGG_SUM, FDB_T_F64, -1, 0});  // a second exact SUM, with NULLs
    s.agg_validity.push_back(true);
  }
  // computed inputs and keys read the columns of base.l8 (x<slot>), a compared column is a leaf with a column of its own
  auto parse_hash = [&](const std::string& spec) {
    return parse_exprs(spec, s.exprs, [&](int slot, bool) { s.n_expr_cols = std::max(s.n_expr_cols, slot + 1); },
      [&](int kind, int wide, bool lut_in_lds, int, bool nullable) {
        fdb::JitLeaf L;
        L.kind = kind; L.slot = 0; L.wide = wide; L.lut_in_lds = lut_in_lds; if (wide) L.op = 5;
        s.leaves.push_back(L); s.leaf_validity.push_back(nullable);
        return (int)s.leaves.size() - 1;
      }).at(0);
  };
  if (!agg_arg.empty()) { std::string spec; const fdb::JitAgg A = computed_agg(agg_arg, &spec); replace_sum(s.aggs, A, parse_hash(spec)); }
  if (!key_arg.empty() && !s.cols.empty()) { const int root = parse_hash(key_arg); s.cols.back() = {2, false, false, root, false}; }
  std::fputs(fdb::jit_hash_source(s).c_str(), stdout);
  return 0;
}
