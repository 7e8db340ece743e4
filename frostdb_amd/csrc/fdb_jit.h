// fdb_jit.h — plan-specialised scan kernels (fdb_jitgen.cpp writes their source, fdb_jit.cpp compiles, caches and launches them).
#pragma once
#include <cstdlib>

#include <hip/hip_runtime_api.h>

#include <cstdint>
#include <string>
#include <vector>

#include "fdb_kernels.h"
#include "fdb_record.h"

namespace fdb {

// has_validity: 0 no record has a bitmap, 1 every record, 2 some (checked per record). form (4-byte slots of fdb_plan_kernel only): what
// sits behind `values` — 4: the uint32 column, else a form of the records' narrow-index caches (fdb_record.h, ScanForm; FdbScanArgs.w4 /
// wl4), unpacked after the load
struct JitSlot { bool has_values = false; int has_validity = 0; ScanForm form = kScanForm4; };
struct JitLeaf { int kind = 0, slot = -1, wide = 0, op = 0; bool lut_in_lds = false; };
struct JitGroup { int slot = -1; bool lut_in_lds = false; };
struct JitAgg { int func = 0, type = 0, slot = -1; int expr = 0; };  // expr: 1 + root node of a computed input, 0 = stored column
struct JitExprNode { int kind = 0, op = 0, left = -1, right = -1, slot = -1, type = 0; };  // literal values stay run-time arguments

// Everything that changes the generated CODE. Pointers, literals, truth-table bits, LUT offsets, strides and row counts
// are run-time arguments and deliberately absent, so that queries of the same shape share one compiled kernel.
struct JitShape {
  int block = 512;
  bool lds_acc = true, need_count = false, two_phase = false;
  int n_c4 = 0, n_c8 = 0, n_l4 = 0, n_l8 = 0;
  JitSlot c4[FDB_ARG_C4], c8[FDB_ARG_C8], l4[FDB_ARG_L4], l8[FDB_ARG_L8];
  std::vector<JitLeaf> leaves;
  std::vector<uint8_t> code;  // postfix program over the leaves
  std::vector<JitGroup> gcols;
  std::vector<JitAgg> aggs;
  std::vector<JitExprNode> exprs;  // pre-aggregate arithmetic (FdbScanArgs.expr)
  // Tiny tables (no group-by, or a handful of slots): every lane keeps the WHOLE table in registers across all its tiles and
  // the table is reduced across the wave once, at the end — per-row LDS atomics on ≤ 8 addresses serialise almost completely
  // (`sum(value)` without group-by ran at 0.7 TB/s with them). 0 = off, else the exact slot count the kernel is built for.
  int reg_slots = 0;
  // Tables too big for LDS (lds_acc = false): a per-workgroup combining cache in LDS (direct-mapped by a hash of the slot, first
  // come first served, no eviction) absorbs the rows of the keys it holds and is flushed with one global atomic per entry and
  // aggregate at the end; rows of other keys update the global table directly. Hot keys — which serialise on their cache
  // line in L2 when every row is a global atomic (sum by (path, instance): 11 ms per 50 M rows) — are first to get a place.
  bool cache = false;
  // Reproducible float sums (fdb_plan_set_deterministic): every WAVE accumulates into an LDS table of its own — rows reach a table in
  // program order, lane order inside an instruction — and the flush adds the waves' tables up in wave order; with shared tables the
  // order in which the waves' LDS atomics interleave differs from run to run, and float64 addition is not associative.
  bool wave_tables = false;
  // LDS tables: when the slots of a wave's selected rows agree (sorted input) the updates go to a wave-uniform address, so that the compiler
  // folds them across the lanes (fdb_jitgen.cpp, "Sorted input")
  bool uniform_fold = true;  // ($FDB_NO_UNIFORM_FOLD, A/B aid: a plan reads it at create, Plan::Knobs)
  // fdb_plan_kernel, set when a slot of the launch is narrow (JitSlot::form != 4): the unit of work (FdbScanArgs tile_begin / tile_end,
  // total_tiles) is block × 16 rows instead of block × 4 — each wave takes one block of 1 024 rows as four sub-steps of 64 lanes × 4 rows
  // and reads the narrow slots of a full block with 16-byte loads, in the order the records' caches keep them (scan_cache_at).
  bool quad = false;
  // fdb_plan_kernel: the per-record fields come from a packed table (jit_part_fields: W words per record), not from the array of 3 KB
  // FdbScanArgs — a record switch reads W adjacent words, and the host ships those words only. The kernel takes
  // `const unsigned long long* ptab` in the place of `parts` (jit_launch_ptab). Set by the launch (fdb_dense.cpp).
  bool part_table = false;
  // fdb_select_kernel only (not part of key()): early slots whose values the kernel compacts itself, bit i = slot i of c4 / c8
  int fuse4 = 0, fuse8 = 0;
  // fdb_project_kernel only (not part of key()): root node of every computed field, in output order
  std::vector<int> proj_roots;
  std::string key(bool with_validity = true) const;
  int row_bytes() const {  // bytes of column data a scan of this shape reads per row (slots with values, 4-byte slots at their form), rounded up once
    int bits = 0;
    for (int k = 0; k < n_c4; k++) bits += c4[k].has_values ? scan_form_bits(c4[k].form) : 0;
    for (int k = 0; k < n_l4; k++) bits += l4[k].has_values ? scan_form_bits(l4[k].form) : 0;
    for (int k = 0; k < n_c8; k++) bits += c8[k].has_values ? 64 : 0;
    for (int k = 0; k < n_l8; k++) bits += l8[k].has_values ? 64 : 0;
    return (bits + 7) / 8;
  }
};

// Shape of a high-cardinality (hash table) scan: fdb_hash_kernel.
struct JitHashCol { int kind = 0; bool has_validity = false, lut_in_lds = false; int expr_root = -1; bool lut_identity = false; };  // kind 2: computed int64 key; lut_identity: key id = dictionary index + 1 (FdbHashCol.lut == nullptr)
struct JitHashShape {
  std::vector<JitHashCol> cols;
  std::vector<JitLeaf> leaves;  // slot / wide describe the leaf's own column (wide = 8-byte values)
  std::vector<bool> leaf_validity;
  std::vector<uint8_t> code;
  std::vector<JitAgg> aggs;
  std::vector<bool> agg_validity;
  std::vector<JitExprNode> exprs;  // column nodes read base.l8[slot]
  int n_expr_cols = 0;
  bool need_count = true;  // some aggregation is COUNT: otherwise the per-entry row count is never read (occupancy = fingerprint ≠ 0) and its atomic is skipped
  // Table-free OrderedAggregate (FdbHashArgs.runs): no probe, no insert — every wave emits the runs of equal keys among its 256 rows
  // (key ids, row count, folded aggregate) and notes them in the launch's directory. Exactly one aggregation. 1: narrow records —
  // dictionary columns with ≤ 255 values, at most FDB_RUN_TUPLE_BYTES of them, ids packed one byte each while the fingerprint is
  // computed; 2: wide records — the table's own key tuple (any cardinality, int64 / computed keys, absent columns), written by the lanes
  // that end a run from re-loaded columns.
  int runs = 0;
  // Exact float64 SUMs (fdb_plan_set_exact_sums; FdbAgg.acc of such an aggregation = its limb rows): no folding of rows before the
  // table (a float add would round), each row's value goes into the limbs through fdb_exact_add_wave after the tile's probes.
  bool exact = false;
  std::string key() const;
};
// `hcols` = host copy of args.hcols.
JitHashShape jit_hash_shape(const FdbHashArgs& args, const FdbHashCol* hcols);
std::string jit_hash_source(const JitHashShape& shape);
hipFunction_t jit_hash_get(const JitHashShape& shape);
// 256-thread workgroups, 1 024-row tiles.
hipError_t jit_hash_launch(hipFunction_t fn, const FdbHashArgs& args, int grid, size_t lds_bytes, hipStream_t stream);

// The shape of one record's slot-assigned argument block.
JitShape jit_shape(const FdbScanArgs& a, bool two_phase, int block);
// Folds `other` into `into` when the two differ at most in which slots carry validity bitmaps; false otherwise.
bool jit_shape_merge(JitShape* into, const JitShape& other);
// The same for the shape of argument block `b`, decided on the blocks themselves (`a`: the block `into` was made from): no JitShape, no key strings.
bool jit_shape_merge_args(JitShape* into, const FdbScanArgs& a, const FdbScanArgs& b, bool two_phase);
// Workgroups of `block` threads with `lds_bytes` of dynamic LDS that fit one CU (≥ 1).
int jit_blocks_per_cu(hipFunction_t fn, int block, size_t lds_bytes);

// Kernels compiled with hiprtc by this process, the time that took, and code objects loaded from the disk cache instead.
void jit_stats(int64_t* n_compiled, double* compile_ms, int64_t* n_disk_loads);

// filter() (Plan::filter_batches): the selection-bitmap kernel of a predicate shape — 256-thread workgroups, one wave per tile of
// 2 048 rows (FDB_COMPACT_TILE): 64 mask words and one count per tile, plain stores. The argument blocks count tile_begin /
// tile_end in units of FOUR tiles (a workgroup's share, all of one record) and carry the record's first tile in out_tile_base.
std::string jit_flags_source(const JitShape& shape);
hipFunction_t jit_flags_get(const JitShape& shape);
hipError_t jit_flags_launch(hipFunction_t fn, const FdbScanArgs* d_parts, int n_parts, int64_t total_super_tiles, const FdbScanArgs& common, int grid, size_t lds_bytes,
                            uint32_t* masks, uint32_t* tile_counts, hipStream_t stream);

// filter() in one pass over the filter columns (fdb_kernels.h, FdbSelectArgs): fdb_flags_kernel's geometry and bitmap, plus the tile
// offsets (decoupled look-back inside each record, tiles handed out by a ticket counter) and the compacted values of the fused slots
// (shape.fuse4 / fuse8), staged in LDS — jit_select_stage_bytes(shape) per wave (jit_select_block() / 64 of them) behind `stage_off`.
std::string jit_select_source(const JitShape& shape);
hipFunction_t jit_select_kernel_get(const JitShape& shape);
size_t jit_select_stage_bytes(const JitShape& shape);
int jit_select_block();  // threads per workgroup (8 waves, half a tile each)
hipError_t jit_select_launch(hipFunction_t fn, const FdbScanArgs* d_parts, int n_parts, int64_t total_super_tiles, const FdbScanArgs& common, int grid, size_t lds_bytes,
                             uint32_t* masks, uint32_t* offsets, const FdbSelectArgs& sel, hipStream_t stream);

// Projection (Plan::project_batches; fdb_kernels.h, FdbProjectPart): every computed field of a call in one launch — 256-thread workgroups,
// tiles of FDB_PROJECT_TILE rows counted by tile_begin / tile_end of the argument blocks, a lane owns 4 consecutive rows. shape: jit_shape of a
// record's argument block in the two-phase layout (expression columns in l8, leaves of string comparisons in c4 / c8) + proj_roots.
std::string jit_project_source(const JitShape& shape);
hipFunction_t jit_project_get(const JitShape& shape);
hipError_t jit_project_launch(hipFunction_t fn, const FdbScanArgs* d_parts, int n_parts, int64_t total_tiles, int grid, size_t lds_bytes, const FdbProjectPart* d_outs,
                              unsigned long long* d_nulls, hipStream_t stream);

std::string jit_source(const JitShape& shape);

// The packed part table (JitShape::part_table). A shape's kernel reads a handful of values per record; jit_part_fields lists them, in
// the order the record-entry emitter takes them, and BOTH the emitted reads and the host's packer walk that one list, so that field order
// and words per record cannot drift apart. A 64-bit field owns a word; 32-bit fields share words in pairs, low half first, in list order.
struct PartField {
  enum What { TILE_END, TILE_BEGIN, N_ROWS, SLOT_VALUES, SLOT_VALIDITY, LEAF_LIT, LEAF_LUT, LEAF_LEN, LEAF_LDS, LEAF_OP, G_LUT, G_LDS, G_STRIDE, G_LEN, EXPR_LIT, LUT_CLASS };
  What what;
  int pool;    // SLOT_*: 0 c4, 1 c8, 2 l4, 3 l8
  int index;   // slot, leaf, group column or expression node
  int bits;    // 64 or 32
  int word;    // where it sits in the record's W words …
  int shift;   // … 0 or 32
};
std::vector<PartField> jit_part_fields(const JitShape& shape);
int jit_part_words(const JitShape& shape);  // W
int jit_part_words(const std::vector<PartField>& fields);
const char* jit_part_field_name(PartField::What what);
// `out`: n × W words, record k's at out + k × W; tile ranges and everything else as the argument blocks hold them at the call.
void jit_pack_parts(const JitShape& shape, const FdbScanArgs* const* args, size_t n, unsigned long long* out);
// … with the shape's list and W at hand (a launch makes the list once)
void jit_pack_parts(const std::vector<PartField>& fields, int W, const FdbScanArgs* const* args, size_t n, unsigned long long* out);
// The compiled kernel for `shape` (cached in the process and on disk), or nullptr if specialisation is unavailable.
// While one of these with may_defer = true is alive on a thread, a jit_*get of a kernel that is not built yet may return nullptr at once
// and leave the build to a background thread ($FDB_JIT_ASYNC=1 only): set by callers whose launch the interpreting kernels can serve.
class JitDeferScope {
 public:
  explicit JitDeferScope(bool may_defer);
  ~JitDeferScope();
  JitDeferScope(const JitDeferScope&) = delete;
  JitDeferScope& operator=(const JitDeferScope&) = delete;
 private:
  bool prev_;
};
hipFunction_t jit_get(const JitShape& shape);
// jit_get plus the launch geometry: workgroup size and workgroups per CU such that ≈64 KB of loads are in flight per CU
// (`row_bytes` = bytes of column data the scan reads per row; `sorted_input`: the plan is an OrderedAggregate, its input sorted by the
// group columns).
hipFunction_t jit_select(JitShape shape, size_t lds_bytes, int row_bytes, bool sorted_input, int* block_out, int* blocks_per_cu_out);
hipError_t jit_launch(hipFunction_t fn, const FdbScanArgs* d_parts, int n_parts, int64_t total_tiles, const FdbScanArgs& common, int grid, int block,
                      size_t lds_bytes, hipStream_t stream);
// A part_table kernel: `d_ptab` = the packed table (n_parts × W words, jit_pack_parts).
hipError_t jit_launch_ptab(hipFunction_t fn, const unsigned long long* d_ptab, int n_parts, int64_t total_tiles, const FdbScanArgs& common, int grid, int block,
                           size_t lds_bytes, hipStream_t stream);

}  // namespace fdb
