/* frostdb_amd.h — C ABI of the MI355X-native TableScan → PredicateFilter → HashAggregate path.
 *
 * This is the thin cgo surface a FrostDB maintainer binds (see INTEGRATION.md for the Go stub).
 * The reference has no FFI today; the seam is the Go push-operator interface
 *
 *     type PhysicalPlan interface {                     // query/physicalplan/physicalplan.go:24-30
 *         Callback(ctx, arrow.Record) error             //   → fdb_plan_push / fdb_plan_push_batch
 *         Finish(ctx) error                             //   → fdb_plan_finish
 *         SetNext(PhysicalPlan)                         //   (stays in Go: the shim forwards the finish record)
 *         Draw() *Diagram                               //   → fdb_plan_draw
 *         Close()                                       //   → fdb_plan_close
 *     }
 *
 * One fdb_plan replaces one operator chain  PredicateFilter → HashAggregate(final=false)
 * (physicalplan.go:417-474). Plain pointers and sizes only; record batches cross the boundary as
 * Arrow C Data Interface structs (arrow-go: arrow/cdata; pyarrow: _export_to_c).
 *
 * Every function returns FDB_OK (0) or an fdb_status error code and never aborts the process;
 * the text of the last error is available per handle (fdb_plan_last_error) or per thread
 * (fdb_last_error) — the Go shim turns rc != 0 into `errors.New(text)`.
 */
#ifndef FROSTDB_AMD_H
#define FROSTDB_AMD_H

#include <stdint.h>
#include "arrow_c_data.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The library is built with -fvisibility=hidden: the prototypes marked FDB_API are its whole dynamic symbol surface
 * (tests/test_capi_cpu.py compares `nm -D --defined-only` with this header), so a cgo binary that links other C++ sees none of
 * the library's internals. */
#if defined(__GNUC__) || defined(__clang__)
#define FDB_API __attribute__((visibility("default")))
#else
#define FDB_API
#endif

typedef enum fdb_status {
  FDB_OK = 0,
  FDB_ERR_INVALID = 1,      /* malformed descriptor / arguments */
  FDB_ERR_UNSUPPORTED = 2,  /* ≙ ErrUnsupportedBooleanExpression (filter.go:46), ErrUnsupportedBinaryOperation
                               (binaryscalarexpr.go:82), ErrUnsupportedSumType/MinType/MaxType (aggregate.go:736,782,862) */
  FDB_ERR_NOT_FOUND = 3,    /* ≙ "aggregate field(s) not found" (aggregate.go:367-380) */
  FDB_ERR_DEVICE = 4,       /* HIP runtime error (text carries hipGetErrorString) */
  FDB_ERR_OOM = 5,          /* host or device allocation failed */
  FDB_ERR_STATE = 6         /* call order violated (push after finish, …) */
} fdb_status;

/* logicalplan.Op (query/logicalplan/expr.go:17-35) — same numeric values as the reference's iota
 * and as storage.proto's Op enum, so a Go shim can pass `int32(expr.Op)` through unchanged. */
typedef enum fdb_op {
  FDB_OP_UNKNOWN = 0,
  FDB_OP_EQ = 1,
  FDB_OP_NOT_EQ = 2,
  FDB_OP_LT = 3,
  FDB_OP_LT_EQ = 4,
  FDB_OP_GT = 5,
  FDB_OP_GT_EQ = 6,
  FDB_OP_REGEX_MATCH = 7,
  FDB_OP_REGEX_NOT_MATCH = 8,
  FDB_OP_AND = 9,
  FDB_OP_OR = 10,
  FDB_OP_ADD = 11,
  FDB_OP_SUB = 12,
  FDB_OP_MUL = 13,
  FDB_OP_DIV = 14,
  FDB_OP_CONTAINS = 15,
  FDB_OP_NOT_CONTAINS = 16
} fdb_op;

/* logicalplan.AggFunc (query/logicalplan/expr.go:718-729), same numeric values. */
typedef enum fdb_agg_func {
  FDB_AGG_UNKNOWN = 0,
  FDB_AGG_SUM = 1,
  FDB_AGG_MIN = 2,
  FDB_AGG_MAX = 3,
  FDB_AGG_COUNT = 4,
  FDB_AGG_AVG = 5,    /* never reaches the operator: lowered to SUM+COUNT+Projection (logicalplan/builder.go:205-238) */
  FDB_AGG_UNIQUE = 6, /* int64 only: the group's value if all its rows carry the same non-NULL value, else NULL (aggregate.go:677-732) */
  FDB_AGG_AND = 7     /* bool only: AND over the valid values, true if there is none (aggregate.go:635-675) */
} fdb_agg_func;

/* scalar.Scalar of a LiteralExpr (the right-hand side of a filter leaf, filter.go:95-103). */
typedef enum fdb_literal_type {
  FDB_LIT_NULL = 0,   /* scalar.ScalarNull: `col = null` ≙ IS NULL, `col != null` ≙ IS NOT NULL */
  FDB_LIT_INT64 = 1,
  FDB_LIT_UINT64 = 2,
  FDB_LIT_FLOAT64 = 3,
  FDB_LIT_STRING = 4, /* scalar.String */
  FDB_LIT_BINARY = 5, /* scalar.Binary */
  FDB_LIT_BOOL = 6
} fdb_literal_type;

typedef struct fdb_literal {
  int32_t type;      /* fdb_literal_type */
  int32_t _pad;
  int64_t i64;       /* INT64, BOOL (0/1) */
  uint64_t u64;      /* UINT64 */
  double f64;        /* FLOAT64 */
  const char* data;  /* STRING / BINARY bytes (not NUL-terminated) */
  int64_t len;
} fdb_literal;

/* One node of the filter expression tree, flattened into an array.
 *   leaf:    op ∈ {EQ … GT_EQ, REGEX_*, CONTAINS, NOT_CONTAINS}, `column` ⟨op⟩ `literal`
 *            (left must be a column, right a literal: filter.go:79-103)
 *   branch:  op ∈ {AND, OR}, `left`/`right` are indices into the same array (filter.go:129-160) */
typedef struct fdb_expr {
  int32_t op;          /* fdb_op */
  int32_t left;        /* child index for AND/OR, else -1 */
  int32_t right;       /* child index for AND/OR, else -1 */
  int32_t _pad;
  const char* column;  /* NUL-terminated exact column name (ArrayRef.ColumnName, binaryscalarexpr.go:18-29) */
  fdb_literal literal;
} fdb_expr;

/* One AggregationFunction (aggregate.go:104-110): `func(column)`; the output column is named
 * "<func>(<column>)" exactly like AggregationFunction.Name() (logicalplan/expr.go:700-702). */
typedef struct fdb_aggregation {
  int32_t func;        /* fdb_agg_func */
  int32_t dynamic;     /* 1 ⇔ the aggregated expression is a DynamicColumn: `column` is the set's name and `max(foo)` means max over
                          every `foo.*` column (Aggregate() marks these, aggregate.go:38-46; HashAggregate turns each matching field
                          into a concrete aggregation when a record first carries it, :306-336). The result column is named after
                          the FIELD by a partial-stage plan and `max(foo.bar)` by a final-stage one; a record without a field adds
                          nothing to it; a record with no field of the set is FDB_ERR_NOT_FOUND. sum / min / max / count only.
                          Such a plan is a family of ordinary plans (one more scan per concrete column): fdb_plan_merge works, the
                          single-table entry points (state arrays, hash exchange) return FDB_ERR_UNSUPPORTED. 0 otherwise. */
  const char* column;
} fdb_aggregation;

/* One group-by matcher (aggregate.go:286-289): Column ≙ exact name (logicalplan/expr.go:353-355),
 * DynamicColumn ≙ every column whose name starts with name+"." (expr.go:564-566). */
typedef struct fdb_group_expr {
  const char* name;
  int32_t dynamic;
  int32_t _pad;
} fdb_group_expr;

/* ---- pre-aggregate Projection (physicalplan/project.go:58-395) --------------------------------------
 * `Projection (value * timestamp, stacktrace) - HashAggregate (sum(value * timestamp) by stacktrace)` and
 * `Projection (value, timestamp / 1000 * 1000 as timestamp_bucket) - HashAggregate (sum(value) by timestamp_bucket)`
 * (logictest/testdata/plan/aggregate/aggregate:66-69, plan/aggregate/window) are fused into the scan: a projection gives a
 * NAME to an arithmetic expression over int64 / float64 columns and literals; an aggregation whose `column`, or a plain
 * (non-dynamic) group matcher whose `name`, equals that name reads the computed value instead of a stored column.
 * Semantics of binaryExprProjection (project.go:73-161 and the Add/Sub/Mul/Div loops :163-399): both operands have the same
 * type (int64 or float64; a literal is a constant array of its own type); + - * use the RAW slot values of their operands
 * and always produce a valid value; / yields NULL where the divisor is 0, else Go's quotient (integers truncate toward
 * zero, MinInt64 / -1 wraps). Only the outermost operation's validity survives: a NULL produced by an inner division is
 * read back as its raw slot (0) by the enclosing + - *. */
typedef struct fdb_proj_node {
  int32_t kind;        /* 0 column, 1 literal, 2 binary arithmetic, 3 comparison → bool (boolExprProjection, project.go:401-470:
                          `distinct(labels.label1, value > 0)`; a NULL operand compares false; usable as a group / distinct key),
                          4 convert(left, float64): int64 → float64 of the RAW slot, always valid (convertProjection, project.go:493-556),
                          5 isnull(left) → bool, always valid; `left` must be a column node (isNullProjection, :558-601),
                          6 if(cond) { left } else { right }: int64 branches; cond (node index in `op`) is a comparison / isnull
                            node; a row takes `left`'s raw slot where cond is true, else `right`'s; always valid
                            (ifExprProjection + conditionalAddInt64, :603-702) */
  int32_t op;          /* binary: FDB_OP_ADD / SUB / MUL / DIV; comparison: FDB_OP_EQ … FDB_OP_GT_EQ over numeric children — or over a
                          COLUMN node and a LITERAL node of any filter literal type (string, binary, NULL …): that comparison is evaluated
                          the way a filter leaf is (boolExprProjection runs BooleanExpression.Eval, project.go:409-447 → BinaryScalarExpr,
                          binaryscalarexpr.go:41-152: dictionary / plain string columns, the missing-column rules) —,
                          or FDB_OP_AND / FDB_OP_OR over two comparison nodes (AndExpr / OrExpr, filter.go:172-220) */
  int32_t left;        /* binary: child indices into the projection's node array */
  int32_t right;
  const char* column;  /* column: exact name (ArrayRef.ColumnName) */
  fdb_literal literal; /* literal: INT64, FLOAT64 or UINT64 (arithmetic: both operands of one type, project.go:104-160 — int64, float64 or uint64; uint64 quotients are unsigned, a zero divisor gives NULL); any filter literal on the right of a column comparison */
} fdb_proj_node;

typedef struct fdb_projection {
  const char* name;    /* BinaryExpr.Name() = "value * timestamp" (logicalplan/expr.go:181-183) or the alias (AliasExpr.Name, :1029-1031) */
  const fdb_proj_node* nodes;
  int32_t n_nodes;
  int32_t root;
} fdb_projection;

/* Optional regular-expression engine of the HOST application. The reference compiles `=~` / `!~` literals with Go's regexp
 * (RE2 syntax, filter.go:105-124) and matches unanchored (regexpfilter.go:84-166). The library evaluates a regex leaf once per
 * DISTINCT value (dictionary entry) on the host — never per row, never on the device — so handing that evaluation back to the
 * caller costs one call per distinct value and makes the result identical to the reference's by construction: the Go shim passes
 * a cgo-exported function around regexp.Regexp.Match. Returns 1 = matches, 0 = does not, < 0 = the pattern
 * does not compile / internal error (the call that triggered it fails with FDB_ERR_INVALID). Without one (NULL) the library
 * uses its own RE2-syntax engine (fdb_regex_match below): flags, named groups, POSIX classes, \Q…\E, \A \z \b, Unicode general
 * categories (\pL \p{Lu} \P{Nd} \p{^Zs} \p{Any}) and case folding by orbits under (?i); Unicode SCRIPT classes (\p{Greek}) are not
 * covered and rejected at fdb_plan_create. Must be callable from any thread that calls into the plan. */
typedef int32_t (*fdb_regex_match_fn)(void* user, const char* pattern, int64_t pattern_len, const uint8_t* value, int64_t value_len);

typedef struct fdb_plan_desc {
  const fdb_expr* filter;      /* NULL / n_filter == 0 ⇒ no PredicateFilter in the chain */
  int32_t n_filter;
  int32_t filter_root;         /* index of the root node */
  const fdb_aggregation* aggs; /* n_aggs == 0: with n_groups > 0 the chain is Filter → Distinction (distinct.go:21-170; push/finish emit
                                  the distinct key tuples), with n_groups == 0 a filter-only plan (only fdb_plan_filter / _select) */
  int32_t n_aggs;
  int32_t n_groups;
  const fdb_group_expr* groups;
  int32_t final_stage;         /* 1 ⇒ behave like HashAggregate(finalStage=true): aggregate columns are matched
                                  by result name and COUNT merges by SUM (aggregate.go:340-348, :965-969) */
  int32_t n_projections;       /* computed columns of the Projection between filter and aggregate (0 ⇒ none) */
  const fdb_projection* projections;
  fdb_regex_match_fn regex_match;  /* NULL ⇒ std::regex */
  void* regex_user;                /* passed back as `user` */
  int32_t ordered;                 /* 1 ⇒ the chain's aggregate is an OrderedAggregate (ordered_aggregate.go; planned by
                                      physicalplan.go:433-449 when the scan is ordered by the group columns): exactly ONE aggregation;
                                      the result record is emitted SORTED by the group columns (first-seen column order, bytewise /
                                      numeric ascending, NULLs last — the order of the reference's merge of its ordered sets,
                                      ordered_aggregate.go:449-470, arrowutils/merge.go:84-112); a partial-stage plan names its result
                                      column after the aggregated COLUMN, a final-stage one after the aggregation (:551-557). The
                                      groups and their values are those of the hash aggregate: the reference's ordered sets merge by
                                      key. Input need NOT arrive ordered for the result to be right: records out of key order (several
                                      ordered sets, none at all) cost a sort of the collected runs on the device at Finish. */
  int32_t _pad2;
} fdb_plan_desc;

typedef struct fdb_plan fdb_plan;   /* one operator chain; push is single-threaded per handle (table.go:783-860) */
typedef struct fdb_batch fdb_batch; /* an Arrow record resident in HBM (a cached part / row group) */

/* ---- library ---------------------------------------------------------------------------------- */
FDB_API const char* fdb_version(void);
/* Text of the last error raised on the calling thread by a call that had no plan handle. */
FDB_API const char* fdb_last_error(void);
FDB_API int fdb_device_count(int* n_devices);
/* Measurement aid ("the measured ceiling of a plain read kernel on the same box in the same run"): streams
 * `bytes` of HBM through a load-only kernel `reps` times (hipEvent-timed, one launch each) and returns the best rate. */
FDB_API int fdb_read_ceiling(int device, int64_t bytes, int32_t reps, double* gb_per_s);

/* Host-only self-check of the Arrow C data code every entry point below relies on — what fdb_plan_push reads (column views
 * at any offset, dictionaries with any index width, plain string / binary columns encoded to distinct values + one id per row)
 * and what fdb_plan_finish / fdb_plan_filter write (dictionary, plain string, bool and fixed-width columns): `batch` comes back
 * in `out` with every column's type, values and NULLs unchanged, except that dictionary indices are uint32 and dictionaries with
 * large value types are narrowed. No device is touched, so it runs where there is no GPU. */
FDB_API int fdb_arrow_roundtrip(struct ArrowArray* batch, struct ArrowSchema* schema, struct ArrowArray* out, struct ArrowSchema* out_schema);
/* The library's built-in regular-expression engine (used for `=~` / `!~` when fdb_plan_desc.regex_match is NULL), exposed for
 * host-only checks: RE2 syntax — what Go's regexp compiles (filter.go:105-124) — matched unanchored on the value's bytes like
 * regexp.Regexp.Match (regexpfilter.go:84-166); linear-time (Thompson / Pike), no backreferences or look-around. *matched = 1 / 0;
 * FDB_ERR_INVALID with Go-style wording ("error parsing regexp: …") when the pattern does not compile. Not covered: Unicode script
 * classes (\p{Greek}); the category and case-folding tables are Unicode 13.0 (Go 1.22: 15.0). */
FDB_API int fdb_regex_match(const char* pattern, int64_t pattern_len, const uint8_t* value, int64_t value_len, int32_t* matched);
/* Host-only self-check of the widening step of a big Finish (dictionary indices cross PCIe at the narrowest width their dictionary
 * allows — `width` 1, 2 or 4 BYTES, or -2 / -4: that many BITS per index, rows packed low bits first — and are widened to Arrow's
 * uint32 by host threads): dst[i] = src[i] for i < n, through the same routine (AVX2 / AVX-512 with streaming stores where the CPU has
 * them). `width` -12 / -14: the 2- / 4-bit road THROUGH a rank → index table (what a Finish that ships the ids present uses), with the
 * table t[r] = 3 r + 5: dst[i] = 3 src[i] + 5. No device is touched. */
FDB_API int fdb_selftest_widen(const void* src, int32_t width, uint32_t* dst, int64_t n);
/* Self-check of the narrow-index cache's builder (the buffers a dense generated scan reads instead of a record's uint32 dictionary
 * indices; their bytes are a private, wave-interleaved layout): runs the builder on `device` over `rows` uint32 `indices` at `width` 1 or 2
 * bytes and copies the buffer's first `out_bytes` = rows x width rounded up to 16 bytes to `out` — the indices in the cache's order and
 * zeros behind the last row. FDB_ERR_INVALID also when a row is not where the library's own position formula puts it. */
FDB_API int fdb_selftest_scan_cache(const uint32_t* indices, int64_t rows, int32_t width, int device, uint8_t* out, int64_t out_bytes);
/* … of its null-folded form, which a column with NULLs gets when its dictionary of `entries` entries leaves room for one more index at
 * `width` (entries <= 255 at 1 byte, <= 65 535 at 2): `validity` is the column's Arrow bitmap at bit offset 0, (rows + 7) / 8 bytes, and
 * the buffer holds `entries` under every NULL row, whatever `indices` holds there. `out` as above; nothing is checked beyond the arguments. */
FDB_API int fdb_selftest_scan_cache_nulls(const uint32_t* indices, const uint8_t* validity, int64_t rows, int64_t entries, int32_t width, int device, uint8_t* out,
                                          int64_t out_bytes);
/* … of its packed forms (4 bits per index: form 5, 12 bits: form 6; frostdb_amd/csrc/fdb_record.h): builds the buffer of `rows` rows
 * for a dictionary of `entries` entries exactly as a dense scan's first launch would — null-folded (`entries` under every row whose bit
 * of `validity` is clear) when `validity` is given — and copies its whole frames, ceil(rows / 1024) x 512 or 1 536 bytes, to `out`. */
FDB_API int fdb_selftest_scan_cache_packed(const uint32_t* indices, const uint8_t* validity, int64_t rows, int64_t entries, int32_t form, int device, uint8_t* out,
                                           int64_t out_bytes);
/* Self-check of the device prefix sums: uploads `in`, runs ONE of the library's three launch sequences on `device` exactly as the
 * library runs it (scratch buffers at the sizes the launchers document) and copies the results out. Exclusive prefix sums of 32-bit
 * counts, modulo 2^32 in `out`, in full in `totals`. 0 <= n <= 2^28.
 *   kind 0: the in-place exclusive scan (interpreting filter(), hash Finish, Parquet rank scan) of in[n]. `option` 0: with its block-sum
 *           scratch (one workgroup up to n = 4 096, three launches beyond); 1: without (one workgroup at any n). out[n], totals[0] = the sum.
 *   kind 1: filter()'s step over in[n] selected-row counts per tile (n >= 1) and the record table `recs` — n_recs pairs {first tile,
 *           rows}, records with rows only, each owning the tiles of its rows, end to end from tile 0. `option` 0: one or two levels as
 *           filter() chooses; 1: one level; 2: two levels (block sums first). out[n] = every tile's offset, totals[n_recs + 1] = the sum
 *           in front of every record's first tile, then the grand total.
 *   kind 2: the strided scan (run-store Finish) of in[i x stride], i < n; `option` = stride, 1 to 16, `in` holds n x stride words.
 *           out[n], totals[0] = the sum.
 * `recs` NULL and n_recs 0 for kinds 0 and 2. FDB_ERR_INVALID, before anything is launched, for arguments outside these rules. */
FDB_API int fdb_selftest_prefix_sums(int32_t kind, int device, const uint32_t* in, int64_t n, int32_t option, const int64_t* recs, int32_t n_recs, uint32_t* out,
                                     uint64_t* totals);

/* ---- plan life cycle (≙ physicalplan.Build for one chain, physicalplan.go:417-474) -------------- */
/* `desc` and everything it points at (expression nodes, names, literals, patterns) is copied: the caller may free it as soon
 * as the call has returned (the Go shim builds it in C memory and frees that right away, integration/go/gpuplan/operator.go). */
FDB_API int fdb_plan_create(const fdb_plan_desc* desc, int device, fdb_plan** out);
/* ≙ PhysicalPlan.Callback: borrows `batch` for the duration of the call only (the reference releases
 * the record right after Callback returns, table.go:808,:827). The record is validated against the plan (errors it
 * would raise are returned by THIS call) and the columns the plan references are copied out before returning. Records
 * above 8 MiB of referenced data are scanned right away; smaller ones — the reference hands records of ≥ 1 024 rows
 * (table.go:780) — are queued in HBM and scanned together, ONE launch per ≈2 M pending rows, or when the plan's state
 * is next needed (finish, merge, num_groups, state_*, push of resident batches …).
 * Column types (Arrow C data formats) the plan can reference: int64 "l", uint64 "L" (filter only), float64 "g", bool "b"
 * (filter leaves, AND aggregation), dictionary<any integer index, utf8 / binary / large variants> (filter leaves, group keys),
 * and plain utf8 / binary / large_utf8 / large_binary "u" "z" "U" "Z" (filter leaves, group keys: encoded to key ids on the host
 * during this call, emitted with their input type). Columns the plan does not reference may have any type: they are not read. */
FDB_API int fdb_plan_push(fdb_plan* plan, struct ArrowArray* batch, struct ArrowSchema* schema);
/* `n` Callbacks in one call, in order (≙ a chain handing over the records it has collected: table.go:783-860 calls Callback once
 * per record; a host behind cgo / JNI pays its boundary crossing once per call instead of once per record). Stops at the first
 * record that fails and returns its error; *n_pushed (may be NULL) = records accepted. */
FDB_API int fdb_plan_push_many(fdb_plan* plan, struct ArrowArray* const* batches, struct ArrowSchema* const* schemas, int32_t n, int32_t* n_pushed);
/* Same, for a record that is already resident in HBM. */
FDB_API int fdb_plan_push_batch(fdb_plan* plan, const fdb_batch* batch);
/* Same, for `n` resident records at once (≙ the TableScan handing a chain every part it owns): one fused kernel
 * launch scans all of them, so per-launch costs are paid once per scan instead of once per record. */
FDB_API int fdb_plan_push_batches(fdb_plan* plan, const fdb_batch* const* batches, int32_t n);
/* ≙ PhysicalPlan.Finish: waits for the device, emits a record (group columns in first-seen field
 * order with their input Arrow type, then one column per aggregation named "<func>(<column>)")
 * (aggregate.go:543-633). The caller owns `out`/`out_schema` and must call their release().
 * A plan that saw no selected rows emits a zero-row record and sets *n_rows = 0.
 * The reference emits SEVERAL records when a plain string / binary key column would pass 2 GiB in one (a key builder answers
 * ErrMaxSizeReached, the group is rolled back and starts a new aggregate: aggregate.go:426-468, optbuilders.go:221-224). Same here:
 * fdb_plan_finish emits the first record, fdb_plan_finish_next every further one (*emitted = 1) until *emitted = 0 — the Go shim hands
 * each to next.Callback like finishAggregate does (aggregate.go:617-624). $FDB_TEST_MAX_KEY_BYTES lowers the limit (tests). */
FDB_API int fdb_plan_finish(fdb_plan* plan, struct ArrowArray* out, struct ArrowSchema* out_schema, int64_t* n_rows);
FDB_API int fdb_plan_finish_next(fdb_plan* plan, struct ArrowArray* out, struct ArrowSchema* out_schema, int64_t* n_rows, int32_t* emitted);
/* ≙ Synchronizer + HashAggregate(final=true) on one device (synchronize.go:31-53): folds the partial
 * table of `src` into `dst` (SUM of sums and counts, MIN of mins, MAX of maxes). `src` stays valid. */
FDB_API int fdb_plan_merge(fdb_plan* dst, fdb_plan* src);
/* ≙ filter() (filter.go:276-323): the compacted record of the rows that satisfy the plan's filter.
 * *n_selected == 0 ⇒ `out`/`out_schema` are left untouched (the reference skips empty records, filter.go:264-266). */
FDB_API int fdb_plan_filter(fdb_plan* plan, struct ArrowArray* batch, struct ArrowSchema* schema,
                    struct ArrowArray* out, struct ArrowSchema* out_schema, int64_t* n_selected);
/* Selection vector only: ascending row indices of the rows that satisfy the filter, written to the
 * caller's host buffer `indices` (capacity ≥ batch length). */
FDB_API int fdb_plan_select(fdb_plan* plan, struct ArrowArray* batch, struct ArrowSchema* schema,
                    uint32_t* indices, int64_t capacity, int64_t* n_selected);
/* The same two for a record that is resident in HBM, with results that STAY in HBM (a PredicateFilter whose consumer is another
 * device stage; also what the compaction is measured with — inputs and outputs resident): *out is a new resident
 * batch holding the compacted record (same columns, types and dictionaries; release it with fdb_batch_release; zero rows when
 * nothing qualifies); `dev_indices` is a DEVICE buffer of `capacity` ≥ fdb_batch_num_rows entries. Three launches: selection
 * bitmap + per-tile counts, their prefix sums, and ONE streaming pass that compacts every column (wave prefix sums, LDS staging,
 * coalesced stores) — rows keep their order, the output is allocated at its exact size. */
FDB_API int fdb_plan_filter_batch(fdb_plan* plan, const fdb_batch* batch, fdb_batch** out, int64_t* n_selected);
/* ≙ PhysicalPlan.Finish for a consumer that lives on the device (another device stage, the cross-GPU exchange): the result record
 * as a RESIDENT batch — group columns (dictionary<uint32> with the plan's distinct values, int64 / uint64, bool) then one column per
 * aggregation, same names and types as fdb_plan_finish. A big hash table (cfg 5: 10 M groups × 32 label columns) is materialised in
 * HBM by the same two column passes and nothing crosses PCIe but the per-column NULL counts; small tables take the host route and
 * are imported back (microseconds). Release with fdb_batch_release; fdb_batch_export gives the Arrow record on the host.
 * Not for plans with aggregations over a dynamic column set. */
FDB_API int fdb_plan_finish_batch(fdb_plan* plan, fdb_batch** out, int64_t* n_rows);
/* filter() over `n` resident records in ONE launch sequence (≙ PredicateFilter.Callback for every record of a scan, filter.go:255-323;
 * what fdb_plan_push_batches is to the aggregate): out[i] / n_selected[i] are record i's compacted record and row count. All or
 * nothing: on an error no output batch is returned. */
FDB_API int fdb_plan_filter_batches(fdb_plan* plan, const fdb_batch* const* batches, int32_t n, fdb_batch** out, int64_t* n_selected);
FDB_API int fdb_plan_select_batch(fdb_plan* plan, const fdb_batch* batch, uint32_t* dev_indices, int64_t capacity, int64_t* n_selected);

/* ---- Projection as an operator of its own (≙ Projection.Callback / Project, physicalplan/project.go:906-943) ----------------------
 * `TableScan → PredicateFilter → Projection` and the `sum(x) / convert(count(x), float64) as avg(x)` the planner puts behind a final
 * aggregate (logicalplan/builder.go:205-238). The COMPUTED expressions are the plan's projections[] (a plan with n_aggs == 0,
 * n_groups == 0 and n_projections > 0 is valid; any plan that has projections may be used — the calls do not touch its aggregate
 * state, like fdb_plan_filter*; a filter-only plan's fdb_plan_push keeps answering FDB_ERR_STATE); the output list is passed per call.
 * Output record: fields in `cols` order, each item expanded to 0 … n fields; as many rows as the input; a call that produces no
 * field at all gives a zero-column, zero-row record; a zero-row input gives zero-row columns of the right types. The result is an
 * ordinary resident batch (fdb_batch_export, fdb_plan_push_batch(es), fdb_plan_filter_batch, fdb_batch_release) whose lifetime does not
 * depend on the input's. Pass-through columns keep type, dictionary, values and NULLs bit for bit (device-to-device copies).
 * Computed fields (semantics as at fdb_proj_node): arithmetic has the type of its left operand (int64 / uint64 / float64); + - *
 * use the RAW slots and are always valid; / is NULL where the divisor is 0 (float64: == 0, so -0.0 too), else Go's quotient
 * (truncation toward zero, MinInt64 / -1 wraps); only the OUTERMOST operation's validity survives (an inner NULL reads back as raw 0);
 * comparison / AND / OR / isnull give a bool column without NULLs (a NULL operand compares false); convert gives float64, always
 * valid; if gives int64, always valid; a projection whose root is an int64 / uint64 / float64 literal is a constant column of the
 * record's length (literalProjection, :716-728); a projection whose root is a column is that column under the projection's name
 * (aliasProjection, :40-56: int64 / uint64 / float64). A division column without a NULL is emitted without a validity bitmap.
 * Errors: a column missing inside an expression FDB_ERR_NOT_FOUND, mixed operand types FDB_ERR_INVALID, unsupported node / column
 * types FDB_ERR_UNSUPPORTED, a kind 2 item that names no projection of the plan FDB_ERR_INVALID. Computed items need the run-time
 * generated kernel: without hiprtc (or under FDB_NO_JIT) a call with one answers FDB_ERR_UNSUPPORTED; pass-through-only calls work.
 * A computed bool field is held like every resident bool column — one int64 per row, 1 = false / 2 = true (what fdb_batch_import
 * makes of an Arrow bool column) — not as a bitmap; fdb_batch_export turns it into Arrow's bit-packed form.
 * At most 16 computed fields per call. Not carried over: boolExprProjection's shortcut for a result column that the table scan
 * pre-computed (:411-432) — no scan on this path produces one. */
typedef struct fdb_project_col {
  int32_t kind;      /* 0 column   — plainProjection (project.go:481-491): the FIRST field named exactly `name`; a record
                                     without it contributes NOTHING (no error)
                        1 dynamic  — dynamicProjection (:742-755): every field whose name starts with name + ".", in the
                                     record's field order; may be none
                        2 computed — desc.projections[] entry whose name is `name`; the output field carries that name
                                     (BinaryExpr.Name() or the alias, aliasProjection :40-56)
                        3 all      — allProjection: every field of the record; `name` ignored */
  int32_t _pad;
  const char* name;
} fdb_project_col;
FDB_API int fdb_plan_project_batch(fdb_plan* plan, const fdb_project_col* cols, int32_t n_cols, const fdb_batch* in, fdb_batch** out);
/* `n` resident records (≙ every record of a scan), ONE launch for every computed field of all of them. All or nothing: on an error no
 * output batch is returned. The records must agree in the types of the columns the expressions read. */
FDB_API int fdb_plan_project_batches(fdb_plan* plan, const fdb_project_col* cols, int32_t n_cols, const fdb_batch* const* in, int32_t n, fdb_batch** out);
/* Host record in, host record out: the referenced and passed-through columns are staged (`batch` is only borrowed), projected on
 * the device and exported. */
FDB_API int fdb_plan_project(fdb_plan* plan, const fdb_project_col* cols, int32_t n_cols, struct ArrowArray* batch, struct ArrowSchema* schema,
                             struct ArrowArray* out, struct ArrowSchema* out_schema);
/* ≙ PhysicalPlan.Draw: "PredicateFilter (…) - HashAggregate (sum(value) by labels.path)". Owned by the plan. */
FDB_API const char* fdb_plan_draw(fdb_plan* plan);
/* The same string for a descriptor, without creating a plan or touching a device (≙ `explain`: the operator strings of
 * logictest/testdata/plan/{aggregate,filter}/…): validates `desc` like fdb_plan_create, writes at most `capacity` bytes
 * (NUL-terminated) to `buf` and the size needed to `*needed`. */
FDB_API int fdb_plan_explain(const fdb_plan_desc* desc, char* buf, int64_t capacity, int64_t* needed);
FDB_API const char* fdb_plan_last_error(const fdb_plan* plan);
/* ≙ PhysicalPlan.Close: frees every host and device buffer of the plan. NULL is a no-op. */
FDB_API void fdb_plan_close(fdb_plan* plan);

/* ---- cross-process merge support (the RCCL reduce of per-GPU partial tables) ------- */
/* Number of groups currently in the plan's partial table (waits for the device). */
FDB_API int fdb_plan_num_groups(fdb_plan* plan, int64_t* n_groups);
/* The group-key columns only, one row per table slot, in slot order (same types as fdb_plan_finish). */
FDB_API int fdb_plan_partial_keys(fdb_plan* plan, struct ArrowArray* out, struct ArrowSchema* out_schema);
/* Copies the partial accumulator of aggregation `agg` (n_groups × 8 bytes, slot order; int64 or
 * float64 per fdb_plan_agg_type) to `dst`, a host or device pointer (hipMemcpyDefault). */
FDB_API int fdb_plan_partial_state(fdb_plan* plan, int32_t agg, void* dst, int64_t capacity_bytes);
/* Fast path of the cross-GPU merge: when every rank's table has the SAME slot layout (same group columns, same key
 * dictionaries in the same order — the usual case for parts of one table), slot i means the same group everywhere
 * and the raw table arrays can be all-reduced in place, with no key exchange. `signature` hashes the layout
 * (group column names, key values in id order, radix strides, aggregations); equal signatures ⇔ equal layouts. */
FDB_API int fdb_plan_state_signature(fdb_plan* plan, uint64_t* signature, int64_t* n_slots);
/* Raw table array `array` (0: selected-row counts; 1 + j: accumulator of aggregation j) ⇄ `dst`/`src`, a DEVICE
 * pointer of n_slots × 8 bytes. int64 everywhere except float64 SUM; float64 MIN/MAX are stored as order-preserving
 * int64 keys, so integer MIN/MAX reductions are exact for them too. Both calls wait for the plan's stream. */
/* Zero-copy variant: the device address of array 0, the distance between consecutive arrays (in 8-byte elements) and
 * the slot count, so that a collective library can reduce the arrays IN PLACE on the plan's stream (fdb_plan_stream);
 * nothing is synchronised. Dense tables only (n_slots = 0 otherwise). */
FDB_API int fdb_plan_state_pointers(fdb_plan* plan, void** base, int64_t* array_stride, int64_t* n_slots);
FDB_API int fdb_plan_state_read(fdb_plan* plan, int32_t array, void* dst, int64_t capacity_bytes);
FDB_API int fdb_plan_state_write(fdb_plan* plan, int32_t array, const void* src, int64_t bytes);
/* How table array `array` merges across plans / ranks (0 = the row counts, 1 + j = PHYSICAL accumulator j — UNIQUE owns two,
 * see DESIGN.md §3): 0 unused, 1 integer sum, 2 float64 sum, 3 integer min, 4 integer max. *n_arrays = 1 + accumulators. */
FDB_API int fdb_plan_state_arrays(fdb_plan* plan, int32_t* n_arrays);
FDB_API int fdb_plan_state_array_op(fdb_plan* plan, int32_t array, int32_t* op);
/* 'l' (int64) or 'g' (float64): the Arrow format of aggregation `agg`'s output column; 0 until the first push. */
FDB_API int fdb_plan_agg_type(fdb_plan* plan, int32_t agg, char* format_out);

/* ---- high-cardinality merge: hash-partitioned exchange of partial hash tables ("G large") -------------
 * ≙ Synchronizer + HashAggregate(final=true) (synchronize.go:31-53, aggregate.go:340-348) when the partial tables hold
 * millions of groups: no rank can afford every other rank's table, so each group is sent to the ONE rank that owns
 * fingerprint % n_ranks (all-to-all over the 7 xGMI links), merged there, and the result stays sharded.
 *   1. every rank exports its group schema (fdb_plan_group_schema: a zero-row record whose dictionary columns carry the
 *      distinct key values seen so far, int64 key columns as plain int64, plus one zero-row column per typed aggregate),
 *      the host side agrees on one global schema (frostdb_amd/distributed.py) and seeds a fresh plan of the same
 *      descriptor with it (fdb_plan_seed_groups) — now key ids mean the same thing on every rank;
 *   2. fdb_plan_hash_export(local, layout = the seeded plan, n_parts) re-keys and packs the local table on the device into
 *      n_parts contiguous partitions of fixed-size rows (row_words32 × 4 bytes each; counts[p] rows in partition p);
 *   3. after the exchange, fdb_plan_hash_import(seeded plan, rows, n) merges the received rows (SUM/COUNT add, MIN, MAX);
 *   4. fdb_plan_finish on the seeded plan emits this rank's shard of the final groups.
 * The same two calls with n_parts = 1 are the device-only path of fdb_plan_merge between two plans of one GPU. */
FDB_API int fdb_plan_group_schema(fdb_plan* plan, struct ArrowArray* out, struct ArrowSchema* out_schema);
FDB_API int fdb_plan_seed_groups(fdb_plan* plan, struct ArrowArray* schema_record, struct ArrowSchema* schema);
/* *dev_rows: DEVICE pointer owned by `src` until its next push or close (NULL if the table is empty). */
FDB_API int fdb_plan_hash_export(fdb_plan* src, fdb_plan* layout, int32_t n_parts, void** dev_rows, int64_t* counts, int32_t* row_words32);
/* dev_rows: DEVICE pointer to n_rows rows packed for `plan`'s layout; may be released when the call returns. */
FDB_API int fdb_plan_hash_import(fdb_plan* plan, const void* dev_rows, int64_t n_rows);

/* ---- cross-GPU merge behind the C ABI: RCCL over xGMI, no Python in the loop -------------------------------
 * ≙ Synchronizer + HashAggregate(final=true) (synchronize.go:31-53, physicalplan.go:438-471) when the N chains of a query run
 * on N GPUs. The reference runs its N chains in ONE process (physicalplan.go:22, :337-347); both deployment shapes exist here:
 *   one process, N devices:  fdb_comm_init_all(devices, n, comms)   → ncclCommInitAll; each chain's goroutine / thread drives
 *                                                                     its own handle (collective calls block until all joined)
 *   one process per GPU:     rank 0 calls fdb_comm_unique_id, the host ships the 128 bytes over whatever it already has
 *                            (FrostDB: its own control plane; bench.py: the launcher's rendezvous), every rank calls
 *                            fdb_comm_init_rank.
 *   fdb_comm_init_local is the same interface over direct peer-to-peer loads / copies between the ranks' buffers inside one
 *   process — no RCCL: the ranks may share a device (RCCL refuses two ranks on one GPU), which is how the multi-rank paths are
 *   tested on a 1-GPU box, and on an xGMI node it is the low-latency route for the 8 KiB tables of low-cardinality queries.
 * librccl is bound at run time (dlopen: the copy already in the process, else librccl.so.1, else $FDB_RCCL_LIB), so a host
 * without RCCL can still load this library; fdb_comm_unique_id / _init_rank / _init_all then fail with FDB_ERR_UNSUPPORTED. */
typedef struct fdb_comm fdb_comm;
#define FDB_COMM_ID_BYTES 128
FDB_API int fdb_comm_unique_id(uint8_t id[FDB_COMM_ID_BYTES]);
FDB_API int fdb_comm_init_rank(const uint8_t id[FDB_COMM_ID_BYTES], int32_t n_ranks, int32_t rank, int device, fdb_comm** out);
FDB_API int fdb_comm_init_all(const int* devices, int32_t n, fdb_comm** out /* [n] */);
FDB_API int fdb_comm_init_local(const int* devices, int32_t n, fdb_comm** out /* [n] */);
FDB_API int32_t fdb_comm_rank(const fdb_comm* comm);
FDB_API int32_t fdb_comm_size(const fdb_comm* comm);
/* The size the TRANSPORT itself reports for this communicator (RCCL: ncclCommCount) — evidence that an N-GPU merge really ran
 * over N ranks; -1 if the bound library has no such entry point. */
FDB_API int32_t fdb_comm_transport_ranks(fdb_comm* comm);
FDB_API const char* fdb_comm_last_error(const fdb_comm* comm);
FDB_API void fdb_comm_destroy(fdb_comm* comm);
/* Low-cardinality merge (cfgs 2-4): when every rank's dense table has the same slot layout (fdb_plan_state_signature — parts of
 * one table share their dictionaries), slot i means the same group everywhere and the tables are merged on the plan's own
 * stream. Small tables (≤ 32 MiB over all ranks: every configuration of the benchmark's low-cardinality queries): the packed
 * table of every rank is all-gathered — ONE collective — and folded locally in RANK ORDER into the table and its host copy, so
 * float64 sums come out bit-identical on every rank and in every run whatever order the ranks arrived in. Bigger dense tables:
 * the arrays are all-reduced in place, one grouped launch (SUM for counts and sums, integer MIN / MAX for MIN / MAX — float64
 * MIN / MAX live as order-preserving int64 keys). The layout check is one tiny MAX all-reduce issued on the communicator's own
 * stream, so it overlaps the scan kernel. *aligned = 1: every rank now holds the
 * merged table (call fdb_plan_finish on the rank that emits; the others just close). *aligned = 0: layouts differ (or the plan
 * is in hash mode — always so for a plan with exact sums, fdb_plan_set_exact_sums) — nothing was changed, use fdb_plan_exchange.
 * Collective: every rank of `comm` must call it. */
FDB_API int fdb_plan_allreduce(fdb_plan* plan, fdb_comm* comm, int32_t* aligned);
/* General merge (any table mode, any key sets; cfg 5): ranks agree on one group schema (all-gather of column names + distinct key
 * values, union in rank order), every table is re-keyed and hash-partitioned on the device (fdb_plan_hash_export), partitions
 * travel point-to-point to their owners (grouped send / recv: all 7 xGMI links of a GPU busy at once; slices of ≤ 128 MiB per
 * peer), owners merge on the device. The result STAYS SHARDED: *shard is a new plan of the same descriptor holding this rank's
 * share of the final groups (fingerprint % n_ranks == rank) — fdb_plan_finish + fdb_plan_close it. Collective.
 * Exact sums (fdb_plan_set_exact_sums): every group's float64 SUMs travel as their normalized limb rows (276 bytes each behind the
 * packed row) and the owner adds them into its own, so a shard's sums are the correctly rounded exact sums of ALL ranks' rows — the
 * same bits for 1 or N ranks, any split of the rows between them and any rank order. Every rank must agree on the flag: if some
 * ranks are exact and others not, every rank answers FDB_ERR_INVALID (before any data moves). */
FDB_API int fdb_plan_exchange(fdb_plan* plan, fdb_comm* comm, fdb_plan** shard);

/* Device memory owned by the library right now (≙ the reference's leak-checked allocator, memory.CheckedAllocator.AssertSize(0),
 * logictest/logic_test.go:169-177): blocks handed out by the per-device caching allocator and not yet returned, plus the arenas
 * of live resident batches; `pinned` counts result blocks whose Arrow release callback has not run. Cached-but-idle blocks are
 * not counted. All three are 0 once every plan, batch, communicator and result record has been closed / released. */
FDB_API int fdb_live_allocations(int64_t* device_blocks, int64_t* device_bytes, int64_t* pinned_blocks);

/* ---- resident batches (a part kept in HBM between queries; 288 GB per GPU) ---------------------- */
FDB_API int fdb_batch_import(struct ArrowArray* batch, struct ArrowSchema* schema, int device, fdb_batch** out);
FDB_API int64_t fdb_batch_num_rows(const fdb_batch* batch);
/* Bytes this batch occupies in HBM (values/indices + validity bitmaps; dictionaries stay on the host). */
FDB_API int64_t fdb_batch_device_bytes(const fdb_batch* batch);
/* Bytes of the batch's narrow-index cache, which is NOT part of fdb_batch_device_bytes: the first dense generated scan that references a
 * dictionary column of ≤ 65 536 entries in a batch of ≥ 1 Mi rows keeps the column's indices at 1 or 2 bytes beside the batch and later
 * scans read those (up to 3 bytes per row and scanned dictionary column; freed with the batch). 0 until such a scan. */
FDB_API int64_t fdb_batch_scan_cache_bytes(const fdb_batch* batch);
FDB_API void fdb_batch_release(fdb_batch* batch);
/* The record of a resident batch as Arrow in host memory (the caller owns `out` / `out_schema` and calls their release()). */
FDB_API int fdb_batch_export(const fdb_batch* batch, struct ArrowArray* out, struct ArrowSchema* out_schema);

/* ---- Parquet column chunks decoded on the device ------------------------------------------------------------
 * ≙ pqarrow/arrow.go:711-823 (writeColumnToArray) + pqarrow/writer/writer.go:391-405: instead of decoding a row group into an
 * arrow.Record on the CPU (one dictionary-builder probe per row) and pushing that, the host hands over the column chunks'
 * BYTES as they sit in the file and gets a resident batch with the layout fdb_batch_import produces — usable with
 * fdb_plan_push_batch(es), fdb_plan_filter_batch, fdb_batch_export. The host side of this call reads page headers, the dictionary
 * page and the headers of RLE / bit-packed runs; definition levels → validity bitmaps, value ranks and the per-row dictionary
 * indices / values are computed in HBM. Covered — the types pqarrow/convert/convert.go:28-102 maps to Arrow, in the encodings and
 * codecs a FrostDB schema can ask for (schema.proto:54-86): flat schemas; BOOLEAN (PLAIN, RLE → bool); INT64 (PLAIN,
 * DELTA_BINARY_PACKED → int64, or uint64 for the logical type Int(64, unsigned)); DOUBLE (PLAIN); INT64 / DOUBLE also with a
 * dictionary page + RLE_DICTIONARY / PLAIN_DICTIONARY data pages, PLAIN pages behind them included (a writer's dictionary fallback
 * inside a chunk) — the dictionary is resolved on the device, the column is 8 bytes per row like any other, and an index beyond the
 * dictionary is FDB_ERR_INVALID; BYTE_ARRAY with a dictionary page +
 * RLE_DICTIONARY data pages and / or PLAIN, DELTA_LENGTH_BYTE_ARRAY, DELTA_BYTE_ARRAY data pages (their values are dictionary-encoded
 * on the host) (→ dictionary<uint32, binary>, convert.go:64-70; utf8 = 1 → dictionary<uint32, utf8>); required or optional; data
 * pages V1 / V2; codecs as listed at `codec`. Repeated (list) columns and everything else: FDB_ERR_UNSUPPORTED (the caller falls
 * back to its Arrow path for that row group). */
typedef struct fdb_parquet_chunk {
  const char* name;        /* field name of the column in the record */
  int32_t physical_type;   /* parquet Type: 0 BOOLEAN, 2 INT64, 5 DOUBLE, 6 BYTE_ARRAY */
  int32_t optional;        /* max definition level: 0 required, 1 optional (> 1: nested / repeated columns — refused) */
  int32_t utf8;            /* BYTE_ARRAY: logical type String; INT64: 1 = logical type Int(64, unsigned) → uint64 column */
  int32_t codec;           /* parquet CompressionCodec of the chunk's pages: 0 UNCOMPRESSED, 1 SNAPPY, 2 GZIP, 4 BROTLI, 6 ZSTD, 7 LZ4_RAW
                              (5, the deprecated LZ4, is read as raw blocks or Hadoop-framed blocks). The compressed pages of a row group
                              are inflated on host threads, page by page in parallel — SNAPPY pages of PLAIN INT64 / DOUBLE values that did
                              not compress (≥ 32 KiB, compressed ≥ 0.9 × plain) on the device instead; the device decodes the values. */
  const uint8_t* data;     /* [dictionary page] data pages …, each preceded by its thrift PageHeader, exactly as in the file */
  int64_t n_bytes;         /* ColumnMetaData.total_compressed_size */
} fdb_parquet_chunk;
FDB_API int fdb_batch_from_parquet(const fdb_parquet_chunk* chunks, int32_t n_chunks, int64_t n_rows, int device, fdb_batch** out);
/* Several row groups in ONE call (≙ the row groups a ParquetConverter is handed one after the other, pqarrow/arrow.go:264-405, and the
 * parts table.go:740-868 iterates): out[g] = the batch of groups[g], each exactly what fdb_batch_from_parquet returns for it. The call
 * walks the page headers of every chunk first, queues every chunk that crosses PCIe as it is on one copy queue — row group after row
 * group, so the link does not idle while a later row group is still on the host —, inflates the compressed pages of all row groups and
 * parses all chunks on host threads side by side, and launches a row group's decode kernels as soon as ITS chunks are parsed. The
 * chunks (or inflated images) of all the call's row groups are in device memory at once: bound a call by bytes, not by row groups.
 * On error no batch is returned (out[0 … n_groups) = NULL). */
typedef struct fdb_parquet_row_group {
  const fdb_parquet_chunk* chunks;  /* the row group's column chunks (one per column of the record) */
  int32_t n_chunks;
  int64_t n_rows;                   /* RowGroup.num_rows */
} fdb_parquet_row_group;
FDB_API int fdb_batches_from_parquet(const fdb_parquet_row_group* groups, int32_t n_groups, int device, fdb_batch** out);

/* ---- a resident batch written as a Parquet row group, encoded on the device --------------------------------------------------
 * ≙ Table.writeRecordsToParquet → pqarrow.RecordsToFile → recordToRows (table.go:1436-1459, pqarrow/parquet.go:85-139, :375-400), the
 * step that ends compaction, block rotation and snapshots: instead of one parquet.Value per cell built on the CPU (after an export of
 * the record at 8 bytes per row and 4 per index), the record stays in HBM and the device writes every payload of the file — definition
 * levels, values compacted past their NULLs, BOOLEAN bits, dictionary indices bit-packed at the dictionary's width — straight to its
 * final file offset in one image; the host reads back one small table per page to size the file, copies the image out once, and writes
 * page headers, dictionary pages and the footer. `batch` may come from anywhere: fdb_batch_import, fdb_batch(es)_from_parquet,
 * fdb_plan_filter_batch(es), fdb_plan_project_batch, fdb_batch_take / _limit / _sort, fdb_batches_merge(_named), fdb_plan_finish_batch.
 *
 * The file: PAR1, ONE row group, FileMetaData, PAR1 — a flat schema, the batch's columns in their order under their names,
 * UNCOMPRESSED, data pages V1 of `page_rows` rows, definition levels RLE-encoded (one RLE run where a page has no NULL or only NULLs,
 * else one bit-packed run), no repetition levels. int64 → INT64 PLAIN; uint64 → INT64 PLAIN with the logical type Int(64, unsigned),
 * the bits as they are (writeUint64, parquet.go:154-165); float64 → DOUBLE PLAIN, every bit kept; bool → BOOLEAN PLAIN; dictionary
 * columns and plain string / binary columns → BYTE_ARRAY (String where the values are utf8) with one PLAIN dictionary page — the
 * column's dictionary entry by entry, duplicates included — and RLE_DICTIONARY data pages at width bits(entries − 1): one bit-packed
 * run per page, or one RLE run where all of a page's non-NULL indices are equal. A column that is all NULL over an empty dictionary has
 * no dictionary page and PLAIN pages of zero values. The footer carries what a reader needs (types, encodings, sizes, page offsets)
 * and Statistics.null_count per column; min / max statistics, the page index and sorting_columns are written by
 * fdb_batch_to_parquet_indexed (below) and by no other call. A zero-row batch gives a valid file
 * whose row group has zero rows. The record's own columns are the schema: a field the record lacks is not written as all-NULL, as the
 * reference does for a schema it is handed (writeNull).
 *
 * Everything that can refuse the call does so before anything is launched: FDB_ERR_INVALID — page_rows not a multiple of 64 in
 * [64, 2^24] (0 = the default, 65 536), an `optional` array of another length than the batch has columns or with an entry outside
 * −1 … 1, "required" asked of a column that holds NULLs; FDB_ERR_UNSUPPORTED — a column type the resident record does not hold, a
 * dictionary of 2^32 entries or more, a dictionary page past 2^31 − 1 bytes (a data page cannot pass it: 2^24 rows of 8 bytes).
 * Two exceptions, which only the record's rows can show: a non-NULL row whose dictionary index lies past its dictionary, and a non-NULL
 * row over an EMPTY dictionary. Both are found by the survey pass and answered FDB_ERR_INVALID after it, before the encode pass: nothing
 * has been written by then.
 *
 * *bytes is host memory of the library holding *n_bytes bytes: give it back with fdb_bytes_free (NULL is a no-op). */
typedef struct fdb_parquet_write_options {
  int32_t page_rows;       /* rows per data page: a multiple of 64 in [64, 2^24]; 0 = 65 536 */
  int32_t n_optional;      /* entries of `optional`: 0 (every column auto) or the batch's column count */
  const int8_t* optional;  /* per column: −1 auto — optional iff the column holds NULLs or is a dictionary / plain string column (dynamic
                              label columns are optional in every FrostDB schema) —, 0 required, 1 optional */
} fdb_parquet_write_options;
FDB_API int fdb_batch_to_parquet(const fdb_batch* batch, const fdb_parquet_write_options* options /* NULL: defaults */, uint8_t** bytes, int64_t* n_bytes);
FDB_API void fdb_bytes_free(uint8_t* bytes);
/* The same writer over a HOST record, the two kernels replaced by a host walk of the code they compile (fdb_pqwrite.h: page geometry,
 * bit positions, word assembly): byte for byte the file fdb_batch_to_parquet writes for the record, and no GPU is touched — what makes
 * the file format checkable on a CPU-only machine, as fdb_selftest_merge_path does for the merge kernels. */
FDB_API int fdb_selftest_parquet_write(struct ArrowArray* batch, struct ArrowSchema* schema, const fdb_parquet_write_options* options, uint8_t** bytes, int64_t* n_bytes);
/* The same two calls with an encoding per column (≙ the `delta_binary_packed` struct tag and parquet.DeltaBinaryPacked of the reference's
 * schemas, dynparquet/schema.go:429-430): a column asked to be DELTA_BINARY_PACKED is written in blocks of 128 deltas with 4 miniblocks
 * of 32, per data page over the page's non-NULL values — deltas of the 64-bit patterns, wrapping; per block the signed minimum, per
 * miniblock the bit length (0 … 64) of its largest delta − minimum; the last miniblock that holds a delta padded with zero bits,
 * miniblocks that hold none with width byte 0 and no body; a page of one value is its header, a page of none `80 01 04 00 00` — and
 * its chunk names DELTA_BINARY_PACKED (and RLE when optional) instead of PLAIN. Levels, null_count, optionality and page geometry are as
 * above, and so is every other column: with n_encodings == 0 or all entries 0 the file is fdb_batch_to_parquet's, byte for byte. The
 * deltas, widths and sizes are found on the device (fdb_pqdelta.hip: compaction of columns with NULLs, block survey, page walk) before
 * the layout, and the pages encoded on the device after it. Refused before anything is launched: FDB_ERR_INVALID — n_encodings neither
 * 0 nor the column count, an entry outside 0 … 1; FDB_ERR_UNSUPPORTED, naming the column — DELTA asked of a column that is not
 * int64 / uint64 (a uint64 column is written as INT64 Int(64, unsigned), bits as they are). */
/* encodings: per column 0 = as fdb_batch_to_parquet writes it, 1 = DELTA_BINARY_PACKED (int64 / uint64 columns);
   n_encodings: 0 (all 0) or the batch's column count */
FDB_API int fdb_batch_to_parquet_encoded(const fdb_batch* batch, const fdb_parquet_write_options* options, const int8_t* encodings, int32_t n_encodings, uint8_t** bytes, int64_t* n_bytes);
FDB_API int fdb_selftest_parquet_write_encoded(struct ArrowArray* batch, struct ArrowSchema* schema, const fdb_parquet_write_options* options, const int8_t* encodings, int32_t n_encodings, uint8_t** bytes, int64_t* n_bytes);
/* The same two calls with a compression codec per column as well (≙ the `compression` of a FrostDB column's storage layout,
 * dynparquet/schema.go:434-443, :571-580): every page of a column asked to be SNAPPY — its dictionary page and all its data pages — is
 * written as ONE Snappy block: PageHeader.uncompressed_page_size is the body as the calls above write it (level length + levels +
 * values, or the DELTA bytes), compressed_page_size the block, ColumnMetaData.codec is SNAPPY, total_uncompressed_size and
 * total_compressed_size each count the page headers, and every page offset follows the compressed sizes. The block is the varint of the
 * body's length, then the elements of the body's FRAGMENTS of 32 768 bytes (FDB_PQS_FRAGMENT) in order, each compressed on its own: no
 * copy reaches before its fragment's first byte, so no offset passes 32 767 — within the 65 472 that fdb_snappy_decode_pages reaches back
 * on the device — and a body of 0 bytes is the block `00`. Inside a fragment (the rule is spelled out in fdb_pqsnappy.h): windows of 64
 * positions; a position is held against the nearest earlier position of its window, at most 16 back, with the same 4 bytes, else against the one a hash
 * table of the positions before the window holds (the largest under each hash); the lowest position with a match wins, the match is
 * extended to its end, literals are tagged in 1 / 2 / 3 bytes, copies cut into elements of at most 64 bytes, the 1-byte-offset form
 * where length 4 … 11 and offset < 2 048 allow it. A page never exceeds 32 + U + U/6 bytes for a body of U. DELTA and SNAPPY go together
 * on one column. With n_codecs == 0 or all entries 0 the file is fdb_batch_to_parquet_encoded's, byte for byte, made by the same path:
 * no further launch, allocation or copy. Otherwise the uncompressed file body is encoded into a staging image in HBM, the host's few
 * bytes inside the page bodies are uploaded and placed, the fragments are compressed on the device (fdb_pqsnappy.hip, one wave each)
 * into scratch of Snappy's bound, the sizes are summed per page on the device and only those come back, in one more wait; the host lays
 * the file out again (compressing the dictionary pages itself: they are host bytes), one gather launch moves every fragment's elements
 * and the chunks of the uncompressed columns into the final image, and that — the smaller one — is what crosses the link. Device memory
 * for the length of the call: staging + scratch + final image, about 3 × the file body — accepted; all of it is the call's own and
 * freed on every path. Refused before anything is launched: FDB_ERR_INVALID — n_codecs neither 0 nor the column count, an entry that
 * is none of 0, 1 and 7; and everything the calls above refuse, unchanged. fdb_parquet_write_options keeps its layout.
 * A column asked to be LZ4_RAW (7, the COMPRESSION_LZ4_RAW of the same schema.go lines): every page of it is ONE LZ4 block, bare —
 * parquet's LZ4_RAW has no preamble, uncompressed_page_size is the body's length U — and ColumnMetaData.codec is 7; sizes and offsets
 * follow the compressed sizes as for SNAPPY. The matches are found exactly as above, fragment by fragment (no match reaches before its
 * fragment's first byte: offsets stay below 32 768, inside LZ4's 65 535 and the 65 472 the device decoder reaches back), under the block
 * format's two end conditions, which are the BODY's: a position may win only if it is at most U − 12, and a match is extended only up to
 * body position U − 5 — liblz4 refuses a block that ends otherwise. They touch the last fragment and, when that one is shorter than 12
 * bytes, the one before it. The sequences of all fragments in order form the block: a sequence's literals are every body byte since the
 * previous match's end, across fragment boundaries and whole fragments without a match (a run may exceed 32 768 literals); lengths are
 * coded as the format says (nibble 15, bytes of 255, a last byte below 255); the block ends in a sequence of literals only, and a body
 * of 0 bytes is the one byte `00`. A page never exceeds U + U/255 + 16 bytes, LZ4_compressBound. The rule is spelled out in fdb_pqlz4.h.
 * On the device (fdb_pqlz4.hip) a wave per fragment leaves the literals before its first match and behind its last as counts and the
 * sequences between them in scratch; a walk per page with the pending literals as its carry places every fragment and the closing
 * sequence and sizes the page; a gather writes the joined runs from the staging image and the scratch's middles. SNAPPY, LZ4_RAW and
 * uncompressed columns may stand side by side; a call without an LZ4_RAW column launches, allocates and copies nothing of this. */
/* codecs: per column parquet's CompressionCodec number, 0 = UNCOMPRESSED, 1 = SNAPPY, 7 = LZ4_RAW; n_codecs: 0 (all 0) or the batch's column count */
FDB_API int fdb_batch_to_parquet_compressed(const fdb_batch* batch, const fdb_parquet_write_options* options, const int8_t* encodings, int32_t n_encodings, const int8_t* codecs, int32_t n_codecs, uint8_t** bytes, int64_t* n_bytes);
FDB_API int fdb_selftest_parquet_write_compressed(struct ArrowArray* batch, struct ArrowSchema* schema, const fdb_parquet_write_options* options, const int8_t* encodings, int32_t n_encodings, const int8_t* codecs, int32_t n_codecs, uint8_t** bytes, int64_t* n_bytes);
/* The same two calls with min / max statistics, the Parquet page index and RowGroup.sorting_columns as well — what FrostDB's own scan
 * reads of a part: BinaryScalarOperation opens each chunk's ColumnIndex() for per-page NullCount, MinValue and MaxValue
 * (query/expr/binaryscalarexpr.go:87-178), filter.go:174-178 and pqarrow/arrow.go:725-770, :935-971 do the same for all-NULL chunks,
 * single-value chunks and Distinct, and a sorted part is known by its sorting_columns (dynparquet/schema.go:342, :837-847). All of it is
 * written only when asked for: with index == NULL, or statistics == 0 and no sorting column, the file is
 * fdb_batch_to_parquet_compressed's, byte for byte, made by the same path — no further launch, allocation, copy or footer field.
 *
 * statistics ≥ 1: FileMetaData.column_orders (field 7, one TypeDefinedOrder per column: without it readers ignore the bounds) and, per
 * chunk, Statistics.min_value / max_value (fields 6 / 5, beside null_count; the deprecated fields 1 / 2 are not written) over the chunk's
 * non-NULL values, exact and never cut, BYTE_ARRAY included; a column without a non-NULL, non-NaN value has neither. int64: signed order,
 * 8 bytes little-endian; uint64: unsigned order (Int(64, unsigned)), 8 bytes; float64: numeric order, NaNs left out, 8 bytes — a minimum
 * equal to zero is written −0.0 and a maximum equal to zero +0.0 whatever signs occurred (parquet-format's rule); bool: false < true, one
 * byte 0 / 1; dictionary and plain string / binary columns: the entries' bytes compared as unsigned bytes, shorter first on a common
 * prefix, over the entries that non-NULL rows REFER to — an unused entry never shows, duplicate entries are one value.
 *
 * statistics == 2: after the last chunk's pages and before the footer every column's ColumnIndex, then every column's OffsetIndex;
 * each ColumnChunk names them (fields 4 … 7); RowGroup.total_compressed_size keeps counting the pages only. OffsetIndex: one
 * PageLocation per data page (the dictionary page is not one) — the offset of the page header, header + body as stored (for a SNAPPY
 * column: of the final layout), first_row_index = page × page_rows. ColumnIndex: null_pages, min_values, max_values, boundary_order,
 * null_counts; a page without a non-NULL value is a null page with empty bounds; bounds as above, but a BYTE_ARRAY bound longer than
 * index_size_limit is cut — a minimum to its prefix, a maximum to its prefix with trailing 0xFF bytes dropped and the last remaining
 * byte incremented (a prefix of 0xFF only: the maximum stays whole); boundary_order, judged on the non-null pages' bounds as written:
 * ASCENDING when mins and maxes are both non-decreasing (also for zero or one such page), else DESCENDING when both are non-increasing,
 * else UNORDERED. A float64 column in which some page has values but only NaNs gets no ColumnIndex (the format cannot say it; Arrow
 * does the same); it keeps its OffsetIndex, and its chunk bounds come from the other pages.
 *
 * sorting_columns: RowGroup.sorting_columns (field 4) as given — metadata only, the rows are not checked against it.
 *
 * The bounds are found on the device (fdb_pqstats.hip): one more pass after the survey, a workgroup per (column, page, tile) folding
 * order-preserving 64-bit keys (fdb_pqstats.h; a dictionary column's through its dense byte-order ranks, the ranks Sort and Merge use,
 * uploaded from the call's arena) into a (column, page) table with one atomicMin and one atomicMax per tile; the table comes back with
 * the survey's in the wait that is there already — the call waits no more often than without statistics. The host folds pages into
 * chunk bounds, maps the keys back, applies the zero rule and the cut, and writes the thrift; the index bytes are the host's and follow
 * the image. The 8-byte columns must be 16-byte aligned on the device (every resident record's are).
 *
 * Refused before anything is launched, FDB_ERR_INVALID: statistics outside 0 … 2; index_size_limit outside 0 … 65 536;
 * n_sorting_columns negative, or positive without the array; a sorting column outside the record's columns or named twice; and
 * everything the calls above refuse, unchanged. fdb_parquet_write_options keeps its layout. */
typedef struct fdb_parquet_sorting_column { int32_t column; int8_t descending; int8_t nulls_first; int8_t pad[2]; } fdb_parquet_sorting_column;
typedef struct fdb_parquet_index_options {
  int32_t statistics;        /* 0 none · 1 chunk Statistics.min_value / max_value · 2 the same + ColumnIndex and OffsetIndex */
  int32_t index_size_limit;  /* BYTE_ARRAY bounds in the ColumnIndex are cut to this many bytes; 0 = 16 (dynparquet.ColumnIndexSize), else 1 … 65 536 */
  const fdb_parquet_sorting_column* sorting_columns;  /* RowGroup.sorting_columns, in this order; metadata only, the rows are not checked */
  int32_t n_sorting_columns;
} fdb_parquet_index_options;
FDB_API int fdb_batch_to_parquet_indexed(const fdb_batch* batch, const fdb_parquet_write_options* options, const int8_t* encodings, int32_t n_encodings, const int8_t* codecs, int32_t n_codecs, const fdb_parquet_index_options* index /* NULL: none */, uint8_t** bytes, int64_t* n_bytes);
FDB_API int fdb_selftest_parquet_write_indexed(struct ArrowArray* batch, struct ArrowSchema* schema, const fdb_parquet_write_options* options, const int8_t* encodings, int32_t n_encodings, const int8_t* codecs, int32_t n_codecs, const fdb_parquet_index_options* index /* NULL: none */, uint8_t** bytes, int64_t* n_bytes);
/* The same two calls with a split-block bloom filter per column as well (parquet-format's BloomFilter.md) — the other thing FrostDB's
 * scan reads of a part: its writer puts one, at 10 bits per value, on every sorting column that is not boolean (Schema.NewWriter,
 * dynparquet/schema.go:1109-1143), and BinaryScalarOperation asks a chunk's BloomFilter() for `=` before it looks at the bounds
 * (query/expr/binaryscalarexpr.go:104-118) — what prunes a label column whose values span the whole range in every part, where min /
 * max never does. With bloom == NULL, n_columns == 0 or every entry 0 the file is fdb_batch_to_parquet_indexed's, byte for byte, made
 * by the same path — no further launch, allocation, copy or footer field.
 *
 * The rule (fdb_pqbloom.h): a value's hash is XXH64, seed 0, of its PLAIN bytes — an int64 / uint64 / float64 value's 8 bytes,
 * little-endian, the bits as they are (a NaN with its payload; −0.0 and +0.0 are two values); a dictionary or plain string / binary
 * entry's bytes without a length prefix. Its block is ((hash >> 32) × n_blocks) >> 32, a block being 32 bytes, eight 32-bit little-endian
 * words, and in word i it sets bit ((uint32)hash × SALT[i]) >> 27, SALT = 47b6137b 44974d91 8824ad5b a2b7289d 705495c7 2df1424b 9efc4947
 * 5c6bfb31. Every non-NULL row's value goes in; of a dictionary column only the entries a non-NULL row REFERS to — an unused entry
 * never answers "maybe". The bitset has 32 × max(1, ⌈⌈n × b / 8⌉ / 32⌉) bytes, at most 134 217 728 and not rounded to a power of two:
 * b = bits_per_value (0 = 10), n = the column's non-NULL rows, of a dictionary or string column the smaller of that and its dictionary's
 * length; a column without a non-NULL value gets one zero block. Each filter is a BloomFilterHeader — `15`, the zigzag varint of the
 * bitset's bytes, `1c 1c 00 00 1c 1c 00 00 1c 1c 00 00 00`: BLOCK, XXHASH, UNCOMPRESSED — and then the bitset, never compressed; the
 * filters follow the last chunk's pages in column order without padding, ColumnIndex / OffsetIndex come after them when asked for,
 * then the footer; ColumnMetaData.bloom_filter_offset / bloom_filter_length (fields 14 / 15: the header's offset, header + bitset) name
 * each, for a file with SNAPPY columns in the final layout; RowGroup.total_compressed_size keeps counting the pages only.
 *
 * The bits are set on the device (fdb_pqbloom.hip): once the survey's table has sized the filters, one more pass on the same stream, a
 * workgroup per (filtered column, page, tile); an 8-byte value is hashed in registers, an index gathers its entry's hash from a table
 * the host computed and uploaded from the call's arena; a value equal to the row before it is skipped, an insert reads its block and
 * issues 64-bit atomic ORs only for the pairs of words that lack a bit. The bitsets live in one zeroed table of the call's arena, each
 * 32-byte aligned (a file offset is not), and come back after the image, one copy per filter straight to its place in the returned
 * bytes; the call waits no more often than without filters. The 8-byte columns must be 16-byte aligned on the device (every resident
 * record's are).
 *
 * Refused before anything is launched: FDB_ERR_INVALID — n_columns neither 0 nor the column count, an entry outside 0 … 1,
 * bits_per_value outside 0 … 64; FDB_ERR_UNSUPPORTED, naming the column — a filter asked of a bool column (the reference skips
 * booleans too); and everything the calls above refuse, unchanged. fdb_parquet_write_options and fdb_parquet_index_options keep their
 * layouts. */
typedef struct fdb_parquet_bloom_options {
  const int8_t* columns;   /* per column: 0 = none, 1 = a bloom filter */
  int32_t n_columns;       /* 0 (no filter) or the batch's column count */
  int32_t bits_per_value;  /* 0 = 10 (bloomFilterBitsPerValue), else 1 … 64 */
} fdb_parquet_bloom_options;
FDB_API int fdb_batch_to_parquet_filtered(const fdb_batch* batch, const fdb_parquet_write_options* options, const int8_t* encodings, int32_t n_encodings, const int8_t* codecs, int32_t n_codecs, const fdb_parquet_index_options* index /* NULL: none */, const fdb_parquet_bloom_options* bloom /* NULL: none */, uint8_t** bytes, int64_t* n_bytes);
FDB_API int fdb_selftest_parquet_write_filtered(struct ArrowArray* batch, struct ArrowSchema* schema, const fdb_parquet_write_options* options, const int8_t* encodings, int32_t n_encodings, const int8_t* codecs, int32_t n_codecs, const fdb_parquet_index_options* index /* NULL: none */, const fdb_parquet_bloom_options* bloom /* NULL: none */, uint8_t** bytes, int64_t* n_bytes);

/* The same two calls with RLE runs INSIDE a page's dictionary indices and definition levels — what a record sorted by its label columns
 * asks for: there a label column is long stretches of one index and a dynamic column long stretches of NULL and of not-NULL, which the
 * calls above write at the column's full width unless a whole page is one value. With runs == NULL, n_columns == 0 or every entry 0 the
 * file is fdb_batch_to_parquet_filtered's, byte for byte, made by the same path — no further launch, allocation or wait.
 *
 * The rule (fdb_pqruns.h). A stream is n symbols at width w >= 1: a page's definition levels (w = 1, n = the page's rows) or an INDEX
 * column's page values (w = the column's width, n = the page's non-NULL rows, by rank). It applies only where the calls above emit ONE
 * bit-packed run; a page that is one RLE run, a column of width 0, an empty page and V64 / BOOL / DELTA payloads stay byte for byte.
 * G = n / 8 full groups, then n mod 8 tail symbols. A group is uniform when its 8 symbols are equal, a stretch a maximal range of
 * consecutive uniform groups of one value, T = ⌈16 / w⌉. A stretch of at least T groups is an RLE run: varint(count << 1), the value in
 * ⌈w / 8⌉ little-endian bytes. The tail joins the last RLE run when the stretch ending at group G − 1 is one and every tail symbol
 * equals its value. Every maximal range of the remaining groups is a bit-packed run: varint((groups << 1) | 1), groups × w bytes,
 * LSB first; a tail that joined nothing is one more zero-padded group at the end of the last bit-packed run, or a run of one group of
 * its own right after an RLE run. Two RLE runs may follow each other. An RLE run replaces at least 16 packed bytes and costs at most
 * 4 + 4 + 4 (its header, its value, the header of the bit-packed run it splits off), so no page gets longer.
 *
 * The sizes now depend on the data, so the passes sit where DELTA's do (fdb_pqruns.hip): after the survey a compaction of the indices
 * of the chosen columns that have a bitmap (4 bytes a row of scratch from the call's arena) and the run survey, a workgroup per
 * (stream, page), whose table of sizes comes back with the survey's in the wait the call already pays; after the layout the run
 * encoder, beside the encode pass, into the same image. A SNAPPY column's pages go through the staging image as ever. Statistics, the
 * page index, bloom filters, sorting_columns and the encodings lists are untouched; sizes and PageLocations follow the new bodies.
 *
 * Refused before anything is launched: FDB_ERR_INVALID — n_columns neither 0 nor the column count, an entry outside 0 … 3;
 * FDB_ERR_UNSUPPORTED, naming the column — bit 0 on a column that is not a dictionary / string / binary column. Bit 1 on a required
 * column is ignored. Everything the calls above refuse, unchanged; their structs keep their layouts. */
typedef struct fdb_parquet_run_options {
  const int8_t* columns;   /* per column: bit 0 = dictionary indices, bit 1 = definition levels */
  int32_t n_columns;       /* 0 or the record's column count */
  int32_t pad;
} fdb_parquet_run_options;
FDB_API int fdb_batch_to_parquet_runs(const fdb_batch* batch, const fdb_parquet_write_options* options, const int8_t* encodings, int32_t n_encodings, const int8_t* codecs, int32_t n_codecs, const fdb_parquet_index_options* index /* NULL: none */, const fdb_parquet_bloom_options* bloom /* NULL: none */, const fdb_parquet_run_options* runs /* NULL: none */, uint8_t** bytes, int64_t* n_bytes);
FDB_API int fdb_selftest_parquet_write_runs(struct ArrowArray* batch, struct ArrowSchema* schema, const fdb_parquet_write_options* options, const int8_t* encodings, int32_t n_encodings, const int8_t* codecs, int32_t n_codecs, const fdb_parquet_index_options* index /* NULL: none */, const fdb_parquet_bloom_options* bloom /* NULL: none */, const fdb_parquet_run_options* runs /* NULL: none */, uint8_t** bytes, int64_t* n_bytes);

/* … and with dictionaries of USED entries only. After filter(), take, limit, a sampler or a merge over a dictionary union a resident
 * column refers to a fraction of its dictionary; fdb_batch_to_parquet_runs still writes every entry and packs the indices at the whole
 * dictionary's width. With `dictionaries` = 1 the dictionary page of a dictionary / string / binary column holds the entries that at
 * least one non-NULL row refers to, in entry order (entries of equal bytes and different indices both stay when both are used), its
 * num_values is their count U, every index is re-keyed to its rank among them and the pages are packed at bits(U − 1). A column whose
 * rows are all NULL takes the form of an empty dictionary: no dictionary page, PLAIN pages of zero values. Statistics, the page index
 * and the bloom filters are over the same byte values as before; a filter's size is capped by U instead of the dictionary's length.
 *
 * Two more passes (fdb_pqdict.hip): behind the survey every non-NULL row's index sets a bit of the column's presence bitmap (one zeroed
 * table of the call's arena, back in the survey's wait); the host counts the used entries in front of every 64-entry word, and a remap
 * pass writes a re-keyed copy of the index column (4 bytes a row of the call's arena) that the encode and run passes read from then on.
 * The run survey needs the re-keyed width, so with `runs` it follows the remap pass and the call waits once more.
 *
 * `row_group_rows` (≙ TableConfig.RowGroupSize, table.go:77-80; here a multiple of 64, so that a group starts on a validity word, where
 * the reference takes any number): rows [g·R, min(rows, (g + 1)·R)) are row group g, the last one shorter; a record of 0 rows keeps its
 * one zero-row group. A group is cut into pages of page_rows on its own (page_rows need not divide R). The file is PAR1, group after
 * group and in a group column after column ([dictionary page] data pages), then the bloom filters, then every ColumnIndex, then every
 * OffsetIndex — each in (group, column) order, first_row_index relative to the group — then the footer: per group what the one RowGroup
 * of the calls above carries (chunk metadata and statistics over the group's pages only, null_count, num_rows, sizes, file_offset),
 * sorting_columns repeated, ordinal = g (written under non-zero options only). A bloom filter is per (group, column), sized from the
 * group's non-NULL rows and capped by the chunk's dictionary length; with `dictionaries` = 1 every group's chunk has the dictionary of
 * its own rows. With `dictionaries` = 0 a group's chunks are byte for byte those of the file written for its rows alone. No pass is
 * launched per group: (group, column) is a column of a record of R rows to every kernel, so a pass runs once for the full groups and
 * once more for a shorter last one, and the call waits no more often than without groups.
 *
 * `groups` == NULL or all zero: fdb_batch_to_parquet_runs' path and bytes, no launch, allocation or wait more. Refused before anything
 * is launched, after everything the calls above refuse: FDB_ERR_INVALID — row_group_rows negative or not a multiple of 64, more than
 * 32 767 row groups, dictionaries outside 0 … 1, pad != 0. */
typedef struct fdb_parquet_group_options {
  int64_t row_group_rows;  /* 0: one row group; else a multiple of 64: rows per row group, the last one shorter */
  int32_t dictionaries;    /* 0: every chunk carries the column's whole dictionary; 1: only the entries its non-NULL rows refer to */
  int32_t pad;             /* 0 */
} fdb_parquet_group_options;
FDB_API int fdb_batch_to_parquet_grouped(const fdb_batch* batch, const fdb_parquet_write_options* options, const int8_t* encodings, int32_t n_encodings, const int8_t* codecs, int32_t n_codecs, const fdb_parquet_index_options* index /* NULL: none */, const fdb_parquet_bloom_options* bloom /* NULL: none */, const fdb_parquet_run_options* runs /* NULL: none */, const fdb_parquet_group_options* groups /* NULL: none */, uint8_t** bytes, int64_t* n_bytes);
FDB_API int fdb_selftest_parquet_write_grouped(struct ArrowArray* batch, struct ArrowSchema* schema, const fdb_parquet_write_options* options, const int8_t* encodings, int32_t n_encodings, const int8_t* codecs, int32_t n_codecs, const fdb_parquet_index_options* index /* NULL: none */, const fdb_parquet_bloom_options* bloom /* NULL: none */, const fdb_parquet_run_options* runs /* NULL: none */, const fdb_parquet_group_options* groups /* NULL: none */, uint8_t** bytes, int64_t* n_bytes);

/* … and with the VALUES of a dictionary / string / binary column in its pages instead of a dictionary page and indices: what FrostDB's
 * own default is for a string column without the `rle_dict` tag (PLAIN; dynparquet/schema.go:531-563) and what its schemas can name
 * (`delta_length_byte_array`), and what a column of mostly distinct values — ids, stack traces, whatever filter() or take has thinned
 * out — asks for, where a dictionary page repeats every value and the indices come on top. `forms`[k] = 1 or 2 on such a column: its
 * chunk has no dictionary page and no dictionary_page_offset, data_page_offset is the first data page, ColumnMetaData.encodings is
 * [PLAIN] or [DELTA_LENGTH_BYTE_ARRAY] (+ RLE when the column is optional) and every DataPageHeader.encoding 0 or 6. A page's body is its
 * definition levels exactly as before (cut into runs when `runs` bit 1 asks) and then its non-NULL values in row order — PLAIN: per
 * value the 4-byte little-endian length and the entry's bytes; DELTA_LENGTH_BYTE_ARRAY: the lengths as DELTA_BINARY_PACKED (blocks of
 * 128, 4 miniblocks, the rule of the int64 columns: lengths lie in [0, 2^31), so its bytes are a 32-bit encoder's), then all the bytes
 * back to back; a page without a value holds the header of zero lengths, 80 01 04 00 00. Entries of equal bytes write the same bytes, an
 * unused entry never shows. A column that is all NULL over an empty dictionary keeps its present form (PLAIN pages of zero values) under
 * form 1 and gets pages of zero lengths under form 2. Statistics, the page index, bloom filters, sorting_columns and row groups are over
 * the record's indices and entries and do not change, PageLocations and sizes follow the new bodies; SNAPPY / LZ4_RAW columns go through
 * the staging image as ever; `dictionaries` = 1 has no effect on such a column (no present or remap pass runs for it).
 *
 * Two more passes (fdb_pqbytes.hip; the rule: fdb_pqbytes.h) over tables of the entries' offsets and bytes, uploaded once per call and
 * shared by its row groups: behind the survey a byte survey sums the entry lengths of every tile's non-NULL rows (its table comes back
 * in the survey's wait; the host scans it into page sizes and per-tile byte bases) and, of a DELTA_LENGTH column, writes the rows'
 * lengths as one more 64-bit column for the DELTA passes; after the layout a byte encode pass writes every tile's output range by OUTPUT
 * position — each lane owns consecutive output bytes and finds the value they belong to in the tile's byte offsets — so stores are
 * contiguous whatever the lengths are.
 *
 * `strings` == NULL, n_columns == 0 or every entry 0: fdb_batch_to_parquet_grouped's path and bytes, no launch, allocation, upload or
 * wait more. Refused before anything is launched, after everything the calls above refuse: FDB_ERR_INVALID — n_columns neither 0 nor the
 * column count, an entry outside 0 … 2, pad != 0; FDB_ERR_UNSUPPORTED, naming the column — a form on a column that is not a dictionary
 * / string / binary column, `runs` bit 0 on a column with a form (it has no index pages). After the survey, before the image is
 * allocated: FDB_ERR_INVALID, naming column and page — a page whose uncompressed body would not fit the i32 of its header. */
typedef struct fdb_parquet_string_options {
  const int8_t* forms;     /* per column: 0 = as ever (dictionary page + RLE_DICTIONARY), 1 = PLAIN, 2 = DELTA_LENGTH_BYTE_ARRAY */
  int32_t n_columns;       /* 0 (all 0) or the record's column count */
  int32_t pad;             /* 0 */
} fdb_parquet_string_options;
FDB_API int fdb_batch_to_parquet_strings(const fdb_batch* batch, const fdb_parquet_write_options* options, const int8_t* encodings, int32_t n_encodings, const int8_t* codecs, int32_t n_codecs, const fdb_parquet_index_options* index /* NULL: none */, const fdb_parquet_bloom_options* bloom /* NULL: none */, const fdb_parquet_run_options* runs /* NULL: none */, const fdb_parquet_group_options* groups /* NULL: none */, const fdb_parquet_string_options* strings /* NULL: none */, uint8_t** bytes, int64_t* n_bytes);
FDB_API int fdb_selftest_parquet_write_strings(struct ArrowArray* batch, struct ArrowSchema* schema, const fdb_parquet_write_options* options, const int8_t* encodings, int32_t n_encodings, const int8_t* codecs, int32_t n_codecs, const fdb_parquet_index_options* index /* NULL: none */, const fdb_parquet_bloom_options* bloom /* NULL: none */, const fdb_parquet_run_options* runs /* NULL: none */, const fdb_parquet_group_options* groups /* NULL: none */, const fdb_parquet_string_options* strings /* NULL: none */, uint8_t** bytes, int64_t* n_bytes);

/* Snappy pages inflated on the device (one wave per page, fdb_kernels.h snappy_decode_kernel) — the building block for pages that cross
 * PCIe compressed (pqarrow/arrow.go:711-823 inflates them on the host; so does fdb_batch_from_parquet today). This entry
 * point takes HOST buffers, for tests and measurement: `src` holds the compressed pages (pages[i] = {src_off, dst_off, src_len,
 * dst_len}: where page i starts in `src`, where its bytes go in `dst`, its compressed and uncompressed sizes), they are copied to the
 * device, decoded by ONE launch, and `dst` is copied back. status[i]: 0 = ok, 1 length preamble ≠ dst_len, 2 truncated input,
 * 3 output overrun, 4 copy offset outside the output, 5 output shorter than announced, 6 a copy from more than 65 472 bytes back (the
 * format allows it, no compressor emits it: matches stay inside a 64 KiB fragment) (a page that fails leaves its part of `dst`
 * undefined; the others are unaffected). *kernel_ms (may be NULL): device time of the launch. device < 0: the library's HOST decoder
 * runs over the same page table and no GPU is touched (the same status codes but 6: any offset is fine there; *kernel_ms = 0) — the
 * decoder fdb_batch_from_parquet uses for the Snappy pages the device does not take. */
typedef struct fdb_snappy_page { uint64_t src_off; uint64_t dst_off; uint32_t src_len; uint32_t dst_len; } fdb_snappy_page;
FDB_API int fdb_snappy_decode_pages(const uint8_t* src, int64_t src_bytes, const fdb_snappy_page* pages, int32_t n_pages, uint8_t* dst, int64_t dst_bytes,
                            int device, uint32_t* status, double* kernel_ms);
/* The same for LZ4 blocks (Parquet's LZ4_RAW: no frame, no length preamble — dst_len is the page's uncompressed size; lz4_decode_kernel).
 * status[i]: 0 = ok, 2 truncated input, 3 output overrun, 4 match offset 0 or before the page's first byte, 5 output shorter than
 * announced, 6 a match from more than 65 472 bytes back (legal LZ4, offsets go up to 65 535: fdb_batch_from_parquet leaves such pages
 * to the host). device < 0: the library's built-in HOST decoder runs over the same page table and no GPU is touched (the same
 * status codes but 6: offsets up to 65 535 are fine there; *kernel_ms = 0) — the decoder fdb_batch_from_parquet uses for LZ4
 * pages where liblz4 is not installed. */
typedef fdb_snappy_page fdb_lz4_page;
FDB_API int fdb_lz4_decode_pages(const uint8_t* src, int64_t src_bytes, const fdb_lz4_page* pages, int32_t n_pages, uint8_t* dst, int64_t dst_bytes,
                         int device, uint32_t* status, double* kernel_ms);

/* ---- measurement hooks (bench.py / rocprof correlation; not needed by the Go shim) -------------- */
/* Algorithmic bytes (values-or-indices + validity of every referenced column, once per
 * row) and accumulated device time in ms (hipEvent pairs on the plan's stream around each scan
 * kernel) since the plan was created; `n_launches` scan-kernel launches. */
FDB_API int fdb_plan_stats(fdb_plan* plan, int64_t* algorithmic_bytes, double* kernel_ms, int64_t* n_launches,
                   int64_t* rows_scanned);
/* fdb_batch_from_parquet, accumulated over the process: calls, wall time of the host part (page-header walk, inflating compressed
 * pages, dictionary pages) and of the device part (copies, pq_* kernels, the waits), bytes of column chunks read and of columns
 * produced. */
FDB_API int fdb_parquet_stats(int64_t* calls, double* host_ms, double* device_ms, int64_t* file_bytes, int64_t* out_bytes);
/* Pages of compression codec `codec` (parquet.thrift CompressionCodec: 1 SNAPPY, 7 LZ4_RAW) that fdb_batch(es)_from_parquet had the
 * DEVICE inflate, accumulated over the process, and their uncompressed bytes (calls that failed count nothing). */
FDB_API int fdb_parquet_device_pages(int codec, int64_t* pages, int64_t* bytes);
/* Run-time specialisation (hiprtc): kernels this process compiled, the wall time the compiler took (ms), and code objects it
 * loaded from the on-disk cache ($FDB_JIT_CACHE) instead — what the FIRST query of a shape pays on top of its scan. */
FDB_API int fdb_jit_stats(int64_t* n_compiled, double* compile_ms, int64_t* n_disk_loads);
/* Accumulated device time in ms of the cross-GPU merges this plan took part in (hipEvent pairs on the plan's stream around the
 * collectives of fdb_plan_allreduce / the all-to-all of fdb_plan_exchange); 0 unless timing is enabled. Read it after
 * fdb_plan_finish (or anything else that waits for the plan's stream). */
FDB_API int fdb_plan_merge_ms(fdb_plan* plan, double* merge_ms);
/* Enables/disables the per-launch hipEvent timing above (off by default; costs two events per launch). */
FDB_API int fdb_plan_set_timing(fdb_plan* plan, int32_t enabled);
/* The hipStream_t the plan launches on, as an opaque pointer. */
FDB_API int fdb_plan_stream(fdb_plan* plan, void** stream_out);
/* Kernel geometry knobs for bench.py's variant sweeps: rows_per_thread 0 = load-hoisting slot kernel (default),
 * 4 / 8 = sequential kernel with that many rows per lane; grid_blocks bits 0-19 = persistent grid size (0 = default),
 * bits 25-27 = variant (1/2/3: 512/256/1024-thread workgroups, 4: interpreting kernels only, no run-time specialisation). */
FDB_API int fdb_plan_set_tuning(fdb_plan* plan, int32_t rows_per_thread, int32_t grid_blocks);
/* Reproducible float sums. float64 addition is not associative and the default scan accumulates a workgroup's rows with LDS atomics
 * whose interleaving across waves differs from run to run: SUM(float64) (and AVG, which is lowered to it) agrees with the reference
 * to ~1e-12 relative but not bit for bit between two runs. With `enabled` every wave accumulates into an LDS table of its own, the
 * tables are added up in wave order and the workgroups' tables in workgroup order (no atomics anywhere): the same records pushed in
 * the same calls give the same bits on every run (NOT the reference's bits: it adds in row order, aggregate.go:822-840). Costs LDS
 * (4 tables per workgroup: ~10 % on cfg 2). Only the dense path of the run-time specialised kernel has it: a scan that needs the
 * hash table, the combining cache (table too big for LDS), the interpreting kernels or 4 tables that do not fit LDS answers
 * FDB_ERR_UNSUPPORTED — from the call that launches it: the push, or for queued small host records a later push / Finish — when the
 * plan has a float64 SUM. MIN / MAX / COUNT and integer sums are exact in every mode.
 * Across GPUs: fdb_plan_allreduce's merge of small tables folds in rank order (reproducible, see there); the in-place all-reduce
 * of big dense tables and the exchange of hash tables are not covered. An ordered plan (fdb_plan_desc.ordered) with this flag does
 * not collect runs (their Finish folds cut groups with atomics): it keeps the dense kernel. */
FDB_API int fdb_plan_set_deterministic(fdb_plan* plan, int32_t enabled);
/* Exact float64 sums. With `enabled`, every SUM over a float64 input — AVG (lowered to SUM + COUNT), computed inputs such as
 * sum(value * 2.5), final-stage plans and the member plans of a dynamic aggregation included — returns the EXACT sum of the group's
 * values, rounded once to nearest, ties to even: the same bits under any permutation of the rows, any split into records, any mix of
 * push / push_many / push_batch(es) / queued small records and any order of fdb_plan_merge calls, and the bits of
 * float(sum(Fraction(v) for v in values)). A zero sum is +0.0, NULL rows contribute 0; NaN, or both +Inf and −Inf, give NaN, one
 * infinity gives that infinity, a finite sum beyond the double range rounds to ±Inf. Each such SUM keeps 66 64-bit integer limbs per
 * group beside the hash table (576 bytes with its flag word and padding); the plan always scans into the hash table. COUNT, MIN, MAX,
 * UNIQUE, AND and integer SUMs are unchanged, as are the output schema and column names. Valid only before the plan's first push,
 * merge or seed (FDB_ERR_STATE afterwards). It wins over fdb_plan_set_deterministic: nothing is refused for its shape. Merging an
 * exact plan with a non-exact one is FDB_ERR_INVALID. Across GPUs, fdb_plan_exchange carries the limbs (exact shards, see there) and
 * fdb_plan_allreduce answers *aligned = 0. Entry points that hand out or move raw accumulator state — fdb_plan_state_*,
 * fdb_plan_hash_export / _import, fdb_plan_group_schema / _seed_groups — answer FDB_ERR_UNSUPPORTED for an exact plan;
 * fdb_plan_partial_keys / _partial_state hand out the rounded sums. */
FDB_API int fdb_plan_set_exact_sums(fdb_plan* plan, int32_t enabled);
/* Host-only self-check of the exact summation (no device): out[0] = the correctly rounded exact sum of x[0 … n), computed by the same
 * digit split, normalize and rounding code the device kernels run. */
FDB_API int fdb_selftest_exact_sum(const double* x, int64_t n, double* out);
/* Name of the scan kernel the latest push launched ("fdb_plan_kernel" = the run-time specialised kernel,
 * "scan_slots_kernel" / "scan_dense_kernel" = the interpreting kernels, "scan_hash_kernel" = the hash-table path);
 * "" before the first push. The string is static. */
FDB_API const char* fdb_plan_last_kernel(fdb_plan* plan);


/* ---- Take, Limit and the reservoir Sampler on resident records ------------------------------------------------------------------
 * The two physical operators of the reference that cut a record to K rows (Limiter, limit.go; ReservoirSampler, sampler.go) and the
 * row gather both rest on (arrowutils.Take), for records that fdb_plan_filter_batch / fdb_plan_project_batch left in HBM: nothing
 * crosses PCIe but the row numbers. Errors of these calls are read with fdb_last_error().
 *
 * fdb_batch_take ≙ arrowutils.Take(ctx, r, indices): row indices[i] of `in` becomes row i of *out — any order, duplicates allowed —,
 * a new resident batch with the same fields, types and dictionaries whose lifetime is independent of `in`'s. n == 0 gives a zero-row
 * record of the same schema. A negative index or one ≥ the record's rows answers FDB_ERR_INVALID before anything is launched. A
 * column without a NULL among the taken rows is emitted without a validity bitmap. */
FDB_API int fdb_batch_take(const fdb_batch* in, const int32_t* indices, int64_t n, fdb_batch** out);
/* ≙ Limiter.Callback (limit.go:63-98), including its quirk: `count` is applied to EVERY record and never decremented, so the call is
 * stateless. rows ≤ count: the whole record (copied device to device: *out does not depend on `in`); count == 0: zero rows, same
 * schema; otherwise the first `count` rows. */
FDB_API int fdb_batch_limit(const fdb_batch* in, uint64_t count, fdb_batch** out);

/* ---- Sort of a resident record ------------------------------------------------------------------------------------------------------
 * ≙ arrowutils.SortRecord (pqarrow/arrowutils/sort.go:48-65) and the "sort indices, then Take" pair the reference's ordered paths use
 * (merge_test.go:356-375), for a record that is already in HBM: nothing crosses PCIe but the column list (and, for
 * fdb_batch_sort_indices, the indices on their way out). fdb_sort_col has the vocabulary of arrowutils.SortingColumn: `index` = the
 * column's position in the record, `direction` 0 = Ascending / 1 = Descending (the numeric values of arrowutils.Direction),
 * `nulls_first` != 0 = the column's NULLs before all its values, else after them — in both cases whatever the direction (:534-564).
 * Columns are compared left to right, the first on which two rows differ decides (:517-532). Values: int64 (and what imports as int64:
 * timestamps) signed; uint64 unsigned; float64 as Go's cmp.Compare — every NaN equals every other NaN and sorts below -Inf, -0.0
 * equals +0.0 (NOT pyarrow's order); dictionary and plain string / binary columns by the bytes of the entry (bytes.Compare), two
 * dictionary entries that hold the same bytes being equal. The raw slot under a NULL is never looked at.
 * The result is STABLE: rows equal on every sorting column keep their input order. The reference's sort.Sort is not stable — any order
 * of such rows is legal there; this one is deterministic.
 * Errors, all answered before anything is launched: n_cols == 0 FDB_ERR_INVALID "at least one column is needed for sorting" (checked
 * first); then a record of 0 or 1 rows gives the empty / {0} permutation without a look at the columns (:412-417); a column index
 * outside the record, a direction other than 0 / 1, more than 2^31 - 1 rows (indices are int32): FDB_ERR_INVALID; a bool column, or a
 * column of a type the resident record cannot hold: FDB_ERR_UNSUPPORTED "unsupported column type for sorting … for column …" (:477).
 * Not bound by the Go shim yet. */
typedef struct fdb_sort_col { int32_t index; uint32_t direction; uint32_t nulls_first; } fdb_sort_col;
/* ≙ arrowutils.SortRecord: indices_out[i] (caller's buffer, one int32 per row of `in`) = the input row that is row i of the sorted record */
FDB_API int fdb_batch_sort_indices(const fdb_batch* in, const fdb_sort_col* cols, int32_t n_cols, int32_t* indices_out);
/* = SortRecord + Take without the indices leaving HBM: *out is a new resident batch, independent of `in` */
FDB_API int fdb_batch_sort(const fdb_batch* in, const fdb_sort_col* cols, int32_t n_cols, fdb_batch** out);
/* host-only: the 64-bit value field of one non-NULL value (kind = the column kinds of the header: int64 / uint64 / float64; raw = its bits) */
FDB_API int fdb_selftest_sort_key(int32_t kind, uint32_t direction, uint64_t raw, uint64_t* key_out);
/* Measurement aid (tools/sort_bench.py): *sort_ms = the device time (HIP events on the call's stream, median of `reps` calls after
 * `warmup` calls) of what fdb_batch_sort_indices runs on the device before its copy-out — key kernels + radix passes —; *bare_ms = the
 * same for bare radix sorts of (uint64 key, uint64 value) pairs with the same pass count (*n_passes) and bit widths: the yardstick. The
 * record needs at least 2 rows. */
FDB_API int fdb_sort_bench(const fdb_batch* in, const fdb_sort_col* cols, int32_t n_cols, int32_t reps, int32_t warmup, double* sort_ms, double* bare_ms,
                           int32_t* n_passes);
/* ---- MergeRecords over resident records --------------------------------------------------------------------------------------------
 * ≙ arrowutils.MergeRecords (pqarrow/arrowutils/merge.go:23-68), what OrderedSynchronizer.mergeRecordsLocked and OrderedAggregate run
 * where several ordered streams meet: `n` >= 1 resident records of one schema (field lists equal in length, names, order and kind), each
 * already ordered by `cols` (the vocabulary of fdb_batch_sort), become ONE new resident record, independent of its inputs, holding all
 * their rows in that order, cut to `limit` rows when limit > 0. Neither keys nor permutation leave HBM. The result is the STABLE sort of
 * the concatenation in[0] ‖ in[1] ‖ … under fdb_batch_sort's comparison: rows equal on every sorting column come out in record order,
 * inside a record in row order (container/heap promises no order of ties: this is one of the legal ones, always the same).
 * Deviations from the reference: two rows both NULL in a column are decided by the NEXT column (cursorHeap.Less returns false at once,
 * merge.go:91-98); float64 sorting columns are accepted (the reference panics, :169-171) and compare as Go's cmp.Compare; descending
 * and mixed directions are supported (the reference's comment says ascending only, its TestMerge vectors say otherwise); dictionaries
 * may differ between the inputs — entries compare by their bytes, the output column carries the union of the entries in first-seen
 * order, and when every input shares one dictionary's content that dictionary is the output's, untranslated; the inputs' order is
 * CHECKED on the device before any merge launch — an unordered input is FDB_ERR_INVALID naming the record and the first offending row.
 * n == 1 is fdb_batch_limit of the record (its order is not looked at); a total of 0 rows gives a zero-row record of the schema.
 * FDB_ERR_INVALID: n == 0, a null record, records on different devices, no sorting columns, a column index or direction out of range,
 * differing field lists, more than 2^31 - 1 rows in total. FDB_ERR_UNSUPPORTED: a bool sorting column, a column the resident record
 * cannot hold, a field that is utf8 in one record and binary in another. Records whose field lists differ (ensureSameSchema's virtual NULL
 * columns, ordered_synchronizer.go:143-241) go through fdb_batches_merge_named below. Not bound by the Go shim yet. */
FDB_API int fdb_batches_merge(const fdb_batch* const* in, int32_t n, const fdb_sort_col* cols, int32_t n_cols, uint64_t limit, fdb_batch** out);
/* ---- MergeRecords over resident records whose field lists differ; OrderedSynchronizer --------------------------------------------------
 * ≙ OrderedSynchronizer.ensureSameSchema + arrowutils.MergeRecords (query/physicalplan/ordered_synchronizer.go:143-241, :116-137): the
 * merge of fdb_batches_merge for records that need not carry the same fields — dynamic columns (`labels.*`) differ from row group to row
 * group. The sorting columns are NAMED: `name` / `dynamic` have the vocabulary of fdb_group_expr — dynamic == 0 matches the field
 * called `name`, dynamic != 0 every field called `name.<something>`; direction / nulls_first as in fdb_sort_col, they apply to every
 * column the expression matches. The unified schema is computed on the host before any launch (:155-208): for each order expression in
 * turn, the fields that match it in ANY input (inputs without rows take part in the schema) become sorting columns, several matches in
 * byte order of their names (dynparquet.MergeDeduplicatedDynCols is sort.Strings); an expression that matches nothing is skipped
 * ("this field will just be considered to be null", :173-177); after the sorting columns come all remaining fields, each once. A record's
 * rows are NULL in every column it lacks — where the reference builds a virtual NULL array per such column, here the kernels are told
 * that the (input, column) pair is absent and nothing is allocated, filled or read for it; such a column always has its validity bitmap,
 * and null_count is exact. Inputs that lack a sorting column sit where its NULLs sit and are ordered by the remaining columns. The output
 * always has the unified column order, also for n == 1 (the record's columns rearranged, cut to `limit`; its order is not looked at, as
 * in fdb_batches_merge). If no expression matches any field the key is empty and the result is the concatenation in input order, cut to
 * `limit`: the stable sort under an empty key, one of the orders the reference may produce. A dictionary column is united over the
 * inputs that have it ("every input shares one dictionary" means every input that has the column); one that only inputs without rows
 * carry comes out all NULL with such an input's dictionary (an empty binary one if it has none).
 * Deviations from the reference, besides those of fdb_batches_merge: the remaining fields come in first-seen order — input order, then
 * field order — where the reference iterates a Go map (any order is legal there, this one is deterministic); a field is never emitted
 * twice — with two or more order expressions the reference's leftoverCols also receives the columns that matched ANOTHER expression
 * (:159-168) and its schema duplicates them; a field an earlier expression matched is not matched again by a later one; each expression
 * carries its own direction and NULL placement (the reference merges ascending, NULLs last only, SortingColumn{Index: i}, :198-201).
 * Refusals, all answered before any launch: n == 0, a null record, records on different devices, order == NULL, n_order <= 0, a null
 * `name`, a direction above 1: FDB_ERR_INVALID; a record with two fields of one name: FDB_ERR_INVALID "found multiple fields … for name
 * …" (:219-227); a name whose column kind differs between two inputs: FDB_ERR_INVALID naming both records; more than 2^31 - 1 rows in
 * total: FDB_ERR_INVALID; a bool sorting column, a field that is utf8 in one record and binary in another: FDB_ERR_UNSUPPORTED, as
 * fdb_batches_merge. An unordered input is FDB_ERR_INVALID naming the record's place in the call and the first offending row.
 * Not bound by the Go shim yet. */
typedef struct fdb_order_col { const char* name; int32_t dynamic; uint32_t direction; uint32_t nulls_first; } fdb_order_col;
FDB_API int fdb_batches_merge_named(const fdb_batch* const* in, int32_t n, const fdb_order_col* order, int32_t n_order, uint64_t limit, fdb_batch** out);
/* host-only: the schema union and the per-input column map behind fdb_batches_merge_named. names / kinds of all fields of all records
 * back to back (n_fields[r] of record r); out_fields[i] = position, in that flat list, of the first occurrence of output column i;
 * *n_sort = how many leading output columns are sorting columns; col_map[r * *n_out + i] = the field's position inside record r, or -1.
 * out_fields has room for `cap` columns, col_map for n_records * cap entries; *n_out and *n_sort are set even where *n_out > cap, which
 * writes nothing else and answers FDB_ERR_INVALID. Directions are not looked at. Refuses what the schema rules refuse: a record with two
 * fields of one name, a name whose kind differs between two records. */
FDB_API int fdb_selftest_merge_schema(const char* const* names, const int32_t* kinds, const int32_t* n_fields, int32_t n_records, const fdb_order_col* order,
                                      int32_t n_order, int32_t* out_fields, int32_t* col_map, int32_t cap, int32_t* n_out, int32_t* n_sort);
/* ≙ OrderedSynchronizer (ordered_synchronizer.go:59-137) over resident records, without the blocking — a C ABI driven from one thread
 * cannot park its caller on a channel; a caller that wants the reference's blocking (the Go shim) keeps the channel on its side.
 * `inputs` chains feed the synchronizer; each contributes at most one record to a ROUND. fdb_osync_push parks `batch` as input `input`'s
 * contribution to the current round — the batch is BORROWED: the caller keeps it alive until the round it belongs to has been merged.
 * The call that makes "inputs waiting == inputs still running" completes the round: it merges the parked records with
 * fdb_batches_merge_named (limit 0; the records in input order, so the order of ties does not depend on who arrived first), returns
 * the result in *merged (a new batch the caller owns) and empties the round; every other push sets *merged = NULL. fdb_osync_finish
 * retires an input; if after it running > 0 && running == waiting this call completes the round (:96-104); *done = 1 when the last
 * input has finished. The schema is computed anew every round, so rounds may differ in their fields. A round whose merge fails (an
 * unordered input, say) returns that error to the completing call and is discarded; the synchronizer stays usable.
 * FDB_ERR_STATE: a push from an input that has finished or that already waits in this round (the reference cannot get there: it
 * blocks), a finish from an input that has finished or waits in this round, one more finish than inputs ("too many OrderedSynchronizer
 * Finish calls"). FDB_ERR_INVALID: inputs <= 0, an order list fdb_batches_merge_named refuses, an input number outside the inputs, a
 * null argument. Calls may come from different threads: one mutex guards the state, the merge of a round included. Closing with records
 * parked forgets them. Errors are read with fdb_last_error() on the calling thread. Not bound by the Go shim yet. */
typedef struct fdb_osync fdb_osync;
FDB_API int fdb_osync_create(int32_t inputs, const fdb_order_col* order, int32_t n_order, fdb_osync** out);
FDB_API int fdb_osync_push(fdb_osync* s, int32_t input, const fdb_batch* batch, fdb_batch** merged);
FDB_API int fdb_osync_finish(fdb_osync* s, int32_t input, fdb_batch** merged, int32_t* done);
FDB_API void fdb_osync_close(fdb_osync* s);
/* the output tile (rows) of the merge kernel for a key of `words` 64-bit words: tests track the kernel through it */
FDB_API int32_t fdb_merge_tile_rows(int32_t words);
/* host-only: the kernels' merge-path code (diagonal search, per-lane serial merge, tile by tile and lane by lane) over two sorted runs
 * of `words`-word keys, row-major; src_out[o] (na + nb entries) = the source of output o: i for a[i], na + j for b[j] */
FDB_API int fdb_selftest_merge_path(const uint64_t* a, int64_t na, const uint64_t* b, int64_t nb, int32_t words, uint32_t* src_out);
/* Measurement aid (tools/merge_bench.py): device time between HIP events on the call's stream, medians of `reps` calls after `warmup`
 * calls — *merge_ms: key kernels + order check (one host round trip included) + rounds; *gather_ms: the gather; round_ms[k]
 * (k < min(*n_rounds, round_cap)): round k alone; *words: the key's words. At least two records with rows. */
FDB_API int fdb_merge_bench(const fdb_batch* const* in, int32_t n, const fdb_sort_col* cols, int32_t n_cols, int32_t reps, int32_t warmup, double* merge_ms,
                            double* gather_ms, double* round_ms, int32_t round_cap, int32_t* n_rounds, int32_t* words);
/* Name of column `index` of a resident batch (for callers that name sorting columns); NULL past the last column. The string lives as
 * long as the batch. */
FDB_API const char* fdb_batch_column_name(const fdb_batch* batch, int32_t index);
/* Its Arrow format string ("l", "L", "g", "b", "u", a dictionary's index format, …), for callers that choose columns by type — the
 * bloom filters of the sorting columns that are not boolean; NULL past the last column. The string lives as long as the batch. */
FDB_API const char* fdb_batch_column_format(const fdb_batch* batch, int32_t index);

/* ≙ ReservoirSampler (sampler.go): keeps up to `size` rows of everything pushed, each row of the input with the same probability.
 * Push is single-threaded per handle, like a plan. The handle holds a `size`-slot reservoir record in HBM and nothing else — a row
 * that enters is copied into its slot before push returns and no input record is referenced afterwards —, so the reference's
 * sizeLimit / materialize (sampler.go:228-289), which bound the bytes such references pin, have nothing to bound and are not part
 * of this interface. Splitting K over the chains of a query (physicalplan.go:478-486) is the caller's job.
 *
 * Which rows are kept is Algorithm L exactly as sampler.go:128-198 runs it: the fill phase in order; then i, w and the `s.i == 0`
 * sentinel; the pending index carried into the next record; one slot draw and one update of w per replacement. (One repair: the
 * reference indexes the unsliced record with a row number counted from the slice its fill phase cut off; here the slice is indexed.)
 * The draws come from splitmix64 seeded with `seed` (state += 0x9E3779B97F4A7C15; z = state; z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9;
 * z = (z ^ z >> 27) * 0x94D049BB133111EB; x = z ^ z >> 31), one output x per draw: a unit draw (rand.Float64) is
 * ((x >> 11) + 0.5) * 2^-53, a slot draw (rand.Intn(size)) is (x * size) >> 64; where 1 - w rounds to 0 the skip is 1. The first draw
 * of a sampler is the unit draw of its initial w. A push of a zero-row record is a no-op; size == 0 keeps nothing.
 *
 * The result is always in materialize's form (the reference emits the source records and one-row slices when it never
 * materialised): ONE record — the fields of the records whose rows are in the reservoir, sorted by name bytewise (:244-254); a row
 * is NULL in a field its record lacked (:264-267), dynamic columns and a field first seen after the reservoir filled included; rows
 * in slot order. A field whose type differs between records answers FDB_ERR_UNSUPPORTED. A dictionary (or plain string / binary)
 * field's output dictionary is the union of the contributing records' dictionaries in first-seen order, entries compared by their
 * bytes; unreferenced entries may stay in it; binary against utf8 in one field is FDB_ERR_UNSUPPORTED. Finish with nothing kept gives
 * a record without columns or rows, *n_rows = 0. Finish does not empty the reservoir. */
typedef struct fdb_sampler fdb_sampler;
FDB_API int fdb_sampler_create(int64_t size, uint64_t seed, int device, fdb_sampler** out);
FDB_API int fdb_sampler_push_batch(fdb_sampler* sampler, const fdb_batch* batch);
/* … a host record: staged for the call, the caller's buffers are only borrowed. */
FDB_API int fdb_sampler_push(fdb_sampler* sampler, struct ArrowArray* batch, struct ArrowSchema* schema);
FDB_API int fdb_sampler_finish_batch(fdb_sampler* sampler, fdb_batch** out, int64_t* n_rows);
FDB_API int fdb_sampler_finish(fdb_sampler* sampler, struct ArrowArray* out, struct ArrowSchema* out_schema, int64_t* n_rows);
FDB_API void fdb_sampler_close(fdb_sampler* sampler);
/* Host-only self-check of the Sampler's selection (no device): records of record_rows[0 … n_records) rows are pushed in turn into a
 * sampler of `size` slots seeded with `seed`; rows_out[slot] = the row the slot ends with, numbered across the records in push
 * order. rows_out has min(size, Σ record_rows) entries. */
FDB_API int fdb_selftest_reservoir(uint64_t seed, int64_t size, const int64_t* record_rows, int32_t n_records, int64_t* rows_out);

#ifdef __cplusplus
}
#endif

#endif /* FROSTDB_AMD_H */
