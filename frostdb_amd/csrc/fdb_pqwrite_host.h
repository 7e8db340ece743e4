// fdb_pqwrite_host.h — host side of the Parquet writer (fdb_pqwrite.cpp): column description, file layout, the host walk. The pieces are
// declared one by one so that a stand-alone program can drive them without a device (tools/asan_parquet_write_main.cpp, built with
// FDB_PQWRITE_HOST_ONLY).
#pragma once

#include <memory>
#include <string>
#include <vector>

#include "fdb_arrow.h"
#include "fdb_pqbloom.h"
#include "fdb_pqbytes.h"
#include "fdb_pqdelta.h"
#include "fdb_pqdict.h"
#include "fdb_pqruns.h"
#include "fdb_pqlz4.h"
#include "fdb_pqsnappy.h"
#include "fdb_pqstats.h"
#include "fdb_pqwrite.h"
#ifndef FDB_PQWRITE_HOST_ONLY
#include "fdb_plan.h"
#endif

namespace fdb {

constexpr int PQW_SNAPPY = 1, PQW_LZ4_RAW = 7;  // parquet.thrift CompressionCodec, the two the writer compresses with
constexpr int PQW_NO_VALUES = -1;  // PqwColumn::pq_kind of a BYTE_ARRAY column that is all NULL and has an empty dictionary

// A column as the writer is handed it: the resident form, on the device (fdb_batch_to_parquet) or in host arrays (the self-test).
struct PqwInput {
  std::string name, format;
  ColKind kind = ColKind::OTHER;
  std::shared_ptr<HostDict> dict;
  int64_t null_count = 0;
  const void* values = nullptr;
  const unsigned char* validity = nullptr;
};

struct PqwColumn {
  std::string name;
  size_t real = 0;               // the record's column this one is — itself, or with several row groups the column it is one group's rows of
  int pq_kind = FDB_PQW_V64;     // FDB_PQW_V64 / _BOOL / _INDEX or PQW_NO_VALUES
  int physical = 0;              // parquet Type
  bool is_u64 = false, utf8 = false, optional = false;
  int delta_slot = -1;            // >= 0: written DELTA_BINARY_PACKED, and its place among the columns that are (the tables of fdb_pqdelta.h)
  int codec = 0;                  // parquet CompressionCodec of the chunk's pages: 0 UNCOMPRESSED, PQW_SNAPPY, PQW_LZ4_RAW
  int run_values = -1, run_levels = -1;  // >= 0: the pages' indices / definition levels are cut into runs (fdb_pqruns.h), and the stream's place in the tables of that
  uint32_t width = 0;
  uint64_t entries = 0;
  int used_slot = -1;             // >= 0: the chunk's dictionary keeps the used entries only (fdb_pqdict.h), and the column's place in PqgPlan. Once
                                  // pqg_resolve has run, `entries` counts the used ones, `width` is theirs and `values` the re-keyed copy
  const void* raw_values = nullptr;  // … and the indices as the record holds them, which the bloom pass keeps reading
  int form = 0;                   // FDB_PQY_*: 1 / 2 = no dictionary page, the values themselves in PLAIN / DELTA_LENGTH_BYTE_ARRAY pages (fdb_pqbytes.h)
  int bytes_slot = -1;            // >= 0: … whose byte streams the byte passes size and write, and the column's place in their tables. (A DELTA_LENGTH
                                  // column has a delta_slot too: its lengths. All NULL over an empty dictionary: neither — the host writes its pages)
  const HostDict* dict = nullptr;
  const void* values = nullptr;
  const unsigned char* validity = nullptr;  // nullptr: every row counts
};

// Where everything goes: the host's bytes (page headers, level and run headers, RLE runs, dictionary pages) as pieces of `blob` with
// their file offsets, the device's payload offsets per (column, page), the footer.
struct PqwLayout {
  struct Piece { uint64_t off; size_t pos, len; };
  std::string blob;
  std::vector<Piece> pieces;
  // Per part of the plan (PqwPlan: one, or with several row groups the full groups and the short last one), in that part's own tables:
  struct Part {
    std::vector<FdbPqwPageOut> out;
    std::vector<uint64_t> delta_out;  // [delta_slot × n_pages + page]: where a DELTA page's value bytes start (its `out` says FDB_PQW_NONE for the values)
    std::vector<uint64_t> run_out;    // [run stream × n_pages + page]: where a stream cut into runs starts (FDB_PQW_NONE: the page's is not; then `out` says where it goes)
    std::vector<uint64_t> bytes_out;  // [bytes_slot × n_pages + page]: where a page's byte stream starts (FDB_PQW_NONE: the page has no value)
  };
  std::vector<Part> parts;
  uint64_t body_bytes = 0;       // PAR1 + column chunks: what the image holds; the footer starts here
  std::string footer;
  void put(uint64_t off, const std::string& s);
  // With compressed columns the file is laid out twice — as it is before compression (the staging image) and as it is written — and
  // both layouts list the data pages of the compressed columns in the same order: in the staging layout `off` / `body` are where a
  // page's body starts and how long it is, in the final one where the elements of its Snappy block, or its LZ4 block, go. `body_pieces` (of `body_blob`):
  // the host's bytes inside those bodies, which have to be in the staging image before the compressor reads it. chunk_off / chunk_len:
  // every column's chunk, which for an uncompressed column moves from one image to the other as it is.
  struct Page { uint64_t off, body; int codec; };
  std::vector<Page> pages;
  std::string body_blob;
  std::vector<Piece> body_pieces;
  std::vector<uint64_t> chunk_off, chunk_len;
  std::vector<int> chunk_codec;  // (chunks in file order: group after group, column after column)
  void put_body(uint64_t off, const std::string& s);
  // The page index (statistics == 2): every column's ColumnIndex, then every column's OffsetIndex — host bytes that follow the body in
  // the file, before the footer; empty otherwise. The image stays the body.
  std::string tail;
  // The bloom filters (fdb_pqbloom.h), in (group, column) order between the body and the page index: each a header — a piece of `blob` like any
  // other host byte — and then its bitset, which the insert pass fills and the caller moves to `bits_off`. Empty: none was asked for.
  struct Bloom { size_t part, col; uint64_t bits_off, bytes; };  // `col`: the column's place in its part
  std::vector<Bloom> blooms;
  uint64_t bloom_bytes = 0;      // headers + bitsets
  size_t file_bytes() const { return (size_t)body_bytes + (size_t)bloom_bytes + tail.size() + footer.size() + 8; }
};

// What fdb_parquet_bloom_options asks for, checked (pqb_plan); the entry hashes of the filtered index columns (pqw_plan); and, once
// the survey has counted the non-NULL rows, every filter's size and its place in the table of bitsets (pqb_size).
struct PqbPlan {
  std::vector<int8_t> on;                      // per column: 1 = gets a filter (empty: none does)
  uint32_t bits_per_value = FDB_PQB_DEFAULT_BITS;
  std::vector<std::vector<uint64_t>> hashes;   // per filtered index column of the RECORD (PqwColumn::real): XXH64 of every entry
  std::vector<uint32_t> bytes;                 // per column: the bitset's bytes (0: no filter)
  std::vector<uint64_t> table_off;             // per column: where its bitset starts in the table (a multiple of 32)
  uint64_t table_bytes = 0;
  bool any() const { return !on.empty(); }
};
// Every refusal of the bloom options: FDB_ERR_INVALID — n_columns neither 0 nor the column count, an entry outside 0 … 1,
// bits_per_value outside 0 … 64; FDB_ERR_UNSUPPORTED, naming the column — a BOOL column. Nothing has been launched yet. `bloom` ==
// nullptr or no entry set: nothing asked (any() is false).
PqbPlan pqb_plan(const fdb_parquet_bloom_options* bloom, const std::vector<PqwColumn>& cols);
void pqb_size(const std::vector<PqwColumn>& cols, const FdbPqwGeom& g, const std::vector<FdbPqwPageStat>& stats, PqbPlan* b);
// The pass over host arrays: every non-NULL row's value into the column's bitset of `table` (table_bytes long, zeroed).
void pqb_insert_host(const std::vector<PqwColumn>& cols, const FdbPqwGeom& g, const PqbPlan& b, unsigned char* table);

// What fdb_parquet_index_options asks for, checked (pqx_plan), the columns' modes and ranks when statistics > 0 (pqw_plan), and what
// the min / max pass found (fdb_pqstats.h) — the table of the kernel on the device, of pqx_minmax_host in the self-test. With it
// pqw_layout writes Statistics.min_value / max_value, column_orders, the page index and sorting_columns; when nothing is asked
// (any() is false) the file of the calls before.
struct PqxIndex {
  int statistics = 0;                                 // 0 none, 1 chunk bounds, 2 + ColumnIndex and OffsetIndex
  uint32_t limit = 16;                                // BYTE_ARRAY bounds of the ColumnIndex are cut to this many bytes
  std::vector<fdb_parquet_sorting_column> sorting;
  std::vector<int> modes;                             // per column: FDB_PQX_*
  std::vector<std::vector<uint32_t>> ranks, entry_of_rank;  // per INDEX column of the RECORD (PqwColumn::real; all its groups share them): the dense rank of every entry, and an entry of every rank
  std::vector<uint64_t> table;                        // 2 × columns × pages keys: mins, then maxes
  bool any() const { return statistics > 0 || !sorting.empty(); }
};
// Every refusal of the index options (FDB_ERR_INVALID): nothing has been launched yet. `index` == nullptr: nothing asked.
PqxIndex pqx_plan(const fdb_parquet_index_options* index, size_t n_cols);
// The pass over host arrays: the table set to empty, then every tile folded in — in descending order, which min and max do not mind.
void pqx_minmax_host(const std::vector<PqwColumn>& cols, const FdbPqwGeom& g, PqxIndex* x);

// What one call asks for beside the record: the arguments of fdb_batch_to_parquet_runs, which the narrower entry points fill in part.
// The pointers are borrowed; null / 0: not asked. `encodings`: per column 0 (as ever) or 1 (DELTA_BINARY_PACKED; I64 and U64 columns
// only); `codecs`: per column 0 (UNCOMPRESSED), 1 (SNAPPY) or 7 (LZ4_RAW); n_encodings / n_codecs: 0 or the column count.
struct PqwSpec {
  const fdb_parquet_write_options* options = nullptr;
  const int8_t* encodings = nullptr; int32_t n_encodings = 0;
  const int8_t* codecs = nullptr; int32_t n_codecs = 0;
  const fdb_parquet_index_options* index = nullptr;
  const fdb_parquet_bloom_options* bloom = nullptr;
  const fdb_parquet_run_options* runs = nullptr;
  const fdb_parquet_group_options* groups = nullptr;
  const fdb_parquet_string_options* strings = nullptr;
};
// The write options, encodings and codecs of `spec` and the columns checked, every refusal of theirs made (FDB_ERR_INVALID /
// FDB_ERR_UNSUPPORTED): nothing has been launched yet.
std::vector<PqwColumn> pqw_columns(const std::vector<PqwInput>& in, int64_t rows, const PqwSpec& spec, int32_t* page_rows);
size_t pqw_delta_columns(const std::vector<PqwColumn>& cols);
// What fdb_parquet_run_options asks for, checked, into the columns' run_values / run_levels; returns the streams. Every refusal:
// FDB_ERR_INVALID — n_columns neither 0 nor the column count, an entry outside 0 … 3; FDB_ERR_UNSUPPORTED, naming the column — bit 0
// on a column that is not an INDEX column. Nothing has been launched yet. A stream that could never hold more than one run gets no
// place: levels of a required column or of one without a bitmap, indices of a dictionary of fewer than two entries.
size_t pqr_plan(const fdb_parquet_run_options* runs, std::vector<PqwColumn>* cols);
size_t pqr_streams(const std::vector<PqwColumn>& cols);
size_t pqw_compressed_columns(const std::vector<PqwColumn>& cols);
// The Snappy block of `n` bytes: the preamble and every fragment's elements, by the host walk of fdb_pqsnappy.h.
std::string pqs_block_host(const unsigned char* body, size_t n);
// The LZ4 block of `n` bytes, bare, by the host walk of fdb_pqlz4.h.
std::string pql_block_host(const unsigned char* body, size_t n);
FdbPqwGeom pqw_geometry(int64_t rows, int32_t page_rows, size_t n_cols);

// Used-entry dictionaries (fdb_parquet_group_options::dictionaries = 1; fdb_pqdict.h): the pruned columns, each with its place in ONE
// table of presence bitmaps — the present pass's on the device, pqg_present_host's in the self-test — and, once pqg_resolve has looked
// at the table, the used entries in front of every word and their count.
struct PqgPlan {
  struct Col { size_t col; uint64_t entries, word_off, words; uint32_t used = 0; };
  std::vector<Col> cols;
  std::vector<unsigned long long> bits;   // the table: every column's bitmap, one after the other
  std::vector<uint32_t> before;           // per word of the table: the column's used entries in front of it
  bool any() const { return !cols.empty(); }
};
// Every refusal of the group options (FDB_ERR_INVALID): nothing has been launched yet. `groups` == nullptr or all zero: nothing asked.
// Returns the pruned columns of `cols` — the record's, or one part's virtual columns — their used_slot set.
PqgPlan pqg_plan(const fdb_parquet_group_options* groups, int64_t rows, std::vector<PqwColumn>* cols);
// … the refusals alone (pqg_plan makes them too): pqw_plan checks the group options, then the string options — whose columns the plan leaves out.
void pqg_check(const fdb_parquet_group_options* groups, int64_t rows);
// The pass over host arrays: every non-NULL row's index into its column's bitmap of d->bits (zeroed).
void pqg_present_host(const std::vector<PqwColumn>& cols, const FdbPqwGeom& g, PqgPlan* d);
// After the wait: an index out of range refused (as the layout would), the used entries counted, d->before made; the columns' `entries`
// and `width` become the used entries', a column without one takes the form of an empty dictionary. `values` is the caller's to swap.
void pqg_resolve(const std::vector<FdbPqwPageStat>& stats, const FdbPqwGeom& g, std::vector<PqwColumn>* cols, PqgPlan* d);
// The pass over host arrays: `out`[slot] = the column's re-keyed indices (rows + 8 of them).
void pqg_remap_host(const std::vector<PqwColumn>& cols, const FdbPqwGeom& g, const PqgPlan& d, std::vector<std::vector<uint32_t>>* out);

// Value pages of BYTE_ARRAY columns (fdb_parquet_string_options; fdb_pqbytes.h): the entry tables of the record's columns with a form —
// the call's parts share them, as they share ranks and entry hashes — and, per part, what the byte survey found, scanned.
struct PqyTables {  // entries + 1 offsets into the entries' bytes laid end to end: the dictionary's own (HostDict::arrow_offsets / joined), made once per dictionary, borrowed here
  const uint32_t* off = nullptr; const unsigned char* bytes = nullptr; size_t n_bytes = 0;
};
struct PqyPlan {
  std::vector<std::shared_ptr<const PqyTables>> tables;  // per column of the RECORD (PqwColumn::real); null: the column has no byte stream
  std::vector<uint64_t> tile_bytes;   // [(bytes_slot × n_pages + page) × tiles_per_page + tile]: the byte survey's table …
  std::vector<uint64_t> page_bytes;   // [bytes_slot × n_pages + page]: … summed per page: the page's byte stream (pqy_scan)
  std::vector<uint64_t> byte_base;    // … and per tile the bytes of its page's tiles before it
};
// Every refusal of the string options: FDB_ERR_INVALID — n_columns neither 0 nor the column count, an entry outside 0 … 2, pad != 0;
// FDB_ERR_UNSUPPORTED, naming the column — a form on a column that is not a dictionary / string / binary column, `runs` bit 0 on a column
// with a form. Nothing has been launched yet. Sets the columns' form, bytes_slot and — DELTA_LENGTH: the lengths are one more DELTA
// column — delta_slot, and makes the entry tables; returns the columns with a byte stream. `strings` == nullptr or all zero: nothing.
size_t pqy_plan(const fdb_parquet_string_options* strings, const fdb_parquet_run_options* runs, std::vector<PqwColumn>* cols, PqyPlan* y);
// The pass over host arrays: y->tile_bytes, tile by tile.
void pqy_survey_host(const std::vector<PqwColumn>& cols, const FdbPqwGeom& g, size_t n_bytes_cols, PqyPlan* y);
// After the wait: the table summed into y->page_bytes and y->byte_base.
void pqy_scan(const FdbPqwGeom& g, size_t n_bytes_cols, PqyPlan* y);
// The pass over host arrays: every tile's share of its page's byte stream, word by word (fdb_pqy_word) as the kernel writes it.
void pqy_encode_host(const std::vector<PqwColumn>& cols, const FdbPqwGeom& g, const PqyPlan& y, const std::vector<uint64_t>& bytes_out, unsigned char* image);

// Everything a call decides before anything is launched: the columns, the geometry, the index and bloom options checked and prepared
// (modes and ranks; entry hashes), how many columns are DELTA, how many compressed, how many streams are cut into runs. What the
// passes find later goes into it: x.table (the min / max pass), the filters' sizes (pqb_size).
struct PqwPlan {
  std::vector<PqwColumn> cols;
  FdbPqwGeom g;
  PqxIndex x; PqbPlan bloom; PqgPlan dict; PqyPlan strings;
  size_t n_delta = 0, n_compressed = 0, n_runs = 0, n_bytes = 0;  // (n_bytes: the columns with a byte stream)
  bool grouped = false;  // group options that are not all zero: a row group says its ordinal
  // Several row groups (row_group_rows = R cuts the record): the plan is one PART of the call, over VIRTUAL columns — (group, column),
  // group after group: the record's column with its buffers starting (first_group + group) · R rows in, a column of a record of g.rows
  // rows to every pass. One part holds the full groups, a second the shorter last one: at most two launches of a pass, whatever G is.
  int64_t first_group = 0, n_groups = 1, file_rows = 0;
  size_t n_real = 0;     // the record's columns: cols.size() == n_groups × n_real
};
// THE place that checks a call's options and makes every refusal, in the parameters' order: write options and columns (pqw_columns),
// index (pqx_plan), bloom (pqb_plan), runs (pqr_plan), groups (pqg_plan), strings (pqy_plan). Nothing has been launched yet. `in` outlives the plan (its dictionaries).
PqwPlan pqw_plan(const std::vector<PqwInput>& in, int64_t rows, const PqwSpec& spec);
// The call's parts: the plan itself when the record is one row group, else the full groups' part and, if the last group is shorter, its.
std::vector<PqwPlan> pqw_parts(PqwPlan&& plan, const PqwSpec& spec);
// The tables the layout is made from, borrowed (null: no such column or stream). `delta_bytes`[delta_slot × n_pages + page]: the value
// bytes of a DELTA page, as the block survey found them. `run_bytes`[run stream × n_pages + page]: the bytes of a page's stream cut into
// runs, as the run survey found them — held to the rule's bounds before they are trusted; looked at only where fdb_pqr_active says the
// rule applies. `page_elements` == nullptr: every page as it is before compression, whatever the columns' codecs — the file itself
// when no column has one, else the staging image. Otherwise the file as written: [compressed column × n_pages + page] = the bytes of
// the elements of the page's Snappy block (the preamble not counted) or of its whole LZ4 block, as the compressor found them.
struct PqwSizes {
  const std::vector<FdbPqwPageStat>& stats;  // the survey's
  const std::vector<uint32_t>*delta_bytes = nullptr, *run_bytes = nullptr, *page_elements = nullptr;
  const std::vector<uint64_t>* stream_bytes = nullptr;  // [bytes_slot × n_pages + page]: PqyPlan::page_bytes, as the byte survey found them
};
// The page index, sorting_columns and the bloom filters of the plan are laid out when the layout is the file's own — no compressed
// column, or `page_elements` given: a staging image has neither.
PqwLayout pqw_layout(const PqwPlan& plan, const PqwSizes& sizes);
// … of a call in parts: `sizes`[i] are parts[i]'s tables; `page_elements`, every part's the same, lists the pages in file order.
PqwLayout pqw_layout(const std::vector<const PqwPlan*>& parts, const std::vector<PqwSizes>& sizes);
// Fills the holes of `file` (L.file_bytes() long, the payloads in place — the bitsets of L.blooms included) and appends the page index,
// if any, footer, length and magic.
void pqw_finish(const PqwLayout& L, uint8_t* file);
void pqw_survey_host(const std::vector<PqwColumn>& cols, const FdbPqwGeom& g, std::vector<FdbPqwPageStat>* stats, std::vector<uint32_t>* tile_base);
// `image`: zeroed, body_bytes rounded up to whole words (+ 4).
void pqw_encode_host(const std::vector<PqwColumn>& cols, const FdbPqwGeom& g, const std::vector<FdbPqwPageOut>& out, const std::vector<uint32_t>& tile_base,
                     unsigned char* image);

// The DELTA passes over host arrays, the arithmetic of fdb_pqdelta.h that the kernels compile. `dense`[slot]: the column's non-NULL values,
// those of page p from [first row of p] on (left empty for a column without a bitmap, which is read in place).
struct PqdHost {
  std::vector<std::vector<uint64_t>> dense;
  std::vector<FdbPqdBlock> blocks;
  std::vector<uint32_t> page_bytes;
  const uint64_t* values(const PqwColumn& c) const { return c.validity != nullptr || c.form != 0 ? dense[(size_t)c.delta_slot].data() : (const uint64_t*)c.values; }  // (a form: its lengths)
};
void pqd_survey_host(const std::vector<PqwColumn>& cols, const FdbPqwGeom& g, const std::vector<FdbPqwPageStat>& stats, const std::vector<uint32_t>& tile_base, PqdHost* d,
                     const PqyPlan* y = nullptr);  // (`y`: the entry tables, with a DELTA_LENGTH column)
void pqd_encode_host(const std::vector<PqwColumn>& cols, const FdbPqwGeom& g, const std::vector<FdbPqwPageStat>& stats, const PqdHost& d, const std::vector<uint64_t>& delta_out,
                     unsigned char* image);

// The run passes over host arrays, the rule of fdb_pqruns.h that the kernels compile: every stream's runs, page by page, kept as bytes
// (pqr_survey_host; their lengths are the table the layout wants) and then put where the layout says (pqr_encode_host).
struct PqrHost {
  std::vector<std::string> payload;   // [run stream × n_pages + page]; empty where the rule does not apply
  std::vector<uint32_t> page_bytes;
};
// A stream's bytes by the rule: n symbols at width w.
std::string pqr_page_host(const uint32_t* sym, uint32_t n, uint32_t w);
void pqr_survey_host(const std::vector<PqwColumn>& cols, const FdbPqwGeom& g, const std::vector<FdbPqwPageStat>& stats, PqrHost* r);
void pqr_encode_host(const PqrHost& r, const std::vector<uint64_t>& run_out, unsigned char* image);

// The buffer a file is returned in (fdb_bytes_free): malloc'ed, or a block of the pinned result pool when the device copies into it.
uint8_t* pqw_alloc_bytes(size_t n, bool pinned);
void pqw_free_bytes(uint8_t* bytes);

void selftest_parquet_write(const HostRecordView& view, const PqwSpec& spec, uint8_t** bytes, int64_t* n_bytes);
#ifndef FDB_PQWRITE_HOST_ONLY
void batch_to_parquet(const DeviceBatch& b, const PqwSpec& spec, uint8_t** bytes, int64_t* n_bytes);
#endif

}  // namespace fdb
