// fdb_pqwrite.cpp — a resident record as one Parquet file (fdb_batch_to_parquet and its wider entry points), encoded on the device.
//
// ≙ Table.writeRecordsToParquet → pqarrow.RecordsToFile → recordToRows (table.go:1436-1459, pqarrow/parquet.go:85-139, :375-400): the
// reference builds one parquet.Value per cell on the CPU. Here the host decides a layout and writes what is small — page headers, run
// headers, dictionary pages, the page index, the footer (a thrift compact writer of this file's own) — and the device writes every
// payload. Every entry point fills a PqwSpec with the arguments it has (null / 0: not asked) and runs ONE pipeline; a pass in
// [brackets] runs only when asked for, and without it launches, allocations and copies are those of the narrower call.
//   plan     pqw_plan: options and columns checked, every refusal made — in the parameters' order: write options and columns, index,
//            bloom, runs, groups, strings — before anything is launched; the columns' modes and ranks (statistics) and the entry hashes of the filtered
//            index columns (entry_hashes, fdb_sortplan.h) prepared. A record without rows or columns ends here, on the host.
//   survey   pqw_survey_kernel: per (column, page) the non-NULL rows and, of index columns, the smallest and largest index; per tile
//            the rank of its first value. Only the per-page table comes back. Behind it, their tables back in the SAME wait:
//            [min / max] statistics and the page index (rules: include/frostdb_amd.h, keys: fdb_pqstats.h): fdb_pqstats.hip folds an
//                        order-preserving key of every value that counts into a (column, page) table;
//            [DELTA]     an I64 / U64 column written DELTA_BINARY_PACKED (blocks of 128, 4 miniblocks; rule: fdb_pqdelta.h): its page
//                        sizes depend on the values, so fdb_pqdelta.hip compacts the columns with a bitmap, surveys blocks, walks pages;
//            [runs]      RLE runs INSIDE a page's dictionary indices and definition levels (rule: fdb_pqruns.h), what a record sorted by
//                        its label columns asks for: a chosen stream that would be ONE bit-packed run is cut into RLE and bit-packed
//                        runs, never longer; fdb_pqruns.hip compacts the indices of the columns with a bitmap and surveys the runs.
//            [used]      dictionaries of used entries only (fdb_parquet_group_options; rule: fdb_pqdict.h): fdb_pqdict.hip sets a bit per
//                        referenced entry in one table of presence bitmaps. After the wait the host counts the used entries
//                        (pqg_resolve) and a remap pass writes a re-keyed copy of every pruned index column, which IS the column for
//                        every later pass but the bloom insert; the run passes, which need the new width, then follow it and are
//                        waited for once more.
//            [strings]   a dictionary / string / binary column written with a FORM (fdb_parquet_string_options; rule: fdb_pqbytes.h) has no
//                        dictionary page: its pages hold the non-NULL values themselves, PLAIN or DELTA_LENGTH_BYTE_ARRAY. fdb_pqbytes.hip
//                        sums the entry lengths of every tile's non-NULL rows (the host scans the sums into page sizes and per-tile byte
//                        bases) and writes a DELTA_LENGTH column's lengths in rank order as one more column of the DELTA passes. After the
//                        layout a byte encode pass gathers the values from the entry tables, by output position.
//   layout   pqw_layout (host): with these tables every page's size is known, so every payload's file offset is; every DELTA and run
//            size is held to its rule's bounds first. The survey's table sizes the bloom filters (pqb_size). Pages are folded into
//            chunk bounds, keys mapped back (a rank to an entry), the zero rule, the cut of BYTE_ARRAY bounds, the boundary order, the
//            thrift of Statistics, ColumnIndex, OffsetIndex, column_orders and sorting_columns.
//   encode   [bloom] first, on the same stream: a split-block filter per chosen column (rule: fdb_pqbloom.h), inserted by fdb_pqbloom.hip
//            into ONE zeroed table of bitsets from the call's arena, each 32-byte aligned there (the atomics want that; a file offset
//            is arbitrary, so the bitsets are not part of the image). Then pqw_encode_kernel: every payload straight to its offset in
//            ONE image of the file body, holes where the host's bytes go. [DELTA]: the DELTA encoder writes the pages' value bytes, the
//            encode pass such a column's levels only. [runs]: the run encoder writes the runs, headers and all (PqwLayout::run_out; the
//            host's `pre` / `vpre` shrink to the levels' length and the width byte); the encode pass leaves such a stream alone.
//   [SNAPPY] a column written SNAPPY (rule: fdb_pqsnappy.h): the image so far is a STAGING image in HBM, laid out as the uncompressed
//            file. The host's few bytes inside the bodies to be compressed are placed (a body has to be whole), every fragment is
//            compressed into its slot of scratch, the sizes are summed per page and only those come back: the second wait. The host
//            lays the file out again (dictionary pages it compresses itself) and ONE gather launch moves the fragments' elements and
//            the chunks of the uncompressed columns into the final image. Device memory: about 3 × the file body, the call's, freed
//            on every path. The page index and the filters are the FINAL layout's; filters are never compressed.
//   [LZ4_RAW] a column written LZ4_RAW (rule: fdb_pqlz4.h) goes the same way beside the SNAPPY ones: its pages' fragments are searched by
//            fdb_pqlz4.hip's compress kernel, which leaves per fragment the literals before its first match and behind its last as counts
//            and the sequences between in scratch; a walk per page joins them into ONE bare block and sizes it — the sizes come back in
//            the same wait — and a second gather launch writes the blocks. The chunks of uncompressed columns stay the first gather's.
//   deliver  the bitsets, one copy per filter straight to its offset in the returned bytes, then one device→host copy of the image
//            into the returned (pinned) buffer, in one wait; the host fills the holes, appends page index (PqwLayout::tail) and footer.
// fdb_selftest_parquet_write runs the same plan, layout and tail over a host record, every kernel replaced by a host walk of the same
// arithmetic (fdb_pqwrite.h, the *_host functions) — byte-identical files, no GPU. FDB_PQWRITE_HOST_ONLY leaves the device half out.
//
// File: PAR1 | per row group, per column [dictionary page] data pages V1 | [bloom filters] | [page index] | FileMetaData | length | PAR1.
// [row groups] fdb_parquet_group_options::row_group_rows = R cuts the record into groups of R rows (pqw_parts): (group, column) is a
// VIRTUAL column — the column's buffers g · R rows in — of a record of R rows, so the call is at most two PARTS, the full groups' and a
// shorter last group's, each a plan of its own that every pass above is launched for once, into ONE layout, image and set of waits.
// Flat schema, one row group unless asked, definition levels RLE (one RLE run when a page has no NULL or only NULLs, else one bit-packed run whose payload is the
// validity bitmap's bytes), no repetition levels. I64 → INT64 PLAIN; U64 → INT64 PLAIN, Int(64, unsigned) (writeUint64,
// parquet.go:154-165); F64 → DOUBLE PLAIN; BOOL → BOOLEAN PLAIN; dictionary and plain string / binary columns → BYTE_ARRAY, a PLAIN
// dictionary page of the interned dictionary's entries in entry order + RLE_DICTIONARY pages: the width byte, then ONE bit-packed run —
// or one RLE run where all non-NULL indices of the page are equal, as in the leading sorting columns of an ordered record. An all-NULL
// column with an empty dictionary has no dictionary page and PLAIN pages of zero values.
#include "fdb_pqwrite_host.h"
#include "fdb_sortplan.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>

#ifndef FDB_PQWRITE_HOST_ONLY
#include "fdb_context.h"
#include "fdb_plan_internal.h"
#include "fdb_record.h"
#endif

namespace fdb {

namespace {

// ---- thrift compact protocol, as far as parquet.thrift's structs need it ----------------------------------------------------------------
struct Thrift {
  enum { T_TRUE = 1, T_FALSE = 2, T_BYTE = 3, T_I16 = 4, T_I32 = 5, T_I64 = 6, T_BINARY = 8, T_LIST = 9, T_STRUCT = 12 };
  std::string out;
  std::vector<int> stack;
  int last = 0;
  void varint(uint64_t v) { while (v >= 0x80) { out.push_back((char)(v | 0x80)); v >>= 7; } out.push_back((char)v); }
  void zigzag(int64_t v) { varint(((uint64_t)v << 1) ^ (uint64_t)(v >> 63)); }
  void field(int id, int type) {
    const int delta = id - last;
    if (delta > 0 && delta <= 15) out.push_back((char)((delta << 4) | type));
    else { out.push_back((char)type); zigzag(id); }
    last = id;
  }
  void i16(int id, int16_t v) { field(id, T_I16); zigzag(v); }
  void i32(int id, int32_t v) { field(id, T_I32); zigzag(v); }
  void i64(int id, int64_t v) { field(id, T_I64); zigzag(v); }
  void boolean(int id, bool v) { field(id, v ? T_TRUE : T_FALSE); }
  void byte(int id, int8_t v) { field(id, T_BYTE); out.push_back((char)v); }
  void str(const std::string& s) { varint(s.size()); out += s; }
  void string(int id, const std::string& s) { field(id, T_BINARY); str(s); }
  void list(int id, int elem, size_t n) {
    field(id, T_LIST);
    if (n < 15) out.push_back((char)((n << 4) | (size_t)elem));
    else { out.push_back((char)(0xF0 | elem)); varint(n); }
  }
  void open() { stack.push_back(last); last = 0; }               // a struct that is a list element (or the top)
  void open(int id) { field(id, T_STRUCT); open(); }             // … a field
  void close() { out.push_back(0); last = stack.back(); stack.pop_back(); }
};

enum { PT_BOOLEAN = 0, PT_INT64 = 2, PT_DOUBLE = 5, PT_BYTE_ARRAY = 6 };
enum { ENC_PLAIN = 0, ENC_RLE = 3, ENC_DELTA_BINARY_PACKED = 5, ENC_DELTA_LENGTH_BYTE_ARRAY = 6, ENC_RLE_DICTIONARY = 8 };
enum { PAGE_DATA = 0, PAGE_DICTIONARY = 2 };

std::string page_header(int type, int64_t body, int64_t compressed, int64_t num_values, int encoding) {
  Thrift t;
  t.open();
  t.i32(1, type);
  t.i32(2, (int32_t)body);
  t.i32(3, (int32_t)compressed);
  if (type == PAGE_DATA) {
    t.open(5);
    t.i32(1, (int32_t)num_values); t.i32(2, encoding); t.i32(3, ENC_RLE); t.i32(4, ENC_RLE);
    t.close();
  } else {
    t.open(7);
    t.i32(1, (int32_t)num_values); t.i32(2, encoding);
    t.close();
  }
  t.close();
  return t.out;
}

std::string varint_bytes(uint64_t v) { Thrift t; t.varint(v); return t.out; }
std::string le32(uint32_t v) { std::string s(4, '\0'); std::memcpy(&s[0], &v, 4); return s; }

struct PageLoc { uint64_t off, bytes; uint32_t rows, count; };  // a data page: where its header starts, header + body as stored, its rows and non-NULL rows
struct ChunkMeta {
  const PqwColumn* col = nullptr;
  int64_t start = 0, rows = 0;                                              // where the chunk starts; its row group's rows
  int64_t dict_off = -1, data_off = 0, bytes = 0, raw_bytes = 0, nulls = 0;  // bytes: as stored; raw_bytes: the bodies uncompressed (headers in both)
  // with statistics only
  std::vector<PageLoc> pages;
  bool has_bounds = false;
  std::string min, max;                                                     // Statistics.min_value / max_value
  int64_t offset_index_off = -1, offset_index_len = 0, column_index_off = -1, column_index_len = 0;
  int64_t bloom_off = -1, bloom_len = 0;                                    // with a bloom filter only: its header's offset, header + bitset
};

// `chunks`: n_groups × n_cols of them, group after group; the schema is the first group's columns'. `group_rows`: per group.
std::string footer(const std::vector<ChunkMeta>& chunks, size_t n_cols, const std::vector<int64_t>& group_rows, int64_t rows, const PqxIndex* x, bool ordinals) {
  Thrift t;
  t.open();
  t.i32(1, 1);
  t.list(2, Thrift::T_STRUCT, n_cols + 1);
  t.open(); t.i32(3, 0); t.string(4, "schema"); t.i32(5, (int32_t)n_cols); t.close();
  for (size_t k = 0; k < n_cols; k++) {
    const PqwColumn& c = *chunks[k].col;
    t.open();
    t.i32(1, c.physical);
    t.i32(3, c.optional ? 1 : 0);
    t.string(4, c.name);
    if (c.physical == PT_BYTE_ARRAY && c.utf8) { t.i32(6, 0); t.open(10); t.open(1); t.close(); t.close(); }                            // UTF8; LogicalType.STRING
    if (c.is_u64) { t.i32(6, 14); t.open(10); t.open(10); t.byte(1, 64); t.boolean(2, false); t.close(); t.close(); }                    // UINT_64; LogicalType.INTEGER(64, unsigned)
    t.close();
  }
  t.i64(3, rows);
  t.list(4, Thrift::T_STRUCT, group_rows.size());
  for (size_t grp = 0; grp < group_rows.size(); grp++) {
  const int64_t rows = group_rows[grp];  // (from here on: the group's)
  t.open();  // RowGroup
  t.list(1, Thrift::T_STRUCT, n_cols);
  for (size_t k = 0; k < n_cols; k++) {
    const ChunkMeta& m = chunks[grp * n_cols + k];
    const PqwColumn& c = *m.col;
    t.open();  // ColumnChunk
    t.i64(2, m.dict_off >= 0 ? m.dict_off : m.data_off);
    t.open(3);  // ColumnMetaData
    t.i32(1, c.physical);
    const bool dict = c.pq_kind == FDB_PQW_INDEX && c.form == 0;  // (a form: the values are in the pages, PLAIN or DELTA_LENGTH_BYTE_ARRAY)
    t.list(2, Thrift::T_I32, 1 + (c.optional ? 1 : 0) + (dict ? 1 : 0));  // (RLE: the definition levels, which a required column does not have)
    t.zigzag(c.form == FDB_PQY_DELTA_LENGTH ? ENC_DELTA_LENGTH_BYTE_ARRAY : c.delta_slot >= 0 ? ENC_DELTA_BINARY_PACKED : ENC_PLAIN); if (c.optional) t.zigzag(ENC_RLE); if (dict) t.zigzag(ENC_RLE_DICTIONARY);
    t.list(3, Thrift::T_BINARY, 1); t.str(c.name);
    t.i32(4, c.codec);  // 0 UNCOMPRESSED, 1 SNAPPY, 7 LZ4_RAW
    t.i64(5, rows);
    t.i64(6, m.raw_bytes);
    t.i64(7, m.bytes);
    t.i64(9, m.data_off);
    if (m.dict_off >= 0) t.i64(11, m.dict_off);
    t.open(12); t.i64(3, m.nulls); if (m.has_bounds) { t.string(5, m.max); t.string(6, m.min); } t.close();  // Statistics: null_count, max_value, min_value
    if (m.bloom_off >= 0) { t.i64(14, m.bloom_off); t.i32(15, (int32_t)m.bloom_len); }  // bloom_filter_offset, bloom_filter_length
    t.close();
    if (m.offset_index_off >= 0) { t.i64(4, m.offset_index_off); t.i32(5, (int32_t)m.offset_index_len); }
    if (m.column_index_off >= 0) { t.i64(6, m.column_index_off); t.i32(7, (int32_t)m.column_index_len); }
    t.close();
  }
  int64_t raw_bytes = 0, stored_bytes = 0;
  for (size_t k = 0; k < n_cols; k++) { raw_bytes += chunks[grp * n_cols + k].raw_bytes; stored_bytes += chunks[grp * n_cols + k].bytes; }
  t.i64(2, raw_bytes);  // total_byte_size: uncompressed
  t.i64(3, rows);
  if (x != nullptr && !x->sorting.empty()) {
    t.list(4, Thrift::T_STRUCT, x->sorting.size());
    for (const fdb_parquet_sorting_column& sc : x->sorting) { t.open(); t.i32(1, sc.column); t.boolean(2, sc.descending != 0); t.boolean(3, sc.nulls_first != 0); t.close(); }
  }
  t.i64(5, n_cols > 0 ? chunks[grp * n_cols].start : 4);  // file_offset
  t.i64(6, stored_bytes);                                // total_compressed_size
  if (ordinals) t.i16(7, (int16_t)grp);  // (under group options only: the calls before keep their bytes)
  t.close();
  }
  t.string(6, "frostdb_amd 0.1.0");
  if (x != nullptr && x->statistics > 0) {  // column_orders: TypeDefinedOrder for every column
    t.list(7, Thrift::T_STRUCT, n_cols);
    for (size_t k = 0; k < n_cols; k++) { t.open(); t.open(1); t.close(); t.close(); }
  }
  t.close();
  return t.out;
}

// The PLAIN dictionary page's body: every entry as a 4-byte length and its bytes, in entry order, duplicates included.
std::string dictionary_body(const HostDict& d) {
  std::string s;
  size_t total = 0;
  for (const std::string& v : d.values) total += 4 + v.size();
  s.reserve(total);
  for (const std::string& v : d.values) { s += le32((uint32_t)v.size()); s += v; }
  return s;
}

// … of the used entries only (fdb_pqdict.h): those whose bit of `bits` is set, in entry order.
std::string dictionary_body(const HostDict& d, const unsigned long long* bits) {
  std::string s;
  for (size_t i = 0; i < d.values.size(); i++)
    if (fdb_pqg_used(bits, (uint32_t)i)) { s += le32((uint32_t)d.values[i].size()); s += d.values[i]; }
  return s;
}

std::string index_out_of_range(const PqwColumn& c, uint32_t index, uint64_t entries) {
  return "parquet write: dictionary index out of range in column " + c.name + ": a valid row holds " + std::to_string(index) + ", the dictionary has " + std::to_string(entries) + " entries";
}

// ---- statistics and the page index: the host's half of the min / max pass (fdb_pqstats.h) -----------------------------------------------
std::string le64(uint64_t v) { std::string s(8, '\0'); std::memcpy(&s[0], &v, 8); return s; }

// The bytes a bound is written as: the key mapped back, parquet-format's zero rule for doubles (a minimum that is zero is −0.0, a
// maximum +0.0), an index key — a rank — as the bytes of an entry of that rank.
std::string pqx_bound(const PqwColumn& c, const PqxIndex& x, size_t k, uint64_t key, bool is_max) {
  const int mode = x.modes[k];
  if (mode == FDB_PQX_INDEX) {
    const std::vector<uint32_t>& entry_of_rank = x.entry_of_rank[c.real];
    if (key >= entry_of_rank.size()) throw Error(FDB_ERR_STATE, "parquet write: the min / max pass names rank " + std::to_string(key) + " in column " + c.name);
    return c.dict->values[entry_of_rank[(size_t)key]];
  }
  uint64_t bits = fdb_pqx_value(mode, key);
  if (mode == FDB_PQX_BOOL) return std::string(1, (char)(bits != 0));
  if (mode == FDB_PQX_F64 && (bits << 1) == 0) bits = is_max ? 0 : 0x8000000000000000ull;
  return le64(bits);
}

std::string pqx_cut_min(const std::string& s, size_t limit) { return s.size() > limit ? s.substr(0, limit) : s; }
std::string pqx_cut_max(const std::string& s, size_t limit) {
  if (s.size() <= limit) return s;
  std::string p = s.substr(0, limit);
  while (!p.empty() && (unsigned char)p.back() == 0xFF) p.pop_back();
  if (p.empty()) return s;  // the prefix is all 0xFF: no shorter upper bound
  p.back() = (char)((unsigned char)p.back() + 1);
  return p;
}

// a < b in the column's order, of two bounds as written
bool pqx_less(int mode, const std::string& a, const std::string& b) {
  if (mode == FDB_PQX_INDEX) return a < b;  // (std::string: bytewise unsigned, the shorter first)
  if (mode == FDB_PQX_BOOL) return (unsigned char)a[0] < (unsigned char)b[0];
  uint64_t va, vb, ka = 0, kb = 0;
  std::memcpy(&va, a.data(), 8); std::memcpy(&vb, b.data(), 8);
  fdb_pqx_key(mode, va, &ka); fdb_pqx_key(mode, vb, &kb);
  if (mode == FDB_PQX_F64 && (va << 1) == 0 && (vb << 1) == 0) return false;  // −0.0 == +0.0
  return ka < kb;
}

// Chunk bounds into `m`, and with statistics == 2 the column's ColumnIndex (empty: the column gets none) — from the table's slots of
// column k and the pages the layout has listed in `m`.
std::string pqx_column_index(const PqwColumn& c, const PqxIndex& x, size_t k, size_t n_pages, ChunkMeta* m) {
  const int mode = x.modes[k];
  const size_t items = x.table.size() / 2;
  uint64_t cmn = FDB_PQX_EMPTY_MIN, cmx = FDB_PQX_EMPTY_MAX;
  std::vector<std::string> mins(n_pages), maxs(n_pages);
  bool sayable = true;
  for (size_t p = 0; p < n_pages; p++) {
    const uint64_t mn = x.table[k * n_pages + p], mx = x.table[items + k * n_pages + p];
    const bool empty = mn > mx;
    const uint32_t cnt = m->pages[p].count;
    if (empty) {
      if (cnt > 0 && mode != FDB_PQX_F64) throw Error(FDB_ERR_STATE, "parquet write: the min / max pass found no value in a page of " + std::to_string(cnt) + " (" + c.name + ")");
      if (cnt > 0) sayable = false;  // values, and NaNs only: the ColumnIndex has no way to say it
      continue;
    }
    if (cnt == 0) throw Error(FDB_ERR_STATE, "parquet write: the min / max pass found a value in a page of NULLs (" + c.name + ")");
    cmn = mn < cmn ? mn : cmn; cmx = mx > cmx ? mx : cmx;
    if (x.statistics == 2) {
      mins[p] = pqx_bound(c, x, k, mn, false); maxs[p] = pqx_bound(c, x, k, mx, true);
      if (mode == FDB_PQX_INDEX) { mins[p] = pqx_cut_min(mins[p], x.limit); maxs[p] = pqx_cut_max(maxs[p], x.limit); }
    }
  }
  if (cmn <= cmx) { m->has_bounds = true; m->min = pqx_bound(c, x, k, cmn, false); m->max = pqx_bound(c, x, k, cmx, true); }
  if (x.statistics != 2 || !sayable) return std::string();
  bool up = true, down = true;
  size_t prev = n_pages;
  for (size_t p = 0; p < n_pages; p++) {
    if (m->pages[p].count == 0) continue;
    if (prev != n_pages) {
      if (pqx_less(mode, mins[p], mins[prev]) || pqx_less(mode, maxs[p], maxs[prev])) up = false;
      if (pqx_less(mode, mins[prev], mins[p]) || pqx_less(mode, maxs[prev], maxs[p])) down = false;
    }
    prev = p;
  }
  Thrift t;
  t.open();
  t.list(1, Thrift::T_TRUE, n_pages);
  for (size_t p = 0; p < n_pages; p++) t.out.push_back(m->pages[p].count == 0 ? (char)Thrift::T_TRUE : (char)Thrift::T_FALSE);
  t.list(2, Thrift::T_BINARY, n_pages);
  for (size_t p = 0; p < n_pages; p++) t.str(mins[p]);
  t.list(3, Thrift::T_BINARY, n_pages);
  for (size_t p = 0; p < n_pages; p++) t.str(maxs[p]);
  t.i32(4, up ? 1 : down ? 2 : 0);  // BoundaryOrder: UNORDERED 0, ASCENDING 1, DESCENDING 2
  t.list(5, Thrift::T_I64, n_pages);
  for (size_t p = 0; p < n_pages; p++) t.zigzag((int64_t)m->pages[p].rows - (int64_t)m->pages[p].count);
  t.close();
  return t.out;
}

std::string pqx_offset_index(const ChunkMeta& m, int32_t page_rows) {
  Thrift t;
  t.open();
  t.list(1, Thrift::T_STRUCT, m.pages.size());
  for (size_t p = 0; p < m.pages.size(); p++) { t.open(); t.i64(1, (int64_t)m.pages[p].off); t.i32(2, (int32_t)m.pages[p].bytes); t.i64(3, (int64_t)p * page_rows); t.close(); }
  t.close();
  return t.out;
}

constexpr uint64_t kBytesMagic = 0x5051574259544553ull;
struct BytesHeader { uint64_t magic, pinned; unsigned char pad[48]; };
static_assert(sizeof(BytesHeader) == 64, "the returned bytes stay 64-byte aligned");

}  // namespace

uint8_t* pqw_alloc_bytes(size_t n, bool pinned) {
  unsigned char* p = nullptr;
#ifndef FDB_PQWRITE_HOST_ONLY
  if (pinned) {  // (no pinned memory to be had: the copy goes into pageable memory instead, slower and right)
    try { p = (unsigned char*)pinned_pool_alloc(n + sizeof(BytesHeader)); } catch (const Error&) { (void)hipGetLastError(); p = nullptr; }
  }
#else
  pinned = false;
#endif
  if (p == nullptr) { pinned = false; p = (unsigned char*)std::malloc(n + sizeof(BytesHeader)); }
  if (p == nullptr) throw std::bad_alloc();
  BytesHeader h;
  std::memset(&h, 0, sizeof(h));
  h.magic = kBytesMagic; h.pinned = pinned ? 1 : 0;
  std::memcpy(p, &h, sizeof(h));
  return p + sizeof(BytesHeader);
}

void pqw_free_bytes(uint8_t* bytes) {
  if (bytes == nullptr) return;
  unsigned char* p = bytes - sizeof(BytesHeader);
  BytesHeader h;
  std::memcpy(&h, p, sizeof(h));
  if (h.magic != kBytesMagic) return;  // (not ours: leave it alone rather than free a stranger's pointer)
  std::memset(p, 0, 8);
#ifndef FDB_PQWRITE_HOST_ONLY
  if (h.pinned) { pinned_pool_free(p); return; }
#endif
  std::free(p);
}

std::vector<PqwColumn> pqw_columns(const std::vector<PqwInput>& in, int64_t rows, const PqwSpec& spec, int32_t* page_rows) {
  const fdb_parquet_write_options* opt = spec.options;
  const int8_t *encodings = spec.encodings, *codecs = spec.codecs; const int32_t n_encodings = spec.n_encodings, n_codecs = spec.n_codecs;
  int64_t pr = opt != nullptr ? opt->page_rows : 0;
  if (pr == 0) pr = 65536;
  if (pr < 64 || pr > (1 << 24) || pr % 64 != 0)
    throw Error(FDB_ERR_INVALID, "parquet write: page_rows must be a multiple of 64 in [64, 2^24] (0: 65536), got " + std::to_string(pr));
  *page_rows = (int32_t)pr;
  if (rows < 0) throw Error(FDB_ERR_INVALID, "parquet write: negative row count");
  const int32_t n_opt = opt != nullptr ? opt->n_optional : 0;
  if (n_opt != 0 && (n_opt != (int32_t)in.size() || opt->optional == nullptr))
    throw Error(FDB_ERR_INVALID, "parquet write: `optional` has " + std::to_string(n_opt) + " entries, the record " + std::to_string(in.size()) + " columns");
  if (n_encodings != 0 && (n_encodings != (int32_t)in.size() || encodings == nullptr))
    throw Error(FDB_ERR_INVALID, "parquet write: `encodings` has " + std::to_string(n_encodings) + " entries, the record " + std::to_string(in.size()) + " columns");
  if (n_codecs != 0 && (n_codecs != (int32_t)in.size() || codecs == nullptr))
    throw Error(FDB_ERR_INVALID, "parquet write: `codecs` has " + std::to_string(n_codecs) + " entries, the record " + std::to_string(in.size()) + " columns");
  for (int32_t k = 0; k < n_codecs; k++)
    if (codecs[k] != 0 && codecs[k] != PQW_SNAPPY && codecs[k] != PQW_LZ4_RAW)
      throw Error(FDB_ERR_INVALID, "parquet write: codecs[" + std::to_string(k) + "] is " + std::to_string((int)codecs[k]) + " (0 UNCOMPRESSED, 1 SNAPPY, 7 LZ4_RAW)");
  int delta_slots = 0;
  std::vector<PqwColumn> cols;
  for (size_t k = 0; k < in.size(); k++) {
    const PqwInput& c = in[k];
    PqwColumn o;
    o.name = c.name;
    o.codec = n_codecs != 0 ? (int)codecs[k] : 0;
    switch (c.kind) {
      case ColKind::I64: o.pq_kind = FDB_PQW_V64; o.physical = PT_INT64; break;
      case ColKind::U64: o.pq_kind = FDB_PQW_V64; o.physical = PT_INT64; o.is_u64 = true; break;
      case ColKind::F64: o.pq_kind = FDB_PQW_V64; o.physical = PT_DOUBLE; break;
      case ColKind::BOOL: o.pq_kind = FDB_PQW_BOOL; o.physical = PT_BOOLEAN; o.width = 1; break;
      case ColKind::DICT: o.pq_kind = FDB_PQW_INDEX; o.physical = PT_BYTE_ARRAY; break;
      default: throw Error(FDB_ERR_UNSUPPORTED, "parquet write: column type " + c.format + " (" + c.name + ") is not one the writer knows");
    }
    if (c.values == nullptr && rows > 0)
      throw Error(FDB_ERR_UNSUPPORTED, "parquet write: column type " + c.format + " (" + c.name + ") is not held on the device");
    const int enc = n_encodings != 0 ? (int)encodings[k] : 0;
    if (enc < 0 || enc > 1) throw Error(FDB_ERR_INVALID, "parquet write: encodings[" + std::to_string(k) + "] is " + std::to_string(enc) + " (0 as ever, 1 DELTA_BINARY_PACKED)");
    if (enc == 1) {
      if (c.kind != ColKind::I64 && c.kind != ColKind::U64)
        throw Error(FDB_ERR_UNSUPPORTED, "parquet write: DELTA_BINARY_PACKED is for int64 / uint64 columns; column " + c.name + " is " + (c.format.empty() ? std::string("another kind") : c.format));
      o.delta_slot = delta_slots++;
    }
    if (c.kind == ColKind::DICT) {
      if (!c.dict) throw Error(FDB_ERR_INVALID, "parquet write: dictionary column without its dictionary: " + c.name);
      const uint64_t entries = c.dict->values.size();
      if (entries >= (1ull << 32)) throw Error(FDB_ERR_UNSUPPORTED, "parquet write: the dictionary of " + c.name + " has 2^32 entries or more");
      uint64_t page = 0;
      for (const std::string& v : c.dict->values) {
        if (v.size() > 0x7FFFFFFFull) { page = 1ull << 32; break; }
        page += 4 + v.size();
      }
      if (page > 0x7FFFFFFFull) throw Error(FDB_ERR_UNSUPPORTED, "parquet write: the dictionary page of " + c.name + " would pass 2^31 - 1 bytes");
      o.dict = c.dict.get();
      o.entries = entries;
      o.utf8 = c.dict->utf8();
      o.width = entries > 0 ? fdb_pqw_bits(entries - 1) : 0;
      if (entries == 0) o.pq_kind = PQW_NO_VALUES;  // every row is NULL (checked by the survey): PLAIN pages of zero values
    }
    const bool nulls = c.null_count > 0;
    const int want = n_opt != 0 ? (int)opt->optional[k] : -1;
    if (want < -1 || want > 1) throw Error(FDB_ERR_INVALID, "parquet write: optional[" + std::to_string(k) + "] is " + std::to_string(want) + " (-1 auto, 0 required, 1 optional)");
    if (want == 0 && nulls) throw Error(FDB_ERR_INVALID, "parquet write: column " + c.name + " is asked to be required and holds " + std::to_string(c.null_count) + " NULLs");
    if (nulls && c.validity == nullptr) throw Error(FDB_ERR_INVALID, "parquet write: column " + c.name + " counts NULLs and has no validity bitmap");
    o.optional = want < 0 ? (nulls || c.kind == ColKind::DICT) : want == 1;
    o.real = k;
    o.values = c.values;
    o.validity = nulls ? c.validity : nullptr;
    cols.push_back(std::move(o));
  }
  return cols;
}

// The indices as the record holds them, whether or not the column has a re-keyed copy by now.
static const void* pqw_raw(const PqwColumn& c) { return c.raw_values != nullptr ? c.raw_values : c.values; }

size_t pqw_delta_columns(const std::vector<PqwColumn>& cols) {
  size_t n = 0;
  for (const PqwColumn& c : cols) n += c.delta_slot >= 0;
  return n;
}

size_t pqr_streams(const std::vector<PqwColumn>& cols) {
  size_t n = 0;
  for (const PqwColumn& c : cols) n += (size_t)(c.run_values >= 0) + (size_t)(c.run_levels >= 0);
  return n;
}

size_t pqr_plan(const fdb_parquet_run_options* runs, std::vector<PqwColumn>* cols) {
  if (runs == nullptr) return 0;
  if (runs->n_columns != 0 && (runs->n_columns != (int32_t)cols->size() || runs->columns == nullptr))
    throw Error(FDB_ERR_INVALID, "parquet write: the run options' `columns` has " + std::to_string(runs->n_columns) + " entries, the record " + std::to_string(cols->size()) + " columns");
  for (int32_t k = 0; k < runs->n_columns; k++) {
    const int e = (int)runs->columns[k];
    if (e < 0 || e > 3) throw Error(FDB_ERR_INVALID, "parquet write: run options columns[" + std::to_string(k) + "] is " + std::to_string(e) + " (bit 0 dictionary indices, bit 1 definition levels)");
    const PqwColumn& c = (*cols)[(size_t)k];
    if ((e & 1) != 0 && c.pq_kind != FDB_PQW_INDEX && c.pq_kind != PQW_NO_VALUES)
      throw Error(FDB_ERR_UNSUPPORTED, "parquet write: runs of dictionary indices are for dictionary and string / binary columns; column " + c.name + " is not one");
  }
  int next = 0;
  for (int32_t k = 0; k < runs->n_columns; k++) {
    PqwColumn& c = (*cols)[(size_t)k];
    if ((runs->columns[k] & 1) != 0 && c.pq_kind == FDB_PQW_INDEX && c.width > 0) c.run_values = next++;
    if ((runs->columns[k] & 2) != 0 && c.optional && c.validity != nullptr) c.run_levels = next++;
  }
  return (size_t)next;
}

// ---- runs inside a page: the host's half of the run passes (fdb_pqruns.h) ------------------------------------------------------------------
std::string pqr_page_host(const uint32_t* sym, uint32_t n, uint32_t w) {
  const uint32_t G = n / 8, tail = n % 8, GG = fdb_pqw_groups(n), T = fdb_pqr_threshold(w);
  std::vector<uint32_t> key(G), cls(GG);
  for (uint32_t i = 0; i < G; i++) key[i] = fdb_pqr_group_key(sym + (size_t)i * 8, 8);
  for (uint32_t i = 0; i < G; i++) cls[i] = fdb_pqr_class(key.data(), (int32_t)i, 0, (int32_t)G, T);
  if (tail > 0) cls[G] = fdb_pqr_tail_class(fdb_pqr_group_key(sym + (size_t)G * 8, tail), G > 0, G > 0 ? cls[G - 1] : FDB_PQR_MIXED);
  std::string s;
  for (uint32_t i = 0; i < GG;) {
    uint32_t e = i + 1;
    while (e < GG && cls[e] == cls[i]) e++;
    const uint32_t groups = e - i, symbols = (e * 8 < n ? e * 8 : n) - i * 8;
    const uint32_t head = cls[i] == FDB_PQR_MIXED ? fdb_pqr_packed_header(groups) : fdb_pqr_rle_header(symbols);
    for (uint32_t b = 0; b < fdb_pqr_varint_len(head); b++) s.push_back((char)fdb_pqr_varint_byte(head, b));
    if (cls[i] != FDB_PQR_MIXED) {
      for (uint32_t b = 0; b < fdb_pqr_value_bytes(w); b++) s.push_back((char)(cls[i] >> (8 * b)));
    } else {
      for (uint32_t q = i; q < e; q++) {
        uint32_t grp[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        for (uint32_t k = 0; k < 8 && (size_t)q * 8 + k < n; k++) grp[k] = sym[(size_t)q * 8 + k];
        for (uint32_t b = 0; b < w; b++) s.push_back((char)fdb_pqr_group_byte(grp, w, b));
      }
    }
    i = e;
  }
  return s;
}

void pqr_survey_host(const std::vector<PqwColumn>& cols, const FdbPqwGeom& g, const std::vector<FdbPqwPageStat>& stats, PqrHost* r) {
  const size_t n_streams = pqr_streams(cols);
  r->payload.assign(n_streams * (size_t)g.n_pages, std::string());
  r->page_bytes.assign(n_streams * (size_t)g.n_pages, 0);
  std::vector<uint32_t> sym;
  for (size_t k = 0; k < cols.size(); k++) {
    const PqwColumn& c = cols[k];
    for (int pass = 0; pass < 2; pass++) {
      const bool levels = pass == 1;
      const int slot = levels ? c.run_levels : c.run_values;
      if (slot < 0) continue;
      const uint32_t w = levels ? 1u : c.width, mask = w >= 32 ? 0xFFFFFFFFu : ((1u << w) - 1);
      for (int64_t p = 0; p < g.n_pages; p++) {
        const FdbPqwPageStat& s = stats[k * (size_t)g.n_pages + (size_t)p];
        const int64_t first = fdb_pqw_page_first(g, p), end = fdb_pqw_page_end(g, p);
        if (!fdb_pqr_active(levels, s.count, (uint32_t)(end - first), s.mn, s.mx)) continue;
        sym.clear();
        for (int64_t row = first; row < end; row++) {  // the stream's symbols: every row's validity bit, or the non-NULL rows' indices in order
          const bool valid = c.validity == nullptr || ((c.validity[row >> 3] >> (row & 7)) & 1);
          if (levels) sym.push_back(valid ? 1u : 0u);
          else if (valid) sym.push_back(((const uint32_t*)c.values)[row] & mask);
        }
        const size_t at = (size_t)slot * (size_t)g.n_pages + (size_t)p;
        r->payload[at] = pqr_page_host(sym.data(), (uint32_t)sym.size(), w);
        r->page_bytes[at] = (uint32_t)r->payload[at].size();
      }
    }
  }
}

void pqr_encode_host(const PqrHost& r, const std::vector<uint64_t>& run_out, unsigned char* image) {
  for (size_t i = 0; i < r.payload.size(); i++)
    if (run_out[i] != FDB_PQW_NONE && !r.payload[i].empty()) std::memcpy(image + run_out[i], r.payload[i].data(), r.payload[i].size());
}

FdbPqwGeom pqw_geometry(int64_t rows, int32_t page_rows, size_t n_cols) {
  FdbPqwGeom g;
  g.rows = rows; g.page_rows = page_rows; g.n_pages = fdb_pqw_pages(rows, page_rows); g.tiles_per_page = fdb_pqw_tiles_per_page(page_rows);
  g.n_cols = (int32_t)n_cols; g.pad = 0;
  return g;
}

void PqwLayout::put(uint64_t off, const std::string& s) {
  if (s.empty()) return;
  pieces.push_back(Piece{off, blob.size(), s.size()});
  blob += s;
}

void PqwLayout::put_body(uint64_t off, const std::string& s) {
  if (s.empty()) return;
  body_pieces.push_back(Piece{off, body_blob.size(), s.size()});
  body_blob += s;
}

size_t pqw_compressed_columns(const std::vector<PqwColumn>& cols) {
  size_t n = 0;
  for (const PqwColumn& c : cols) n += c.codec != 0;
  return n;
}

PqxIndex pqx_plan(const fdb_parquet_index_options* index, size_t n_cols) {
  PqxIndex x;
  if (index == nullptr) return x;
  if (index->statistics < 0 || index->statistics > 2)
    throw Error(FDB_ERR_INVALID, "parquet write: statistics is " + std::to_string(index->statistics) + " (0 none, 1 chunk bounds, 2 chunk bounds and the page index)");
  if (index->index_size_limit < 0 || index->index_size_limit > 65536)
    throw Error(FDB_ERR_INVALID, "parquet write: index_size_limit is " + std::to_string(index->index_size_limit) + " (0: 16, else 1 to 65536)");
  if (index->n_sorting_columns < 0 || (index->n_sorting_columns > 0 && index->sorting_columns == nullptr))
    throw Error(FDB_ERR_INVALID, "parquet write: `sorting_columns` has " + std::to_string(index->n_sorting_columns) + " entries" + (index->n_sorting_columns > 0 ? " and no array" : ""));
  std::vector<bool> seen(n_cols, false);
  for (int32_t i = 0; i < index->n_sorting_columns; i++) {
    const fdb_parquet_sorting_column& sc = index->sorting_columns[i];
    if (sc.column < 0 || (size_t)sc.column >= n_cols)
      throw Error(FDB_ERR_INVALID, "parquet write: sorting column " + std::to_string(sc.column) + " is outside the record's " + std::to_string(n_cols) + " columns");
    if (seen[(size_t)sc.column]) throw Error(FDB_ERR_INVALID, "parquet write: sorting column " + std::to_string(sc.column) + " is named twice");
    seen[(size_t)sc.column] = true;
    x.sorting.push_back(sc);
  }
  x.statistics = index->statistics;
  x.limit = index->index_size_limit == 0 ? 16u : (uint32_t)index->index_size_limit;
  return x;
}

// modes, ranks and entry_of_rank of the columns (statistics > 0).
static void pqx_prepare(const std::vector<PqwColumn>& cols, PqxIndex* x) {
  x->modes.assign(cols.size(), FDB_PQX_U64);
  x->ranks.assign(cols.size(), std::vector<uint32_t>());
  x->entry_of_rank.assign(cols.size(), std::vector<uint32_t>());
  for (size_t k = 0; k < cols.size(); k++) {
    const PqwColumn& c = cols[k];
    if (c.pq_kind == FDB_PQW_BOOL) x->modes[k] = FDB_PQX_BOOL;
    else if (c.pq_kind == FDB_PQW_V64) x->modes[k] = c.physical == PT_DOUBLE ? FDB_PQX_F64 : c.is_u64 ? FDB_PQX_U64 : FDB_PQX_I64;
    else {
      x->modes[k] = FDB_PQX_INDEX;
      if (c.dict == nullptr || c.entries == 0) continue;  // (all NULL over an empty dictionary: no rank, no value that counts)
      uint32_t distinct = 0;
      x->ranks[k] = dense_ranks(*c.dict, &distinct);
      x->entry_of_rank[k].assign(distinct, 0);
      for (size_t i = x->ranks[k].size(); i-- > 0;) x->entry_of_rank[k][x->ranks[k][i]] = (uint32_t)i;  // (the first entry of equal ones: the same bytes)
    }
  }
}

void pqx_minmax_host(const std::vector<PqwColumn>& cols, const FdbPqwGeom& g, PqxIndex* x) {
  const size_t items = cols.size() * (size_t)g.n_pages;
  x->table.assign(2 * items, FDB_PQX_EMPTY_MAX);
  std::fill(x->table.begin(), x->table.begin() + (std::ptrdiff_t)items, FDB_PQX_EMPTY_MIN);
  for (size_t k = 0; k < cols.size(); k++) {
    const PqwColumn& c = cols[k];
    const int mode = x->modes[k];
    const std::vector<uint32_t>& ranks = x->ranks[c.real];
    const uint32_t per = mode == FDB_PQX_INDEX ? FDB_PQX_UNIT_INDEX : FDB_PQX_UNIT_V64, rank_len = (uint32_t)ranks.size();
    for (int64_t p = g.n_pages; p-- > 0;) {
      for (int32_t t = g.tiles_per_page; t-- > 0;) {
        int64_t first, end;
        fdb_pqw_tile_rows(g, p, t, &first, &end);
        if (first >= end) continue;
        uint64_t mn = FDB_PQX_EMPTY_MIN, mx = FDB_PQX_EMPTY_MAX, key;
        for (uint32_t u = 0; (int64_t)u * per < end - first; u++) {
          const uint32_t bits = fdb_pqx_unit_bits(c.validity, first, end, u, per);
          for (uint32_t i = 0; i < per; i++) {
            if (!((bits >> i) & 1)) continue;
            const size_t row = (size_t)first + (size_t)u * per + i;
            bool counts;
            if (mode == FDB_PQX_INDEX) counts = fdb_pqx_index_key(ranks.data(), rank_len, ((const uint32_t*)pqw_raw(c))[row], &key);
            else { uint64_t v; std::memcpy(&v, (const unsigned char*)c.values + row * 8, 8); counts = fdb_pqx_key(mode, v, &key); }
            if (counts) fdb_pqx_fold(key, &mn, &mx);
          }
        }
        if (mn > mx) continue;  // (the tile issues nothing)
        uint64_t& smn = x->table[k * (size_t)g.n_pages + (size_t)p];
        uint64_t& smx = x->table[items + k * (size_t)g.n_pages + (size_t)p];
        smn = mn < smn ? mn : smn; smx = mx > smx ? mx : smx;
      }
    }
  }
}

// ---- bloom filters: the host's half of the insert pass (fdb_pqbloom.h) -------------------------------------------------------------------
PqbPlan pqb_plan(const fdb_parquet_bloom_options* bloom, const std::vector<PqwColumn>& cols) {
  PqbPlan b;
  if (bloom == nullptr) return b;
  if (bloom->n_columns != 0 && (bloom->n_columns != (int32_t)cols.size() || bloom->columns == nullptr))
    throw Error(FDB_ERR_INVALID, "parquet write: the bloom filter `columns` has " + std::to_string(bloom->n_columns) + " entries, the record " + std::to_string(cols.size()) + " columns");
  if (bloom->bits_per_value < 0 || bloom->bits_per_value > 64)
    throw Error(FDB_ERR_INVALID, "parquet write: bloom filter bits_per_value is " + std::to_string(bloom->bits_per_value) + " (0: " + std::to_string(FDB_PQB_DEFAULT_BITS) + ", else 1 to 64)");
  bool some = false;
  for (int32_t k = 0; k < bloom->n_columns; k++) {
    const int e = (int)bloom->columns[k];
    if (e < 0 || e > 1) throw Error(FDB_ERR_INVALID, "parquet write: bloom filter columns[" + std::to_string(k) + "] is " + std::to_string(e) + " (0 none, 1 a bloom filter)");
    if (e == 1 && cols[(size_t)k].pq_kind == FDB_PQW_BOOL) throw Error(FDB_ERR_UNSUPPORTED, "parquet write: a bloom filter is not written for a boolean column (" + cols[(size_t)k].name + ")");
    some = some || e == 1;
  }
  if (!some) return b;
  b.on.assign(bloom->columns, bloom->columns + bloom->n_columns);
  b.bits_per_value = fdb_pqb_bits_per_value(bloom->bits_per_value);
  return b;
}

static void pqb_prepare(const std::vector<PqwColumn>& cols, PqbPlan* b) {
  b->hashes.assign(cols.size(), std::vector<uint64_t>());
  for (size_t k = 0; k < cols.size() && b->any(); k++)
    if (b->on[k] != 0 && cols[k].pq_kind == FDB_PQW_INDEX && cols[k].dict != nullptr)
      b->hashes[k] = entry_hashes(*cols[k].dict, [](const unsigned char* p, size_t n) { return fdb_pqb_hash(p, n); });
}

// ---- used-entry dictionaries: the host's half of the present and remap passes (fdb_pqdict.h) ---------------------------------------------
void pqg_check(const fdb_parquet_group_options* groups, int64_t rows) {
  if (groups == nullptr) return;
  const int64_t R = groups->row_group_rows;
  if (R < 0 || R % 64 != 0) throw Error(FDB_ERR_INVALID, "parquet write: row_group_rows must be a multiple of 64 (0: one row group), got " + std::to_string(R));
  const int64_t n_groups = R > 0 && rows > 0 ? (rows - 1) / R + 1 : 1;
  if (n_groups > 32767)
    throw Error(FDB_ERR_INVALID, "parquet write: row_group_rows " + std::to_string(R) + " cuts " + std::to_string(rows) + " rows into " + std::to_string(n_groups) + " row groups, more than 32767 (RowGroup.ordinal is an i16)");
  if (groups->dictionaries < 0 || groups->dictionaries > 1)
    throw Error(FDB_ERR_INVALID, "parquet write: dictionaries is " + std::to_string(groups->dictionaries) + " (0 the whole dictionary, 1 the used entries only)");
  if (groups->pad != 0) throw Error(FDB_ERR_INVALID, "parquet write: the group options' pad is " + std::to_string(groups->pad) + " (0)");
}

PqgPlan pqg_plan(const fdb_parquet_group_options* groups, int64_t rows, std::vector<PqwColumn>* cols) {
  PqgPlan d;
  pqg_check(groups, rows);
  if (groups == nullptr) return d;
  uint64_t words = 0;
  for (size_t k = 0; k < cols->size() && groups->dictionaries == 1; k++) {
    PqwColumn& c = (*cols)[k];
    if (c.pq_kind != FDB_PQW_INDEX || c.form != 0) continue;  // (an empty dictionary has nothing to prune, a column with a form no dictionary page)
    c.used_slot = (int)d.cols.size();
    PqgPlan::Col o;
    o.col = k; o.entries = c.entries; o.word_off = words; o.words = fdb_pqg_words(c.entries);
    d.cols.push_back(o);
    words += o.words;
  }
  d.bits.assign((size_t)words, 0);
  return d;
}

void pqg_present_host(const std::vector<PqwColumn>& cols, const FdbPqwGeom& g, PqgPlan* d) {
  for (const PqgPlan::Col& o : d->cols) {
    const PqwColumn& c = cols[o.col];
    unsigned long long* bits = d->bits.data() + o.word_off;
    for (int64_t p = 0; p < g.n_pages; p++) {
      for (int32_t t = 0; t < g.tiles_per_page; t++) {
        int64_t first, end;
        fdb_pqw_tile_rows(g, p, t, &first, &end);
        for (uint32_t u = 0; (int64_t)u * FDB_PQX_UNIT_INDEX < end - first; u++) {
          const uint32_t unit = fdb_pqx_unit_bits(c.validity, first, end, u, FDB_PQX_UNIT_INDEX);
          for (uint32_t i = 0; i < FDB_PQX_UNIT_INDEX; i++) {
            if (!((unit >> i) & 1)) continue;
            const uint32_t v = ((const uint32_t*)c.values)[(size_t)first + (size_t)u * FDB_PQX_UNIT_INDEX + i];
            if (v < o.entries) bits[v >> 6] |= fdb_pqg_bit(v);  // (at or past: the survey's to refuse)
          }
        }
      }
    }
  }
}

void pqg_resolve(const std::vector<FdbPqwPageStat>& stats, const FdbPqwGeom& g, std::vector<PqwColumn>* cols, PqgPlan* d) {
  d->before.assign(d->bits.size(), 0);
  for (PqgPlan::Col& o : d->cols) {
    PqwColumn& c = (*cols)[o.col];
    for (int64_t p = 0; p < g.n_pages; p++) {
      const FdbPqwPageStat& s = stats[o.col * (size_t)g.n_pages + (size_t)p];
      if (s.count > 0 && (s.mn > s.mx || s.mx >= o.entries)) throw Error(FDB_ERR_INVALID, index_out_of_range(c, s.mx, o.entries));
    }
    const uint64_t spare = o.entries & 63;  // bits past the last entry: never set by a pass that works
    if (spare != 0 && (d->bits[(size_t)(o.word_off + o.words - 1)] >> spare) != 0) throw Error(FDB_ERR_STATE, "parquet write: the present pass names an entry past the dictionary of " + c.name);
    uint32_t used = 0;
    for (uint64_t w = 0; w < o.words; w++) { d->before[(size_t)(o.word_off + w)] = used; used += (uint32_t)fdb_pqw_popc(d->bits[(size_t)(o.word_off + w)]); }
    o.used = used;
    c.entries = used;
    c.width = used > 0 ? fdb_pqw_bits((uint64_t)used - 1) : 0;
    if (used == 0) c.pq_kind = PQW_NO_VALUES;  // every row is NULL: the form of an empty dictionary
  }
}

void pqg_remap_host(const std::vector<PqwColumn>& cols, const FdbPqwGeom& g, const PqgPlan& d, std::vector<std::vector<uint32_t>>* out) {
  out->assign(d.cols.size(), std::vector<uint32_t>());
  for (size_t slot = 0; slot < d.cols.size(); slot++) {
    const PqgPlan::Col& o = d.cols[slot];
    const PqwColumn& c = cols[o.col];
    const unsigned long long* bits = d.bits.data() + o.word_off;
    const uint32_t* before = d.before.data() + o.word_off;
    std::vector<uint32_t>& dst = (*out)[slot];
    dst.assign((size_t)g.rows + 8, 0);
    for (int64_t row = 0; row < g.rows; row++) {
      if (c.validity != nullptr && !((c.validity[row >> 3] >> (row & 7)) & 1)) continue;
      const uint32_t v = ((const uint32_t*)pqw_raw(c))[row];
      if (v < o.entries) dst[(size_t)row] = fdb_pqg_rank(bits, before, v);
    }
  }
}

// ---- value pages of BYTE_ARRAY columns: the host's half of the byte passes (fdb_pqbytes.h) ------------------------------------------------
size_t pqy_plan(const fdb_parquet_string_options* strings, const fdb_parquet_run_options* runs, std::vector<PqwColumn>* cols, PqyPlan* y) {
  if (strings == nullptr) return 0;
  if (strings->n_columns != 0 && (strings->n_columns != (int32_t)cols->size() || strings->forms == nullptr))
    throw Error(FDB_ERR_INVALID, "parquet write: the string options' `forms` has " + std::to_string(strings->n_columns) + " entries, the record " + std::to_string(cols->size()) + " columns");
  for (int32_t k = 0; k < strings->n_columns; k++) {
    const int e = (int)strings->forms[k];
    if (e < 0 || e > 2) throw Error(FDB_ERR_INVALID, "parquet write: string options forms[" + std::to_string(k) + "] is " + std::to_string(e) + " (0 as ever, 1 PLAIN, 2 DELTA_LENGTH_BYTE_ARRAY)");
  }
  if (strings->pad != 0) throw Error(FDB_ERR_INVALID, "parquet write: the string options' pad is " + std::to_string(strings->pad) + " (0)");
  for (int32_t k = 0; k < strings->n_columns; k++) {
    const PqwColumn& c = (*cols)[(size_t)k];
    if (strings->forms[k] == 0) continue;
    const char* form = strings->forms[k] == FDB_PQY_PLAIN ? "PLAIN" : "DELTA_LENGTH_BYTE_ARRAY";
    if (c.pq_kind != FDB_PQW_INDEX && c.pq_kind != PQW_NO_VALUES)
      throw Error(FDB_ERR_UNSUPPORTED, std::string("parquet write: ") + form + " value pages are for dictionary and string / binary columns; column " + c.name + " is not one");
    if (runs != nullptr && k < runs->n_columns && (runs->columns[k] & 1) != 0)
      throw Error(FDB_ERR_UNSUPPORTED, "parquet write: runs of dictionary indices are asked for column " + c.name + ", which is written " + form + " and has no index pages");
  }
  size_t next = 0, deltas = pqw_delta_columns(*cols);
  y->tables.assign(cols->size(), nullptr);
  for (int32_t k = 0; k < strings->n_columns; k++) {
    PqwColumn& c = (*cols)[(size_t)k];
    c.form = (int)strings->forms[k];
    if (c.form == 0) continue;
    if (c.pq_kind == PQW_NO_VALUES) {  // all NULL over an empty dictionary: PLAIN pages of zero values are its form already; pages of zero lengths are the host's
      if (c.form == FDB_PQY_PLAIN) c.form = 0;
      continue;
    }
    c.bytes_slot = (int)next++;
    if (c.form == FDB_PQY_DELTA_LENGTH) c.delta_slot = (int)deltas++;  // the lengths: one more column of the DELTA passes
    auto t = std::make_shared<PqyTables>();
    const std::vector<int32_t>& offsets = c.dict->arrow_offsets();  // (entries + 1; below 2^31: pqw_columns has held the dictionary to it)
    const std::string& bytes = c.dict->joined();                    // (both computed once per dictionary and kept with it: nothing is copied per call)
    t->off = (const uint32_t*)offsets.data(); t->bytes = (const unsigned char*)bytes.data(); t->n_bytes = bytes.size();
    y->tables[(size_t)k] = std::move(t);
  }
  return next;
}

void pqy_survey_host(const std::vector<PqwColumn>& cols, const FdbPqwGeom& g, size_t n_bytes_cols, PqyPlan* y) {
  y->tile_bytes.assign(n_bytes_cols * (size_t)g.n_pages * (size_t)g.tiles_per_page, 0);
  for (const PqwColumn& c : cols) {
    if (c.bytes_slot < 0) continue;
    const PqyTables& tb = *y->tables[c.real];
    for (int64_t p = 0; p < g.n_pages; p++) {
      for (int32_t t = 0; t < g.tiles_per_page; t++) {
        int64_t first, end;
        fdb_pqw_tile_rows(g, p, t, &first, &end);
        uint64_t sum = 0;
        for (int wi = 0; wi < FDB_PQW_TILE_WORDS && first < end; wi++) {
          const uint64_t w = fdb_pqw_valid_word(c.validity, first, wi, end);
          for (int b = 0; b < 64; b++)
            if ((w >> b) & 1) sum += fdb_pqy_value_bytes(fdb_pqy_entry_len(tb.off, (uint32_t)c.entries, ((const uint32_t*)c.values)[first + wi * 64 + b]), c.form == FDB_PQY_PLAIN);
        }
        y->tile_bytes[((size_t)c.bytes_slot * (size_t)g.n_pages + (size_t)p) * (size_t)g.tiles_per_page + (size_t)t] = sum;
      }
    }
  }
}

void pqy_scan(const FdbPqwGeom& g, size_t n_bytes_cols, PqyPlan* y) {
  const size_t pages = n_bytes_cols * (size_t)g.n_pages, tpp = (size_t)g.tiles_per_page;
  if (y->tile_bytes.size() != pages * tpp) throw Error(FDB_ERR_STATE, "parquet write: the byte survey's table does not match the record");
  y->page_bytes.assign(pages, 0);
  y->byte_base.assign(pages * tpp, 0);
  for (size_t cp = 0; cp < pages; cp++) {
    uint64_t run = 0;
    for (size_t t = 0; t < tpp; t++) { y->byte_base[cp * tpp + t] = run; run += y->tile_bytes[cp * tpp + t]; }
    y->page_bytes[cp] = run;
  }
}

void pqy_encode_host(const std::vector<PqwColumn>& cols, const FdbPqwGeom& g, const PqyPlan& y, const std::vector<uint64_t>& bytes_out, unsigned char* image) {
  std::vector<uint32_t> off(FDB_PQW_TILE + 1), idx(FDB_PQW_TILE);
  for (const PqwColumn& c : cols) {
    if (c.bytes_slot < 0) continue;
    const PqyTables& tb = *y.tables[c.real];
    const bool plain = c.form == FDB_PQY_PLAIN;
    for (int64_t p = 0; p < g.n_pages; p++) {
      const size_t cp = (size_t)c.bytes_slot * (size_t)g.n_pages + (size_t)p;
      if (bytes_out[cp] == FDB_PQW_NONE) continue;
      for (int32_t t = 0; t < g.tiles_per_page; t++) {
        int64_t first, end;
        fdb_pqw_tile_rows(g, p, t, &first, &end);
        if (first >= end) continue;
        uint32_t count = 0, total = 0;  // the tile's values by rank: entry and exclusive byte offset
        for (int wi = 0; wi < FDB_PQW_TILE_WORDS; wi++) {
          const uint64_t w = fdb_pqw_valid_word(c.validity, first, wi, end);
          for (int b = 0; b < 64; b++) {
            if (!((w >> b) & 1)) continue;
            const uint32_t e = ((const uint32_t*)c.values)[first + wi * 64 + b];
            idx[count] = e < c.entries ? e : 0u;
            off[count++] = total;
            total += fdb_pqy_value_bytes(fdb_pqy_entry_len(tb.off, (uint32_t)c.entries, e), plain);
          }
        }
        off[count] = total;
        if (total == 0) continue;
        const uint64_t dst = bytes_out[cp] + y.byte_base[cp * (size_t)g.tiles_per_page + (size_t)t];
        for (uint64_t k = fdb_pqy_first_word(dst); k <= fdb_pqy_last_word(dst, total); k++) {
          uint32_t mask, cur;
          const uint32_t word = fdb_pqy_word(off.data(), idx.data(), count, plain, tb.off, tb.bytes, dst, total, k, &mask);
          std::memcpy(&cur, image + k * 4, 4);
          cur = mask == 0xFFFFFFFFu ? word : cur | word;  // (stored, or OR-ed into the zeroed image: the kernel's two ways)
          std::memcpy(image + k * 4, &cur, 4);
        }
      }
    }
  }
}

PqwPlan pqw_plan(const std::vector<PqwInput>& in, int64_t rows, const PqwSpec& spec) {
  PqwPlan P;
  int32_t page_rows = 0;
  P.cols = pqw_columns(in, rows, spec, &page_rows);
  P.x = pqx_plan(spec.index, P.cols.size());
  P.bloom = pqb_plan(spec.bloom, P.cols);
  P.n_runs = pqr_plan(spec.runs, &P.cols);
  pqg_check(spec.groups, rows);  // (the group options' refusals come before the string options'; the plan below leaves a column with a form out)
  P.n_bytes = pqy_plan(spec.strings, spec.runs, &P.cols, &P.strings);
  P.dict = pqg_plan(spec.groups, rows, &P.cols);
  P.grouped = spec.groups != nullptr && (spec.groups->row_group_rows != 0 || spec.groups->dictionaries != 0);
  if (P.x.statistics > 0) pqx_prepare(P.cols, &P.x);
  if (P.bloom.any()) pqb_prepare(P.cols, &P.bloom);
  P.g = pqw_geometry(rows, page_rows, P.cols.size());
  P.n_delta = pqw_delta_columns(P.cols); P.n_compressed = pqw_compressed_columns(P.cols);
  P.n_real = P.cols.size(); P.file_rows = rows;
  return P;
}

// Groups [first, first + n) of R rows — the last of `rows` — as one plan over virtual columns: every table and slot is the part's own,
// the ranks and entry hashes stay the record's columns' (PqwColumn::real).
static PqwPlan pqw_part(const PqwPlan& P, const fdb_parquet_group_options* groups, int64_t first, int64_t n, int64_t R, int64_t rows) {
  PqwPlan A;
  A.x = P.x; A.x.modes.clear();
  A.bloom = P.bloom; A.bloom.on.clear();
  A.grouped = true; A.first_group = first; A.n_groups = n; A.n_real = P.n_real; A.file_rows = P.file_rows;
  A.strings.tables = P.strings.tables;
  int deltas = 0, runs = 0, streams = 0;
  for (int64_t gi = 0; gi < n; gi++) {
    const size_t at = (size_t)((first + gi) * R);
    for (size_t k = 0; k < P.cols.size(); k++) {
      PqwColumn c = P.cols[k];
      const bool index = c.pq_kind == FDB_PQW_INDEX || c.pq_kind == PQW_NO_VALUES;
      if (c.values != nullptr) c.values = (const unsigned char*)c.values + at * (index ? 4 : 8);  // (R is a multiple of 64: 256-byte steps)
      if (c.validity != nullptr) c.validity += at / 8;                                              // (… and whole validity words)
      if (c.delta_slot >= 0) c.delta_slot = deltas++;
      if (c.run_values >= 0) c.run_values = runs++;
      if (c.run_levels >= 0) c.run_levels = runs++;
      if (c.bytes_slot >= 0) c.bytes_slot = streams++;
      A.cols.push_back(std::move(c));
      if (!P.x.modes.empty()) A.x.modes.push_back(P.x.modes[k]);
      if (P.bloom.any()) A.bloom.on.push_back(P.bloom.on[k]);
    }
  }
  A.dict = pqg_plan(groups, rows, &A.cols);
  A.g = pqw_geometry(rows, P.g.page_rows, A.cols.size());
  A.n_delta = (size_t)deltas; A.n_runs = (size_t)runs; A.n_bytes = (size_t)streams; A.n_compressed = pqw_compressed_columns(A.cols);
  return A;
}

std::vector<PqwPlan> pqw_parts(PqwPlan&& plan, const PqwSpec& spec) {
  std::vector<PqwPlan> parts;
  const int64_t R = spec.groups != nullptr ? spec.groups->row_group_rows : 0, rows = plan.g.rows;
  if (R == 0 || rows <= R) { parts.push_back(std::move(plan)); return parts; }
  const int64_t full = rows / R, rest = rows % R;
  parts.push_back(pqw_part(plan, spec.groups, 0, full, R, R));
  if (rest > 0) parts.push_back(pqw_part(plan, spec.groups, full, 1, R, rest));
  return parts;
}

void pqb_size(const std::vector<PqwColumn>& cols, const FdbPqwGeom& g, const std::vector<FdbPqwPageStat>& stats, PqbPlan* b) {
  b->bytes.assign(cols.size(), 0);
  b->table_off.assign(cols.size(), 0);
  b->table_bytes = 0;
  for (size_t k = 0; k < cols.size() && b->any(); k++) {
    if (b->on[k] == 0) continue;
    uint64_t n = 0;
    for (int64_t p = 0; p < g.n_pages; p++) n += stats[k * (size_t)g.n_pages + (size_t)p].count;
    if (cols[k].pq_kind == FDB_PQW_INDEX || cols[k].pq_kind == PQW_NO_VALUES) n = std::min<uint64_t>(n, cols[k].entries);
    b->bytes[k] = fdb_pqb_bytes(n, b->bits_per_value);
    b->table_off[k] = b->table_bytes;
    b->table_bytes += b->bytes[k];  // (a multiple of 32)
  }
}

void pqb_insert_host(const std::vector<PqwColumn>& cols, const FdbPqwGeom& g, const PqbPlan& b, unsigned char* table) {
  for (size_t k = 0; k < cols.size() && b.any(); k++) {
    if (b.on[k] == 0) continue;
    const PqwColumn& c = cols[k];
    const bool index = c.pq_kind != FDB_PQW_V64;
    const std::vector<uint64_t>& hashes = b.hashes[c.real];
    const uint32_t per = index ? FDB_PQX_UNIT_INDEX : FDB_PQX_UNIT_V64, n_blocks = b.bytes[k] / FDB_PQB_BLOCK_BYTES;
    unsigned char* bits = table + b.table_off[k];
    for (int64_t p = 0; p < g.n_pages; p++) {
      for (int32_t t = 0; t < g.tiles_per_page; t++) {
        int64_t first, end;
        fdb_pqw_tile_rows(g, p, t, &first, &end);
        for (uint32_t u = 0; (int64_t)u * per < end - first; u++) {
          const uint32_t unit = fdb_pqx_unit_bits(c.validity, first, end, u, per);
          for (uint32_t i = 0; i < per; i++) {
            if (!((unit >> i) & 1)) continue;
            const size_t row = (size_t)first + (size_t)u * per + i;
            uint64_t h;
            if (index) {
              const uint32_t v = ((const uint32_t*)pqw_raw(c))[row];
              if (v >= hashes.size()) continue;  // (the survey's to refuse)
              h = hashes[v];
            } else { uint64_t v; std::memcpy(&v, (const unsigned char*)c.values + row * 8, 8); h = fdb_pqb_hash8(v); }
            unsigned char* blk = bits + (size_t)fdb_pqb_block(h, n_blocks) * FDB_PQB_BLOCK_BYTES;
            for (int q = 0; q < 4; q++) { uint64_t w; std::memcpy(&w, blk + q * 8, 8); w |= fdb_pqb_pair_mask(h, q); std::memcpy(blk + q * 8, &w, 8); }
          }
        }
      }
    }
  }
}

// The elements of every fragment of a body, by the host walk of fdb_pqsnappy.h: a Snappy block without its preamble.
static std::string pqs_elements_host(const unsigned char* body, size_t n) {
  std::string elements;
  std::vector<uint32_t> table(FDB_PQS_TABLE);
  std::vector<unsigned char> out(fdb_pqs_slot_bytes());
  for (size_t at = 0; at < n; at += FDB_PQS_FRAGMENT) {
    const uint32_t len = (uint32_t)std::min<size_t>(FDB_PQS_FRAGMENT, n - at);
    elements.append((const char*)out.data(), fdb_pqs_compress_fragment_host(body + at, len, table.data(), out.data()));
  }
  return elements;
}
std::string pqs_block_host(const unsigned char* body, size_t n) { return varint_bytes(n) + pqs_elements_host(body, n); }
std::string pql_block_host(const unsigned char* body, size_t n) {
  std::vector<uint32_t> table(FDB_PQS_TABLE);
  std::vector<unsigned char> mid(fdb_pql_slot_bytes());
  std::string block((size_t)fdb_pql_bound(n), '\0');
  block.resize((size_t)fdb_pql_block_host(body, n, table.data(), mid.data(), (unsigned char*)&block[0]));
  return block;
}

PqwLayout pqw_layout(const PqwPlan& plan, const PqwSizes& sizes) { return pqw_layout(std::vector<const PqwPlan*>{&plan}, std::vector<PqwSizes>{sizes}); }

PqwLayout pqw_layout(const std::vector<const PqwPlan*>& parts, const std::vector<PqwSizes>& part_sizes) {
  static const std::vector<uint32_t> no_table;
  if (parts.empty() || parts.size() != part_sizes.size()) throw Error(FDB_ERR_STATE, "parquet write: the layout's tables do not match its parts");
  size_t n_compressed = 0, compressed_pages = 0, next_compressed = 0;
  for (const PqwPlan* part : parts) { n_compressed += part->n_compressed; compressed_pages += part->n_compressed * (size_t)part->g.n_pages; }
  const std::vector<uint32_t>* page_elements = part_sizes[0].page_elements;
  const bool final_form = page_elements != nullptr;  // else: every page as it is before compression — the file of a record without codecs, the staging image of one with
  const bool own = final_form || n_compressed == 0;  // the file's own layout: a compressed file's index and filters belong to the final one
  if (page_elements != nullptr && page_elements->size() != compressed_pages) throw Error(FDB_ERR_STATE, "parquet write: the table of compressed page sizes does not match the record");
  PqwLayout L;
  L.parts.resize(parts.size());
  uint64_t cur = 0;
  L.put(cur, "PAR1");
  cur += 4;
  std::vector<ChunkMeta> chunks;       // in file order: part after part, and in a part group after group, column after column
  std::vector<size_t> chunk_base;      // per part: its first chunk
  std::vector<int64_t> group_rows;
  for (size_t pi = 0; pi < parts.size(); pi++) {
  const PqwPlan& plan = *parts[pi]; const PqwSizes& sizes = part_sizes[pi];
  PqwLayout::Part& LP = L.parts[pi];
  chunk_base.push_back(chunks.size());
  chunks.resize(chunks.size() + plan.cols.size());
  for (int64_t gi = 0; gi < plan.n_groups; gi++) group_rows.push_back(plan.g.rows);
  const std::vector<PqwColumn>& cols = plan.cols; const FdbPqwGeom& g = plan.g; const std::vector<FdbPqwPageStat>& stats = sizes.stats;
  const std::vector<uint32_t>& delta_bytes = sizes.delta_bytes != nullptr ? *sizes.delta_bytes : no_table;
  const std::vector<uint32_t>* run_bytes = sizes.run_bytes;
  const PqxIndex* x = own && plan.x.any() ? &plan.x : nullptr;
  const PqbPlan* bloom = own && plan.bloom.any() ? &plan.bloom : nullptr;
  if (bloom != nullptr && bloom->bytes.size() != cols.size()) throw Error(FDB_ERR_STATE, "parquet write: the bloom filter sizes do not match the record");
  const bool bounds = x != nullptr && x->statistics > 0;
  if (bounds && (x->table.size() != 2 * stats.size() || x->modes.size() != cols.size())) throw Error(FDB_ERR_STATE, "parquet write: the min / max table does not match the record");
  if (stats.size() != cols.size() * (size_t)g.n_pages) throw Error(FDB_ERR_STATE, "parquet write: the survey table does not match the record");
  if (delta_bytes.size() != plan.n_delta * (size_t)g.n_pages) throw Error(FDB_ERR_STATE, "parquet write: the table of DELTA page sizes does not match the record");
  if ((sizes.stream_bytes != nullptr ? sizes.stream_bytes->size() : 0) != plan.n_bytes * (size_t)g.n_pages) throw Error(FDB_ERR_STATE, "parquet write: the table of byte stream sizes does not match the record");
  const size_t n_run_streams = plan.n_runs;
  if ((run_bytes != nullptr ? run_bytes->size() : 0) != n_run_streams * (size_t)g.n_pages) throw Error(FDB_ERR_STATE, "parquet write: the table of run-encoded sizes does not match the record");
  // The bytes of a page's stream cut into runs, held to the rule's bounds: no more than its one bit-packed run, no less than a run.
  const auto run_payload = [&](const PqwColumn& c, int slot, int64_t p, uint32_t n, uint32_t w) {
    const uint32_t bytes = (*run_bytes)[(size_t)slot * (size_t)g.n_pages + (size_t)p];
    if (bytes > fdb_pqr_max_bytes(n, w) || bytes < fdb_pqr_min_bytes(w))
      throw Error(FDB_ERR_STATE, "parquet write: the run survey sizes a stream of " + std::to_string(n) + " symbols of " + std::to_string(w) + " bits at " + std::to_string(bytes) + " bytes (" + c.name + ")");
    return (uint64_t)bytes;
  };
  LP.delta_out.assign(delta_bytes.size(), FDB_PQW_NONE);
  LP.out.assign(stats.size(), FdbPqwPageOut{FDB_PQW_NONE, FDB_PQW_NONE});
  LP.run_out.assign(n_run_streams * (size_t)g.n_pages, FDB_PQW_NONE);
  LP.bytes_out.assign(plan.n_bytes * (size_t)g.n_pages, FDB_PQW_NONE);
  for (size_t k = 0; k < cols.size(); k++) {
    const PqwColumn& c = cols[k];
    ChunkMeta& m = chunks[chunk_base[pi] + k];
    const uint64_t chunk_start = cur;
    m.col = &c; m.start = (int64_t)chunk_start; m.rows = g.rows;
    const bool squeeze = final_form && c.codec != 0;  // this chunk's pages are written as Snappy or LZ4 blocks
    const bool lz4 = c.codec == PQW_LZ4_RAW;
    const unsigned long long* used = c.used_slot >= 0 ? plan.dict.bits.data() + plan.dict.cols[(size_t)c.used_slot].word_off : nullptr;  // the chunk's presence bitmap
    if (used != nullptr && plan.dict.before.size() != plan.dict.bits.size()) throw Error(FDB_ERR_STATE, "parquet write: the used entries of " + c.name + " have not been counted");
    if (c.pq_kind == FDB_PQW_INDEX && c.form == 0) {
      const std::string body = used != nullptr ? dictionary_body(*c.dict, used) : dictionary_body(*c.dict);
      const std::string stored = !squeeze ? std::string() : lz4 ? pql_block_host((const unsigned char*)body.data(), body.size()) : pqs_block_host((const unsigned char*)body.data(), body.size());  // (host bytes already: the header's walk)
      const std::string hdr = page_header(PAGE_DICTIONARY, (int64_t)body.size(), (int64_t)(squeeze ? stored.size() : body.size()), (int64_t)c.entries, ENC_PLAIN);
      m.dict_off = (int64_t)cur;
      m.raw_bytes += (int64_t)(hdr.size() + body.size());
      L.put(cur, hdr); cur += hdr.size();
      L.put(cur, squeeze ? stored : body); cur += squeeze ? stored.size() : body.size();
    }
    m.data_off = (int64_t)cur;
    int64_t valid = 0;
    for (int64_t p = 0; p < g.n_pages; p++) {
      const FdbPqwPageStat& s = stats[k * (size_t)g.n_pages + (size_t)p];
      const uint32_t n = (uint32_t)(fdb_pqw_page_end(g, p) - fdb_pqw_page_first(g, p)), cnt = s.count;
      if (cnt > n || (c.validity == nullptr && cnt != n)) throw Error(FDB_ERR_STATE, "parquet write: the survey counts " + std::to_string(cnt) + " values in a page of " + std::to_string(n) + " rows (" + c.name + ")");
      if (c.pq_kind == PQW_NO_VALUES && cnt != 0) throw Error(FDB_ERR_INVALID, "parquet write: column " + c.name + " has values and an empty dictionary");
      valid += cnt;
      std::string pre, vpre;
      uint64_t level_payload = 0, value_payload = 0;
      const bool level_runs = c.run_levels >= 0 && fdb_pqr_active(true, cnt, n, s.mn, s.mx), value_runs = c.run_values >= 0 && fdb_pqr_active(false, cnt, n, s.mn, s.mx);
      if (c.optional) {
        if (cnt == n || cnt == 0) {
          const std::string run = varint_bytes((uint64_t)n << 1) + std::string(1, cnt == n ? '\1' : '\0');
          pre = le32((uint32_t)run.size()) + run;
        } else if (level_runs) {  // the runs, headers and all, are the device's
          level_payload = run_payload(c, c.run_levels, p, n, 1);
          pre = le32((uint32_t)level_payload);
        } else {
          level_payload = fdb_pqw_level_bytes(n);
          const std::string run = varint_bytes(((uint64_t)fdb_pqw_level_bytes(n) << 1) | 1);
          pre = le32((uint32_t)(run.size() + level_payload)) + run;
        }
      }
      int encoding = ENC_PLAIN;
      uint64_t stream_payload = 0;  // a column with a form: the page's byte stream, which follows the DELTA lengths, if any
      if (c.form != 0) {  // the values themselves: PLAIN, or their lengths as a DELTA page and then their bytes (fdb_pqbytes.h)
        encoding = c.form == FDB_PQY_DELTA_LENGTH ? ENC_DELTA_LENGTH_BYTE_ARRAY : ENC_PLAIN;
        if (c.bytes_slot < 0) vpre = std::string("\x80\x01\x04\x00\x00", 5);  // (all NULL over an empty dictionary: the header of zero lengths)
        else {
          if (cnt > 0 && (s.mn > s.mx || s.mx >= c.entries)) throw Error(FDB_ERR_INVALID, index_out_of_range(c, s.mx, c.entries));
          stream_payload = (*sizes.stream_bytes)[(size_t)c.bytes_slot * (size_t)g.n_pages + (size_t)p];
          if (c.form == FDB_PQY_DELTA_LENGTH) {
            value_payload = delta_bytes[(size_t)c.delta_slot * (size_t)g.n_pages + (size_t)p];
            if (value_payload < 5 || value_payload > fdb_pqd_max_page_bytes(cnt) || (cnt <= 1 && value_payload > FDB_PQD_MAX_HEADER))
              throw Error(FDB_ERR_STATE, "parquet write: the block survey sizes the lengths of " + std::to_string(cnt) + " values at " + std::to_string(value_payload) + " bytes (" + c.name + ")");
          }
          // (a value is at most 2^31 - 1 bytes and a page 2^24 rows: no sum here wraps)
          if (stream_payload < (c.form == FDB_PQY_PLAIN ? 4ull * cnt : 0ull) || pre.size() + level_payload + value_payload + stream_payload > 0x7FFFFFFFull)
            throw Error(FDB_ERR_INVALID, "parquet write: page " + std::to_string(p) + " of column " + c.name + " would hold " + std::to_string(pre.size() + level_payload + value_payload + stream_payload) +
                        " bytes, more than the 2^31 - 1 a page header can say; write fewer rows a page (page_rows)");
        }
      } else if (c.delta_slot >= 0) {
        encoding = ENC_DELTA_BINARY_PACKED;
        value_payload = delta_bytes[(size_t)c.delta_slot * (size_t)g.n_pages + (size_t)p];
        // (the smallest page is 80 01 04 + a count byte + a first-value byte; the first value's length is the device's to know)
        if (value_payload < 5 || value_payload > fdb_pqd_max_page_bytes(cnt) || (cnt <= 1 && value_payload > FDB_PQD_MAX_HEADER))
          throw Error(FDB_ERR_STATE, "parquet write: the block survey sizes a DELTA page of " + std::to_string(cnt) + " values at " + std::to_string(value_payload) + " bytes (" + c.name + ")");
      } else if (c.pq_kind == FDB_PQW_V64) value_payload = (uint64_t)cnt * 8;
      else if (c.pq_kind == FDB_PQW_BOOL) value_payload = fdb_pqw_packed_bytes(cnt, 1);
      else if (c.pq_kind == FDB_PQW_INDEX) {
        encoding = ENC_RLE_DICTIONARY;
        vpre = std::string(1, (char)c.width);
        if (cnt > 0) {
          if (s.mn > s.mx || (used == nullptr && s.mx >= c.entries))  // (a pruned column's range: pqg_resolve has looked)
            throw Error(FDB_ERR_INVALID, index_out_of_range(c, s.mx, c.entries));
          if (s.mn == s.mx) {  // one RLE run: the count, the value — of a pruned dictionary the entry's rank — in ⌈w/8⌉ bytes
            const uint32_t value = used != nullptr ? fdb_pqg_rank(used, plan.dict.before.data() + plan.dict.cols[(size_t)c.used_slot].word_off, s.mn) : s.mn;
            vpre += varint_bytes((uint64_t)cnt << 1);
            for (uint32_t b = 0; b < (c.width + 7) / 8; b++) vpre.push_back((char)(value >> (8 * b)));
          } else if (value_runs) {
            value_payload = run_payload(c, c.run_values, p, cnt, c.width);
          } else {
            vpre += varint_bytes(((uint64_t)fdb_pqw_groups(cnt) << 1) | 1);
            value_payload = fdb_pqw_packed_bytes(cnt, c.width);
          }
        }
      }
      const uint64_t body = pre.size() + level_payload + vpre.size() + value_payload + stream_payload;
      if (squeeze) {  // header, the block's preamble (SNAPPY; an LZ4_RAW block is bare), then what the compressor made of the body
        const uint64_t elements = (*page_elements)[next_compressed++];
        if (lz4 ? elements < 1 || elements > fdb_pql_bound(body) : elements > (uint64_t)fdb_pqs_fragments(body) * fdb_pqs_bound(FDB_PQS_FRAGMENT) || (body > 0) != (elements > 0))
          throw Error(FDB_ERR_STATE, "parquet write: the compressor sizes a page body of " + std::to_string(body) + " bytes at " + std::to_string(elements) + " (" + c.name + ")");
        const std::string preamble = lz4 ? std::string() : varint_bytes(body);
        const std::string hdr = page_header(PAGE_DATA, (int64_t)body, (int64_t)(preamble.size() + elements), n, encoding);
        m.raw_bytes += (int64_t)(hdr.size() + body);
        if (bounds) m.pages.push_back(PageLoc{cur, hdr.size() + preamble.size() + elements, n, cnt});
        L.put(cur, hdr + preamble); cur += hdr.size() + preamble.size();
        L.pages.push_back(PqwLayout::Page{cur, body, c.codec});
        cur += elements;
        continue;
      }
      const std::string hdr = page_header(PAGE_DATA, (int64_t)body, (int64_t)body, n, encoding);
      m.raw_bytes += (int64_t)(hdr.size() + body);
      if (bounds) m.pages.push_back(PageLoc{cur, hdr.size() + body, n, cnt});
      FdbPqwPageOut& o = LP.out[k * (size_t)g.n_pages + (size_t)p];
      if (c.codec == 0) { L.put(cur, hdr + pre); cur += hdr.size() + pre.size(); }
      else {  // the staging image of a page to be compressed: the host's bytes inside the body are placed on their own, before the compressor runs
        cur += hdr.size();
        L.pages.push_back(PqwLayout::Page{cur, body, c.codec});
        L.put_body(cur, pre); cur += pre.size();
      }
      if (level_runs) { LP.run_out[(size_t)c.run_levels * (size_t)g.n_pages + (size_t)p] = cur; cur += level_payload; }
      else if (level_payload > 0) { o.levels_off = cur; cur += level_payload; }
      if (c.codec == 0) L.put(cur, vpre); else L.put_body(cur, vpre);
      cur += vpre.size();
      if (value_runs && c.pq_kind == FDB_PQW_INDEX) { LP.run_out[(size_t)c.run_values * (size_t)g.n_pages + (size_t)p] = cur; cur += value_payload; }
      else if (c.delta_slot >= 0) { LP.delta_out[(size_t)c.delta_slot * (size_t)g.n_pages + (size_t)p] = cur; cur += value_payload; }  // (the encode pass leaves the values alone)
      else if (value_payload > 0) { o.values_off = cur; cur += value_payload; }
      if (stream_payload > 0) { LP.bytes_out[(size_t)c.bytes_slot * (size_t)g.n_pages + (size_t)p] = cur; cur += stream_payload; }  // (behind the lengths, if any)
    }
    m.bytes = (int64_t)(cur - chunk_start);
    m.nulls = g.rows - valid;
    L.chunk_off.push_back(chunk_start);
    L.chunk_len.push_back(cur - chunk_start);
    L.chunk_codec.push_back(c.codec);
  }
  }
  L.body_bytes = cur;
  const PqwPlan& head = *parts[0];
  const PqxIndex* x = own && head.x.any() ? &head.x : nullptr;
  const bool bounds = x != nullptr && x->statistics > 0;
  // after the last group's pages, in (group, column) order: header, bitset, no padding
  for (size_t pi = 0; pi < parts.size() && own && head.bloom.any(); pi++) {
    const PqbPlan& bloom = parts[pi]->bloom;
    for (size_t k = 0; k < parts[pi]->cols.size(); k++) {
      if (bloom.on[k] == 0) continue;
      ChunkMeta& m = chunks[chunk_base[pi] + k];
      unsigned char hdr[FDB_PQB_MAX_HEADER];
      const uint32_t len = fdb_pqb_header(bloom.bytes[k], hdr);
      m.bloom_off = (int64_t)cur; m.bloom_len = (int64_t)len + bloom.bytes[k];
      L.put(cur, std::string((const char*)hdr, len)); cur += len;
      L.blooms.push_back(PqwLayout::Bloom{pi, k, cur, bloom.bytes[k]}); cur += bloom.bytes[k];
    }
  }
  L.bloom_bytes = cur - L.body_bytes;
  // chunk bounds; with statistics == 2 every chunk's ColumnIndex, then every chunk's OffsetIndex, after the pages and the filters
  for (size_t pi = 0; pi < parts.size() && bounds; pi++) {
    for (size_t k = 0; k < parts[pi]->cols.size(); k++) {
      ChunkMeta& m = chunks[chunk_base[pi] + k];
      const std::string ci = pqx_column_index(parts[pi]->cols[k], parts[pi]->x, k, (size_t)parts[pi]->g.n_pages, &m);
      if (ci.empty()) continue;
      m.column_index_off = (int64_t)(cur + L.tail.size()); m.column_index_len = (int64_t)ci.size();
      L.tail += ci;
    }
  }
  for (size_t pi = 0; pi < parts.size() && bounds && x->statistics == 2; pi++) {
    for (size_t k = 0; k < parts[pi]->cols.size(); k++) {
      ChunkMeta& m = chunks[chunk_base[pi] + k];
      const std::string oi = pqx_offset_index(m, parts[pi]->g.page_rows);
      m.offset_index_off = (int64_t)(cur + L.tail.size()); m.offset_index_len = (int64_t)oi.size();
      L.tail += oi;
    }
  }
  L.footer = footer(chunks, head.n_real, group_rows, head.file_rows, x, head.grouped);
  return L;
}

void pqw_finish(const PqwLayout& L, uint8_t* file) {
  for (const PqwLayout::Piece& p : L.pieces) std::memcpy(file + p.off, L.blob.data() + p.pos, p.len);
  uint8_t* end = file + L.body_bytes + L.bloom_bytes;
  if (!L.tail.empty()) { std::memcpy(end, L.tail.data(), L.tail.size()); end += L.tail.size(); }  // the page index: the host's, after the image
  std::memcpy(end, L.footer.data(), L.footer.size());
  const uint32_t len = (uint32_t)L.footer.size();
  std::memcpy(end + L.footer.size(), &len, 4);
  std::memcpy(end + L.footer.size() + 4, "PAR1", 4);
}

// ---- the host walk: what the two kernels do, tile by tile, over host arrays ---------------------------------------------------------------
void pqw_survey_host(const std::vector<PqwColumn>& cols, const FdbPqwGeom& g, std::vector<FdbPqwPageStat>* stats, std::vector<uint32_t>* tile_base) {
  stats->assign(cols.size() * (size_t)g.n_pages, FdbPqwPageStat{0, 0, 0, 0});
  tile_base->assign(stats->size() * (size_t)g.tiles_per_page, 0);
  for (size_t k = 0; k < cols.size(); k++) {
    const PqwColumn& c = cols[k];
    for (int64_t p = 0; p < g.n_pages; p++) {
      const size_t item = k * (size_t)g.n_pages + (size_t)p;
      uint32_t run = 0, mn = 0xFFFFFFFFu, mx = 0;
      for (int32_t t = 0; t < g.tiles_per_page; t++) {
        (*tile_base)[item * (size_t)g.tiles_per_page + (size_t)t] = run;
        int64_t first, end;
        fdb_pqw_tile_rows(g, p, t, &first, &end);
        if (first >= end) continue;
        for (int wi = 0; wi < FDB_PQW_TILE_WORDS; wi++) {
          const uint64_t w = fdb_pqw_valid_word(c.validity, first, wi, end);
          run += (uint32_t)fdb_pqw_popc(w);
          if (c.pq_kind != FDB_PQW_INDEX && c.pq_kind != PQW_NO_VALUES) continue;
          for (int b = 0; b < 64; b++)
            if ((w >> b) & 1) { const uint32_t v = ((const uint32_t*)c.values)[first + wi * 64 + b]; mn = v < mn ? v : mn; mx = v > mx ? v : mx; }
        }
      }
      (*stats)[item] = FdbPqwPageStat{run, mn, mx, 0};
    }
  }
}

void pqw_encode_host(const std::vector<PqwColumn>& cols, const FdbPqwGeom& g, const std::vector<FdbPqwPageOut>& out, const std::vector<uint32_t>& tile_base,
                     unsigned char* image) {
  std::vector<uint32_t> vals(FDB_PQW_STAGE_WORDS, 0);
  const auto or_word = [&](uint64_t k, uint32_t word) { uint32_t cur; std::memcpy(&cur, image + k * 4, 4); cur |= word; std::memcpy(image + k * 4, &cur, 4); };
  for (size_t k = 0; k < cols.size(); k++) {
    const PqwColumn& c = cols[k];
    for (int64_t p = 0; p < g.n_pages; p++) {
      const size_t cp = k * (size_t)g.n_pages + (size_t)p;
      const FdbPqwPageOut po = out[cp];
      for (int32_t t = 0; t < g.tiles_per_page; t++) {
        int64_t first, end;
        fdb_pqw_tile_rows(g, p, t, &first, &end);
        if (first >= end) continue;
        if (po.levels_off == FDB_PQW_NONE && po.values_off == FDB_PQW_NONE) continue;
        const uint32_t n = (uint32_t)(end - first);
        uint64_t word[FDB_PQW_TILE_WORDS];
        uint32_t before[FDB_PQW_TILE_WORDS], count = 0;
        for (int wi = 0; wi < FDB_PQW_TILE_WORDS; wi++) { word[wi] = fdb_pqw_valid_word(c.validity, first, wi, end); before[wi] = count; count += (uint32_t)fdb_pqw_popc(word[wi]); }
        const uint64_t base = tile_base[cp * (size_t)g.tiles_per_page + (size_t)t];
        const bool packed = c.pq_kind != FDB_PQW_V64;
        if (po.levels_off != FDB_PQW_NONE) {
          const uint64_t at = po.levels_off + (uint64_t)((first - fdb_pqw_page_first(g, p)) >> 3);
          for (uint32_t i = 0; i < fdb_pqw_level_bytes(n); i++) {
            const unsigned char byte = (unsigned char)(word[i >> 3] >> (8 * (i & 7)));
            if (packed) or_word((at + i) >> 2, (uint32_t)byte << (8 * (uint32_t)((at + i) & 3)));
            else image[at + i] = byte;
          }
        }
        if (po.values_off == FDB_PQW_NONE || count == 0) continue;
        if (!packed) {
          for (uint32_t lr = 0; lr < n; lr++) {
            const uint64_t w = word[lr >> 6];
            if (!((w >> (lr & 63)) & 1)) continue;
            const uint64_t rank = base + before[lr >> 6] + (uint32_t)fdb_pqw_popc(w & ((1ull << (lr & 63)) - 1));
            std::memcpy(image + po.values_off + rank * 8, (const unsigned char*)c.values + (size_t)(first + lr) * 8, 8);
          }
        } else if (c.width > 0) {
          const uint32_t mask = c.width >= 32 ? 0xFFFFFFFFu : ((1u << c.width) - 1);
          for (uint32_t lr = 0; lr < n; lr++) {
            const uint64_t w = word[lr >> 6];
            if (!((w >> (lr & 63)) & 1)) continue;
            const uint32_t j = before[lr >> 6] + (uint32_t)fdb_pqw_popc(w & ((1ull << (lr & 63)) - 1));
            uint32_t v;
            if (c.pq_kind == FDB_PQW_BOOL) { int64_t b; std::memcpy(&b, (const unsigned char*)c.values + (size_t)(first + lr) * 8, 8); v = b >= 2; }
            else v = ((const uint32_t*)c.values)[first + lr];
            vals[fdb_pqw_slot(j)] = v & mask;
          }
          const uint64_t payload_bit = po.values_off * 8;
          const uint64_t k0 = fdb_pqw_first_word(payload_bit, base, c.width), k1 = fdb_pqw_last_word(payload_bit, base, count, c.width);
          for (uint64_t q = k0; q <= k1; q++) {
            const uint32_t wd = fdb_pqw_assemble_word(vals.data(), base, count, payload_bit, c.width, q);
            if (q == k0 || q == k1) or_word(q, wd);
            else std::memcpy(image + q * 4, &wd, 4);
          }
        }
      }
    }
  }
}

// ---- the DELTA passes over host arrays: compaction, block survey and page walk, then the encoder, block by block -------------------------
void pqd_survey_host(const std::vector<PqwColumn>& cols, const FdbPqwGeom& g, const std::vector<FdbPqwPageStat>& stats, const std::vector<uint32_t>& tile_base, PqdHost* d, const PqyPlan* y) {
  const size_t n_d = pqw_delta_columns(cols), bpp = (size_t)fdb_pqd_blocks_per_page(g.page_rows);
  d->dense.assign(n_d, std::vector<uint64_t>());
  d->blocks.assign(n_d * (size_t)g.n_pages * bpp, FdbPqdBlock{0, 0, 0, 0, 0});
  d->page_bytes.assign(n_d * (size_t)g.n_pages, 0);
  for (size_t k = 0; k < cols.size(); k++) {
    const PqwColumn& c = cols[k];
    if (c.delta_slot < 0) continue;
    const size_t slot = (size_t)c.delta_slot;
    const PqyTables* lengths_of = c.form != 0 ? y->tables[c.real].get() : nullptr;
    if (c.validity != nullptr || c.form != 0) {  // compaction, tile by tile: a value goes to the survey's rank of its tile + its rank inside the tile
      std::vector<uint64_t>& dense = d->dense[slot];
      dense.assign((size_t)g.rows, 0);
      for (int64_t p = 0; p < g.n_pages; p++) {
        for (int32_t t = 0; t < g.tiles_per_page; t++) {
          int64_t first, end;
          fdb_pqw_tile_rows(g, p, t, &first, &end);
          if (first >= end) continue;
          uint64_t* dst = dense.data() + fdb_pqw_page_first(g, p) + tile_base[(k * (size_t)g.n_pages + (size_t)p) * (size_t)g.tiles_per_page + (size_t)t];
          uint32_t before = 0;
          for (int wi = 0; wi < FDB_PQW_TILE_WORDS; wi++) {
            const uint64_t w = fdb_pqw_valid_word(c.validity, first, wi, end);
            for (int b = 0; b < 64; b++)
              if (!((w >> b) & 1)) continue;
              else if (c.form == 0) std::memcpy(dst + before + (uint32_t)fdb_pqw_popc(w & ((1ull << b) - 1)), (const unsigned char*)c.values + (size_t)(first + wi * 64 + b) * 8, 8);
              else  // DELTA_LENGTH: the value's length (the byte survey's other product) — in [0, 2^31), so the 64-bit rule packs what a 32-bit encoder would
                dst[before + (uint32_t)fdb_pqw_popc(w & ((1ull << b) - 1))] = fdb_pqy_entry_len(lengths_of->off, (uint32_t)c.entries, ((const uint32_t*)c.values)[first + wi * 64 + b]);
            before += (uint32_t)fdb_pqw_popc(w);
          }
        }
      }
    }
    const uint64_t* values = d->values(c);
    for (int64_t p = 0; p < g.n_pages; p++) {
      const size_t cp = slot * (size_t)g.n_pages + (size_t)p;
      const uint32_t count = stats[k * (size_t)g.n_pages + (size_t)p].count, deltas = fdb_pqd_deltas(count);
      const uint64_t* v = values + fdb_pqw_page_first(g, p);
      uint32_t run = fdb_pqd_header_len(count, count > 0 ? v[0] : 0);
      for (uint32_t b = 0; b < fdb_pqd_blocks(deltas); b++) {
        const uint32_t n = fdb_pqd_block_deltas(deltas, b);
        const uint64_t at = (uint64_t)b * FDB_PQD_BLOCK;
        int64_t mn = INT64_MAX;
        for (uint32_t i = 0; i < n; i++) { const int64_t dl = (int64_t)fdb_pqd_delta(v, at + i); mn = dl < mn ? dl : mn; }
        uint32_t widths = 0;
        for (uint32_t m = 0; m < fdb_pqd_minis(n); m++) {
          uint64_t mx = 0;
          for (uint32_t i = m * FDB_PQD_MINI; i < n && i < (m + 1) * FDB_PQD_MINI; i++) { const uint64_t r = fdb_pqd_rel(fdb_pqd_delta(v, at + i), mn); mx = r > mx ? r : mx; }
          widths = fdb_pqd_set_width(widths, m, fdb_pqd_bit_length(mx));
        }
        FdbPqdBlock& r = d->blocks[cp * bpp + b];
        r.min = mn; r.widths = widths; r.bytes = fdb_pqd_block_bytes(mn, widths, fdb_pqd_minis(n)); r.off = run;
        run += r.bytes;
      }
      d->page_bytes[cp] = run;
    }
  }
}

void pqd_encode_host(const std::vector<PqwColumn>& cols, const FdbPqwGeom& g, const std::vector<FdbPqwPageStat>& stats, const PqdHost& d, const std::vector<uint64_t>& delta_out,
                     unsigned char* image) {
  const size_t bpp = (size_t)fdb_pqd_blocks_per_page(g.page_rows);
  for (size_t k = 0; k < cols.size(); k++) {
    const PqwColumn& c = cols[k];
    if (c.delta_slot < 0) continue;
    const uint64_t* values = d.values(c);
    for (int64_t p = 0; p < g.n_pages; p++) {
      const size_t cp = (size_t)c.delta_slot * (size_t)g.n_pages + (size_t)p;
      const uint32_t count = stats[k * (size_t)g.n_pages + (size_t)p].count, deltas = fdb_pqd_deltas(count);
      const uint64_t* v = values + fdb_pqw_page_first(g, p);
      unsigned char* out = image + delta_out[cp];
      const uint64_t first = count > 0 ? v[0] : 0;
      for (uint32_t i = 0; i < fdb_pqd_header_len(count, first); i++) out[i] = fdb_pqd_header_byte(count, first, i);
      for (uint32_t b = 0; b < fdb_pqd_blocks(deltas); b++) {
        const uint32_t n = fdb_pqd_block_deltas(deltas, b);
        const FdbPqdBlock& r = d.blocks[cp * bpp + b];
        uint64_t rel[FDB_PQD_BLOCK];
        for (uint32_t i = 0; i < FDB_PQD_BLOCK; i++) rel[i] = i < n ? fdb_pqd_rel(fdb_pqd_delta(v, (uint64_t)b * FDB_PQD_BLOCK + i), r.min) : 0;
        unsigned char* q = out + r.off;
        const uint32_t head = fdb_pqd_block_head_len(r.min);
        for (uint32_t i = 0; i < head; i++) q[i] = fdb_pqd_block_head_byte(r.min, r.widths, i);
        q += head;
        for (uint32_t m = 0; m < fdb_pqd_minis(n); m++) {
          const uint32_t w = fdb_pqd_width(r.widths, m);
          for (uint32_t kk = 0; kk < w; kk++, q += 4) { const uint32_t word = fdb_pqd_assemble_word(rel + m * FDB_PQD_MINI, w, kk); std::memcpy(q, &word, 4); }
        }
      }
    }
  }
}

// ---- fdb_selftest_parquet_write: the pipeline over a host record ------------------------------------------------------------------------
// A host record in the resident form: 8 bytes per value (a bool widened to 1 / 2), a uint32 per index, bitmaps at bit 0 in whole
// words. `keep`: what had to be made for that, for as long as the columns are looked at.
struct HostResident { std::vector<std::vector<uint32_t>> idx; std::vector<std::vector<int64_t>> i64; std::vector<std::vector<uint8_t>> bits; };
static std::vector<PqwInput> resident_form(const HostRecordView& view, HostResident* keep) {
  const size_t rows = (size_t)view.rows;
  keep->idx.resize(view.cols.size()); keep->i64.resize(view.cols.size()); keep->bits.resize(view.cols.size());
  std::vector<PqwInput> in;
  for (size_t k = 0; k < view.cols.size(); k++) {
    const HostColView& c = view.cols[k];
    PqwInput o;
    o.name = c.name; o.format = c.format; o.kind = c.kind; o.null_count = c.null_count;
    if (c.kind == ColKind::I64 || c.kind == ColKind::U64 || c.kind == ColKind::F64) {
      o.values = rows > 0 ? (const unsigned char*)c.values + (size_t)c.offset * 8 : nullptr;
    } else if (c.kind == ColKind::BOOL) {
      keep->i64[k].assign(rows + 1, 0);
      const uint8_t* bits = (const uint8_t*)c.values;
      for (size_t i = 0; i < rows; i++) keep->i64[k][i] = 1 + ((bits[(c.offset + (int64_t)i) >> 3] >> ((c.offset + (int64_t)i) & 7)) & 1);
      o.values = keep->i64[k].data();
    } else if (c.kind == ColKind::DICT) {
      o.dict = read_dictionary(c);
      keep->idx[k].assign(rows + 1, 0);
      for (size_t i = 0; i < rows; i++) {
        const size_t at = (size_t)c.offset + i;
        switch (c.index_width) {
          case 1: keep->idx[k][i] = ((const uint8_t*)c.values)[at]; break;
          case 2: keep->idx[k][i] = ((const uint16_t*)c.values)[at]; break;
          case 4: keep->idx[k][i] = ((const uint32_t*)c.values)[at]; break;
          default: keep->idx[k][i] = (uint32_t)((const uint64_t*)c.values)[at]; break;
        }
      }
      o.values = keep->idx[k].data();
    } else if (c.kind == ColKind::STR) {
      o.dict = encode_plain(c, &keep->idx[k]);
      keep->idx[k].resize(rows + 1, 0);
      o.kind = ColKind::DICT;
      o.values = keep->idx[k].data();
    }
    if (c.null_count > 0 && c.validity != nullptr) {
      keep->bits[k].assign((rows + 63) / 64 * 8 + 8, 0);
      copy_bits(c.validity, c.offset, c.length, keep->bits[k].data());
      o.validity = keep->bits[k].data();
    }
    in.push_back(std::move(o));
  }
  return in;
}

// The pipeline with every kernel replaced by its host walk, over columns in host memory — or over a record without rows or columns,
// which gives the device nothing to do (no data page: the dictionary pages are the host's, compressed or not).
struct PqwHostPart { std::vector<FdbPqwPageStat> stats; std::vector<uint32_t> tile_base; std::vector<std::vector<uint32_t>> rekeyed; PqdHost delta; PqrHost rn; };
static void pqw_write_host(std::vector<PqwPlan>& plans, uint8_t** bytes, int64_t* n_bytes) {
  std::vector<PqwHostPart> host(plans.size());
  std::vector<const PqwPlan*> parts;
  std::vector<PqwSizes> sizes;
  size_t n_compressed = 0;
  for (size_t pi = 0; pi < plans.size(); pi++) {  // the survey passes
    PqwPlan& P = plans[pi]; PqwHostPart& h = host[pi];
    const std::vector<PqwColumn>& cols = P.cols; const FdbPqwGeom& g = P.g;
    pqw_survey_host(cols, g, &h.stats, &h.tile_base);
    if (P.x.statistics > 0) pqx_minmax_host(cols, g, &P.x);
    if (P.dict.any()) {  // the present pass, the used entries counted, the remap pass: from here on a pruned column is its re-keyed copy
      pqg_present_host(cols, g, &P.dict);
      pqg_resolve(h.stats, g, &P.cols, &P.dict);
      pqg_remap_host(cols, g, P.dict, &h.rekeyed);
      for (size_t slot = 0; slot < P.dict.cols.size(); slot++) { PqwColumn& c = P.cols[P.dict.cols[slot].col]; c.raw_values = c.values; c.values = h.rekeyed[slot].data(); }
    }
    if (P.bloom.any()) pqb_size(cols, g, h.stats, &P.bloom);
    if (P.n_bytes > 0) { pqy_survey_host(cols, g, P.n_bytes, &P.strings); pqy_scan(g, P.n_bytes, &P.strings); }  // the byte survey, and the host's scan of its table
    pqd_survey_host(cols, g, h.stats, h.tile_base, &h.delta, &P.strings);
    if (P.n_runs > 0) pqr_survey_host(cols, g, h.stats, &h.rn);
    parts.push_back(&P);
    sizes.push_back(PqwSizes{h.stats, &h.delta.page_bytes, P.n_runs > 0 ? &h.rn.page_bytes : nullptr, nullptr, P.n_bytes > 0 ? &P.strings.page_bytes : nullptr});
    n_compressed += P.n_compressed;
  }
  // layout, and the encode passes
  const PqwLayout L = pqw_layout(parts, sizes);
  std::vector<unsigned char> image(((size_t)L.body_bytes + 8 + 3) / 4 * 4, 0);
  for (size_t pi = 0; pi < plans.size(); pi++) {
    const PqwPlan& P = plans[pi]; const PqwHostPart& h = host[pi];
    pqw_encode_host(P.cols, P.g, L.parts[pi].out, h.tile_base, image.data());
    pqd_encode_host(P.cols, P.g, h.stats, h.delta, L.parts[pi].delta_out, image.data());
    if (P.n_runs > 0) pqr_encode_host(h.rn, L.parts[pi].run_out, image.data());
    if (P.n_bytes > 0) pqy_encode_host(P.cols, P.g, P.strings, L.parts[pi].bytes_out, image.data());
  }
  // the file's body: the image, or — `image` being the staging image — what the compressor made of it, laid out again and gathered
  PqwLayout F; uint8_t* file = nullptr;
  if (n_compressed == 0) {
    file = pqw_alloc_bytes(L.file_bytes(), false);
    std::memcpy(file, image.data(), (size_t)L.body_bytes);
  } else {
    for (const PqwLayout::Piece& p : L.body_pieces) std::memcpy(image.data() + p.off, L.body_blob.data() + p.pos, p.len);  // the bodies made whole
    std::vector<std::string> elements;
    std::vector<uint32_t> page_elements;
    for (const PqwLayout::Page& pg : L.pages) {
      elements.push_back(pg.codec == PQW_LZ4_RAW ? pql_block_host(image.data() + pg.off, (size_t)pg.body) : pqs_elements_host(image.data() + pg.off, (size_t)pg.body));
      page_elements.push_back((uint32_t)elements.back().size());
    }
    std::vector<PqwSizes> final_sizes;
    for (const PqwSizes& z : sizes) final_sizes.push_back(PqwSizes{z.stats, z.delta_bytes, z.run_bytes, &page_elements, z.stream_bytes});
    F = pqw_layout(parts, final_sizes);
    file = pqw_alloc_bytes(F.file_bytes(), false);
    for (size_t i = 0; i < F.pages.size(); i++) std::memcpy(file + F.pages[i].off, elements[i].data(), elements[i].size());
    for (size_t k = 0; k < L.chunk_off.size(); k++)
      if (L.chunk_codec[k] == 0) std::memcpy(file + F.chunk_off[k], image.data() + L.chunk_off[k], (size_t)L.chunk_len[k]);
  }
  const PqwLayout& at = n_compressed == 0 ? L : F;
  if (!at.blooms.empty()) {  // the insert pass, and every bitset to its place in the file
    std::vector<std::vector<unsigned char>> bitsets;
    for (const PqwPlan& P : plans) {
      bitsets.emplace_back((size_t)P.bloom.table_bytes, 0);
      pqb_insert_host(P.cols, P.g, P.bloom, bitsets.back().data());
    }
    for (const PqwLayout::Bloom& f : at.blooms) std::memcpy(file + f.bits_off, bitsets[f.part].data() + plans[f.part].bloom.table_off[f.col], (size_t)f.bytes);
  }
  pqw_finish(at, file);
  *bytes = file; *n_bytes = (int64_t)at.file_bytes();
}

void selftest_parquet_write(const HostRecordView& view, const PqwSpec& spec, uint8_t** bytes, int64_t* n_bytes) {
  HostResident keep;
  const std::vector<PqwInput> in = resident_form(view, &keep);  // (owns the dictionaries the plan's columns point at)
  std::vector<PqwPlan> parts = pqw_parts(pqw_plan(in, view.rows, spec), spec);
  pqw_write_host(parts, bytes, n_bytes);
}

#ifndef FDB_PQWRITE_HOST_ONLY
// ---- fdb_batch_to_parquet: the pipeline on the device ------------------------------------------------------------------------------------
struct PqwBytes { uint8_t* p = nullptr; ~PqwBytes() { pqw_free_bytes(p); } };  // the file until it is handed over
struct PoolBlock {  // an image of the file body in HBM
  int device; unsigned char* p = nullptr;
  void alloc(size_t bytes) { p = (unsigned char*)device_pool_alloc(device, bytes); }
  ~PoolBlock() { if (p != nullptr) device_pool_free(device, p); }
};

// What the parts of one call share beside scope, stream and images: the pass queued last, and the device copies of the rank and hash
// tables, which belong to the record's columns — every group of a column reads the same one.
struct PqwShared {
  const char* queued = nullptr; std::vector<const uint32_t*> d_ranks; std::vector<const uint64_t*> d_hashes;
  std::vector<const uint32_t*> d_entry_off; std::vector<const unsigned char*> d_entry_bytes;  // the entry tables of the columns with a form (fdb_pqbytes.h)
};

// One part's side of the device (a call without row groups has one): the plan, its scope, stream and timer, its images (with a compressed column: staging image,
// scratch, final image), the tables of the survey and of the optional passes (the call's arena) and the host tables its wait fills.
struct PqwCall {
  PqwPlan& P;
  CallScope& cs;
  hipStream_t stream;
  PoolBlock &image, &scratch, &final_image;
  PhaseTimer& pt;  // FDB_PROFILE=1: the passes timed apart (every pass is then waited for on its own)
  PqwShared& shared;
  const char*& queued;  // FDB_PROFILE: the pass queued last and not waited for yet — the name the next wait is marked with
  size_t items = 0, d_items = 0, r_items = 0;  // columns, DELTA columns, run streams × pages
  const FdbPqwCol* d_cols = nullptr; FdbPqwPageStat* d_stats = nullptr; uint32_t* d_tile_base = nullptr;
  const FdbPqdCol* d_dcols = nullptr; FdbPqdBlock* d_blocks = nullptr; uint32_t* d_page_bytes = nullptr;
  const FdbPqrStream* d_streams = nullptr; uint32_t* d_run_bytes = nullptr; unsigned char* d_bitsets = nullptr;
  unsigned long long* d_present = nullptr;  // used-entry dictionaries: the table of presence bitmaps
  const FdbPqyCol* d_ycols = nullptr; uint64_t* d_tile_bytes = nullptr; std::vector<uint64_t*> d_lengths;  // columns with a form: the byte survey's table; per DELTA slot the scratch column of lengths (null: not one)
  bool compact = false, run_compact = false;  // a DELTA column / a column whose indices are cut into runs has a bitmap
  std::vector<FdbPqwPageStat> stats; std::vector<uint32_t> delta_bytes, run_bytes;  // what the survey's wait fills
  void wait() { hip_check(hipStreamSynchronize(stream), "hipStreamSynchronize"); }
  void timed(const char* what) { if (pt.on) { wait(); pt.mark(what); } }  // FDB_PROFILE: a pass waited for by itself
  void settle() { timed(queued != nullptr ? queued : "pqwrite wait"); queued = nullptr; }  // … the pass queued last ("pqwrite wait": none was)
  void* upload(const void* host, size_t n, const char* what) {  // (`host` outlives the next wait)
    void* d = cs.alloc(std::max<size_t>(n, 8));
    if (n > 0) hip_check(hipMemcpyAsync(d, host, n, hipMemcpyHostToDevice, stream), what);
    return d;
  }
};

// The columns as the survey and encode kernels see them, the survey's two tables.
static void pqw_stage_cols(PqwCall* c) {
  const std::vector<PqwColumn>& cols = c->P.cols;
  std::vector<FdbPqwCol> kc(cols.size());
  for (size_t k = 0; k < cols.size(); k++) {
    std::memset(&kc[k], 0, sizeof(FdbPqwCol));
    kc[k].values = cols[k].values; kc[k].validity = cols[k].validity; kc[k].width = (int32_t)cols[k].width;
    kc[k].kind = cols[k].pq_kind == PQW_NO_VALUES ? FDB_PQW_INDEX : cols[k].pq_kind;
  }
  c->d_cols = (const FdbPqwCol*)c->cs.ctx->stage(kc.data(), kc.size() * sizeof(FdbPqwCol));
}

static void pqw_tables(PqwCall* c) {
  const std::vector<PqwColumn>& cols = c->P.cols;
  c->items = cols.size() * (size_t)c->P.g.n_pages;
  pqw_stage_cols(c);
  c->d_stats = (FdbPqwPageStat*)c->cs.alloc(c->items * sizeof(FdbPqwPageStat));
  c->d_tile_base = (uint32_t*)c->cs.alloc(c->items * (size_t)c->P.g.tiles_per_page * 4);
  c->stats.resize(c->items);
}

// The DELTA columns: scratch for the dense values of those with a bitmap, the block table, the page sizes.
static void pqd_tables(PqwCall* c) {
  const std::vector<PqwColumn>& cols = c->P.cols;
  const FdbPqwGeom& g = c->P.g;
  c->d_items = c->P.n_delta * (size_t)g.n_pages;
  c->delta_bytes.resize(c->d_items);
  std::vector<FdbPqdCol> dc(c->P.n_delta);
  for (size_t k = 0; k < cols.size(); k++) {
    if (cols[k].delta_slot < 0) continue;
    FdbPqdCol& o = dc[(size_t)cols[k].delta_slot];
    std::memset(&o, 0, sizeof(FdbPqdCol));
    o.col = (int32_t)k;
    if (cols[k].form != 0) {  // DELTA_LENGTH: the values' lengths, a dense column of the call's arena that the byte survey fills in rank order
      o.dense = (uint64_t*)c->cs.alloc(((size_t)g.rows + 1) * 8); o.values = o.dense;
      c->d_lengths.resize(c->P.n_delta, nullptr); c->d_lengths[(size_t)cols[k].delta_slot] = o.dense;
      continue;
    }
    o.values = (const uint64_t*)cols[k].values; o.validity = cols[k].validity;
    o.dense = cols[k].validity != nullptr ? (uint64_t*)c->cs.alloc(((size_t)g.rows + 1) * 8) : (uint64_t*)const_cast<void*>(cols[k].values);  // (only ever read when it is the column)
    c->compact = c->compact || cols[k].validity != nullptr;
  }
  c->d_dcols = (const FdbPqdCol*)c->cs.ctx->stage(dc.data(), dc.size() * sizeof(FdbPqdCol));
  c->d_blocks = (FdbPqdBlock*)c->cs.alloc(c->d_items * (size_t)fdb_pqd_blocks_per_page(g.page_rows) * sizeof(FdbPqdBlock));
  c->d_page_bytes = (uint32_t*)c->cs.alloc(c->d_items * 4);
}

// The streams to be cut into runs: scratch for the dense indices of the columns with a bitmap, the table of sizes.
static void pqr_tables(PqwCall* c) {
  const std::vector<PqwColumn>& cols = c->P.cols;
  const FdbPqwGeom& g = c->P.g;
  c->r_items = c->P.n_runs * (size_t)g.n_pages;
  c->run_bytes.resize(c->r_items);
  std::vector<FdbPqrStream> rs(c->P.n_runs);
  for (size_t k = 0; k < cols.size(); k++) {
    const PqwColumn& col = cols[k];
    if (col.run_values >= 0) {
      FdbPqrStream& o = rs[(size_t)col.run_values];
      std::memset(&o, 0, sizeof(FdbPqrStream));
      o.values = (const uint32_t*)col.values; o.validity = col.validity; o.col = (int32_t)k; o.width = (int32_t)col.width;
      o.dense = col.validity != nullptr ? (uint32_t*)c->cs.alloc(((size_t)g.rows + 8) * 4) : (uint32_t*)const_cast<void*>(col.values);  // (only ever read when it is the column)
      c->run_compact = c->run_compact || col.validity != nullptr;
    }
    if (col.run_levels >= 0) {
      FdbPqrStream& o = rs[(size_t)col.run_levels];
      std::memset(&o, 0, sizeof(FdbPqrStream));
      o.validity = col.validity; o.col = (int32_t)k; o.width = 1; o.levels = 1;
    }
  }
  c->d_streams = (const FdbPqrStream*)c->cs.ctx->stage(rs.data(), rs.size() * sizeof(FdbPqrStream));
  c->d_run_bytes = (uint32_t*)c->cs.alloc(c->r_items * 4);
}

// The columns with a form as fdb_pqbytes.hip sees them — their entry tables uploaded once per call, every group of a column reads the
// same ones — and the byte survey's table. After pqd_tables: a DELTA_LENGTH column's lengths are that pass's scratch.
static void pqy_tables(PqwCall* c) {
  const std::vector<PqwColumn>& cols = c->P.cols;
  std::vector<FdbPqyCol> yc(c->P.n_bytes);
  for (size_t k = 0; k < cols.size(); k++) {
    const PqwColumn& col = cols[k];
    if (col.bytes_slot < 0) continue;
    const PqyTables& tb = *c->P.strings.tables[col.real];
    const uint32_t*& d_off = c->shared.d_entry_off[col.real];
    if (d_off == nullptr) {  // (the plan outlives the wait)
      d_off = (const uint32_t*)c->upload(tb.off, ((size_t)col.entries + 1) * 4, "hipMemcpyAsync(entry offsets)");
      c->shared.d_entry_bytes[col.real] = (const unsigned char*)c->upload(tb.bytes, tb.n_bytes, "hipMemcpyAsync(entry bytes)");
    }
    FdbPqyCol& o = yc[(size_t)col.bytes_slot];
    std::memset(&o, 0, sizeof(FdbPqyCol));
    o.values = (const uint32_t*)col.values; o.validity = col.validity; o.entry_off = d_off; o.entry_bytes = c->shared.d_entry_bytes[col.real];
    o.lengths = col.delta_slot >= 0 ? c->d_lengths[(size_t)col.delta_slot] : nullptr;
    o.entries = (uint32_t)col.entries; o.col = (int32_t)k; o.plain = col.form == FDB_PQY_PLAIN;
  }
  c->d_ycols = (const FdbPqyCol*)c->cs.ctx->stage(yc.data(), yc.size() * sizeof(FdbPqyCol));
  const size_t tiles = c->P.n_bytes * (size_t)c->P.g.n_pages * (size_t)c->P.g.tiles_per_page;
  c->d_tile_bytes = (uint64_t*)c->cs.alloc(tiles * 8);
  c->P.strings.tile_bytes.resize(tiles);
}

// The byte survey (fdb_pqbytes.hip): behind the survey, whose tile ranks it reads, and in front of the DELTA passes, whose lengths it
// writes; its table back in the same wait.
static void pqy_survey_pass(PqwCall* c) {
  if (c->queued != nullptr) c->settle();
  std::vector<uint64_t>& tile_bytes = c->P.strings.tile_bytes;
  hip_check(fdb_launch_pqy_survey(c->d_ycols, (int32_t)c->P.n_bytes, c->P.g, c->d_tile_base, c->d_tile_bytes, c->stream), "parquet write: byte survey launch");
  hip_check(hipMemcpyAsync(tile_bytes.data(), c->d_tile_bytes, tile_bytes.size() * 8, hipMemcpyDeviceToHost, c->stream), "hipMemcpyAsync(byte survey table)");
  c->queued = "pqwrite bytes survey";
}

// The min / max pass (fdb_pqstats.hip): behind the survey, its table back in the same wait.
static void pqx_minmax_pass(PqwCall* c) {
  const std::vector<PqwColumn>& cols = c->P.cols;
  PqxIndex& x = c->P.x;
  c->settle();
  std::vector<FdbPqxCol> xc(cols.size());
  for (size_t k = 0; k < cols.size(); k++) {
    std::memset(&xc[k], 0, sizeof(FdbPqxCol));
    xc[k].values = cols[k].values; xc[k].validity = cols[k].validity; xc[k].mode = x.modes[k];
    const std::vector<uint32_t>& r = x.ranks[cols[k].real];
    if (r.empty()) continue;
    const uint32_t*& shared_ranks = c->shared.d_ranks[cols[k].real];
    if (shared_ranks == nullptr) {
      uint32_t* d_ranks = (uint32_t*)c->cs.alloc(r.size() * 4);
      hip_check(hipMemcpyAsync(d_ranks, r.data(), r.size() * 4, hipMemcpyHostToDevice, c->stream), "hipMemcpyAsync(dictionary ranks)");  // (the plan outlives the wait)
      shared_ranks = d_ranks;
    }
    xc[k].ranks = shared_ranks; xc[k].rank_len = (uint32_t)r.size();
  }
  const FdbPqxCol* d_xcols = (const FdbPqxCol*)c->cs.ctx->stage(xc.data(), xc.size() * sizeof(FdbPqxCol));
  unsigned long long* d_table = (unsigned long long*)c->cs.alloc(2 * c->items * 8);
  hip_check(hipMemsetAsync(d_table, 0xFF, c->items * 8, c->stream), "hipMemsetAsync(min table)");
  hip_check(hipMemsetAsync(d_table + c->items, 0, c->items * 8, c->stream), "hipMemsetAsync(max table)");
  hip_check(fdb_launch_pqx_minmax(d_xcols, c->P.g, d_table, c->stream), "parquet write: min / max launch");
  x.table.assign(2 * c->items, 0);
  hip_check(hipMemcpyAsync(x.table.data(), d_table, 2 * c->items * 8, hipMemcpyDeviceToHost, c->stream), "hipMemcpyAsync(min / max table)");
  c->timed("pqwrite stats");
}

// The DELTA passes of fdb_pqdelta.hip that size the pages: compaction of the columns with a bitmap, block survey and page walk.
static void pqd_survey_pass(PqwCall* c) {
  const int32_t n = (int32_t)c->P.n_delta;
  if (c->queued != nullptr) c->settle();
  if (c->compact) hip_check(fdb_launch_pqd_compact(c->d_dcols, n, c->P.g, c->d_tile_base, c->stream), "parquet write: DELTA compaction launch");
  c->timed("pqwrite delta compact");
  hip_check(fdb_launch_pqd_survey(c->d_dcols, n, c->P.g, c->d_stats, c->d_blocks, c->d_page_bytes, c->stream), "parquet write: DELTA block survey launch");
  hip_check(hipMemcpyAsync(c->delta_bytes.data(), c->d_page_bytes, c->d_items * 4, hipMemcpyDeviceToHost, c->stream), "hipMemcpyAsync(DELTA page sizes)");
  c->queued = "pqwrite delta survey";
}

// The run passes of fdb_pqruns.hip that size the streams: compaction of the indices of the columns with a bitmap, the run survey.
static void pqr_survey_pass(PqwCall* c) {
  const int32_t n = (int32_t)c->P.n_runs;
  c->settle();
  if (c->run_compact) hip_check(fdb_launch_pqr_compact(c->d_streams, n, c->P.g, c->d_tile_base, c->stream), "parquet write: run compaction launch");
  hip_check(fdb_launch_pqr_survey(c->d_streams, n, c->P.g, c->d_stats, c->d_run_bytes, c->stream), "parquet write: run survey launch");
  hip_check(hipMemcpyAsync(c->run_bytes.data(), c->d_run_bytes, c->r_items * 4, hipMemcpyDeviceToHost, c->stream), "hipMemcpyAsync(run-encoded sizes)");
  c->queued = "pqwrite run survey";
}

// The pruned columns as fdb_pqdict.hip sees them; `before` / `copies`: null for the present pass.
static const FdbPqgCol* pqg_stage_cols(PqwCall* c, const uint32_t* d_before, const std::vector<uint32_t*>* copies) {
  const PqgPlan& d = c->P.dict;
  std::vector<FdbPqgCol> gc(d.cols.size());
  for (size_t slot = 0; slot < d.cols.size(); slot++) {
    const PqwColumn& col = c->P.cols[d.cols[slot].col];
    std::memset(&gc[slot], 0, sizeof(FdbPqgCol));
    gc[slot].values = (const uint32_t*)(col.raw_values != nullptr ? col.raw_values : col.values); gc[slot].validity = col.validity;
    gc[slot].bits = c->d_present + d.cols[slot].word_off; gc[slot].entries = (uint32_t)d.cols[slot].entries;
    if (d_before != nullptr) { gc[slot].before = d_before + d.cols[slot].word_off; gc[slot].out = (*copies)[slot]; }
  }
  return (const FdbPqgCol*)c->cs.ctx->stage(gc.data(), gc.size() * sizeof(FdbPqgCol));
}

// The present pass (fdb_pqdict.hip): behind the survey, into one zeroed table of presence bitmaps, back in the same wait.
static void pqg_present_pass(PqwCall* c) {
  PqgPlan& d = c->P.dict;
  if (c->queued != nullptr) c->settle();
  const size_t bytes = d.bits.size() * 8;
  c->d_present = (unsigned long long*)c->cs.alloc(std::max<size_t>(bytes, 8));
  hip_check(hipMemsetAsync(c->d_present, 0, std::max<size_t>(bytes, 8), c->stream), "hipMemsetAsync(presence bitmaps)");
  hip_check(fdb_launch_pqg_present(pqg_stage_cols(c, nullptr, nullptr), (int32_t)d.cols.size(), c->P.g, c->stream), "parquet write: dictionary present launch");
  if (bytes > 0) hip_check(hipMemcpyAsync(d.bits.data(), c->d_present, bytes, hipMemcpyDeviceToHost, c->stream), "hipMemcpyAsync(presence bitmaps)");
  c->queued = "pqwrite dict present";
}

// After the wait: the used entries counted (pqg_resolve), their counts up, the remap pass into a re-keyed copy of every pruned column —
// which is the column from here on, for the table the encode pass reads as well.
static void pqg_remap_pass(PqwCall* c) {
  PqgPlan& d = c->P.dict;
  if (c->queued != nullptr) c->settle();
  pqg_resolve(c->stats, c->P.g, &c->P.cols, &d);
  const uint32_t* d_before = (const uint32_t*)c->upload(d.before.data(), d.before.size() * 4, "hipMemcpyAsync(used entry counts)");  // (the plan outlives the wait)
  std::vector<uint32_t*> copies;
  for (size_t slot = 0; slot < d.cols.size(); slot++) copies.push_back((uint32_t*)c->cs.alloc(((size_t)c->P.g.rows + 8) * 4));
  hip_check(fdb_launch_pqg_remap(pqg_stage_cols(c, d_before, &copies), (int32_t)d.cols.size(), c->P.g, c->stream), "parquet write: dictionary remap launch");
  c->timed("pqwrite dict remap");
  for (size_t slot = 0; slot < d.cols.size(); slot++) { PqwColumn& col = c->P.cols[d.cols[slot].col]; col.raw_values = col.values; col.values = copies[slot]; }
  pqw_stage_cols(c);
}

// The insert pass of fdb_pqbloom.hip, into one zeroed table of bitsets the survey's table has sized.
static void pqb_insert_pass(PqwCall* c) {
  const std::vector<PqwColumn>& cols = c->P.cols;
  const PqbPlan& bl = c->P.bloom;
  std::vector<FdbPqbCol> bc;
  c->d_bitsets = (unsigned char*)c->cs.alloc((size_t)bl.table_bytes);
  for (size_t k = 0; k < cols.size(); k++) {
    if (bl.on[k] == 0) continue;
    FdbPqbCol o;
    std::memset(&o, 0, sizeof(FdbPqbCol));
    o.values = pqw_raw(cols[k]); o.validity = cols[k].validity; o.index = cols[k].pq_kind != FDB_PQW_V64;
    o.bits = (unsigned long long*)(c->d_bitsets + bl.table_off[k]); o.n_blocks = bl.bytes[k] / FDB_PQB_BLOCK_BYTES;
    const std::vector<uint64_t>& h = bl.hashes[cols[k].real];
    if (!h.empty()) {
      const uint64_t*& shared_hashes = c->shared.d_hashes[cols[k].real];
      if (shared_hashes == nullptr) {
        uint64_t* d_hashes = (uint64_t*)c->cs.alloc(h.size() * 8);
        hip_check(hipMemcpyAsync(d_hashes, h.data(), h.size() * 8, hipMemcpyHostToDevice, c->stream), "hipMemcpyAsync(entry hashes)");  // (the plan outlives the wait)
        shared_hashes = d_hashes;
      }
      o.hashes = shared_hashes; o.hash_len = (uint32_t)h.size();
    }
    bc.push_back(o);
  }
  const FdbPqbCol* d_bcols = (const FdbPqbCol*)c->cs.ctx->stage(bc.data(), bc.size() * sizeof(FdbPqbCol));
  hip_check(hipMemsetAsync(c->d_bitsets, 0, (size_t)bl.table_bytes, c->stream), "hipMemsetAsync(bloom filter bitsets)");
  hip_check(fdb_launch_pqb_insert(d_bcols, (int32_t)bc.size(), c->P.g, c->stream), "parquet write: bloom filter launch");
  c->timed("pqwrite bloom insert");
}

// The image, zeroed: once for the call.
static void pqw_image(PqwCall* c, const PqwLayout& whole) {
  const size_t image_bytes = align_up((size_t)whole.body_bytes + 8, 256);
  c->image.alloc(image_bytes);
  hip_check(hipMemsetAsync(c->image.p, 0, image_bytes, c->stream), "hipMemsetAsync(file image)");
}

// A part's encode passes into the image, every payload to where `L` says: the encode pass, then the DELTA and the run encoder.
static void pqw_encode_passes(PqwCall* c, const PqwLayout::Part& L) {
  const FdbPqwGeom& g = c->P.g;
  unsigned char* image = c->image.p;
  FdbPqwPageOut* d_out = (FdbPqwPageOut*)c->cs.alloc(c->items * sizeof(FdbPqwPageOut));
  hip_check(hipMemcpyAsync(d_out, L.out.data(), c->items * sizeof(FdbPqwPageOut), hipMemcpyHostToDevice, c->stream), "hipMemcpyAsync(page offsets)");
  hip_check(fdb_launch_pqw_encode(c->d_cols, g, d_out, c->d_tile_base, image, c->stream), "parquet write: encode launch");
  c->timed("pqwrite encode");
  if (c->P.n_delta > 0) {
    uint64_t* d_delta_out = (uint64_t*)c->cs.alloc(c->d_items * 8);
    hip_check(hipMemcpyAsync(d_delta_out, L.delta_out.data(), c->d_items * 8, hipMemcpyHostToDevice, c->stream), "hipMemcpyAsync(DELTA page offsets)");
    hip_check(fdb_launch_pqd_encode(c->d_dcols, (int32_t)c->P.n_delta, g, c->d_stats, c->d_blocks, d_delta_out, image, c->stream), "parquet write: DELTA encode launch");
    c->timed("pqwrite delta encode");
  }
  if (c->P.n_runs > 0) {
    uint64_t* d_run_out = (uint64_t*)c->cs.alloc(c->r_items * 8);
    hip_check(hipMemcpyAsync(d_run_out, L.run_out.data(), c->r_items * 8, hipMemcpyHostToDevice, c->stream), "hipMemcpyAsync(run-encoded page offsets)");
    hip_check(fdb_launch_pqr_encode(c->d_streams, (int32_t)c->P.n_runs, g, c->d_stats, c->d_run_bytes, d_run_out, image, c->stream), "parquet write: run encode launch");
    c->timed("pqwrite run encode");
  }
  if (c->P.n_bytes > 0) {  // (behind the DELTA encoder: a word the lengths and the bytes share is stored by the one, OR-ed by the other)
    const PqyPlan& y = c->P.strings;
    const uint64_t* d_bytes_out = (const uint64_t*)c->upload(L.bytes_out.data(), L.bytes_out.size() * 8, "hipMemcpyAsync(byte stream offsets)");
    const uint64_t* d_byte_base = (const uint64_t*)c->upload(y.byte_base.data(), y.byte_base.size() * 8, "hipMemcpyAsync(tile byte bases)");  // (the plan outlives the wait)
    hip_check(fdb_launch_pqy_encode(c->d_ycols, (int32_t)c->P.n_bytes, g, d_bytes_out, d_byte_base, image, c->stream), "parquet write: byte encode launch");
    c->timed("pqwrite bytes encode");
  }
}

// SNAPPY (fdb_pqsnappy.hip) and LZ4_RAW (fdb_pqlz4.hip): the host tables of the compress and gather passes — they outlive the waits of
// both — and their device copies. Each codec has the pages of its columns in tables of its own; `page_elements` lists both in the
// layout's order. Without an LZ4_RAW column its tables stay empty: nothing of it is allocated, copied or launched.
struct PqsTables {
  std::vector<FdbPqsRange> pieces, ranges; std::vector<FdbPqsPage> pages; std::vector<FdbPqsFrag> frags;
  std::vector<uint64_t> page_dst; std::vector<uint32_t> page_elements, snappy_elements;
  const FdbPqsFrag* d_frags = nullptr; uint32_t *d_frag_bytes = nullptr, *d_frag_off = nullptr;
  std::vector<FdbPqlPage> lz_pages; std::vector<FdbPqlFrag> lz_frags; std::vector<uint64_t> lz_page_dst; std::vector<uint32_t> lz_bytes;
  const FdbPqlFrag* d_lz_frags = nullptr; const FdbPqlPage* d_lz_pages = nullptr; FdbPqlOut* d_lz_outs = nullptr; FdbPqlPlace *d_lz_places = nullptr, *d_lz_closes = nullptr;
  size_t lz_scratch = 0;  // where the LZ4 fragments' slots start in the call's scratch
};

// The staging image, laid out by `L`, compressed: the fragment and page tables of the pages it lists, the host's bytes inside their
// bodies placed, every fragment into its slot of scratch, the sizes summed per page (t->page_elements) — the call's second wait.
static void pqs_compress_pass(PqwCall* c, const PqwLayout& L, PqsTables* t) {
  for (const PqwLayout::Piece& p : L.body_pieces) t->pieces.push_back(FdbPqsRange{(uint64_t)p.pos, p.off, (uint32_t)p.len, 0});
  for (const PqwLayout::Page& pg : L.pages) {
    if (pg.codec == PQW_LZ4_RAW) {
      t->lz_pages.push_back(FdbPqlPage{pg.off + pg.body, (uint32_t)t->lz_frags.size(), fdb_pqs_fragments(pg.body)});
      for (uint64_t at = 0; at < pg.body; at += FDB_PQS_FRAGMENT) {
        const uint32_t len = (uint32_t)std::min<uint64_t>(FDB_PQS_FRAGMENT, pg.body - at);
        t->lz_frags.push_back(FdbPqlFrag{pg.off + at, len, (uint32_t)(t->lz_pages.size() - 1), fdb_pql_stop(at, len, pg.body), fdb_pql_reach(at, len, pg.body)});
      }
      continue;
    }
    t->pages.push_back(FdbPqsPage{(uint32_t)t->frags.size(), fdb_pqs_fragments(pg.body)});
    for (uint64_t at = 0; at < pg.body; at += FDB_PQS_FRAGMENT)
      t->frags.push_back(FdbPqsFrag{pg.off + at, (uint32_t)std::min<uint64_t>(FDB_PQS_FRAGMENT, pg.body - at), (uint32_t)(t->pages.size() - 1)});
  }
  if (t->frags.size() + t->lz_frags.size() > 0x7FFFFFFFull / 2) throw Error(FDB_ERR_UNSUPPORTED, "parquet write: more than 2^30 fragments to compress");
  const size_t n_frags = std::max<size_t>(t->frags.size(), 1);
  t->lz_scratch = n_frags * fdb_pqs_slot_bytes();
  c->scratch.alloc(t->lz_scratch + t->lz_frags.size() * fdb_pql_slot_bytes());
  const unsigned char* d_blob = (const unsigned char*)c->upload(L.body_blob.data(), L.body_blob.size(), "hipMemcpyAsync(page body pieces)");
  const FdbPqsRange* d_pieces = (const FdbPqsRange*)c->upload(t->pieces.data(), t->pieces.size() * sizeof(FdbPqsRange), "hipMemcpyAsync(page body piece table)");
  t->d_frags = (const FdbPqsFrag*)c->upload(t->frags.data(), t->frags.size() * sizeof(FdbPqsFrag), "hipMemcpyAsync(fragment table)");
  const FdbPqsPage* d_pages = (const FdbPqsPage*)c->upload(t->pages.data(), t->pages.size() * sizeof(FdbPqsPage), "hipMemcpyAsync(compressed page table)");
  t->d_frag_bytes = (uint32_t*)c->cs.alloc(n_frags * 4);
  t->d_frag_off = (uint32_t*)c->cs.alloc(n_frags * 4);
  uint32_t* d_page_elements = (uint32_t*)c->cs.alloc(std::max<size_t>(t->pages.size(), 1) * 4);
  t->snappy_elements.assign(t->pages.size(), 0);
  hip_check(fdb_launch_pqs_place(d_pieces, (int32_t)t->pieces.size(), d_blob, c->image.p, c->stream), "parquet write: body piece launch");
  hip_check(fdb_launch_pqs_compress(t->d_frags, (int32_t)t->frags.size(), c->image.p, c->scratch.p, t->d_frag_bytes, c->stream), "parquet write: compress launch");
  c->timed("pqwrite compress");
  hip_check(fdb_launch_pqs_scan(d_pages, (int32_t)t->pages.size(), t->d_frag_bytes, t->d_frag_off, d_page_elements, c->stream), "parquet write: compressed size scan launch");
  if (!t->pages.empty()) hip_check(hipMemcpyAsync(t->snappy_elements.data(), d_page_elements, t->pages.size() * 4, hipMemcpyDeviceToHost, c->stream), "hipMemcpyAsync(compressed page sizes)");
  if (!t->lz_pages.empty()) {  // (a page without a byte has no fragment, and still a block: its closing sequence)
    t->d_lz_frags = (const FdbPqlFrag*)c->upload(t->lz_frags.data(), t->lz_frags.size() * sizeof(FdbPqlFrag), "hipMemcpyAsync(LZ4 fragment table)");
    t->d_lz_pages = (const FdbPqlPage*)c->upload(t->lz_pages.data(), t->lz_pages.size() * sizeof(FdbPqlPage), "hipMemcpyAsync(LZ4 page table)");
    const size_t n_lz = std::max<size_t>(t->lz_frags.size(), 1);
    t->d_lz_outs = (FdbPqlOut*)c->cs.alloc(n_lz * sizeof(FdbPqlOut));
    t->d_lz_places = (FdbPqlPlace*)c->cs.alloc(n_lz * sizeof(FdbPqlPlace));
    t->d_lz_closes = (FdbPqlPlace*)c->cs.alloc(t->lz_pages.size() * sizeof(FdbPqlPlace));
    uint32_t* d_lz_bytes = (uint32_t*)c->cs.alloc(t->lz_pages.size() * 4);
    t->lz_bytes.assign(t->lz_pages.size(), 0);
    hip_check(fdb_launch_pql_compress(t->d_lz_frags, (int32_t)t->lz_frags.size(), c->image.p, c->scratch.p + t->lz_scratch, t->d_lz_outs, c->stream), "parquet write: LZ4 compress launch");
    c->timed("pqwrite lz compress");
    hip_check(fdb_launch_pql_scan(t->d_lz_pages, (int32_t)t->lz_pages.size(), t->d_lz_outs, t->d_lz_places, t->d_lz_closes, d_lz_bytes, c->stream), "parquet write: LZ4 size scan launch");
    hip_check(hipMemcpyAsync(t->lz_bytes.data(), d_lz_bytes, t->lz_pages.size() * 4, hipMemcpyDeviceToHost, c->stream), "hipMemcpyAsync(LZ4 page sizes)");
  }
  c->wait();
  c->pt.mark("pqwrite scan");
  size_t next_snappy = 0, next_lz = 0;
  for (const PqwLayout::Page& pg : L.pages) t->page_elements.push_back(pg.codec == PQW_LZ4_RAW ? t->lz_bytes[next_lz++] : t->snappy_elements[next_snappy++]);
}

// ONE gather launch moves the SNAPPY fragments' elements and the chunks of the uncompressed columns from the staging image (`L`) to
// where the final layout `F` wants them in the final image — with or without a SNAPPY column, the chunks are its ranges; a second
// one, with an LZ4_RAW column, writes the LZ4 blocks.
static void pqs_gather_pass(PqwCall* c, const PqwLayout& L, const PqwLayout& F, PqsTables* t) {
  std::vector<uint64_t>& page_dst = t->page_dst; std::vector<FdbPqsRange>& ranges = t->ranges;
  for (const PqwLayout::Page& pg : F.pages) (pg.codec == PQW_LZ4_RAW ? t->lz_page_dst : page_dst).push_back(pg.off);
  for (size_t k = 0; k < L.chunk_off.size(); k++) {  // the chunks of the uncompressed columns, in pieces a workgroup moves at a time
    if (L.chunk_codec[k] != 0) continue;
    for (uint64_t at = 0; at < L.chunk_len[k]; at += FDB_PQS_COPY_PIECE)
      ranges.push_back(FdbPqsRange{L.chunk_off[k] + at, F.chunk_off[k] + at, (uint32_t)std::min<uint64_t>(FDB_PQS_COPY_PIECE, L.chunk_len[k] - at), 0});
  }
  if (ranges.size() > 0x7FFFFFFFull / 2) throw Error(FDB_ERR_UNSUPPORTED, "parquet write: more than 2^30 pieces to move");
  const uint64_t* d_page_dst = (const uint64_t*)c->upload(page_dst.data(), page_dst.size() * 8, "hipMemcpyAsync(compressed page offsets)");
  const FdbPqsRange* d_ranges = (const FdbPqsRange*)c->upload(ranges.data(), ranges.size() * sizeof(FdbPqsRange), "hipMemcpyAsync(chunk piece table)");
  c->final_image.alloc(align_up((size_t)F.body_bytes + 8, 256));
  hip_check(fdb_launch_pqs_gather(t->d_frags, (int32_t)t->frags.size(), t->d_frag_bytes, t->d_frag_off, d_page_dst, c->scratch.p, d_ranges, (int32_t)ranges.size(), c->image.p, c->final_image.p,
                                  c->stream), "parquet write: gather launch");
  c->timed("pqwrite gather");
  if (t->lz_pages.empty()) return;
  if (t->lz_page_dst.size() != t->lz_pages.size()) throw Error(FDB_ERR_STATE, "parquet write: the final layout's LZ4 pages do not match the staging image's");
  const uint64_t* d_lz_dst = (const uint64_t*)c->upload(t->lz_page_dst.data(), t->lz_page_dst.size() * 8, "hipMemcpyAsync(LZ4 page offsets)");
  hip_check(fdb_launch_pql_gather(t->d_lz_frags, (int32_t)t->lz_frags.size(), t->d_lz_pages, (int32_t)t->lz_pages.size(), t->d_lz_outs, t->d_lz_places, t->d_lz_closes, d_lz_dst,
                                  c->scratch.p + t->lz_scratch, c->image.p, c->final_image.p, c->stream), "parquet write: LZ4 gather launch");
  c->timed("pqwrite lz gather");
}

// The one ending: the pinned file, every bitset straight to its place in it, the image in one parallel copy, the host's holes and tail.
static size_t pqw_deliver(std::vector<PqwCall>& calls, const PqwLayout& at, const void* image, PqwBytes* file) {
  PqwCall* c = &calls[0];
  const size_t file_bytes = at.file_bytes();
  file->p = pqw_alloc_bytes(file_bytes, true);
  for (const PqwLayout::Bloom& f : at.blooms)
    hip_check(hipMemcpyAsync(file->p + f.bits_off, calls[f.part].d_bitsets + calls[f.part].P.bloom.table_off[f.col], (size_t)f.bytes, hipMemcpyDeviceToHost, c->stream), "hipMemcpyAsync(bloom filter bitset)");
  if (!at.blooms.empty()) c->timed("pqwrite bloom copy");
  c->cs.ctx->copy_out_parallel(file->p, image, (size_t)at.body_bytes);
  c->pt.mark("pqwrite copy");
  pqw_finish(at, file->p);
  c->pt.mark("pqwrite host tail");
  return file_bytes;
}

void batch_to_parquet(const DeviceBatch& b, const PqwSpec& spec, uint8_t** bytes, int64_t* n_bytes) {
  std::vector<PqwInput> in;
  for (const DevColumn& c : b.cols) {
    PqwInput o;
    o.name = c.name; o.format = c.format; o.kind = c.kind; o.dict = c.dict; o.null_count = c.null_count; o.values = c.d_values; o.validity = c.d_validity;
    in.push_back(std::move(o));
  }
  // plan: every refusal of the options, then the device's own two — the min / max and the insert pass load 16 bytes of values at a time
  PqwPlan whole = pqw_plan(in, b.rows, spec);
  {
    const std::vector<PqwColumn>& cols = whole.cols;
    for (size_t k = 0; k < cols.size() && whole.x.statistics > 0; k++)
      if (((uintptr_t)cols[k].values & 15u) != 0) throw Error(FDB_ERR_UNSUPPORTED, "parquet write: the values of column " + cols[k].name + " are not 16-byte aligned (statistics)");
    for (size_t k = 0; k < cols.size() && whole.bloom.any(); k++)
      if (whole.bloom.on[k] != 0 && ((uintptr_t)cols[k].values & 15u) != 0)
        throw Error(FDB_ERR_UNSUPPORTED, "parquet write: the values of column " + cols[k].name + " are not 16-byte aligned (bloom filter)");
    for (const PqgPlan::Col& o : whole.dict.cols)
      if (((uintptr_t)cols[o.col].values & 15u) != 0) throw Error(FDB_ERR_UNSUPPORTED, "parquet write: the values of column " + cols[o.col].name + " are not 16-byte aligned (used-entry dictionary)");
  }
  const size_t n_real = whole.n_real;
  // the call's parts: one, or with several row groups the full groups' and the short last one's — every pass below is launched per part
  std::vector<PqwPlan> plans = pqw_parts(std::move(whole), spec);
  if (b.rows == 0 || n_real == 0) { pqw_write_host(plans, bytes, n_bytes); return; }
  const PqwPlan& head = plans[0];
  const bool bounds = head.x.statistics > 0, blooms = head.bloom.any();
  const bool pruned = head.dict.any();  // the run passes then read the re-keyed copies: they follow the remap pass, and the call waits once more
  size_t n_compressed = 0, n_runs = 0;
  for (const PqwPlan& P : plans) { n_compressed += P.n_compressed; n_runs += P.n_runs; }
  PqwBytes file;
  PhaseTimer pt;
  PoolBlock image{b.device}, scratch{b.device}, final_image{b.device};  // (before the scope: freed after its wait; the last two: compressed columns only)
  CallScope cs(b.device);
  DrainOnUnwind drain{cs.ctx->stream};
  PqwShared shared;
  shared.d_ranks.assign(n_real, nullptr); shared.d_hashes.assign(n_real, nullptr); shared.d_entry_off.assign(n_real, nullptr); shared.d_entry_bytes.assign(n_real, nullptr);
  std::vector<PqwCall> calls;
  for (PqwPlan& P : plans) calls.push_back(PqwCall{P, cs, cs.ctx->stream, image, scratch, final_image, pt, shared, shared.queued});
  hipStream_t stream = cs.ctx->stream;
  for (PqwCall& c : calls) {
    pqw_tables(&c);
    if (c.P.n_delta > 0) pqd_tables(&c);
    if (c.P.n_bytes > 0) pqy_tables(&c);
    if (c.P.n_runs > 0 && !pruned) pqr_tables(&c);
  }
  // the survey passes, their tables back in ONE wait
  b.note_reader(stream);
  for (PqwCall& c : calls) {
    if (c.queued != nullptr) c.settle();
    hip_check(fdb_launch_pqw_survey(c.d_cols, c.P.g, c.d_stats, c.d_tile_base, c.stream), "parquet write: survey launch");
    hip_check(hipMemcpyAsync(c.stats.data(), c.d_stats, c.items * sizeof(FdbPqwPageStat), hipMemcpyDeviceToHost, c.stream), "hipMemcpyAsync(page table)");
    c.queued = "pqwrite survey";
    if (bounds) pqx_minmax_pass(&c);
    if (c.P.n_bytes > 0) pqy_survey_pass(&c);
    if (c.P.n_delta > 0) pqd_survey_pass(&c);
    if (pruned) pqg_present_pass(&c);
    if (c.P.n_runs > 0 && !pruned) pqr_survey_pass(&c);
  }
  calls[0].wait();
  pt.mark(shared.queued != nullptr ? shared.queued : "pqwrite wait");
  shared.queued = nullptr;
  if (pruned) {
    for (PqwCall& c : calls) {
      pqg_remap_pass(&c);
      if (c.P.n_runs > 0) { pqr_tables(&c); pqr_survey_pass(&c); }
    }
    if (n_runs > 0) {
      calls[0].wait();
      pt.mark("pqwrite run survey");
      shared.queued = nullptr;
    }
  }
  // layout: the file's own, or — with a compressed column — the staging image's
  std::vector<const PqwPlan*> parts;
  std::vector<PqwSizes> sizes;
  for (PqwCall& c : calls) {
    if (blooms) pqb_size(c.P.cols, c.P.g, c.stats, &c.P.bloom);
    if (c.P.n_bytes > 0) pqy_scan(c.P.g, c.P.n_bytes, &c.P.strings);
    parts.push_back(&c.P);
    sizes.push_back(PqwSizes{c.stats, &c.delta_bytes, c.P.n_runs > 0 ? &c.run_bytes : nullptr, nullptr, c.P.n_bytes > 0 ? &c.P.strings.page_bytes : nullptr});
  }
  const PqwLayout L = pqw_layout(parts, sizes);
  pt.mark("pqwrite layout");
  // the encode passes, the filters' insert pass in front of them
  for (PqwCall& c : calls) if (blooms) pqb_insert_pass(&c);
  pqw_image(&calls[0], L);
  for (size_t pi = 0; pi < calls.size(); pi++) pqw_encode_passes(&calls[pi], L.parts[pi]);
  // with a compressed column `image` is the staging image: compress it (the second wait), lay the file out again, gather
  const bool squeezed = n_compressed > 0;
  PqwLayout F; PqsTables t;
  if (squeezed) {
    pqs_compress_pass(&calls[0], L, &t);
    std::vector<PqwSizes> final_sizes;
    for (const PqwSizes& z : sizes) final_sizes.push_back(PqwSizes{z.stats, z.delta_bytes, z.run_bytes, &t.page_elements, z.stream_bytes});
    F = pqw_layout(parts, final_sizes);
    pt.mark("pqwrite final layout");
    pqs_gather_pass(&calls[0], L, F, &t);
  }
  // deliver: what crosses the link is the file's own image
  *n_bytes = (int64_t)pqw_deliver(calls, squeezed ? F : L, squeezed ? final_image.p : image.p, &file);
  *bytes = file.p; file.p = nullptr;
}
#endif

}  // namespace fdb
