// fdb_pqwrite.cpp — a resident record as one Parquet file (fdb_batch_to_parquet), the encoders running on the device.
//
// ≙ Table.writeRecordsToParquet → pqarrow.RecordsToFile → recordToRows (table.go:1436-1459, pqarrow/parquet.go:85-139, :375-400): the
// reference builds one parquet.Value per cell on the CPU. Here the host decides a layout and writes what is small — page headers, run
// headers, dictionary pages, the footer (a thrift compact writer of this file's own) — and the device writes every payload:
//   1. survey (pqw_survey_kernel): per (column, page) the non-NULL rows and, of index columns, the smallest and largest index; per tile
//      the rank of its first value. Only the per-page table comes back.
//   2. layout (host): with it every page's size is known, so every payload's final file offset is.
//   3. encode (pqw_encode_kernel): every payload straight to that offset in ONE image of the file body, holes where the host's bytes go.
//   4. one device→host copy of the image into the returned buffer; the host fills the holes and appends the footer.
// fdb_selftest_parquet_write runs the same layout and tail over a host record, the two kernels replaced by a host walk of the same
// arithmetic (fdb_pqwrite.h) — byte-identical files, no GPU. Compiled with FDB_PQWRITE_HOST_ONLY the device half is left out
// (tools/asan_parquet_write.sh).
//
// File: PAR1 | per column [dictionary page] data pages V1 | FileMetaData | length | PAR1. Flat schema, one row group, UNCOMPRESSED,
// definition levels RLE (one RLE run when a page has no NULL or only NULLs, else one bit-packed run whose payload is the validity
// bitmap's bytes), no repetition levels. I64 → INT64 PLAIN; U64 → INT64 PLAIN, Int(64, unsigned) (writeUint64, parquet.go:154-165);
// F64 → DOUBLE PLAIN; BOOL → BOOLEAN PLAIN; dictionary and plain string / binary columns → BYTE_ARRAY, a PLAIN dictionary page of the
// interned dictionary's entries in entry order + RLE_DICTIONARY pages: the width byte, then ONE bit-packed run — or one RLE run where all
// non-NULL indices of the page are equal, as in the leading sorting columns of an ordered record. An all-NULL column with an empty
// dictionary has no dictionary page and PLAIN pages of zero values.
//
// fdb_batch_to_parquet_encoded: an I64 / U64 column may be asked to be written DELTA_BINARY_PACKED instead (blocks of 128, 4 miniblocks; the
// rule is spelled out in fdb_pqdelta.h). Its pages' sizes depend on the values, so between survey and layout the DELTA passes of
// fdb_pqdelta.hip run — compaction of the columns with a bitmap, block survey, page walk — and the page sizes come back with the survey's
// table, in the same wait; after the layout the DELTA encoder writes the pages' value bytes into the same image, beside the encode pass,
// which for such a column writes the definition levels only. The host walk has its counterparts (pqd_survey_host / pqd_encode_host).
//
// fdb_batch_to_parquet_compressed: a column may be asked to be SNAPPY as well (the rule is spelled out in fdb_pqsnappy.h). Steps 1 – 3 are
// then what they were, but the image they fill is a STAGING image in HBM, laid out as the uncompressed file; after them
//   4. the host's few bytes inside the bodies of the pages to be compressed are uploaded and placed (a body has to be whole),
//   5. every fragment of every such body is compressed into its slot of scratch, the sizes are summed per page, and only those come back,
//   6. the host lays the file out again (pqw_layout with the sizes; dictionary pages it compresses itself), and ONE gather launch moves
//      the fragments' elements and the chunks of the uncompressed columns into the final image,
//   7. which is what is copied out; headers, block preambles, dictionary pages and the footer are the host's, as before.
// Device memory: staging + scratch + final image, about 3 × the file body, all of it the call's and freed on every path. Without a
// compressed column nothing of this runs: the path, its launches, allocations and copies are those of fdb_batch_to_parquet_encoded.
//
// fdb_batch_to_parquet_indexed: min / max statistics, the page index and sorting_columns, when asked for (the rules are spelled out in
// include/frostdb_amd.h, the keys in fdb_pqstats.h). After the survey — before the DELTA passes — the min / max pass of fdb_pqstats.hip
// folds an order-preserving key of every value that counts into a (column, page) table, which comes back with the survey's table in the
// same wait. The rest is the host's, inside pqw_layout: pages folded into chunk bounds, keys mapped back (a rank to an entry), the zero
// rule, the cut of BYTE_ARRAY bounds, the boundary order, and the thrift of Statistics, ColumnIndex, OffsetIndex, column_orders and
// sorting_columns. The index bytes follow the body in the file (PqwLayout::tail, written by pqw_finish); the image stays the body. For a
// compressed file the index is the final layout's. Without index options nothing of this runs.
//
// fdb_batch_to_parquet_filtered: a split-block bloom filter per chosen column (the rule is spelled out in fdb_pqbloom.h and in
// include/frostdb_amd.h). The host hashes the entries of the chosen index columns once (entry_hashes, fdb_sortplan.h). The survey's
// table gives every filter its size (pqb_size), so the layout can place them — after the last chunk's pages, in column order, each a
// header (a host piece) and then its bitset (PqwLayout::blooms), in front of the page index — and the insert pass of fdb_pqbloom.hip
// runs then, on the call's stream beside the encode pass, into ONE zeroed table of bitsets from the call's arena, each 32-byte aligned
// there (the atomics want that; a file offset is arbitrary, so the bitsets are not part of the image). They come back after the image,
// one copy per filter straight to its offset in the returned bytes, in the wait of the image's copy: no wait is added. For a compressed
// file the offsets are the final layout's; filters are never compressed. The host walk is pqb_insert_host. Without a chosen column
// nothing of this runs.
//
// fdb_batch_to_parquet_runs: RLE runs INSIDE a page's dictionary indices and definition levels, on the columns chosen (the rule is
// spelled out in fdb_pqruns.h and in include/frostdb_amd.h) — what a record sorted by its label columns asks for. A chosen stream of a
// page that would be ONE bit-packed run is cut into RLE and bit-packed runs instead, never longer. Its size depends on the data, so the
// run passes of fdb_pqruns.hip sit where DELTA's do: after the survey the compaction of the indices of the chosen columns with a bitmap
// (scratch of the call's arena) and the run survey, whose table of sizes comes back with the survey's in the same wait; pqw_layout holds
// every size to the rule's bounds and places the stream (PqwLayout::run_out; the run headers are the device's, so the host's `pre` / `vpre`
// shrink to the levels' length and the width byte); after the layout the run encoder writes the runs into the same image, beside the
// encode pass, which leaves such a stream alone. A SNAPPY column's pages go through the staging image as ever. The host walk is
// pqr_survey_host / pqr_encode_host. Without a chosen stream nothing of this runs.
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
  enum { T_TRUE = 1, T_FALSE = 2, T_BYTE = 3, T_I32 = 5, T_I64 = 6, T_BINARY = 8, T_LIST = 9, T_STRUCT = 12 };
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
enum { ENC_PLAIN = 0, ENC_RLE = 3, ENC_DELTA_BINARY_PACKED = 5, ENC_RLE_DICTIONARY = 8 };
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
  int64_t dict_off = -1, data_off = 0, bytes = 0, raw_bytes = 0, nulls = 0;  // bytes: as stored; raw_bytes: the bodies uncompressed (headers in both)
  // with statistics only
  std::vector<PageLoc> pages;
  bool has_bounds = false;
  std::string min, max;                                                     // Statistics.min_value / max_value
  int64_t offset_index_off = -1, offset_index_len = 0, column_index_off = -1, column_index_len = 0;
  int64_t bloom_off = -1, bloom_len = 0;                                    // with a bloom filter only: its header's offset, header + bitset
};

std::string footer(const std::vector<PqwColumn>& cols, const std::vector<ChunkMeta>& chunks, int64_t rows, int64_t body_bytes, const PqxIndex* x) {
  Thrift t;
  t.open();
  t.i32(1, 1);
  t.list(2, Thrift::T_STRUCT, cols.size() + 1);
  t.open(); t.i32(3, 0); t.string(4, "schema"); t.i32(5, (int32_t)cols.size()); t.close();
  for (const PqwColumn& c : cols) {
    t.open();
    t.i32(1, c.physical);
    t.i32(3, c.optional ? 1 : 0);
    t.string(4, c.name);
    if (c.physical == PT_BYTE_ARRAY && c.utf8) { t.i32(6, 0); t.open(10); t.open(1); t.close(); t.close(); }                            // UTF8; LogicalType.STRING
    if (c.is_u64) { t.i32(6, 14); t.open(10); t.open(10); t.byte(1, 64); t.boolean(2, false); t.close(); t.close(); }                    // UINT_64; LogicalType.INTEGER(64, unsigned)
    t.close();
  }
  t.i64(3, rows);
  t.list(4, Thrift::T_STRUCT, 1);
  t.open();  // RowGroup
  t.list(1, Thrift::T_STRUCT, cols.size());
  for (size_t k = 0; k < cols.size(); k++) {
    const PqwColumn& c = cols[k];
    const ChunkMeta& m = chunks[k];
    t.open();  // ColumnChunk
    t.i64(2, m.dict_off >= 0 ? m.dict_off : m.data_off);
    t.open(3);  // ColumnMetaData
    t.i32(1, c.physical);
    const bool dict = c.pq_kind == FDB_PQW_INDEX;
    t.list(2, Thrift::T_I32, 1 + (c.optional ? 1 : 0) + (dict ? 1 : 0));  // (RLE: the definition levels, which a required column does not have)
    t.zigzag(c.delta_slot >= 0 ? ENC_DELTA_BINARY_PACKED : ENC_PLAIN); if (c.optional) t.zigzag(ENC_RLE); if (dict) t.zigzag(ENC_RLE_DICTIONARY);
    t.list(3, Thrift::T_BINARY, 1); t.str(c.name);
    t.i32(4, c.codec);  // 0 UNCOMPRESSED, 1 SNAPPY
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
  int64_t raw_bytes = 0;
  for (const ChunkMeta& m : chunks) raw_bytes += m.raw_bytes;
  t.i64(2, raw_bytes);  // total_byte_size: uncompressed
  t.i64(3, rows);
  if (x != nullptr && !x->sorting.empty()) {
    t.list(4, Thrift::T_STRUCT, x->sorting.size());
    for (const fdb_parquet_sorting_column& sc : x->sorting) { t.open(); t.i32(1, sc.column); t.boolean(2, sc.descending != 0); t.boolean(3, sc.nulls_first != 0); t.close(); }
  }
  t.i64(5, 4);
  t.i64(6, body_bytes - 4);
  t.close();
  t.string(6, "frostdb_amd 0.1.0");
  if (x != nullptr && x->statistics > 0) {  // column_orders: TypeDefinedOrder for every column
    t.list(7, Thrift::T_STRUCT, cols.size());
    for (size_t k = 0; k < cols.size(); k++) { t.open(); t.open(1); t.close(); t.close(); }
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

// ---- statistics and the page index: the host's half of the min / max pass (fdb_pqstats.h) -----------------------------------------------
std::string le64(uint64_t v) { std::string s(8, '\0'); std::memcpy(&s[0], &v, 8); return s; }

// The bytes a bound is written as: the key mapped back, parquet-format's zero rule for doubles (a minimum that is zero is −0.0, a
// maximum +0.0), an index key — a rank — as the bytes of an entry of that rank.
std::string pqx_bound(const PqwColumn& c, const PqxIndex& x, size_t k, uint64_t key, bool is_max) {
  const int mode = x.modes[k];
  if (mode == FDB_PQX_INDEX) {
    if (key >= x.entry_of_rank[k].size()) throw Error(FDB_ERR_STATE, "parquet write: the min / max pass names rank " + std::to_string(key) + " in column " + c.name);
    return c.dict->values[x.entry_of_rank[k][(size_t)key]];
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

// Everything that can refuse the record, before anything is launched.
std::vector<PqwColumn> pqw_columns(const std::vector<PqwInput>& in, int64_t rows, const fdb_parquet_write_options* opt, int32_t* page_rows, const int8_t* encodings,
                                   int32_t n_encodings, const int8_t* codecs, int32_t n_codecs) {
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
    if (codecs[k] < 0 || codecs[k] > 1) throw Error(FDB_ERR_INVALID, "parquet write: codecs[" + std::to_string(k) + "] is " + std::to_string((int)codecs[k]) + " (0 UNCOMPRESSED, 1 SNAPPY)");
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
    o.values = c.values;
    o.validity = nulls ? c.validity : nullptr;
    cols.push_back(std::move(o));
  }
  return cols;
}

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

void pqx_prepare(const std::vector<PqwColumn>& cols, PqxIndex* x) {
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
    const uint32_t per = mode == FDB_PQX_INDEX ? FDB_PQX_UNIT_INDEX : FDB_PQX_UNIT_V64, rank_len = (uint32_t)x->ranks[k].size();
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
            if (mode == FDB_PQX_INDEX) counts = fdb_pqx_index_key(x->ranks[k].data(), rank_len, ((const uint32_t*)c.values)[row], &key);
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

void pqb_prepare(const std::vector<PqwColumn>& cols, PqbPlan* b) {
  b->hashes.assign(cols.size(), std::vector<uint64_t>());
  for (size_t k = 0; k < cols.size() && b->any(); k++)
    if (b->on[k] != 0 && cols[k].pq_kind == FDB_PQW_INDEX && cols[k].dict != nullptr)
      b->hashes[k] = entry_hashes(*cols[k].dict, [](const unsigned char* p, size_t n) { return fdb_pqb_hash(p, n); });
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
    const std::vector<uint64_t>& hashes = b.hashes[k];
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
              const uint32_t v = ((const uint32_t*)c.values)[row];
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

std::string pqs_block_host(const unsigned char* body, size_t n) {
  std::string block = varint_bytes(n);
  std::vector<uint32_t> table(FDB_PQS_TABLE);
  std::vector<unsigned char> out(fdb_pqs_bound(FDB_PQS_FRAGMENT));
  for (size_t at = 0; at < n; at += FDB_PQS_FRAGMENT) {
    const uint32_t len = (uint32_t)std::min<size_t>(FDB_PQS_FRAGMENT, n - at);
    block.append((const char*)out.data(), fdb_pqs_compress_fragment_host(body + at, len, table.data(), out.data()));
  }
  return block;
}

PqwLayout pqw_layout(const std::vector<PqwColumn>& cols, const FdbPqwGeom& g, const std::vector<FdbPqwPageStat>& stats, const std::vector<uint32_t>& delta_bytes,
                     const std::vector<uint32_t>* page_elements, const PqxIndex* x, const PqbPlan* bloom, const std::vector<uint32_t>* run_bytes) {
  if (x != nullptr && !x->any()) x = nullptr;
  if (bloom != nullptr && !bloom->any()) bloom = nullptr;
  if (bloom != nullptr && bloom->bytes.size() != cols.size()) throw Error(FDB_ERR_STATE, "parquet write: the bloom filter sizes do not match the record");
  const bool bounds = x != nullptr && x->statistics > 0;
  if (bounds && (x->table.size() != 2 * stats.size() || x->modes.size() != cols.size())) throw Error(FDB_ERR_STATE, "parquet write: the min / max table does not match the record");
  if (stats.size() != cols.size() * (size_t)g.n_pages) throw Error(FDB_ERR_STATE, "parquet write: the survey table does not match the record");
  if (delta_bytes.size() != pqw_delta_columns(cols) * (size_t)g.n_pages) throw Error(FDB_ERR_STATE, "parquet write: the table of DELTA page sizes does not match the record");
  if (page_elements != nullptr && page_elements->size() != pqw_compressed_columns(cols) * (size_t)g.n_pages)
    throw Error(FDB_ERR_STATE, "parquet write: the table of compressed page sizes does not match the record");
  const size_t n_run_streams = pqr_streams(cols);
  if ((run_bytes != nullptr ? run_bytes->size() : 0) != n_run_streams * (size_t)g.n_pages) throw Error(FDB_ERR_STATE, "parquet write: the table of run-encoded sizes does not match the record");
  // The bytes of a page's stream cut into runs, held to the rule's bounds: no more than its one bit-packed run, no less than a run.
  const auto run_payload = [&](const PqwColumn& c, int slot, int64_t p, uint32_t n, uint32_t w) {
    const uint32_t bytes = (*run_bytes)[(size_t)slot * (size_t)g.n_pages + (size_t)p];
    if (bytes > fdb_pqr_max_bytes(n, w) || bytes < fdb_pqr_min_bytes(w))
      throw Error(FDB_ERR_STATE, "parquet write: the run survey sizes a stream of " + std::to_string(n) + " symbols of " + std::to_string(w) + " bits at " + std::to_string(bytes) + " bytes (" + c.name + ")");
    return (uint64_t)bytes;
  };
  const bool final_form = page_elements != nullptr;  // else: every page as it is before compression — the file of a record without codecs, the staging image of one with
  size_t next_compressed = 0;
  PqwLayout L;
  L.chunk_off.assign(cols.size(), 0);
  L.chunk_len.assign(cols.size(), 0);
  L.delta_out.assign(delta_bytes.size(), FDB_PQW_NONE);
  L.out.assign(stats.size(), FdbPqwPageOut{FDB_PQW_NONE, FDB_PQW_NONE});
  L.run_out.assign(n_run_streams * (size_t)g.n_pages, FDB_PQW_NONE);
  uint64_t cur = 0;
  L.put(cur, "PAR1");
  cur += 4;
  std::vector<ChunkMeta> chunks(cols.size());
  for (size_t k = 0; k < cols.size(); k++) {
    const PqwColumn& c = cols[k];
    ChunkMeta& m = chunks[k];
    const uint64_t chunk_start = cur;
    const bool squeeze = final_form && c.codec != 0;  // this chunk's pages are written as Snappy blocks
    if (c.pq_kind == FDB_PQW_INDEX) {
      const std::string body = dictionary_body(*c.dict);
      const std::string stored = squeeze ? pqs_block_host((const unsigned char*)body.data(), body.size()) : std::string();  // (host bytes already: the header's walk)
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
      if (c.delta_slot >= 0) {
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
          if (s.mn > s.mx || s.mx >= c.entries)
            throw Error(FDB_ERR_INVALID, "parquet write: dictionary index out of range in column " + c.name + ": a valid row holds " + std::to_string(s.mx) + ", the dictionary has " + std::to_string(c.entries) + " entries");
          if (s.mn == s.mx) {  // one RLE run: the count, the value in ⌈w/8⌉ bytes
            vpre += varint_bytes((uint64_t)cnt << 1);
            for (uint32_t b = 0; b < (c.width + 7) / 8; b++) vpre.push_back((char)(s.mn >> (8 * b)));
          } else if (value_runs) {
            value_payload = run_payload(c, c.run_values, p, cnt, c.width);
          } else {
            vpre += varint_bytes(((uint64_t)fdb_pqw_groups(cnt) << 1) | 1);
            value_payload = fdb_pqw_packed_bytes(cnt, c.width);
          }
        }
      }
      const uint64_t body = pre.size() + level_payload + vpre.size() + value_payload;
      if (squeeze) {  // header, the block's preamble, then the elements the compressor made of the body
        const uint64_t elements = (*page_elements)[next_compressed++];
        if (elements > (uint64_t)fdb_pqs_fragments(body) * fdb_pqs_bound(FDB_PQS_FRAGMENT) || (body > 0) != (elements > 0))
          throw Error(FDB_ERR_STATE, "parquet write: the compressor sizes a page body of " + std::to_string(body) + " bytes at " + std::to_string(elements) + " (" + c.name + ")");
        const std::string preamble = varint_bytes(body);
        const std::string hdr = page_header(PAGE_DATA, (int64_t)body, (int64_t)(preamble.size() + elements), n, encoding);
        m.raw_bytes += (int64_t)(hdr.size() + body);
        if (bounds) m.pages.push_back(PageLoc{cur, hdr.size() + preamble.size() + elements, n, cnt});
        L.put(cur, hdr + preamble); cur += hdr.size() + preamble.size();
        L.pages.push_back(PqwLayout::Page{cur, body});
        cur += elements;
        continue;
      }
      const std::string hdr = page_header(PAGE_DATA, (int64_t)body, (int64_t)body, n, encoding);
      m.raw_bytes += (int64_t)(hdr.size() + body);
      if (bounds) m.pages.push_back(PageLoc{cur, hdr.size() + body, n, cnt});
      FdbPqwPageOut& o = L.out[k * (size_t)g.n_pages + (size_t)p];
      if (c.codec == 0) { L.put(cur, hdr + pre); cur += hdr.size() + pre.size(); }
      else {  // the staging image of a page to be compressed: the host's bytes inside the body are placed on their own, before the compressor runs
        cur += hdr.size();
        L.pages.push_back(PqwLayout::Page{cur, body});
        L.put_body(cur, pre); cur += pre.size();
      }
      if (level_runs) { L.run_out[(size_t)c.run_levels * (size_t)g.n_pages + (size_t)p] = cur; cur += level_payload; }
      else if (level_payload > 0) { o.levels_off = cur; cur += level_payload; }
      if (c.codec == 0) L.put(cur, vpre); else L.put_body(cur, vpre);
      cur += vpre.size();
      if (value_runs && c.pq_kind == FDB_PQW_INDEX) { L.run_out[(size_t)c.run_values * (size_t)g.n_pages + (size_t)p] = cur; cur += value_payload; }
      else if (c.delta_slot >= 0) { L.delta_out[(size_t)c.delta_slot * (size_t)g.n_pages + (size_t)p] = cur; cur += value_payload; }  // (the encode pass leaves the values alone)
      else if (value_payload > 0) { o.values_off = cur; cur += value_payload; }
    }
    m.bytes = (int64_t)(cur - chunk_start);
    m.nulls = g.rows - valid;
    L.chunk_off[k] = chunk_start;
    L.chunk_len[k] = cur - chunk_start;
  }
  L.body_bytes = cur;
  if (bloom != nullptr) {  // after the last chunk's pages, in column order: header, bitset, no padding
    for (size_t k = 0; k < cols.size(); k++) {
      if (bloom->on[k] == 0) continue;
      unsigned char hdr[FDB_PQB_MAX_HEADER];
      const uint32_t len = fdb_pqb_header(bloom->bytes[k], hdr);
      chunks[k].bloom_off = (int64_t)cur; chunks[k].bloom_len = (int64_t)len + bloom->bytes[k];
      L.put(cur, std::string((const char*)hdr, len)); cur += len;
      L.blooms.push_back(PqwLayout::Bloom{k, cur, bloom->bytes[k]}); cur += bloom->bytes[k];
    }
    L.bloom_bytes = cur - L.body_bytes;
  }
  if (bounds) {  // chunk bounds; with statistics == 2 every column's ColumnIndex, then every column's OffsetIndex, after the pages
    for (size_t k = 0; k < cols.size(); k++) {
      const std::string ci = pqx_column_index(cols[k], *x, k, (size_t)g.n_pages, &chunks[k]);
      if (ci.empty()) continue;
      chunks[k].column_index_off = (int64_t)(cur + L.tail.size()); chunks[k].column_index_len = (int64_t)ci.size();
      L.tail += ci;
    }
    for (size_t k = 0; k < cols.size() && x->statistics == 2; k++) {
      const std::string oi = pqx_offset_index(chunks[k], g.page_rows);
      chunks[k].offset_index_off = (int64_t)(cur + L.tail.size()); chunks[k].offset_index_len = (int64_t)oi.size();
      L.tail += oi;
    }
  }
  L.footer = footer(cols, chunks, g.rows, (int64_t)L.body_bytes, x);
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
void pqd_survey_host(const std::vector<PqwColumn>& cols, const FdbPqwGeom& g, const std::vector<FdbPqwPageStat>& stats, const std::vector<uint32_t>& tile_base, PqdHost* d) {
  const size_t n_d = pqw_delta_columns(cols), bpp = (size_t)fdb_pqd_blocks_per_page(g.page_rows);
  d->dense.assign(n_d, std::vector<uint64_t>());
  d->blocks.assign(n_d * (size_t)g.n_pages * bpp, FdbPqdBlock{0, 0, 0, 0, 0});
  d->page_bytes.assign(n_d * (size_t)g.n_pages, 0);
  for (size_t k = 0; k < cols.size(); k++) {
    const PqwColumn& c = cols[k];
    if (c.delta_slot < 0) continue;
    const size_t slot = (size_t)c.delta_slot;
    if (c.validity != nullptr) {  // compaction, tile by tile: a value goes to the survey's rank of its tile + its rank inside the tile
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
              if ((w >> b) & 1) std::memcpy(dst + before + (uint32_t)fdb_pqw_popc(w & ((1ull << b) - 1)), (const unsigned char*)c.values + (size_t)(first + wi * 64 + b) * 8, 8);
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

void selftest_parquet_write(const HostRecordView& view, const fdb_parquet_write_options* opt, uint8_t** bytes, int64_t* n_bytes, const int8_t* encodings, int32_t n_encodings,
                            const int8_t* codecs, int32_t n_codecs, const fdb_parquet_index_options* index, const fdb_parquet_bloom_options* bloom,
                            const fdb_parquet_run_options* runs) {
  // the record in the resident form: 8 bytes per value (a bool widened to 1 / 2), a uint32 per index, bitmaps at bit 0 in whole words
  const size_t rows = (size_t)view.rows;
  std::vector<std::vector<uint32_t>> keep_idx(view.cols.size());
  std::vector<std::vector<int64_t>> keep_i64(view.cols.size());
  std::vector<std::vector<uint8_t>> keep_bits(view.cols.size());
  std::vector<PqwInput> in;
  for (size_t k = 0; k < view.cols.size(); k++) {
    const HostColView& c = view.cols[k];
    PqwInput o;
    o.name = c.name; o.format = c.format; o.kind = c.kind; o.null_count = c.null_count;
    if (c.kind == ColKind::I64 || c.kind == ColKind::U64 || c.kind == ColKind::F64) {
      o.values = rows > 0 ? (const unsigned char*)c.values + (size_t)c.offset * 8 : nullptr;
    } else if (c.kind == ColKind::BOOL) {
      keep_i64[k].assign(rows + 1, 0);
      const uint8_t* bits = (const uint8_t*)c.values;
      for (size_t i = 0; i < rows; i++) keep_i64[k][i] = 1 + ((bits[(c.offset + (int64_t)i) >> 3] >> ((c.offset + (int64_t)i) & 7)) & 1);
      o.values = keep_i64[k].data();
    } else if (c.kind == ColKind::DICT) {
      o.dict = read_dictionary(c);
      keep_idx[k].assign(rows + 1, 0);
      for (size_t i = 0; i < rows; i++) {
        const size_t at = (size_t)c.offset + i;
        switch (c.index_width) {
          case 1: keep_idx[k][i] = ((const uint8_t*)c.values)[at]; break;
          case 2: keep_idx[k][i] = ((const uint16_t*)c.values)[at]; break;
          case 4: keep_idx[k][i] = ((const uint32_t*)c.values)[at]; break;
          default: keep_idx[k][i] = (uint32_t)((const uint64_t*)c.values)[at]; break;
        }
      }
      o.values = keep_idx[k].data();
    } else if (c.kind == ColKind::STR) {
      o.dict = encode_plain(c, &keep_idx[k]);
      keep_idx[k].resize(rows + 1, 0);
      o.kind = ColKind::DICT;
      o.values = keep_idx[k].data();
    }
    if (c.null_count > 0 && c.validity != nullptr) {
      keep_bits[k].assign((rows + 63) / 64 * 8 + 8, 0);
      copy_bits(c.validity, c.offset, c.length, keep_bits[k].data());
      o.validity = keep_bits[k].data();
    }
    in.push_back(std::move(o));
  }
  int32_t page_rows = 0;
  std::vector<PqwColumn> cols = pqw_columns(in, view.rows, opt, &page_rows, encodings, n_encodings, codecs, n_codecs);
  PqxIndex x = pqx_plan(index, cols.size());
  PqbPlan bl = pqb_plan(bloom, cols);
  const size_t n_runs = pqr_plan(runs, &cols);
  const FdbPqwGeom g = pqw_geometry(view.rows, page_rows, cols.size());
  std::vector<FdbPqwPageStat> stats;
  std::vector<uint32_t> tile_base;
  pqw_survey_host(cols, g, &stats, &tile_base);
  std::vector<unsigned char> bitsets;
  if (bl.any()) { pqb_prepare(cols, &bl); pqb_size(cols, g, stats, &bl); }
  const auto place_bitsets = [&](const PqwLayout& at, uint8_t* file) {  // the insert pass, walked, and every bitset to its place in the file
    if (at.blooms.empty()) return;
    bitsets.assign((size_t)bl.table_bytes, 0);
    pqb_insert_host(cols, g, bl, bitsets.data());
    for (const PqwLayout::Bloom& f : at.blooms) std::memcpy(file + f.bits_off, bitsets.data() + bl.table_off[f.col], (size_t)f.bytes);
  };
  if (x.statistics > 0) { pqx_prepare(cols, &x); pqx_minmax_host(cols, g, &x); }
  PqdHost delta;
  pqd_survey_host(cols, g, stats, tile_base, &delta);
  PqrHost rn;
  if (n_runs > 0) pqr_survey_host(cols, g, stats, &rn);
  const std::vector<uint32_t>* run_bytes = n_runs > 0 ? &rn.page_bytes : nullptr;
  const bool squeezed = pqw_compressed_columns(cols) > 0;  // then L is the staging image's layout, and the index is the final one's
  const PqwLayout L = pqw_layout(cols, g, stats, delta.page_bytes, nullptr, squeezed ? nullptr : &x, squeezed ? nullptr : &bl, run_bytes);
  std::vector<unsigned char> image(((size_t)L.body_bytes + 8 + 3) / 4 * 4, 0);
  pqw_encode_host(cols, g, L.out, tile_base, image.data());
  pqd_encode_host(cols, g, stats, delta, L.delta_out, image.data());
  if (n_runs > 0) pqr_encode_host(rn, L.run_out, image.data());
  if (!squeezed) {
    const size_t file_bytes = L.file_bytes();
    uint8_t* file = pqw_alloc_bytes(file_bytes, false);
    std::memcpy(file, image.data(), (size_t)L.body_bytes);
    place_bitsets(L, file);
    pqw_finish(L, file);
    *bytes = file;
    *n_bytes = (int64_t)file_bytes;
    return;
  }
  // `image` is the staging image: the bodies made whole, every page compressed fragment by fragment, the file laid out again, the
  // elements and the uncompressed chunks moved to where it wants them — the passes of fdb_pqsnappy.hip, walked
  for (const PqwLayout::Piece& p : L.body_pieces) std::memcpy(image.data() + p.off, L.body_blob.data() + p.pos, p.len);
  std::vector<uint32_t> page_elements(L.pages.size(), 0), table(FDB_PQS_TABLE);
  std::vector<std::string> elements(L.pages.size());
  std::vector<unsigned char> slot(fdb_pqs_slot_bytes());
  for (size_t i = 0; i < L.pages.size(); i++) {
    for (uint64_t at = 0; at < L.pages[i].body; at += FDB_PQS_FRAGMENT) {
      const uint32_t len = (uint32_t)std::min<uint64_t>(FDB_PQS_FRAGMENT, L.pages[i].body - at);
      elements[i].append((const char*)slot.data(), fdb_pqs_compress_fragment_host(image.data() + L.pages[i].off + at, len, table.data(), slot.data()));
    }
    page_elements[i] = (uint32_t)elements[i].size();
  }
  const PqwLayout F = pqw_layout(cols, g, stats, delta.page_bytes, &page_elements, &x, &bl, run_bytes);
  const size_t file_bytes = F.file_bytes();
  uint8_t* file = pqw_alloc_bytes(file_bytes, false);
  for (size_t i = 0; i < F.pages.size(); i++) std::memcpy(file + F.pages[i].off, elements[i].data(), elements[i].size());
  for (size_t k = 0; k < cols.size(); k++)
    if (cols[k].codec == 0) std::memcpy(file + F.chunk_off[k], image.data() + L.chunk_off[k], (size_t)L.chunk_len[k]);
  place_bitsets(F, file);
  pqw_finish(F, file);
  *bytes = file;
  *n_bytes = (int64_t)file_bytes;
}

#ifndef FDB_PQWRITE_HOST_ONLY
void batch_to_parquet(const DeviceBatch& b, const fdb_parquet_write_options* opt, uint8_t** bytes, int64_t* n_bytes, const int8_t* encodings, int32_t n_encodings,
                      const int8_t* codecs, int32_t n_codecs, const fdb_parquet_index_options* index, const fdb_parquet_bloom_options* bloom,
                      const fdb_parquet_run_options* runs) {
  std::vector<PqwInput> in;
  for (const DevColumn& c : b.cols) {
    PqwInput o;
    o.name = c.name; o.format = c.format; o.kind = c.kind; o.dict = c.dict; o.null_count = c.null_count; o.values = c.d_values; o.validity = c.d_validity;
    in.push_back(std::move(o));
  }
  int32_t page_rows = 0;
  std::vector<PqwColumn> cols = pqw_columns(in, b.rows, opt, &page_rows, encodings, n_encodings, codecs, n_codecs);
  PqxIndex x = pqx_plan(index, cols.size());
  const size_t n_runs = pqr_plan(runs, &cols);
  const bool bounds = x.statistics > 0;
  if (bounds) {
    pqx_prepare(cols, &x);
    for (size_t k = 0; k < cols.size(); k++)
      if (((uintptr_t)cols[k].values & 15u) != 0)  // (the pass loads 16 bytes of values at a time)
        throw Error(FDB_ERR_UNSUPPORTED, "parquet write: the values of column " + cols[k].name + " are not 16-byte aligned (statistics)");
  }
  PqbPlan bl = pqb_plan(bloom, cols);
  if (bl.any()) {
    pqb_prepare(cols, &bl);
    for (size_t k = 0; k < cols.size(); k++)
      if (bl.on[k] != 0 && ((uintptr_t)cols[k].values & 15u) != 0)  // (the pass loads 16 bytes of values at a time)
        throw Error(FDB_ERR_UNSUPPORTED, "parquet write: the values of column " + cols[k].name + " are not 16-byte aligned (bloom filter)");
  }
  const FdbPqwGeom g = pqw_geometry(b.rows, page_rows, cols.size());
  const size_t n_delta = pqw_delta_columns(cols), n_compressed = pqw_compressed_columns(cols);
  struct Bytes { uint8_t* p = nullptr; ~Bytes() { pqw_free_bytes(p); } } file;
  if (b.rows == 0 || cols.empty()) {  // nothing for the device to do (no data page: the dictionary pages are the host's, compressed or not)
    const std::vector<uint32_t> no_pages;
    if (bounds) x.table.assign(2 * cols.size() * (size_t)g.n_pages, 0);  // (no page: no slot)
    const std::vector<FdbPqwPageStat> no_stats(cols.size() * (size_t)g.n_pages, FdbPqwPageStat{0, 0, 0, 0});
    if (bl.any()) pqb_size(cols, g, no_stats, &bl);
    const std::vector<uint32_t> no_runs(n_runs * (size_t)g.n_pages, 0);
    const PqwLayout L = pqw_layout(cols, g, no_stats, {}, n_compressed > 0 ? &no_pages : nullptr, &x, &bl, n_runs > 0 ? &no_runs : nullptr);
    const size_t file_bytes = L.file_bytes();
    file.p = pqw_alloc_bytes(file_bytes, false);
    for (const PqwLayout::Bloom& f : L.blooms) std::memset(file.p + f.bits_off, 0, (size_t)f.bytes);  // (no value: one zero block each)
    pqw_finish(L, file.p);
    *bytes = file.p; *n_bytes = (int64_t)file_bytes; file.p = nullptr;
    return;
  }
  PhaseTimer pt;  // FDB_PROFILE=1: the passes timed apart (the encode pass is then waited for on its own)
  struct Image { int device; void* p = nullptr; ~Image() { if (p != nullptr) device_pool_free(device, p); } } image{b.device}, scratch{b.device}, final_image{b.device};  // (before the scope: freed after its wait; the last two: compressed columns only)
  CallScope cs(b.device);
  hipStream_t stream = cs.ctx->stream;
  DrainOnUnwind drain{stream};
  std::vector<FdbPqwCol> kc(cols.size());
  for (size_t k = 0; k < cols.size(); k++) {
    std::memset(&kc[k], 0, sizeof(FdbPqwCol));
    kc[k].values = cols[k].values; kc[k].validity = cols[k].validity; kc[k].width = (int32_t)cols[k].width;
    kc[k].kind = cols[k].pq_kind == PQW_NO_VALUES ? FDB_PQW_INDEX : cols[k].pq_kind;
  }
  const size_t items = cols.size() * (size_t)g.n_pages;
  const FdbPqwCol* d_cols = (const FdbPqwCol*)cs.ctx->stage(kc.data(), kc.size() * sizeof(FdbPqwCol));
  FdbPqwPageStat* d_stats = (FdbPqwPageStat*)cs.alloc(items * sizeof(FdbPqwPageStat));
  uint32_t* d_tile_base = (uint32_t*)cs.alloc(items * (size_t)g.tiles_per_page * 4);
  std::vector<FdbPqwPageStat> stats(items);
  // the DELTA columns: scratch for the dense values of those with a bitmap, the block table, the page sizes — all from the call's arena
  const size_t d_items = n_delta * (size_t)g.n_pages;
  std::vector<uint32_t> delta_bytes(d_items);
  const FdbPqdCol* d_dcols = nullptr;
  FdbPqdBlock* d_blocks = nullptr;
  uint32_t* d_page_bytes = nullptr;
  bool compact = false;
  if (n_delta > 0) {
    std::vector<FdbPqdCol> dc(n_delta);
    for (size_t k = 0; k < cols.size(); k++) {
      if (cols[k].delta_slot < 0) continue;
      FdbPqdCol& o = dc[(size_t)cols[k].delta_slot];
      std::memset(&o, 0, sizeof(FdbPqdCol));
      o.values = (const uint64_t*)cols[k].values; o.validity = cols[k].validity; o.col = (int32_t)k;
      o.dense = cols[k].validity != nullptr ? (uint64_t*)cs.alloc(((size_t)g.rows + 1) * 8) : (uint64_t*)const_cast<void*>(cols[k].values);  // (only ever read when it is the column)
      compact = compact || cols[k].validity != nullptr;
    }
    d_dcols = (const FdbPqdCol*)cs.ctx->stage(dc.data(), dc.size() * sizeof(FdbPqdCol));
    d_blocks = (FdbPqdBlock*)cs.alloc(d_items * (size_t)fdb_pqd_blocks_per_page(g.page_rows) * sizeof(FdbPqdBlock));
    d_page_bytes = (uint32_t*)cs.alloc(d_items * 4);
  }
  // the streams to be cut into runs: scratch for the dense indices of the columns with a bitmap, the table of sizes — from the call's arena
  const size_t r_items = n_runs * (size_t)g.n_pages;
  std::vector<uint32_t> run_bytes(r_items);
  const FdbPqrStream* d_streams = nullptr;
  uint32_t* d_run_bytes = nullptr;
  bool run_compact = false;
  if (n_runs > 0) {
    std::vector<FdbPqrStream> rs(n_runs);
    for (size_t k = 0; k < cols.size(); k++) {
      const PqwColumn& c = cols[k];
      if (c.run_values >= 0) {
        FdbPqrStream& o = rs[(size_t)c.run_values];
        std::memset(&o, 0, sizeof(FdbPqrStream));
        o.values = (const uint32_t*)c.values; o.validity = c.validity; o.col = (int32_t)k; o.width = (int32_t)c.width;
        o.dense = c.validity != nullptr ? (uint32_t*)cs.alloc(((size_t)g.rows + 8) * 4) : (uint32_t*)const_cast<void*>(c.values);  // (only ever read when it is the column)
        run_compact = run_compact || c.validity != nullptr;
      }
      if (c.run_levels >= 0) {
        FdbPqrStream& o = rs[(size_t)c.run_levels];
        std::memset(&o, 0, sizeof(FdbPqrStream));
        o.validity = c.validity; o.col = (int32_t)k; o.width = 1; o.levels = 1;
      }
    }
    d_streams = (const FdbPqrStream*)cs.ctx->stage(rs.data(), rs.size() * sizeof(FdbPqrStream));
    d_run_bytes = (uint32_t*)cs.alloc(r_items * 4);
  }
  b.note_reader(stream);
  hip_check(fdb_launch_pqw_survey(d_cols, g, d_stats, d_tile_base, stream), "parquet write: survey launch");
  hip_check(hipMemcpyAsync(stats.data(), d_stats, items * sizeof(FdbPqwPageStat), hipMemcpyDeviceToHost, stream), "hipMemcpyAsync(page table)");
  if (bounds) {  // the min / max pass (fdb_pqstats.hip): beside the survey, its table back in the same wait
    if (pt.on) { hip_check(hipStreamSynchronize(stream), "hipStreamSynchronize"); pt.mark("pqwrite survey"); }
    std::vector<FdbPqxCol> xc(cols.size());
    for (size_t k = 0; k < cols.size(); k++) {
      std::memset(&xc[k], 0, sizeof(FdbPqxCol));
      xc[k].values = cols[k].values; xc[k].validity = cols[k].validity; xc[k].mode = x.modes[k];
      const std::vector<uint32_t>& r = x.ranks[k];
      if (r.empty()) continue;
      uint32_t* d_ranks = (uint32_t*)cs.alloc(r.size() * 4);
      hip_check(hipMemcpyAsync(d_ranks, r.data(), r.size() * 4, hipMemcpyHostToDevice, stream), "hipMemcpyAsync(dictionary ranks)");  // (`x` outlives the wait)
      xc[k].ranks = d_ranks; xc[k].rank_len = (uint32_t)r.size();
    }
    const FdbPqxCol* d_xcols = (const FdbPqxCol*)cs.ctx->stage(xc.data(), xc.size() * sizeof(FdbPqxCol));
    unsigned long long* d_table = (unsigned long long*)cs.alloc(2 * items * 8);
    hip_check(hipMemsetAsync(d_table, 0xFF, items * 8, stream), "hipMemsetAsync(min table)");
    hip_check(hipMemsetAsync(d_table + items, 0, items * 8, stream), "hipMemsetAsync(max table)");
    hip_check(fdb_launch_pqx_minmax(d_xcols, g, d_table, stream), "parquet write: min / max launch");
    x.table.assign(2 * items, 0);
    hip_check(hipMemcpyAsync(x.table.data(), d_table, 2 * items * 8, hipMemcpyDeviceToHost, stream), "hipMemcpyAsync(min / max table)");
    if (pt.on) { hip_check(hipStreamSynchronize(stream), "hipStreamSynchronize"); pt.mark("pqwrite stats"); }
  }
  if (n_delta > 0) {
    if (pt.on && !bounds) { hip_check(hipStreamSynchronize(stream), "hipStreamSynchronize"); pt.mark("pqwrite survey"); }
    if (compact) hip_check(fdb_launch_pqd_compact(d_dcols, (int32_t)n_delta, g, d_tile_base, stream), "parquet write: DELTA compaction launch");
    if (pt.on) { hip_check(hipStreamSynchronize(stream), "hipStreamSynchronize"); pt.mark("pqwrite delta compact"); }
    hip_check(fdb_launch_pqd_survey(d_dcols, (int32_t)n_delta, g, d_stats, d_blocks, d_page_bytes, stream), "parquet write: DELTA block survey launch");
    hip_check(hipMemcpyAsync(delta_bytes.data(), d_page_bytes, d_items * 4, hipMemcpyDeviceToHost, stream), "hipMemcpyAsync(DELTA page sizes)");
  }
  if (n_runs > 0) {  // the run passes (fdb_pqruns.hip): beside the survey, their table back in the same wait
    if (pt.on) { hip_check(hipStreamSynchronize(stream), "hipStreamSynchronize"); pt.mark(n_delta > 0 ? "pqwrite delta survey" : bounds ? "pqwrite wait" : "pqwrite survey"); }
    if (run_compact) hip_check(fdb_launch_pqr_compact(d_streams, (int32_t)n_runs, g, d_tile_base, stream), "parquet write: run compaction launch");
    hip_check(fdb_launch_pqr_survey(d_streams, (int32_t)n_runs, g, d_stats, d_run_bytes, stream), "parquet write: run survey launch");
    hip_check(hipMemcpyAsync(run_bytes.data(), d_run_bytes, r_items * 4, hipMemcpyDeviceToHost, stream), "hipMemcpyAsync(run-encoded sizes)");
  }
  hip_check(hipStreamSynchronize(stream), "hipStreamSynchronize");
  pt.mark(n_runs > 0 ? "pqwrite run survey" : n_delta > 0 ? "pqwrite delta survey" : bounds && pt.on ? "pqwrite wait" : "pqwrite survey");
  if (bl.any()) pqb_size(cols, g, stats, &bl);
  const std::vector<uint32_t>* run_table = n_runs > 0 ? &run_bytes : nullptr;
  const PqwLayout L = pqw_layout(cols, g, stats, delta_bytes, nullptr, n_compressed > 0 ? nullptr : &x, n_compressed > 0 ? nullptr : &bl, run_table);
  const size_t file_bytes = L.file_bytes(), image_bytes = align_up((size_t)L.body_bytes + 8, 256);
  pt.mark("pqwrite layout");
  // The bloom filters (fdb_pqbloom.hip): the survey's table has sized them, so their bitsets — one zeroed table of the call's arena,
  // every bitset 32-byte aligned in it, which a file offset is not — are filled beside the encode pass, on the same stream. They come
  // back after the image, each straight to its place behind its header (bloom_out), in the wait of the image's copy.
  unsigned char* d_bitsets = nullptr;
  if (bl.any()) {
    std::vector<FdbPqbCol> bc;
    d_bitsets = (unsigned char*)cs.alloc((size_t)bl.table_bytes);
    for (size_t k = 0; k < cols.size(); k++) {
      if (bl.on[k] == 0) continue;
      FdbPqbCol o;
      std::memset(&o, 0, sizeof(FdbPqbCol));
      o.values = cols[k].values; o.validity = cols[k].validity; o.index = cols[k].pq_kind != FDB_PQW_V64;
      o.bits = (unsigned long long*)(d_bitsets + bl.table_off[k]); o.n_blocks = bl.bytes[k] / FDB_PQB_BLOCK_BYTES;
      const std::vector<uint64_t>& h = bl.hashes[k];
      if (!h.empty()) {
        uint64_t* d_hashes = (uint64_t*)cs.alloc(h.size() * 8);
        hip_check(hipMemcpyAsync(d_hashes, h.data(), h.size() * 8, hipMemcpyHostToDevice, stream), "hipMemcpyAsync(entry hashes)");  // (`bl` outlives the wait)
        o.hashes = d_hashes; o.hash_len = (uint32_t)h.size();
      }
      bc.push_back(o);
    }
    const FdbPqbCol* d_bcols = (const FdbPqbCol*)cs.ctx->stage(bc.data(), bc.size() * sizeof(FdbPqbCol));
    hip_check(hipMemsetAsync(d_bitsets, 0, (size_t)bl.table_bytes, stream), "hipMemsetAsync(bloom filter bitsets)");
    hip_check(fdb_launch_pqb_insert(d_bcols, (int32_t)bc.size(), g, stream), "parquet write: bloom filter launch");
    if (pt.on) { hip_check(hipStreamSynchronize(stream), "hipStreamSynchronize"); pt.mark("pqwrite bloom insert"); }
  }
  const auto bloom_out = [&](const PqwLayout& at, uint8_t* out) {
    for (const PqwLayout::Bloom& f : at.blooms)
      hip_check(hipMemcpyAsync(out + f.bits_off, d_bitsets + bl.table_off[f.col], (size_t)f.bytes, hipMemcpyDeviceToHost, stream), "hipMemcpyAsync(bloom filter bitset)");
    if (pt.on && !at.blooms.empty()) { hip_check(hipStreamSynchronize(stream), "hipStreamSynchronize"); pt.mark("pqwrite bloom copy"); }
  };
  image.p = device_pool_alloc(b.device, image_bytes);
  FdbPqwPageOut* d_out = (FdbPqwPageOut*)cs.alloc(items * sizeof(FdbPqwPageOut));
  hip_check(hipMemcpyAsync(d_out, L.out.data(), items * sizeof(FdbPqwPageOut), hipMemcpyHostToDevice, stream), "hipMemcpyAsync(page offsets)");
  hip_check(hipMemsetAsync(image.p, 0, image_bytes, stream), "hipMemsetAsync(file image)");
  hip_check(fdb_launch_pqw_encode(d_cols, g, d_out, d_tile_base, (unsigned char*)image.p, stream), "parquet write: encode launch");
  if (pt.on) { hip_check(hipStreamSynchronize(stream), "hipStreamSynchronize"); pt.mark("pqwrite encode"); }
  if (n_delta > 0) {
    uint64_t* d_delta_out = (uint64_t*)cs.alloc(d_items * 8);
    hip_check(hipMemcpyAsync(d_delta_out, L.delta_out.data(), d_items * 8, hipMemcpyHostToDevice, stream), "hipMemcpyAsync(DELTA page offsets)");
    hip_check(fdb_launch_pqd_encode(d_dcols, (int32_t)n_delta, g, d_stats, d_blocks, d_delta_out, (unsigned char*)image.p, stream), "parquet write: DELTA encode launch");
    if (pt.on) { hip_check(hipStreamSynchronize(stream), "hipStreamSynchronize"); pt.mark("pqwrite delta encode"); }
  }
  if (n_runs > 0) {
    uint64_t* d_run_out = (uint64_t*)cs.alloc(r_items * 8);
    hip_check(hipMemcpyAsync(d_run_out, L.run_out.data(), r_items * 8, hipMemcpyHostToDevice, stream), "hipMemcpyAsync(run-encoded page offsets)");
    hip_check(fdb_launch_pqr_encode(d_streams, (int32_t)n_runs, g, d_stats, d_run_bytes, d_run_out, (unsigned char*)image.p, stream), "parquet write: run encode launch");
    if (pt.on) { hip_check(hipStreamSynchronize(stream), "hipStreamSynchronize"); pt.mark("pqwrite run encode"); }
  }
  if (n_compressed == 0) {
    file.p = pqw_alloc_bytes(file_bytes, true);
    bloom_out(L, file.p);
    cs.ctx->copy_out_parallel(file.p, image.p, (size_t)L.body_bytes);
    pt.mark("pqwrite copy");
    pqw_finish(L, file.p);
    pt.mark("pqwrite host tail");
    *bytes = file.p; *n_bytes = (int64_t)file_bytes; file.p = nullptr;
    return;
  }
  // `image` is the staging image. The host's bytes inside the bodies go in, every fragment is compressed into its slot of scratch, the
  // sizes are summed per page and come back; the file is laid out again, and one gather fills the final image, which is what crosses
  // the link.
  const auto upload = [&](const void* host, size_t n, const char* what) {
    void* d = cs.alloc(std::max<size_t>(n, 8));
    if (n > 0) hip_check(hipMemcpyAsync(d, host, n, hipMemcpyHostToDevice, stream), what);
    return d;
  };
  std::vector<FdbPqsRange> pieces;
  for (const PqwLayout::Piece& p : L.body_pieces) pieces.push_back(FdbPqsRange{(uint64_t)p.pos, p.off, (uint32_t)p.len, 0});
  std::vector<FdbPqsPage> pages;
  std::vector<FdbPqsFrag> frags;
  for (const PqwLayout::Page& pg : L.pages) {
    pages.push_back(FdbPqsPage{(uint32_t)frags.size(), fdb_pqs_fragments(pg.body)});
    for (uint64_t at = 0; at < pg.body; at += FDB_PQS_FRAGMENT)
      frags.push_back(FdbPqsFrag{pg.off + at, (uint32_t)std::min<uint64_t>(FDB_PQS_FRAGMENT, pg.body - at), (uint32_t)(pages.size() - 1)});
  }
  if (frags.size() > 0x7FFFFFFFull / 2) throw Error(FDB_ERR_UNSUPPORTED, "parquet write: more than 2^30 fragments to compress");
  scratch.p = device_pool_alloc(b.device, std::max<size_t>(frags.size(), 1) * fdb_pqs_slot_bytes());
  const unsigned char* d_blob = (const unsigned char*)upload(L.body_blob.data(), L.body_blob.size(), "hipMemcpyAsync(page body pieces)");
  const FdbPqsRange* d_pieces = (const FdbPqsRange*)upload(pieces.data(), pieces.size() * sizeof(FdbPqsRange), "hipMemcpyAsync(page body piece table)");
  const FdbPqsFrag* d_frags = (const FdbPqsFrag*)upload(frags.data(), frags.size() * sizeof(FdbPqsFrag), "hipMemcpyAsync(fragment table)");
  const FdbPqsPage* d_pages = (const FdbPqsPage*)upload(pages.data(), pages.size() * sizeof(FdbPqsPage), "hipMemcpyAsync(compressed page table)");
  uint32_t* d_frag_bytes = (uint32_t*)cs.alloc(std::max<size_t>(frags.size(), 1) * 4);
  uint32_t* d_frag_off = (uint32_t*)cs.alloc(std::max<size_t>(frags.size(), 1) * 4);
  uint32_t* d_page_elements = (uint32_t*)cs.alloc(std::max<size_t>(pages.size(), 1) * 4);
  std::vector<uint32_t> page_elements(pages.size(), 0);
  hip_check(fdb_launch_pqs_place(d_pieces, (int32_t)pieces.size(), d_blob, (unsigned char*)image.p, stream), "parquet write: body piece launch");
  hip_check(fdb_launch_pqs_compress(d_frags, (int32_t)frags.size(), (const unsigned char*)image.p, (unsigned char*)scratch.p, d_frag_bytes, stream), "parquet write: compress launch");
  if (pt.on) { hip_check(hipStreamSynchronize(stream), "hipStreamSynchronize"); pt.mark("pqwrite compress"); }
  hip_check(fdb_launch_pqs_scan(d_pages, (int32_t)pages.size(), d_frag_bytes, d_frag_off, d_page_elements, stream), "parquet write: compressed size scan launch");
  if (!pages.empty()) hip_check(hipMemcpyAsync(page_elements.data(), d_page_elements, pages.size() * 4, hipMemcpyDeviceToHost, stream), "hipMemcpyAsync(compressed page sizes)");
  hip_check(hipStreamSynchronize(stream), "hipStreamSynchronize");
  pt.mark("pqwrite scan");
  const PqwLayout F = pqw_layout(cols, g, stats, delta_bytes, &page_elements, &x, &bl, run_table);
  const size_t out_bytes = F.file_bytes();
  pt.mark("pqwrite final layout");
  std::vector<uint64_t> page_dst(F.pages.size());
  for (size_t i = 0; i < F.pages.size(); i++) page_dst[i] = F.pages[i].off;
  std::vector<FdbPqsRange> ranges;  // the chunks of the uncompressed columns, in pieces a workgroup moves at a time
  for (size_t k = 0; k < cols.size(); k++) {
    if (cols[k].codec != 0) continue;
    for (uint64_t at = 0; at < L.chunk_len[k]; at += FDB_PQS_COPY_PIECE)
      ranges.push_back(FdbPqsRange{L.chunk_off[k] + at, F.chunk_off[k] + at, (uint32_t)std::min<uint64_t>(FDB_PQS_COPY_PIECE, L.chunk_len[k] - at), 0});
  }
  if (ranges.size() > 0x7FFFFFFFull / 2) throw Error(FDB_ERR_UNSUPPORTED, "parquet write: more than 2^30 pieces to move");
  const uint64_t* d_page_dst = (const uint64_t*)upload(page_dst.data(), page_dst.size() * 8, "hipMemcpyAsync(compressed page offsets)");
  const FdbPqsRange* d_ranges = (const FdbPqsRange*)upload(ranges.data(), ranges.size() * sizeof(FdbPqsRange), "hipMemcpyAsync(chunk piece table)");
  final_image.p = device_pool_alloc(b.device, align_up((size_t)F.body_bytes + 8, 256));
  hip_check(fdb_launch_pqs_gather(d_frags, (int32_t)frags.size(), d_frag_bytes, d_frag_off, d_page_dst, (const unsigned char*)scratch.p, d_ranges, (int32_t)ranges.size(),
                                  (const unsigned char*)image.p, (unsigned char*)final_image.p, stream), "parquet write: gather launch");
  if (pt.on) { hip_check(hipStreamSynchronize(stream), "hipStreamSynchronize"); pt.mark("pqwrite gather"); }
  file.p = pqw_alloc_bytes(out_bytes, true);
  bloom_out(F, file.p);
  cs.ctx->copy_out_parallel(file.p, final_image.p, (size_t)F.body_bytes);
  pt.mark("pqwrite copy");
  pqw_finish(F, file.p);
  pt.mark("pqwrite host tail");
  *bytes = file.p; *n_bytes = (int64_t)out_bytes; file.p = nullptr;
}
#endif

}  // namespace fdb
