// fdb_pqwrite_host.h — host side of the Parquet writer (fdb_pqwrite.cpp): column description, file layout, the host walk. The pieces are
// declared one by one so that a stand-alone program can drive them without a device (tools/asan_parquet_write_main.cpp, built with
// FDB_PQWRITE_HOST_ONLY).
#pragma once

#include <memory>
#include <string>
#include <vector>

#include "fdb_arrow.h"
#include "fdb_pqdelta.h"
#include "fdb_pqwrite.h"
#ifndef FDB_PQWRITE_HOST_ONLY
#include "fdb_plan.h"
#endif

namespace fdb {

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
  int pq_kind = FDB_PQW_V64;     // FDB_PQW_V64 / _BOOL / _INDEX or PQW_NO_VALUES
  int physical = 0;              // parquet Type
  bool is_u64 = false, utf8 = false, optional = false;
  int delta_slot = -1;            // >= 0: written DELTA_BINARY_PACKED, and its place among the columns that are (the tables of fdb_pqdelta.h)
  uint32_t width = 0;
  uint64_t entries = 0;
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
  std::vector<FdbPqwPageOut> out;
  std::vector<uint64_t> delta_out;  // [delta_slot × n_pages + page]: where a DELTA page's value bytes start (its `out` says FDB_PQW_NONE for the values)
  uint64_t body_bytes = 0;       // PAR1 + column chunks: what the image holds; the footer starts here
  std::string footer;
  void put(uint64_t off, const std::string& s);
};

// Options and columns checked, every refusal made (FDB_ERR_INVALID / FDB_ERR_UNSUPPORTED): nothing has been launched yet. `encodings`:
// per column 0 (as ever) or 1 (DELTA_BINARY_PACKED; I64 and U64 columns only), n_encodings 0 or the column count.
std::vector<PqwColumn> pqw_columns(const std::vector<PqwInput>& in, int64_t rows, const fdb_parquet_write_options* opt, int32_t* page_rows,
                                   const int8_t* encodings = nullptr, int32_t n_encodings = 0);
size_t pqw_delta_columns(const std::vector<PqwColumn>& cols);
FdbPqwGeom pqw_geometry(int64_t rows, int32_t page_rows, size_t n_cols);
// `delta_bytes`[delta_slot × n_pages + page]: the value bytes of a DELTA page, as the block survey found them.
PqwLayout pqw_layout(const std::vector<PqwColumn>& cols, const FdbPqwGeom& g, const std::vector<FdbPqwPageStat>& stats, const std::vector<uint32_t>& delta_bytes = {});
// Fills the holes of `file` (body_bytes + footer + 8 bytes long, the payloads in place) and appends footer, length and magic.
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
  const uint64_t* values(const PqwColumn& c) const { return c.validity != nullptr ? dense[(size_t)c.delta_slot].data() : (const uint64_t*)c.values; }
};
void pqd_survey_host(const std::vector<PqwColumn>& cols, const FdbPqwGeom& g, const std::vector<FdbPqwPageStat>& stats, const std::vector<uint32_t>& tile_base, PqdHost* d);
void pqd_encode_host(const std::vector<PqwColumn>& cols, const FdbPqwGeom& g, const std::vector<FdbPqwPageStat>& stats, const PqdHost& d, const std::vector<uint64_t>& delta_out,
                     unsigned char* image);

// The buffer a file is returned in (fdb_bytes_free): malloc'ed, or a block of the pinned result pool when the device copies into it.
uint8_t* pqw_alloc_bytes(size_t n, bool pinned);
void pqw_free_bytes(uint8_t* bytes);

void selftest_parquet_write(const HostRecordView& view, const fdb_parquet_write_options* opt, uint8_t** bytes, int64_t* n_bytes, const int8_t* encodings = nullptr,
                            int32_t n_encodings = 0);
#ifndef FDB_PQWRITE_HOST_ONLY
void batch_to_parquet(const DeviceBatch& b, const fdb_parquet_write_options* opt, uint8_t** bytes, int64_t* n_bytes, const int8_t* encodings = nullptr, int32_t n_encodings = 0);
#endif

}  // namespace fdb
