// Stand-alone driver of the host half of the Parquet writer for tools/asan_parquet_write.sh: column checks and options (pqw_plan),
// the survey and encode walk over host arrays (pqw_survey_host / pqw_encode_host: the arithmetic of fdb_pqwrite.h that the kernels
// compile), layout planning with the thrift writer and the dictionary page builder (pqw_layout) and the tail (pqw_finish) — over seeded
// random records and options, every buffer sized exactly. Some int64 / uint64 columns are asked to be DELTA_BINARY_PACKED: the DELTA
// passes' host walk (pqd_survey_host / pqd_encode_host: the arithmetic of fdb_pqdelta.h) sizes and writes their pages. What the walk
// wrote is read back with a bit reader and a DELTA decoder of this file's own. Some columns, DELTA ones among them, are asked to be SNAPPY:
// the compressor's host walk (fdb_pqsnappy.h) runs over the staging image's page bodies, the file is laid out again, and every page of
// the final file — dictionary pages too — is inflated by the library's host decoder (fdb_codec.cpp snappy_block) into a buffer of exactly
// the body's size and compared with the body; bodies of 0 … 2 fragments + 1 bytes of several kinds go through the same two. Others are
// asked to be LZ4_RAW (codec 7): the host walk of fdb_pqlz4.h makes each page body one block, which fdb::lz4_raw inflates again and a
// sequence reader of this file's own holds to the block format's end conditions; the same bodies, and more around the fragment size,
// go through that walk too.
// Every record is also written with index options at random (statistics 0 … 2, a cut limit, sorting columns): the min / max pass's host
// walk (pqx_minmax_host: the keys of fdb_pqstats.h that the kernel compiles) fills the table, the layout writes chunk bounds, ColumnIndex
// and OffsetIndex, and a small thrift reader of this file's own reads the index back out of a buffer sized exactly and holds every
// page's bounds, NULL counts and location against a plain loop over the record.
// And with bloom filter options at random (columns, bits per value): the insert pass's host walk (pqb_insert_host: the hash, block and
// bits of fdb_pqbloom.h that the kernel compiles) fills a table of bitsets sized exactly, the layout puts header and bitset of every
// filter between the pages and the index, and a reader of this file's own — its own XXH64, block and salts — finds every non-NULL
// value of the record in its column's filter, and no bit set that no value set.
// And with run options at random (per column: dictionary indices, definition levels, both, none): the run passes' host walk
// (pqr_survey_host / pqr_encode_host: the rule of fdb_pqruns.h that the kernels compile) sizes and writes the streams, the layout holds
// the sizes to the rule's bounds, and a hybrid reader of this file's own decodes every run-encoded stream out of a buffer sized exactly
// — to the page's validity bits or non-NULL indices — and holds it to "never longer than the one bit-packed run".
// No GPU, no HIP, no python. Prints "asan parquet write ok" and exits 0 when every check holds.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "fdb_codec.h"
#include "fdb_pqwrite_host.h"

using namespace fdb;

#define CHECK(cond) do { if (!(cond)) { std::fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #cond); std::exit(1); } } while (0)

static uint64_t rnd(uint64_t* s) {
  uint64_t z = (*s += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

struct Column {
  ColKind kind;
  std::vector<uint64_t> v64;        // I64 / U64 / F64 / BOOL (1 / 2)
  std::vector<uint32_t> idx;        // DICT
  std::vector<uint8_t> bits;        // validity, whole words; empty: no NULLs
  std::shared_ptr<HostDict> dict;
  int64_t nulls = 0;
  bool valid(int64_t r) const { return bits.empty() || ((bits[(size_t)(r >> 3)] >> (r & 7)) & 1); }
};

static uint32_t read_bits(const uint8_t* p, uint64_t bit, uint32_t w) {
  uint32_t v = 0;
  for (uint32_t b = 0; b < w; b++) v |= (uint32_t)((p[(bit + b) >> 3] >> ((bit + b) & 7)) & 1) << b;
  return v;
}

static uint64_t read_varint(const uint8_t* p, size_t* at) {
  uint64_t v = 0;
  for (int shift = 0;; shift += 7) {
    CHECK(shift < 70);
    const uint8_t b = p[(*at)++];
    v |= (uint64_t)(b & 0x7F) << (shift < 64 ? shift : 63);
    if (b < 0x80) return v;
  }
}
static int64_t unzigzag(uint64_t z) { return (int64_t)((z >> 1) ^ (0 - (z & 1))); }
static uint64_t read_bits64(const uint8_t* p, uint64_t bit, uint32_t w) {
  uint64_t v = 0;
  for (uint32_t b = 0; b < w; b++) v |= (uint64_t)((p[(bit + b) >> 3] >> ((bit + b) & 7)) & 1) << b;
  return v;
}

// A DELTA_BINARY_PACKED page of exactly `bytes` bytes decodes to `want`: blocks of 128 in 4 miniblocks, every miniblock as narrow as its
// largest value allows, padding zero, no width and no body where no delta is.
static void check_delta_page(const uint8_t* p, size_t bytes, const std::vector<uint64_t>& want) {
  size_t at = 0;
  CHECK(read_varint(p, &at) == 128);
  CHECK(read_varint(p, &at) == 4);
  const uint64_t count = read_varint(p, &at);
  CHECK(count == want.size());
  uint64_t prev = (uint64_t)unzigzag(read_varint(p, &at));
  CHECK(prev == (count > 0 ? want[0] : 0));
  for (uint64_t i = 1; i < count;) {
    const uint64_t mn = (uint64_t)unzigzag(read_varint(p, &at));
    const uint8_t* widths = p + at;
    at += 4;
    for (int m = 0; m < 4; m++) {
      const uint32_t w = widths[m];
      if (i >= count) { CHECK(w == 0); continue; }
      CHECK(w <= 64 && at + 4 * (size_t)w <= bytes);
      uint64_t mx = 0;
      for (uint32_t j = 0; j < 32; j++) {
        const uint64_t r = read_bits64(p + at, (uint64_t)j * w, w);
        if (i < count) { prev += mn + r; CHECK(prev == want[i]); i++; mx = r > mx ? r : mx; }
        else CHECK(r == 0);
      }
      CHECK(w == 0 ? mx == 0 : (mx >> (w - 1)) == 1);
      at += 4 * (size_t)w;
    }
  }
  CHECK(at == bytes);
}

// A stream of the RLE / bit-packed hybrid of exactly `bytes` bytes decodes to `want` at width w: padding zero, nothing behind the last run.
static size_t g_rle_inside = 0, g_streams = 0;  // streams read back, and those of more than one run with an RLE run among them
static void check_hybrid(const uint8_t* p, size_t bytes, uint32_t w, const std::vector<uint32_t>& want) {
  size_t at = 0, n = 0, runs = 0, rle = 0;
  while (at < bytes) {
    const uint64_t head = read_varint(p, &at);
    runs++;
    if (head & 1) {
      const uint64_t groups = head >> 1;
      CHECK(groups > 0 && at + groups * w <= bytes && n < want.size() && n + groups * 8 < want.size() + 8);
      for (uint64_t j = 0; j < groups * 8; j++) CHECK(read_bits(p + at, j * w, w) == (n + j < want.size() ? want[n + j] : 0u));
      n = n + groups * 8 < want.size() ? n + (size_t)groups * 8 : want.size();
      at += (size_t)(groups * w);
    } else {
      const uint64_t count = head >> 1;
      uint32_t v = 0;
      CHECK(count >= 8 && at + (w + 7) / 8 <= bytes && n + count <= want.size());
      for (uint32_t b = 0; b < (w + 7) / 8; b++) v |= (uint32_t)p[at + b] << (8 * b);
      for (uint64_t j = 0; j < count; j++) CHECK(want[n + j] == v);
      n += (size_t)count;
      at += (w + 7) / 8;
      rle++;
    }
  }
  CHECK(at == bytes && n == want.size() && runs > 0);
  g_streams++;
  g_rle_inside += runs > 1 && rle > 0;
}

// `block` (sized exactly) inflates to `body` (into a buffer sized exactly), and stays within Snappy's bound.
static void check_block(const std::string& block, const unsigned char* body, size_t n) {
  std::vector<uint8_t> exact(block.begin(), block.end()), out(n);
  CHECK(exact.size() <= 32 + n + n / 6);
  CHECK(snappy_block(exact.data(), exact.size(), out.data(), n, n) == 0);
  CHECK(n == 0 || std::memcmp(out.data(), body, n) == 0);
}

// … an LZ4_RAW block: it inflates under fdb::lz4_raw to `body`, stays within LZ4_compressBound, and — what liblz4 insists on and the
// library's own decoder does not — its sequences end as the format says: no match starts behind n − 12 or ends behind n − 5, the last
// sequence has none.
static void check_lz4_block(const std::string& block, const unsigned char* body, size_t n) {
  std::vector<uint8_t> exact(block.begin(), block.end()), out(n);
  CHECK(exact.size() >= 1 && exact.size() <= n + n / 255 + 16);
  CHECK(lz4_raw(exact.data(), exact.size(), out.data(), n));
  CHECK(n == 0 || std::memcmp(out.data(), body, n) == 0);
  size_t at = 0, pos = 0;
  const auto length = [&](size_t v) { if (v == 15) { uint8_t b; do { CHECK(at < exact.size()); b = exact[at++]; v += b; } while (b == 255); } return v; };
  for (;;) {
    CHECK(at < exact.size());
    const uint8_t token = exact[at++];
    const size_t lit = length(token >> 4);
    CHECK(at + lit <= exact.size());
    at += lit; pos += lit;
    if (at == exact.size()) { CHECK((token & 15) == 0); break; }
    CHECK(at + 2 <= exact.size());
    const size_t off = exact[at] | ((size_t)exact[at + 1] << 8);
    at += 2;
    const size_t len = length(token & 15) + 4;
    CHECK(off >= 1 && off <= pos % FDB_PQS_FRAGMENT && pos / FDB_PQS_FRAGMENT == (pos + len - 1) / FDB_PQS_FRAGMENT);
    CHECK(pos + 12 <= n && pos + len + 5 <= n);
    pos += len;
  }
  CHECK(pos == n);
}

// Bodies around nothing, one and two fragments, of several kinds, through the block compressors and the host decoders.
static void snappy_bodies(uint64_t* seed) {
  static const size_t sizes[] = {0, 1, 2, 3, 4, 5, 11, 12, 13, 14, 17, 18, 63, 64, 65, 4096, FDB_PQS_FRAGMENT - 1, FDB_PQS_FRAGMENT, FDB_PQS_FRAGMENT + 1, FDB_PQS_FRAGMENT + 4, FDB_PQS_FRAGMENT + 5,
                                 FDB_PQS_FRAGMENT + 11, FDB_PQS_FRAGMENT + 12, FDB_PQS_FRAGMENT + 13, 2 * FDB_PQS_FRAGMENT - 1, 2 * FDB_PQS_FRAGMENT, 2 * FDB_PQS_FRAGMENT + 1, 2 * FDB_PQS_FRAGMENT + 3};
  for (size_t n : sizes) {
    for (int kind = 0; kind < 5; kind++) {  // 0 noise, 1 one byte, 2 few distinct 8-byte values, 3 runs of random periods and lengths, 4 noise with repeats from far back
      std::vector<unsigned char> body(n);
      uint64_t few[8];
      for (uint64_t& f : few) f = rnd(seed);
      for (size_t i = 0; i < n;) {
        if (kind == 0) body[i++] = (unsigned char)rnd(seed);
        else if (kind == 1) body[i++] = 7;
        else if (kind == 2) { const uint64_t v = few[rnd(seed) % 8]; for (int b = 0; b < 8 && i < n; b++) body[i++] = (unsigned char)(v >> (8 * b)); }
        else if (kind == 3) { const size_t period = 1 + rnd(seed) % 70, len = 1 + rnd(seed) % 400, at = i; for (size_t j = 0; j < len && i < n; j++, i++) body[i] = j < period ? (unsigned char)rnd(seed) : body[at + j % period]; }
        else { const size_t len = 1 + rnd(seed) % 200, back = i > 0 ? 1 + rnd(seed) % i : 0; const bool copy = back > 0 && (rnd(seed) & 1); for (size_t j = 0; j < len && i < n; j++, i++) body[i] = copy ? body[i - back] : (unsigned char)rnd(seed); }
      }
      const std::vector<unsigned char> exact(body);  // (sized exactly: a walk that reads past the body is caught)
      check_block(pqs_block_host(exact.data(), exact.size()), exact.data(), n);
      check_lz4_block(pql_block_host(exact.data(), exact.size()), exact.data(), n);
    }
  }
}

// ---- the page index, read back ---------------------------------------------------------------------------------------------------------
struct IndexReader {
  const std::vector<uint8_t>& b;
  size_t at = 0;
  uint8_t byte() { CHECK(at < b.size()); return b[at++]; }
  uint64_t varint() { uint64_t v = 0; for (int shift = 0;; shift += 7) { CHECK(shift < 70); const uint8_t x = byte(); v |= (uint64_t)(x & 0x7F) << (shift < 64 ? shift : 63); if (x < 0x80) return v; } }
  int field(int* last) { const uint8_t h = byte(); if (h == 0) return 0; CHECK((h >> 4) != 0); *last += h >> 4; return h & 15; }  // (the writer never needs the long form here)
  size_t list(int elem) { const uint8_t h = byte(); CHECK((h & 15) == elem); return (h >> 4) == 15 ? (size_t)varint() : (size_t)(h >> 4); }
  std::string binary() { const size_t n = (size_t)varint(); CHECK(at + n <= b.size()); std::string v((const char*)b.data() + at, n); at += n; return v; }
};
struct ReadColumnIndex { std::vector<bool> null_pages; std::vector<std::string> mins, maxs; int order = -1; std::vector<int64_t> null_counts; };
static ReadColumnIndex read_column_index(IndexReader* r) {
  ReadColumnIndex ci;
  int last = 0;
  CHECK(r->field(&last) == 9 && last == 1);
  for (size_t n = r->list(1), i = 0; i < n; i++) { const uint8_t v = r->byte(); CHECK(v == 1 || v == 2); ci.null_pages.push_back(v == 1); }
  CHECK(r->field(&last) == 9 && last == 2);
  for (size_t n = r->list(8), i = 0; i < n; i++) ci.mins.push_back(r->binary());
  CHECK(r->field(&last) == 9 && last == 3);
  for (size_t n = r->list(8), i = 0; i < n; i++) ci.maxs.push_back(r->binary());
  CHECK(r->field(&last) == 5 && last == 4);
  ci.order = (int)unzigzag(r->varint());
  CHECK(r->field(&last) == 9 && last == 5);
  for (size_t n = r->list(6), i = 0; i < n; i++) ci.null_counts.push_back(unzigzag(r->varint()));
  CHECK(r->field(&last) == 0);
  return ci;
}
struct ReadLocation { int64_t off, bytes, first_row; };
static std::vector<ReadLocation> read_offset_index(IndexReader* r) {
  std::vector<ReadLocation> out;
  int last = 0;
  CHECK(r->field(&last) == 9 && last == 1);
  for (size_t n = r->list(12), i = 0; i < n; i++) {
    ReadLocation l;
    int f = 0;
    CHECK(r->field(&f) == 6 && f == 1); l.off = unzigzag(r->varint());
    CHECK(r->field(&f) == 5 && f == 2); l.bytes = unzigzag(r->varint());
    CHECK(r->field(&f) == 6 && f == 3); l.first_row = unzigzag(r->varint());
    CHECK(r->field(&f) == 0);
    out.push_back(l);
  }
  CHECK(r->field(&last) == 0);
  return out;
}

// ---- the bloom filters, read back ---------------------------------------------------------------------------------------------------------
static uint64_t rotl64(uint64_t x, int r) { return (x << r) | (x >> (64 - r)); }
// XXH64, seed 0, byte by byte from its description (not the header's under test)
static uint64_t reader_xxh64(const std::string& s) {
  const uint64_t P1 = 0x9E3779B185EBCA87ull, P2 = 0xC2B2AE3D27D4EB4Full, P3 = 0x165667B19E3779F9ull, P4 = 0x85EBCA77C2B2AE63ull, P5 = 0x27D4EB2F165667C5ull;
  const auto le = [&](size_t at, int n) { uint64_t v = 0; for (int b = 0; b < n; b++) v |= (uint64_t)(unsigned char)s[at + (size_t)b] << (8 * b); return v; };
  const auto round = [&](uint64_t acc, uint64_t in) { return rotl64(acc + in * P2, 31) * P1; };
  size_t at = 0;
  uint64_t h;
  if (s.size() >= 32) {
    uint64_t v[4] = {P1 + P2, P2, 0, 0 - P1};
    for (; at + 32 <= s.size(); at += 32) for (int i = 0; i < 4; i++) v[i] = round(v[i], le(at + 8 * (size_t)i, 8));
    h = rotl64(v[0], 1) + rotl64(v[1], 7) + rotl64(v[2], 12) + rotl64(v[3], 18);
    for (int i = 0; i < 4; i++) h = (h ^ round(0, v[i])) * P1 + P4;
  } else h = P5;
  h += s.size();
  for (; at + 8 <= s.size(); at += 8) h = rotl64(h ^ round(0, le(at, 8)), 27) * P1 + P4;
  if (at + 4 <= s.size()) { h = rotl64(h ^ (le(at, 4) * P1), 23) * P2 + P3; at += 4; }
  for (; at < s.size(); at++) h = rotl64(h ^ ((unsigned char)s[at] * P5), 11) * P1;
  h ^= h >> 33; h *= P2; h ^= h >> 29; h *= P3;
  return h ^ (h >> 32);
}

// The record written with filters on the columns of `b`: header and bitset of each where the layout says, every non-NULL value found,
// every set bit accounted for.
static void check_bloom(const std::vector<Column>& cols, const std::vector<PqwColumn>& pc, int64_t rows, const std::vector<FdbPqwPageStat>& stats, size_t n_pages, const PqwLayout& L,
                        const PqbPlan& b, const uint8_t* file) {
  static const uint32_t salt[8] = {0x47b6137bu, 0x44974d91u, 0x8824ad5bu, 0xa2b7289du, 0x705495c7u, 0x2df1424bu, 0x9efc4947u, 0x5c6bfb31u};
  size_t next = 0;
  uint64_t at = L.body_bytes;
  for (size_t k = 0; k < cols.size(); k++) {
    if (!b.any() || b.on[k] == 0) continue;
    CHECK(next < L.blooms.size() && L.blooms[next].col == k);
    const PqwLayout::Bloom& f = L.blooms[next++];
    uint64_t n = 0;
    for (size_t p = 0; p < n_pages; p++) n += stats[k * n_pages + p].count;
    if (cols[k].kind == ColKind::DICT) n = std::min<uint64_t>(n, cols[k].dict->values.size());
    const uint64_t want_bytes = std::min<uint64_t>(32 * std::max<uint64_t>(1, ((n * b.bits_per_value + 7) / 8 + 31) / 32), 128u << 20);
    CHECK(f.bytes == want_bytes && f.bytes % 32 == 0);
    // the header: 15, the zigzag varint of the size, the three empty unions, the stop byte — right in front of the bitset
    size_t h = (size_t)at;
    CHECK(file[h++] == 0x15);
    CHECK(read_varint(file, &h) == 2 * f.bytes);
    static const uint8_t rest[13] = {0x1c, 0x1c, 0, 0, 0x1c, 0x1c, 0, 0, 0x1c, 0x1c, 0, 0, 0};
    CHECK(std::memcmp(file + h, rest, 13) == 0 && h + 13 == f.bits_off);
    const std::vector<uint8_t> exact(file + f.bits_off, file + f.bits_off + f.bytes);  // (sized exactly: a reader that runs past the bitset is caught)
    std::vector<uint8_t> expected(exact.size(), 0);
    for (int64_t r = 0; r < rows; r++) {
      if (!(pc[k].validity == nullptr || cols[k].valid(r))) continue;
      const std::string plain = cols[k].kind == ColKind::DICT ? cols[k].dict->values[cols[k].idx[(size_t)r]] : std::string((const char*)&cols[k].v64[(size_t)r], 8);
      const uint64_t hash = reader_xxh64(plain);
      const size_t block = (size_t)(((hash >> 32) * (f.bytes / 32)) >> 32);
      for (int i = 0; i < 8; i++) {
        const uint32_t bit = ((uint32_t)hash * salt[i]) >> 27;
        const size_t byte = block * 32 + (size_t)i * 4 + bit / 8;
        CHECK((exact[byte] >> (bit % 8)) & 1);  // present
        expected[byte] |= (uint8_t)(1u << (bit % 8));
      }
    }
    CHECK(exact == expected);  // and nothing else is set
    at = f.bits_off + f.bytes;
  }
  CHECK(next == L.blooms.size() && at == L.body_bytes + L.bloom_bytes);
}

// a < b in the column's order, by a plain comparison of the values themselves (not by the keys under test)
static bool value_less(const Column& c, int64_t a, int64_t b) {
  if (c.kind == ColKind::DICT) return c.dict->values[c.idx[(size_t)a]] < c.dict->values[c.idx[(size_t)b]];
  const uint64_t x = c.v64[(size_t)a], y = c.v64[(size_t)b];
  if (c.kind == ColKind::I64) return (int64_t)x < (int64_t)y;
  if (c.kind == ColKind::F64) { double dx, dy; std::memcpy(&dx, &x, 8); std::memcpy(&dy, &y, 8); return dx < dy || (dx == dy && (x >> 63) > (y >> 63)); }  // (−0.0 below +0.0: the zero rule decides what is written)
  if (c.kind == ColKind::BOOL) return (x >= 2) < (y >= 2);
  return x < y;
}
static bool counts(const Column& c, int64_t r) {
  if (c.kind != ColKind::F64) return true;
  double d;
  std::memcpy(&d, &c.v64[(size_t)r], 8);
  return d == d;
}
static std::string written(const Column& c, int64_t r, bool is_max) {
  if (c.kind == ColKind::DICT) return c.dict->values[c.idx[(size_t)r]];
  uint64_t v = c.v64[(size_t)r];
  if (c.kind == ColKind::BOOL) return std::string(1, (char)(v >= 2));
  if (c.kind == ColKind::F64 && (v << 1) == 0) v = is_max ? 0 : 1ull << 63;
  return std::string((const char*)&v, 8);
}

// The record written with `index`: the tail holds what a loop over the record says, page by page.
// The dictionary reader: a chunk that starts with a PLAIN dictionary page of exactly the entries `used` of the column's dictionary, in this order.
static void check_dictionary_page(const std::vector<uint8_t>& chunk, const Column& col, const std::vector<uint32_t>& used) {
  IndexReader r{chunk};
  int last = 0, inner = 0;
  CHECK(r.field(&last) == 5 && last == 1 && unzigzag(r.varint()) == 2);  // PageType DICTIONARY_PAGE
  CHECK(r.field(&last) == 5 && last == 2); const int64_t body = unzigzag(r.varint());
  CHECK(r.field(&last) == 5 && last == 3 && unzigzag(r.varint()) == body);
  CHECK(r.field(&last) == 12 && last == 7);
  CHECK(r.field(&inner) == 5 && inner == 1 && unzigzag(r.varint()) == (int64_t)used.size());
  CHECK(r.field(&inner) == 5 && inner == 2 && unzigzag(r.varint()) == 0);  // PLAIN
  CHECK(r.field(&inner) == 0 && r.field(&last) == 0);
  const size_t start = r.at;
  for (uint32_t e : used) {
    const std::string& v = col.dict->values[e];
    uint32_t len;
    CHECK(r.at + 4 <= chunk.size()); std::memcpy(&len, chunk.data() + r.at, 4); r.at += 4;
    CHECK(len == v.size() && r.at + len <= chunk.size() && std::memcmp(chunk.data() + r.at, v.data(), len) == 0);
    r.at += len;
  }
  CHECK((int64_t)(r.at - start) == body);
}

static void check_index(const std::vector<Column>& cols, const std::vector<PqwColumn>& pc, const FdbPqwGeom& g, const std::vector<FdbPqwPageStat>& stats, const PqwLayout& L,
                        const PqxIndex& x, const std::vector<uint64_t>& chunk_off, const std::vector<uint64_t>& chunk_len) {
  if (x.statistics < 2) { CHECK(L.tail.empty()); return; }
  const std::vector<uint8_t> exact(L.tail.begin(), L.tail.end());  // (sized exactly: a reader that runs past the index is caught)
  IndexReader r{exact};
  const size_t n_pages = (size_t)g.n_pages;
  for (size_t k = 0; k < cols.size(); k++) {
    const Column& c = cols[k];
    std::vector<int64_t> lo(n_pages, -1), hi(n_pages, -1);
    bool sayable = true;
    for (size_t p = 0; p < n_pages; p++) {
      for (int64_t row = fdb_pqw_page_first(g, (int64_t)p); row < fdb_pqw_page_end(g, (int64_t)p); row++) {
        if (!(pc[k].validity == nullptr || c.valid(row)) || !counts(c, row)) continue;
        if (lo[p] < 0 || value_less(c, row, lo[p])) lo[p] = row;
        if (hi[p] < 0 || value_less(c, hi[p], row)) hi[p] = row;
      }
      if (lo[p] < 0 && stats[k * n_pages + p].count > 0) sayable = false;
    }
    if (!sayable) continue;  // a page of NaNs only: the column has no ColumnIndex
    const ReadColumnIndex ci = read_column_index(&r);
    CHECK(ci.null_pages.size() == n_pages && ci.mins.size() == n_pages && ci.maxs.size() == n_pages && ci.null_counts.size() == n_pages && ci.order >= 0 && ci.order <= 2);
    for (size_t p = 0; p < n_pages; p++) {
      const int64_t n = fdb_pqw_page_end(g, (int64_t)p) - fdb_pqw_page_first(g, (int64_t)p);
      CHECK(ci.null_counts[p] == n - (int64_t)stats[k * n_pages + p].count && ci.null_pages[p] == (stats[k * n_pages + p].count == 0));
      if (lo[p] < 0) { CHECK(ci.mins[p].empty() && ci.maxs[p].empty()); continue; }
      std::string mn = written(c, lo[p], false), mx = written(c, hi[p], true);
      if (c.kind == ColKind::DICT) {
        if (mn.size() > x.limit) mn.resize(x.limit);
        if (mx.size() > x.limit) {
          std::string cut = mx.substr(0, x.limit);
          while (!cut.empty() && (unsigned char)cut.back() == 0xFF) cut.pop_back();
          if (!cut.empty()) { cut.back() = (char)(cut.back() + 1); mx = cut; }
        }
      }
      CHECK(ci.mins[p] == mn && ci.maxs[p] == mx);
    }
  }
  for (size_t k = 0; k < cols.size(); k++) {
    const std::vector<ReadLocation> locs = read_offset_index(&r);
    CHECK(locs.size() == n_pages);
    uint64_t at = chunk_off[k];
    for (size_t p = 0; p < n_pages; p++) {
      CHECK(locs[p].first_row == (int64_t)p * g.page_rows && locs[p].bytes > 0 && (uint64_t)locs[p].off >= at);  // (a dictionary page may sit in front of the first)
      CHECK(p == 0 || (uint64_t)locs[p].off == at);
      at = (uint64_t)locs[p].off + (uint64_t)locs[p].bytes;
    }
    CHECK(n_pages == 0 || at == chunk_off[k] + chunk_len[k]);
  }
  CHECK(r.at == exact.size());
}

static void one_record(uint64_t* seed, int round) {
  static const int64_t row_choices[] = {0, 1, 7, 63, 64, 65, 127, 128, 129, 1000, 4095, 4096, 4097, 9000};
  static const int32_t page_choices[] = {0, 64, 128, 4096, 8192, 65536};
  static const uint32_t entry_choices[] = {0, 1, 2, 3, 5, 255, 256, 257, 65537};
  const int64_t rows = row_choices[rnd(seed) % 14];
  const int32_t page_rows = rows > 4097 ? page_choices[2 + rnd(seed) % 4] : page_choices[rnd(seed) % 6];
  const size_t n_cols = 1 + rnd(seed) % 5;
  std::vector<Column> cols(n_cols);
  std::vector<PqwInput> in;
  std::vector<int8_t> optional, encodings;
  for (size_t k = 0; k < n_cols; k++) {
    Column& c = cols[k];
    static const ColKind kinds[] = {ColKind::I64, ColKind::U64, ColKind::F64, ColKind::BOOL, ColKind::DICT, ColKind::DICT};
    c.kind = kinds[rnd(seed) % 6];
    uint32_t entries = entry_choices[rnd(seed) % 9];
    const int null_mode = (int)(rnd(seed) % 5);  // 0 none, 1 all, 2 random, 3 whole tiles, 4 rare
    if (c.kind == ColKind::DICT && entries == 0 && rows > 0 && null_mode != 1) entries = 1;
    if (null_mode != 0 && rows > 0) {
      c.bits.assign((size_t)(rows + 63) / 64 * 8, 0);
      for (int64_t r = 0; r < rows; r++) {
        const bool v = null_mode == 1 ? false : null_mode == 2 ? (rnd(seed) & 1) != 0 : null_mode == 3 ? ((r / 64) % 3 != 1) : rnd(seed) % 97 != 0;
        if (v) c.bits[(size_t)(r >> 3)] |= (uint8_t)(1u << (r & 7)); else c.nulls++;
      }
      for (int64_t r = rows; r < (rows + 63) / 64 * 64; r++) if (rnd(seed) & 1) c.bits[(size_t)(r >> 3)] |= (uint8_t)(1u << (r & 7));  // bits past the end are undefined
      if (c.nulls == 0) c.bits.clear();
    }
    PqwInput o;
    o.name = "c" + std::to_string(k); o.kind = c.kind; o.null_count = c.nulls;
    if (c.kind == ColKind::DICT) {
      std::vector<std::string> values;
      for (uint32_t e = 0; e < entries; e++) values.push_back(e % 7 == 3 ? std::string() : "v" + std::to_string(e % 1000));
      c.dict = (rnd(seed) & 1) ? make_dictionary(std::move(values), (rnd(seed) & 1) ? "u" : "z") : make_plain_dictionary(std::move(values), "u");
      const bool constant = rnd(seed) % 3 == 0;
      c.idx.resize((size_t)rows);
      for (int64_t r = 0; r < rows; r++) c.idx[(size_t)r] = entries == 0 ? 0 : constant ? (uint32_t)((r / 64) % entries) : (uint32_t)(rnd(seed) % entries);
      if (!constant && rows > 0 && entries > 0) c.idx[(size_t)rows - 1] = entries - 1;
      for (int64_t r = 0; r < rows; r++) if (!c.valid(r)) c.idx[(size_t)r] = 0xFFFFFFFFu;  // a NULL row's index must never be looked at
      o.dict = c.dict;
      o.values = rows > 0 ? c.idx.data() : nullptr;
    } else {
      c.v64.resize((size_t)rows);
      const int shape = (int)(rnd(seed) % 4);  // 0 any bits, 1 small steps, 2 constant, 3 steps of either sign around 2^63
      uint64_t run = shape == 3 ? (1ull << 63) - 50 : rnd(seed);
      for (int64_t r = 0; r < rows; r++) {
        if (c.kind == ColKind::BOOL) c.v64[(size_t)r] = 1 + (rnd(seed) & 1);
        else if (shape == 0 || c.kind == ColKind::F64) c.v64[(size_t)r] = rnd(seed);
        else c.v64[(size_t)r] = run += shape == 1 ? rnd(seed) % 2000 : shape == 2 ? 0 : rnd(seed) % 101 - 50;
      }
      o.values = rows > 0 ? c.v64.data() : nullptr;
    }
    encodings.push_back((c.kind == ColKind::I64 || c.kind == ColKind::U64) && rnd(seed) % 3 != 0 ? 1 : 0);
    o.validity = c.bits.empty() ? nullptr : c.bits.data();
    in.push_back(std::move(o));
    optional.push_back(c.nulls > 0 ? (int8_t)((rnd(seed) & 1) ? 1 : -1) : (int8_t)((int)(rnd(seed) % 3) - 1));
  }
  fdb_parquet_write_options opt;
  opt.page_rows = page_rows;
  const bool with_optional = (round & 1) != 0;
  opt.n_optional = with_optional ? (int32_t)n_cols : 0;
  opt.optional = with_optional ? optional.data() : nullptr;

  int32_t pr = 0;
  const bool with_encodings = (round & 2) != 0 || (round & 1) == 0;  // (one round in four writes every column as ever)
  PqwSpec spec{&opt, with_encodings ? encodings.data() : nullptr, with_encodings ? (int32_t)n_cols : 0};
  const std::vector<PqwColumn> pc = pqw_columns(in, rows, spec, &pr);
  CHECK(pr == (page_rows == 0 ? 65536 : page_rows) && pc.size() == n_cols);
  const FdbPqwGeom g = pqw_geometry(rows, pr, n_cols);
  const PqwPlan plain = pqw_plan(in, rows, spec);
  CHECK(plain.cols.size() == n_cols && plain.g.n_pages == g.n_pages && plain.g.page_rows == pr && !plain.x.any() && !plain.bloom.any() && plain.n_runs == 0 && plain.n_compressed == 0);
  std::vector<FdbPqwPageStat> stats;
  std::vector<uint32_t> tile_base;
  pqw_survey_host(pc, g, &stats, &tile_base);
  PqdHost dh;
  pqd_survey_host(pc, g, stats, tile_base, &dh);
  const PqwSizes sizes{stats, &dh.page_bytes};
  const PqwLayout L = pqw_layout(plain, sizes);
  std::vector<unsigned char> image(((size_t)L.body_bytes + 8 + 3) / 4 * 4, 0);
  pqw_encode_host(pc, g, L.parts[0].out, tile_base, image.data());
  pqd_encode_host(pc, g, stats, dh, L.parts[0].delta_out, image.data());
  const size_t file_bytes = L.file_bytes();
  CHECK(L.tail.empty());
  uint8_t* file = pqw_alloc_bytes(file_bytes, false);
  std::memcpy(file, image.data(), (size_t)L.body_bytes);
  for (size_t b = (size_t)L.body_bytes; b < image.size(); b++) CHECK(image[b] == 0);  // nothing is written past the body
  pqw_finish(L, file);
  CHECK(std::memcmp(file, "PAR1", 4) == 0 && std::memcmp(file + file_bytes - 4, "PAR1", 4) == 0);
  uint32_t flen;
  std::memcpy(&flen, file + file_bytes - 8, 4);
  CHECK(flen == L.footer.size());
  // the host's pieces do not overlap the payloads, the payloads hold what the record holds
  std::vector<uint8_t> owner(L.body_bytes, 0);
  for (const PqwLayout::Piece& p : L.pieces) for (size_t b = 0; b < p.len; b++) { CHECK(p.off + b < L.body_bytes && owner[p.off + b] == 0); owner[p.off + b] = 1; }
  for (size_t k = 0; k < n_cols; k++) {
    const Column& c = cols[k];
    for (int64_t p = 0; p < g.n_pages; p++) {
      const FdbPqwPageOut po = L.parts[0].out[k * (size_t)g.n_pages + (size_t)p];
      const FdbPqwPageStat st = stats[k * (size_t)g.n_pages + (size_t)p];
      const int64_t first = fdb_pqw_page_first(g, p), end = fdb_pqw_page_end(g, p);
      uint32_t cnt = 0;
      for (int64_t r = first; r < end; r++) cnt += pc[k].validity == nullptr || c.valid(r);
      CHECK(cnt == st.count);
      if (po.levels_off != FDB_PQW_NONE) {
        for (uint32_t b = 0; b < fdb_pqw_level_bytes((uint32_t)(end - first)); b++) { CHECK(owner[po.levels_off + b] == 0); owner[po.levels_off + b] = 2; }
        for (int64_t r = first; r < first + (int64_t)fdb_pqw_level_bytes((uint32_t)(end - first)) * 8; r++)
          CHECK(read_bits(file + po.levels_off, (uint64_t)(r - first), 1) == (r < end && c.valid(r) ? 1u : 0u));
      }
      CHECK((pc[k].delta_slot >= 0) == (with_encodings && encodings[k] == 1));
      if (pc[k].delta_slot >= 0) {  // the page's value bytes are the survey's count of them, and decode to the page's non-NULL values
        CHECK(po.values_off == FDB_PQW_NONE);
        const size_t dp = (size_t)pc[k].delta_slot * (size_t)g.n_pages + (size_t)p;
        const uint64_t off = L.parts[0].delta_out[dp], bytes = dh.page_bytes[dp];
        for (uint64_t b = 0; b < bytes; b++) { CHECK(off + b < L.body_bytes && owner[off + b] == 0); owner[off + b] = 4; }
        std::vector<uint64_t> want;
        for (int64_t r = first; r < end; r++) if (pc[k].validity == nullptr || c.valid(r)) want.push_back(c.v64[(size_t)r]);
        std::vector<uint8_t> exact(file + off, file + off + bytes);  // (sized exactly: a decoder that reads past the page is caught)
        check_delta_page(exact.data(), exact.size(), want);
        continue;
      }
      if (po.values_off == FDB_PQW_NONE) continue;
      const uint32_t w = pc[k].pq_kind == FDB_PQW_V64 ? 64 : pc[k].width;
      const uint64_t bytes = pc[k].pq_kind == FDB_PQW_V64 ? (uint64_t)cnt * 8 : fdb_pqw_packed_bytes(cnt, w);
      for (uint64_t b = 0; b < bytes; b++) { CHECK(owner[po.values_off + b] == 0); owner[po.values_off + b] = 3; }
      uint64_t j = 0;
      for (int64_t r = first; r < end; r++) {
        if (!(pc[k].validity == nullptr || c.valid(r))) continue;
        if (pc[k].pq_kind == FDB_PQW_V64) { uint64_t v; std::memcpy(&v, file + po.values_off + j * 8, 8); CHECK(v == c.v64[(size_t)r]); }
        else if (pc[k].pq_kind == FDB_PQW_BOOL) CHECK(read_bits(file + po.values_off, j, 1) == (c.v64[(size_t)r] >= 2 ? 1u : 0u));
        else CHECK(read_bits(file + po.values_off, j * w, w) == c.idx[(size_t)r]);
        j++;
      }
      for (uint64_t bit = j * (w == 64 ? 64 : w); bit < bytes * 8; bit++) CHECK(read_bits(file + po.values_off, bit, 1) == 0);  // padding bits zero
    }
  }
  for (uint64_t b = 0; b < L.body_bytes; b++) CHECK(owner[b] != 0);  // every byte of the body belongs to somebody
  // the same record with index options at random: the body is the same, the index follows it, the footer names it
  static const int32_t limit_choices[] = {0, 1, 3, 16, 17, 65536};
  std::vector<fdb_parquet_sorting_column> sorting;
  for (size_t k = 0; k < n_cols; k++) if (rnd(seed) % 3 == 0) sorting.push_back(fdb_parquet_sorting_column{(int32_t)k, (int8_t)(rnd(seed) & 1), (int8_t)(rnd(seed) & 1), {0, 0}});
  const fdb_parquet_index_options iopt{(int32_t)(rnd(seed) % 3), limit_choices[rnd(seed) % 6], sorting.empty() ? nullptr : sorting.data(), (int32_t)sorting.size()};
  spec.index = &iopt;
  PqwPlan indexed_plan = pqw_plan(in, rows, spec);
  PqxIndex& x = indexed_plan.x;
  CHECK(x.statistics == iopt.statistics && x.limit == (iopt.index_size_limit == 0 ? 16u : (uint32_t)iopt.index_size_limit) && x.sorting.size() == sorting.size());
  if (x.statistics > 0) pqx_minmax_host(pc, g, &x);
  {
    const PqwLayout I = pqw_layout(indexed_plan, sizes);
    CHECK(I.body_bytes == L.body_bytes && I.blob == L.blob && (x.any() || I.footer == L.footer) && (x.statistics == 2 || I.tail.empty()));
    check_index(cols, pc, g, stats, I, x, I.chunk_off, I.chunk_len);
    uint8_t* indexed = pqw_alloc_bytes(I.file_bytes(), false);
    std::memcpy(indexed, image.data(), (size_t)I.body_bytes);
    pqw_finish(I, indexed);
    CHECK(std::memcmp(indexed, file, (size_t)L.body_bytes) == 0 && std::memcmp(indexed + I.file_bytes() - 4, "PAR1", 4) == 0);
    CHECK(I.tail.empty() || std::memcmp(indexed + I.body_bytes, I.tail.data(), I.tail.size()) == 0);
    pqw_free_bytes(indexed);
  }
  // … and with bloom filters at random as well: the body is the same, the filters follow it, the index follows them
  static const int32_t bit_choices[] = {0, 1, 7, 10, 33, 64};
  std::vector<int8_t> filtered;
  for (size_t k = 0; k < n_cols; k++) filtered.push_back((int8_t)(cols[k].kind != ColKind::BOOL && rnd(seed) % 3 != 0));
  const bool no_array = rnd(seed) % 8 == 0;
  const fdb_parquet_bloom_options bopt{no_array ? nullptr : filtered.data(), no_array ? 0 : (int32_t)n_cols, bit_choices[rnd(seed) % 6]};
  spec.bloom = &bopt;
  PqwPlan filtered_plan = pqw_plan(in, rows, spec); filtered_plan.x = x;  // (with the table the min / max walk filled)
  PqbPlan& bl = filtered_plan.bloom;
  bool some = false;
  for (int8_t f : filtered) some = some || f != 0;
  CHECK(bl.any() == (some && !no_array) && (!bl.any() || bl.bits_per_value == (bopt.bits_per_value == 0 ? 10u : (uint32_t)bopt.bits_per_value)));
  if (bl.any()) pqb_size(pc, g, stats, &bl);
  {
    const PqwLayout Bf = pqw_layout(filtered_plan, sizes);
    CHECK(Bf.body_bytes == L.body_bytes && Bf.blooms.empty() == !bl.any() && (bl.any() || (Bf.bloom_bytes == 0 && Bf.blob == L.blob)));
    std::vector<unsigned char> bitsets((size_t)bl.table_bytes, 0);  // (sized exactly)
    pqb_insert_host(pc, g, bl, bitsets.data());
    uint8_t* filtered_file = pqw_alloc_bytes(Bf.file_bytes(), false);
    std::memcpy(filtered_file, image.data(), (size_t)Bf.body_bytes);
    for (const PqwLayout::Bloom& f : Bf.blooms) {
      CHECK(bl.table_off[f.col] % 32 == 0 && bl.table_off[f.col] + f.bytes <= bl.table_bytes && f.bits_off + f.bytes <= Bf.body_bytes + Bf.bloom_bytes);
      std::memcpy(filtered_file + f.bits_off, bitsets.data() + bl.table_off[f.col], (size_t)f.bytes);
    }
    pqw_finish(Bf, filtered_file);
    CHECK(std::memcmp(filtered_file, file, (size_t)L.body_bytes) == 0 && std::memcmp(filtered_file + Bf.file_bytes() - 4, "PAR1", 4) == 0);
    CHECK(Bf.tail.empty() || std::memcmp(filtered_file + Bf.body_bytes + Bf.bloom_bytes, Bf.tail.data(), Bf.tail.size()) == 0);
    check_bloom(cols, pc, rows, stats, (size_t)g.n_pages, Bf, bl, filtered_file);
    check_index(cols, pc, g, stats, Bf, x, Bf.chunk_off, Bf.chunk_len);
    pqw_free_bytes(filtered_file);
  }
  // … and with run options at random: no page longer, every stream cut into runs decodes to the page's levels or indices
  std::vector<int8_t> run_flags;
  for (size_t k = 0; k < n_cols; k++) run_flags.push_back((int8_t)(cols[k].kind == ColKind::DICT ? rnd(seed) % 4 : (rnd(seed) & 1) * 2));
  const fdb_parquet_run_options ropt{run_flags.data(), (int32_t)n_cols, 0};
  spec.index = nullptr; spec.bloom = nullptr; spec.runs = &ropt;
  const PqwPlan run_plan = pqw_plan(in, rows, spec); spec.runs = nullptr;
  const std::vector<PqwColumn>& rc = run_plan.cols;
  const size_t n_streams = run_plan.n_runs;
  CHECK(n_streams == pqr_streams(rc) && n_streams <= 2 * n_cols);
  if (n_streams > 0) {
    PqrHost rh;
    pqr_survey_host(rc, g, stats, &rh);
    CHECK(rh.page_bytes.size() == n_streams * (size_t)g.n_pages);
    const PqwLayout Rl = pqw_layout(run_plan, PqwSizes{stats, &dh.page_bytes, &rh.page_bytes});
    CHECK(Rl.body_bytes <= L.body_bytes && Rl.parts[0].run_out.size() == rh.page_bytes.size());
    std::vector<unsigned char> rimage(((size_t)Rl.body_bytes + 8 + 3) / 4 * 4, 0);
    pqw_encode_host(rc, g, Rl.parts[0].out, tile_base, rimage.data());
    pqd_encode_host(rc, g, stats, dh, Rl.parts[0].delta_out, rimage.data());
    pqr_encode_host(rh, Rl.parts[0].run_out, rimage.data());
    for (size_t b = (size_t)Rl.body_bytes; b < rimage.size(); b++) CHECK(rimage[b] == 0);
    std::vector<uint8_t> own(Rl.body_bytes, 0);
    for (const PqwLayout::Piece& p : Rl.pieces) for (size_t b = 0; b < p.len; b++) { CHECK(p.off + b < Rl.body_bytes && own[p.off + b] == 0); own[p.off + b] = 1; }
    for (size_t k = 0; k < n_cols; k++) {
      for (int pass = 0; pass < 2; pass++) {
        const bool levels = pass == 1;
        const int slot = levels ? rc[k].run_levels : rc[k].run_values;
        if (slot < 0) continue;
        CHECK(levels ? (run_flags[k] & 2) != 0 && rc[k].optional : (run_flags[k] & 1) != 0 && cols[k].kind == ColKind::DICT);
        const uint32_t w = levels ? 1 : rc[k].width;
        for (int64_t p = 0; p < g.n_pages; p++) {
          const size_t at = (size_t)slot * (size_t)g.n_pages + (size_t)p;
          const FdbPqwPageStat st = stats[k * (size_t)g.n_pages + (size_t)p];
          const int64_t first = fdb_pqw_page_first(g, p), end = fdb_pqw_page_end(g, p);
          const bool active = fdb_pqr_active(levels, st.count, (uint32_t)(end - first), st.mn, st.mx);
          CHECK(active == (Rl.parts[0].run_out[at] != FDB_PQW_NONE) && active == (rh.page_bytes[at] != 0));
          if (!active) continue;
          std::vector<uint32_t> want;
          for (int64_t r = first; r < end; r++) {
            if (levels) want.push_back(cols[k].valid(r) ? 1u : 0u);
            else if (cols[k].valid(r)) want.push_back(cols[k].idx[(size_t)r]);
          }
          const uint64_t off = Rl.parts[0].run_out[at], bytes = rh.page_bytes[at];
          size_t packed = 1;  // the one bit-packed run: its header, groups × w bytes
          for (uint64_t v = ((uint64_t)fdb_pqw_groups((uint32_t)want.size()) << 1) | 1; v >= 0x80; v >>= 7) packed++;
          packed += (size_t)fdb_pqw_packed_bytes((uint32_t)want.size(), w);
          CHECK(bytes <= packed && bytes >= 2);
          for (uint64_t b = 0; b < bytes; b++) { CHECK(off + b < Rl.body_bytes && own[off + b] == 0); own[off + b] = 5; }
          const std::vector<uint8_t> exact(rimage.begin() + (size_t)off, rimage.begin() + (size_t)(off + bytes));  // (sized exactly: a reader that runs past the stream is caught)
          check_hybrid(exact.data(), exact.size(), w, want);
        }
      }
    }
  }
  // … and with group options at random — a row_group_rows that leaves one row group, dictionaries of used entries only — beside the run
  // options: the present and remap walks (fdb_pqdict.h), and a dictionary reader of the program's own finds in every pruned chunk
  // exactly the used entries, and in every page the ranks among them
  {
    const int64_t whole_words = (rows + 63) / 64 * 64;
    const fdb_parquet_group_options gopt{rnd(seed) % 3 == 0 ? whole_words + 64 * (int64_t)(rnd(seed) % 3) : 0, (int32_t)(rnd(seed) % 4 != 0), 0};
    spec.runs = (rnd(seed) & 1) ? &ropt : nullptr; spec.groups = &gopt;
    PqwPlan used_plan = pqw_plan(in, rows, spec);
    const bool with_runs = spec.runs != nullptr;
    spec.runs = nullptr; spec.groups = nullptr;
    CHECK(used_plan.grouped == (gopt.row_group_rows != 0 || gopt.dictionaries != 0) && used_plan.dict.any() == (gopt.dictionaries == 1 && !used_plan.dict.cols.empty()));
    PqgPlan& dp = used_plan.dict;
    std::vector<std::vector<uint32_t>> rekeyed;
    std::vector<std::vector<uint32_t>> used_entries(n_cols);
    if (dp.any()) {
      pqg_present_host(used_plan.cols, g, &dp);
      pqg_resolve(stats, g, &used_plan.cols, &dp);
      pqg_remap_host(used_plan.cols, g, dp, &rekeyed);
      for (size_t slot = 0; slot < dp.cols.size(); slot++) {
        const size_t k = dp.cols[slot].col;
        PqwColumn& uc = used_plan.cols[k];
        CHECK(cols[k].kind == ColKind::DICT && uc.used_slot == (int)slot && rekeyed[slot].size() == (size_t)rows + 8);
        std::vector<bool> seen(cols[k].dict->values.size(), false);
        for (int64_t r = 0; r < rows; r++) if (cols[k].valid(r)) seen[cols[k].idx[(size_t)r]] = true;
        std::vector<uint32_t> rank(seen.size(), 0);
        for (size_t e = 0; e < seen.size(); e++) if (seen[e]) { rank[e] = (uint32_t)used_entries[k].size(); used_entries[k].push_back((uint32_t)e); }
        CHECK(dp.cols[slot].used == used_entries[k].size() && uc.entries == used_entries[k].size() && uc.width == (used_entries[k].empty() ? 0 : fdb_pqw_bits(used_entries[k].size() - 1)));
        CHECK((uc.pq_kind == PQW_NO_VALUES) == used_entries[k].empty());
        for (int64_t r = 0; r < rows; r++) CHECK(rekeyed[slot][(size_t)r] == (cols[k].valid(r) ? rank[cols[k].idx[(size_t)r]] : 0u));
        for (size_t r = (size_t)rows; r < rekeyed[slot].size(); r++) CHECK(rekeyed[slot][r] == 0);
        uc.raw_values = uc.values; uc.values = rekeyed[slot].data();
      }
    }
    const std::vector<PqwColumn>& uc = used_plan.cols;
    PqrHost rh;
    if (used_plan.n_runs > 0) pqr_survey_host(uc, g, stats, &rh);
    CHECK(with_runs || used_plan.n_runs == 0);
    const PqwLayout U = pqw_layout(used_plan, PqwSizes{stats, &dh.page_bytes, used_plan.n_runs > 0 ? &rh.page_bytes : nullptr});
    CHECK(U.body_bytes <= L.body_bytes && (used_plan.grouped || with_runs || U.footer == L.footer) && (!used_plan.grouped || with_runs || dp.any() || U.footer.size() == L.footer.size() + 2));
    std::vector<unsigned char> uimage(((size_t)U.body_bytes + 8 + 3) / 4 * 4, 0);
    pqw_encode_host(uc, g, U.parts[0].out, tile_base, uimage.data());
    pqd_encode_host(uc, g, stats, dh, U.parts[0].delta_out, uimage.data());
    if (used_plan.n_runs > 0) pqr_encode_host(rh, U.parts[0].run_out, uimage.data());
    for (size_t b = (size_t)U.body_bytes; b < uimage.size(); b++) CHECK(uimage[b] == 0);
    uint8_t* ufile = pqw_alloc_bytes(U.file_bytes(), false);
    std::memcpy(ufile, uimage.data(), (size_t)U.body_bytes);
    pqw_finish(U, ufile);
    for (const PqgPlan::Col& o : dp.cols) {  // the dictionary reader: the chunk's first page, when there is a used entry, holds exactly those
      const size_t k = o.col;
      const std::vector<uint8_t> chunk(ufile + U.chunk_off[k], ufile + U.chunk_off[k] + U.chunk_len[k]);  // (sized exactly)
      if (used_entries[k].empty()) continue;  // (no dictionary page: the chunk starts with a data page — the run of CHECKs on pq_kind above)
      check_dictionary_page(chunk, cols[k], used_entries[k]);
      // the pages the encode pass packed: the ranks at the used entries' width
      for (int64_t p = 0; p < g.n_pages; p++) {
        const FdbPqwPageOut po = U.parts[0].out[k * (size_t)g.n_pages + (size_t)p];
        if (po.values_off == FDB_PQW_NONE) continue;
        uint64_t j = 0;
        for (int64_t row = fdb_pqw_page_first(g, p); row < fdb_pqw_page_end(g, p); row++)
          if (cols[k].valid(row)) { CHECK(read_bits(ufile + po.values_off, j * uc[k].width, uc[k].width) == rekeyed[(size_t)uc[k].used_slot][(size_t)row]); j++; }
      }
    }
    pqw_free_bytes(ufile);
  }
  // … and with a string form drawn per byte-array column (fdb_pqbytes.h), beside runs on levels at random: the byte survey's walk and the
  // host's scan of its table, the lengths as one more column of the DELTA walk, the byte encode walk word by word — and a PLAIN reader and
  // a DELTA_LENGTH reader of the program's own find in every page the values of its non-NULL rows, in exactly the bytes the layout gave it
  {
    std::vector<int8_t> forms, level_flags;
    for (size_t k = 0; k < n_cols; k++) forms.push_back((int8_t)(cols[k].kind == ColKind::DICT ? rnd(seed) % 3 : 0));
    for (size_t k = 0; k < n_cols; k++) level_flags.push_back((int8_t)((rnd(seed) & 1) * 2));
    const fdb_parquet_string_options sopt{forms.data(), (int32_t)n_cols, 0};
    const fdb_parquet_run_options lopt{level_flags.data(), (int32_t)n_cols, 0};
    spec.runs = (rnd(seed) & 1) ? &lopt : nullptr; spec.strings = &sopt;
    PqwPlan sp = pqw_plan(in, rows, spec);
    spec.runs = nullptr; spec.strings = nullptr;
    size_t want_streams = 0;
    for (size_t k = 0; k < n_cols; k++) want_streams += forms[k] != 0 && !cols[k].dict->values.empty();
    CHECK(sp.n_bytes == want_streams && !sp.dict.any());
    PqyPlan& y = sp.strings;
    if (sp.n_bytes > 0) { pqy_survey_host(sp.cols, g, sp.n_bytes, &y); pqy_scan(g, sp.n_bytes, &y); }
    PqdHost sdh;
    pqd_survey_host(sp.cols, g, stats, tile_base, &sdh, &y);
    PqrHost srh;
    if (sp.n_runs > 0) pqr_survey_host(sp.cols, g, stats, &srh);
    const PqwLayout S = pqw_layout(sp, PqwSizes{stats, &sdh.page_bytes, sp.n_runs > 0 ? &srh.page_bytes : nullptr, nullptr, sp.n_bytes > 0 ? &y.page_bytes : nullptr});
    CHECK(S.parts[0].bytes_out.size() == sp.n_bytes * (size_t)g.n_pages);
    std::vector<unsigned char> simage(((size_t)S.body_bytes + 8 + 3) / 4 * 4, 0);
    pqw_encode_host(sp.cols, g, S.parts[0].out, tile_base, simage.data());
    pqd_encode_host(sp.cols, g, stats, sdh, S.parts[0].delta_out, simage.data());
    if (sp.n_runs > 0) pqr_encode_host(srh, S.parts[0].run_out, simage.data());
    if (sp.n_bytes > 0) pqy_encode_host(sp.cols, g, y, S.parts[0].bytes_out, simage.data());
    for (size_t b = (size_t)S.body_bytes; b < simage.size(); b++) CHECK(simage[b] == 0);
    std::vector<uint8_t> own(S.body_bytes, 0);  // no byte of a stream is the host's
    for (const PqwLayout::Piece& p : S.pieces) for (size_t b = 0; b < p.len; b++) { CHECK(p.off + b < S.body_bytes && own[p.off + b] == 0); own[p.off + b] = 1; }
    for (size_t k = 0; k < n_cols; k++) {
      const PqwColumn& c = sp.cols[k];
      CHECK((c.bytes_slot >= 0) == (forms[k] != 0 && !cols[k].dict->values.empty()) && (c.bytes_slot < 0 || c.form == forms[k]));
      CHECK((c.form == FDB_PQY_DELTA_LENGTH && c.bytes_slot >= 0) == (cols[k].kind == ColKind::DICT && c.delta_slot >= 0));
      if (c.bytes_slot < 0) continue;
      for (int64_t p = 0; p < g.n_pages; p++) {
        const size_t at = (size_t)c.bytes_slot * (size_t)g.n_pages + (size_t)p;
        std::vector<const std::string*> want;
        std::vector<uint64_t> lens;
        uint64_t total = 0;
        for (int64_t r = fdb_pqw_page_first(g, p); r < fdb_pqw_page_end(g, p); r++)
          if (cols[k].valid(r)) { want.push_back(&cols[k].dict->values[cols[k].idx[(size_t)r]]); lens.push_back(want.back()->size()); total += want.back()->size(); }
        const uint64_t stream = total + (c.form == FDB_PQY_PLAIN ? 4 * want.size() : 0), off = S.parts[0].bytes_out[at];
        CHECK(y.page_bytes[at] == stream && (off != FDB_PQW_NONE) == (stream > 0));
        if (c.form == FDB_PQY_DELTA_LENGTH) {  // the lengths: a DELTA page of exactly the surveyed bytes, the byte stream right behind it
          const size_t dat = (size_t)c.delta_slot * (size_t)g.n_pages + (size_t)p;
          const uint64_t doff = S.parts[0].delta_out[dat], dbytes = sdh.page_bytes[dat];
          CHECK(doff != FDB_PQW_NONE && doff + dbytes <= S.body_bytes && (stream == 0 || off == doff + dbytes));
          const std::vector<uint8_t> exact(simage.begin() + (size_t)doff, simage.begin() + (size_t)(doff + dbytes));  // (sized exactly)
          check_delta_page(exact.data(), exact.size(), lens);
          if (want.empty()) CHECK(dbytes == 5 && std::memcmp(exact.data(), "\x80\x01\x04\x00\x00", 5) == 0);
          for (uint64_t b = 0; b < dbytes; b++) { CHECK(own[doff + b] == 0); own[doff + b] = 6; }
        }
        if (stream == 0) continue;
        CHECK(off + stream <= S.body_bytes);
        for (uint64_t b = 0; b < stream; b++) { CHECK(own[off + b] == 0); own[off + b] = 7; }
        const std::vector<uint8_t> exact(simage.begin() + (size_t)off, simage.begin() + (size_t)(off + stream));  // (sized exactly: a reader that runs past the stream is caught)
        size_t rd = 0;
        for (const std::string* v : want) {
          if (c.form == FDB_PQY_PLAIN) { uint32_t len; std::memcpy(&len, exact.data() + rd, 4); CHECK(len == v->size()); rd += 4; }
          CHECK(rd + v->size() <= exact.size() && std::memcmp(exact.data() + rd, v->data(), v->size()) == 0);
          rd += v->size();
        }
        CHECK(rd == exact.size());
      }
    }
  }
  // … and cut into several row groups — row_group_rows a multiple of 64 below the rows, the dictionaries whole or of used entries, runs at
  // random: the plan's parts (pqw_parts: the full groups as virtual columns, the shorter last group) walked pass by pass as the self-test
  // walks them, into ONE layout. Every group is then read back: its chunks follow each other from where the group before ended, every
  // chunk of a dictionary column starts with a dictionary page of exactly the entries its own rows use (or of the whole dictionary), and
  // every plainly packed index page holds the rows' indices, re-keyed or as they are.
  if (rows > 64) {
    const int64_t R = 64 * (1 + (int64_t)(rnd(seed) % (uint64_t)((rows - 1) / 64)));
    const fdb_parquet_group_options gopt{R, (int32_t)(rnd(seed) & 1), 0};
    spec.runs = (rnd(seed) & 1) ? &ropt : nullptr; spec.groups = &gopt;
    std::vector<PqwPlan> plans = pqw_parts(pqw_plan(in, rows, spec), spec);
    spec.runs = nullptr; spec.groups = nullptr;
    const int64_t n_groups = (rows + R - 1) / R;
    CHECK(plans.size() == (rows % R == 0 ? 1u : 2u) && plans[0].n_groups == rows / R && plans[0].g.rows == R && (plans.size() == 1 || (plans[1].n_groups == 1 && plans[1].g.rows == rows % R && plans[1].first_group == rows / R)));
    struct Walk { std::vector<FdbPqwPageStat> stats; std::vector<uint32_t> tile_base; std::vector<std::vector<uint32_t>> rekeyed; PqdHost delta; PqrHost runs; };
    std::vector<Walk> walks(plans.size());
    std::vector<const PqwPlan*> parts;
    std::vector<PqwSizes> part_sizes;
    for (size_t pi = 0; pi < plans.size(); pi++) {
      PqwPlan& P = plans[pi]; Walk& w = walks[pi];
      CHECK(P.cols.size() == (size_t)P.n_groups * n_cols && P.n_real == n_cols && P.file_rows == rows && P.grouped);
      pqw_survey_host(P.cols, P.g, &w.stats, &w.tile_base);
      if (P.dict.any()) {
        pqg_present_host(P.cols, P.g, &P.dict);
        pqg_resolve(w.stats, P.g, &P.cols, &P.dict);
        pqg_remap_host(P.cols, P.g, P.dict, &w.rekeyed);
        for (size_t slot = 0; slot < P.dict.cols.size(); slot++) { PqwColumn& c = P.cols[P.dict.cols[slot].col]; c.raw_values = c.values; c.values = w.rekeyed[slot].data(); }
      }
      pqd_survey_host(P.cols, P.g, w.stats, w.tile_base, &w.delta);
      if (P.n_runs > 0) pqr_survey_host(P.cols, P.g, w.stats, &w.runs);
      parts.push_back(&P);
      part_sizes.push_back(PqwSizes{w.stats, &w.delta.page_bytes, P.n_runs > 0 ? &w.runs.page_bytes : nullptr});
    }
    const PqwLayout Gl = pqw_layout(parts, part_sizes);
    CHECK(Gl.parts.size() == plans.size() && Gl.chunk_off.size() == (size_t)n_groups * n_cols && Gl.chunk_len.size() == Gl.chunk_off.size());
    std::vector<unsigned char> gimage(((size_t)Gl.body_bytes + 8 + 3) / 4 * 4, 0);
    for (size_t pi = 0; pi < plans.size(); pi++) {
      pqw_encode_host(plans[pi].cols, plans[pi].g, Gl.parts[pi].out, walks[pi].tile_base, gimage.data());
      pqd_encode_host(plans[pi].cols, plans[pi].g, walks[pi].stats, walks[pi].delta, Gl.parts[pi].delta_out, gimage.data());
      if (plans[pi].n_runs > 0) pqr_encode_host(walks[pi].runs, Gl.parts[pi].run_out, gimage.data());
    }
    for (size_t b = (size_t)Gl.body_bytes; b < gimage.size(); b++) CHECK(gimage[b] == 0);
    uint8_t* gfile = pqw_alloc_bytes(Gl.file_bytes(), false);
    std::memcpy(gfile, gimage.data(), (size_t)Gl.body_bytes);
    pqw_finish(Gl, gfile);
    uint64_t at = 4;
    for (int64_t gi = 0; gi < n_groups; gi++) {
      const size_t pi = gi < plans[0].n_groups ? 0 : 1;
      const PqwPlan& P = plans[pi];
      const int64_t first = gi * R, end = std::min(rows, first + R);
      for (size_t k = 0; k < n_cols; k++) {
        const size_t chunk_at = (size_t)gi * n_cols + k, vk = (size_t)(gi - P.first_group) * n_cols + k;
        CHECK(Gl.chunk_off[chunk_at] == at && Gl.chunk_len[chunk_at] > 0 && at + Gl.chunk_len[chunk_at] <= Gl.body_bytes);
        at += Gl.chunk_len[chunk_at];
        if (cols[k].kind != ColKind::DICT) continue;
        const PqwColumn& vc = P.cols[vk];
        CHECK(vc.real == k);
        std::vector<bool> seen(cols[k].dict->values.size(), gopt.dictionaries == 0);
        for (int64_t r = first; r < end; r++) if (cols[k].valid(r)) seen[cols[k].idx[(size_t)r]] = true;
        std::vector<uint32_t> used, rank(seen.size(), 0);
        for (size_t e = 0; e < seen.size(); e++) if (seen[e]) { rank[e] = (uint32_t)used.size(); used.push_back((uint32_t)e); }
        CHECK(vc.entries == used.size() && (vc.pq_kind == PQW_NO_VALUES) == used.empty() && vc.width == (used.empty() ? 0 : fdb_pqw_bits(used.size() - 1)));
        if (used.empty()) continue;
        check_dictionary_page(std::vector<uint8_t>(gfile + Gl.chunk_off[chunk_at], gfile + Gl.chunk_off[chunk_at] + Gl.chunk_len[chunk_at]), cols[k], used);
        for (int64_t p = 0; p < P.g.n_pages; p++) {
          const FdbPqwPageOut po = Gl.parts[pi].out[vk * (size_t)P.g.n_pages + (size_t)p];
          if (po.values_off == FDB_PQW_NONE) continue;
          uint64_t j = 0;
          for (int64_t row = first + fdb_pqw_page_first(P.g, p); row < first + fdb_pqw_page_end(P.g, p); row++)
            if (cols[k].valid(row)) { CHECK(read_bits(gfile + po.values_off, j * vc.width, vc.width) == rank[cols[k].idx[(size_t)row]]); j++; }
        }
      }
    }
    CHECK(at == Gl.body_bytes);
    pqw_free_bytes(gfile);
  }
  // the same record with a codec per column at random (three rounds in four): what fdb_selftest_parquet_write_compressed does, step by step
  std::vector<int8_t> codecs;
  for (size_t k = 0; k < n_cols; k++) { static const int8_t drawn[3] = {0, 1, 7}; codecs.push_back(drawn[rnd(seed) % 3]); }
  if ((round & 3) != 3) {
    spec.codecs = codecs.data(); spec.n_codecs = (int32_t)n_cols; spec.index = &iopt;
    PqwPlan compressed_plan = pqw_plan(in, rows, spec); compressed_plan.x = x;
    const std::vector<PqwColumn>& cc = compressed_plan.cols;
    const PqwLayout S = pqw_layout(compressed_plan, sizes);  // the staging layout: the payload offsets are those of the uncompressed file
    CHECK(S.body_bytes == L.body_bytes);
    std::vector<unsigned char> staging(image);
    for (const PqwLayout::Piece& p : S.body_pieces) { CHECK(p.off + p.len <= S.body_bytes && p.pos + p.len <= S.body_blob.size()); std::memcpy(staging.data() + p.off, S.body_blob.data() + p.pos, p.len); }
    CHECK(S.pages.size() == pqw_compressed_columns(cc) * (size_t)g.n_pages);
    std::vector<uint32_t> page_elements, table(FDB_PQS_TABLE);
    std::vector<std::string> elements;
    for (const PqwLayout::Page& pg : S.pages) {
      CHECK(pg.off + pg.body <= S.body_bytes);
      CHECK(std::memcmp(staging.data() + pg.off, file + pg.off, (size_t)pg.body) == 0);  // a whole body: what the uncompressed file holds there
      std::string e;
      if (pg.codec == PQW_LZ4_RAW) {  // the whole block, by the walk over a body sized exactly
        const std::vector<unsigned char> body(staging.begin() + (size_t)pg.off, staging.begin() + (size_t)(pg.off + pg.body));
        e = pql_block_host(body.data(), body.size());
      }
      for (uint64_t at = 0; at < pg.body && pg.codec != PQW_LZ4_RAW; at += FDB_PQS_FRAGMENT) {
        const uint32_t len = (uint32_t)std::min<uint64_t>(FDB_PQS_FRAGMENT, pg.body - at);
        const std::vector<unsigned char> frag(staging.begin() + (size_t)(pg.off + at), staging.begin() + (size_t)(pg.off + at) + len);  // (sized exactly)
        std::vector<unsigned char> out(fdb_pqs_bound(len));
        e.append((const char*)out.data(), fdb_pqs_compress_fragment_host(frag.data(), len, table.data(), out.data()));
      }
      page_elements.push_back((uint32_t)e.size());
      elements.push_back(std::move(e));
    }
    const PqwLayout F = pqw_layout(compressed_plan, PqwSizes{stats, &dh.page_bytes, nullptr, &page_elements});
    CHECK(F.pages.size() == S.pages.size());
    check_index(cols, cc, g, stats, F, x, F.chunk_off, F.chunk_len);
    const size_t out_bytes = F.file_bytes();
    uint8_t* out_file = pqw_alloc_bytes(out_bytes, false);
    std::vector<uint8_t> own(F.body_bytes, 0);
    for (const PqwLayout::Piece& p : F.pieces) for (size_t b = 0; b < p.len; b++) { CHECK(p.off + b < F.body_bytes && own[p.off + b] == 0); own[p.off + b] = 1; }
    for (size_t i = 0; i < F.pages.size(); i++) {
      CHECK(F.pages[i].body == S.pages[i].body && F.pages[i].off + elements[i].size() <= F.body_bytes);
      std::memcpy(out_file + F.pages[i].off, elements[i].data(), elements[i].size());
      for (size_t b = 0; b < elements[i].size(); b++) { CHECK(own[F.pages[i].off + b] == 0); own[F.pages[i].off + b] = 2; }
    }
    for (size_t k = 0; k < n_cols; k++) {
      if (cc[k].codec != 0) continue;
      CHECK(F.chunk_len[k] == S.chunk_len[k] && F.chunk_off[k] + F.chunk_len[k] <= F.body_bytes);
      std::memcpy(out_file + F.chunk_off[k], staging.data() + S.chunk_off[k], (size_t)S.chunk_len[k]);
      for (uint64_t b = 0; b < F.chunk_len[k]; b++) if (own[F.chunk_off[k] + b] == 0) own[F.chunk_off[k] + b] = 3;
    }
    for (uint64_t b = 0; b < F.body_bytes; b++) CHECK(own[b] != 0);
    pqw_finish(F, out_file);
    CHECK(std::memcmp(out_file, "PAR1", 4) == 0 && std::memcmp(out_file + out_bytes - 4, "PAR1", 4) == 0);
    for (size_t i = 0; i < F.pages.size(); i++) {  // the preamble sits in front of the elements; the block inflates to the body
      CHECK(F.pages[i].codec == S.pages[i].codec);
      if (F.pages[i].codec == PQW_LZ4_RAW) {  // (bare: no preamble)
        check_lz4_block(std::string((const char*)out_file + F.pages[i].off, elements[i].size()), staging.data() + S.pages[i].off, (size_t)S.pages[i].body);
        continue;
      }
      size_t pl = 1;
      for (uint64_t v = F.pages[i].body; v >= 0x80; v >>= 7) pl++;
      CHECK(F.pages[i].off >= pl);
      check_block(std::string((const char*)out_file + F.pages[i].off - pl, pl + elements[i].size()), staging.data() + S.pages[i].off, (size_t)S.pages[i].body);
    }
    for (size_t k = 0; k < n_cols; k++) {  // a compressed dictionary page: the block the host walk makes of the entries
      if (cc[k].codec == 0 || cc[k].pq_kind != FDB_PQW_INDEX) continue;
      std::string body;
      for (const std::string& v : cc[k].dict->values) { const uint32_t n = (uint32_t)v.size(); body.append((const char*)&n, 4); body += v; }
      const bool lz4 = cc[k].codec == PQW_LZ4_RAW;
      const std::string block = lz4 ? pql_block_host((const unsigned char*)body.data(), body.size()) : pqs_block_host((const unsigned char*)body.data(), body.size());
      if (lz4) check_lz4_block(block, (const unsigned char*)body.data(), body.size()); else check_block(block, (const unsigned char*)body.data(), body.size());
      bool found = false;
      for (size_t at = (size_t)F.chunk_off[k]; at + block.size() <= (size_t)(F.chunk_off[k] + F.chunk_len[k]) && at < (size_t)F.chunk_off[k] + 32 && !found; at++)
        found = std::memcmp(out_file + at, block.data(), block.size()) == 0;
      CHECK(found);  // right behind the dictionary page's header
    }
    pqw_free_bytes(out_file);
  }
  pqw_free_bytes(file);
}

static void refusals() {
  std::vector<PqwInput> in(1);
  std::vector<uint64_t> v(8, 0);
  std::vector<uint8_t> bits(8, 0x0F);
  in[0].name = "x"; in[0].kind = ColKind::I64; in[0].values = v.data(); in[0].validity = bits.data(); in[0].null_count = 4;
  int32_t pr = 0;
  const auto code = [&](const fdb_parquet_write_options& o) { try { pqw_columns(in, 8, PqwSpec{&o}, &pr); } catch (const Error& e) { return e.code; } return (int)FDB_OK; };
  const int8_t required = 0, bad = 3;
  CHECK(code(fdb_parquet_write_options{0, 0, nullptr}) == FDB_OK && pr == 65536);
  CHECK(code(fdb_parquet_write_options{100, 0, nullptr}) == FDB_ERR_INVALID);
  CHECK(code(fdb_parquet_write_options{32, 0, nullptr}) == FDB_ERR_INVALID);
  CHECK(code(fdb_parquet_write_options{(1 << 24) + 64, 0, nullptr}) == FDB_ERR_INVALID);
  CHECK(code(fdb_parquet_write_options{64, 2, &required}) == FDB_ERR_INVALID);
  CHECK(code(fdb_parquet_write_options{64, 1, &required}) == FDB_ERR_INVALID);
  CHECK(code(fdb_parquet_write_options{64, 1, &bad}) == FDB_ERR_INVALID);
  const fdb_parquet_write_options plain_opt{64, 0, nullptr};
  const auto enc_code = [&](const int8_t* e, int32_t n) { try { pqw_columns(in, 8, PqwSpec{&plain_opt, e, n}, &pr); } catch (const Error& e2) { return e2.code; } return (int)FDB_OK; };
  const int8_t delta = 1, two = 2, both[2] = {1, 1};
  CHECK(enc_code(&delta, 1) == FDB_OK && enc_code(nullptr, 0) == FDB_OK);
  CHECK(enc_code(&two, 1) == FDB_ERR_INVALID && enc_code(both, 2) == FDB_ERR_INVALID && enc_code(nullptr, 1) == FDB_ERR_INVALID);
  const auto codec_code = [&](const int8_t* c, int32_t n) { try { pqw_columns(in, 8, PqwSpec{&plain_opt, nullptr, 0, c, n}, &pr); } catch (const Error& e2) { return e2.code; } return (int)FDB_OK; };
  const int8_t minus = -1, lz4 = 7, five = 5, six = 6, eight = 8;
  CHECK(codec_code(&delta, 1) == FDB_OK && codec_code(nullptr, 0) == FDB_OK && codec_code(&lz4, 1) == FDB_OK);
  CHECK(codec_code(&five, 1) == FDB_ERR_INVALID && codec_code(&six, 1) == FDB_ERR_INVALID && codec_code(&eight, 1) == FDB_ERR_INVALID);
  CHECK(codec_code(&two, 1) == FDB_ERR_INVALID && codec_code(&minus, 1) == FDB_ERR_INVALID && codec_code(both, 2) == FDB_ERR_INVALID && codec_code(nullptr, 1) == FDB_ERR_INVALID);
  const auto index_code = [&](const fdb_parquet_index_options& o, size_t n) { try { pqx_plan(&o, n); } catch (const Error& e2) { return e2.code; } return (int)FDB_OK; };
  const fdb_parquet_sorting_column s0{0, 0, 0, {0, 0}}, s2{2, 1, 1, {0, 0}}, twice[2] = {s0, s0}, ok2[2] = {s2, s0};
  CHECK(index_code(fdb_parquet_index_options{0, 0, nullptr, 0}, 1) == FDB_OK && index_code(fdb_parquet_index_options{2, 65536, ok2, 2}, 3) == FDB_OK && !pqx_plan(nullptr, 1).any());
  CHECK(index_code(fdb_parquet_index_options{3, 0, nullptr, 0}, 1) == FDB_ERR_INVALID && index_code(fdb_parquet_index_options{-1, 0, nullptr, 0}, 1) == FDB_ERR_INVALID);
  CHECK(index_code(fdb_parquet_index_options{1, 65537, nullptr, 0}, 1) == FDB_ERR_INVALID && index_code(fdb_parquet_index_options{0, -1, nullptr, 0}, 1) == FDB_ERR_INVALID);
  CHECK(index_code(fdb_parquet_index_options{1, 0, &s2, 1}, 2) == FDB_ERR_INVALID && index_code(fdb_parquet_index_options{1, 0, twice, 2}, 2) == FDB_ERR_INVALID);
  CHECK(index_code(fdb_parquet_index_options{1, 0, nullptr, 1}, 2) == FDB_ERR_INVALID && index_code(fdb_parquet_index_options{1, 0, &s0, -1}, 2) == FDB_ERR_INVALID);
  const auto bloom_code = [&](const fdb_parquet_bloom_options& o) { try { pqb_plan(&o, pqw_columns(in, 8, PqwSpec{&plain_opt}, &pr)); } catch (const Error& e2) { return e2.code; } return (int)FDB_OK; };
  const int8_t none = 0;
  CHECK(bloom_code(fdb_parquet_bloom_options{&delta, 1, 0}) == FDB_OK && bloom_code(fdb_parquet_bloom_options{&delta, 1, 64}) == FDB_OK && bloom_code(fdb_parquet_bloom_options{nullptr, 0, 0}) == FDB_OK);
  CHECK(!pqb_plan(nullptr, pqw_columns(in, 8, PqwSpec{&plain_opt}, &pr)).any() && bloom_code(fdb_parquet_bloom_options{&none, 1, 1}) == FDB_OK);
  CHECK(bloom_code(fdb_parquet_bloom_options{&two, 1, 0}) == FDB_ERR_INVALID && bloom_code(fdb_parquet_bloom_options{&minus, 1, 0}) == FDB_ERR_INVALID);
  CHECK(bloom_code(fdb_parquet_bloom_options{both, 2, 0}) == FDB_ERR_INVALID && bloom_code(fdb_parquet_bloom_options{nullptr, 1, 0}) == FDB_ERR_INVALID);
  CHECK(bloom_code(fdb_parquet_bloom_options{&delta, 1, 65}) == FDB_ERR_INVALID && bloom_code(fdb_parquet_bloom_options{&none, 1, -1}) == FDB_ERR_INVALID);
  const auto run_code = [&](const fdb_parquet_run_options& o) { try { std::vector<PqwColumn> c = pqw_columns(in, 8, PqwSpec{&plain_opt}, &pr); pqr_plan(&o, &c); } catch (const Error& e2) { return e2.code; } return (int)FDB_OK; };
  const int8_t four = 4;
  CHECK(run_code(fdb_parquet_run_options{&two, 1, 0}) == FDB_OK && run_code(fdb_parquet_run_options{&none, 1, 0}) == FDB_OK && run_code(fdb_parquet_run_options{nullptr, 0, 0}) == FDB_OK);
  CHECK(run_code(fdb_parquet_run_options{&delta, 1, 0}) == FDB_ERR_UNSUPPORTED && run_code(fdb_parquet_run_options{&bad, 1, 0}) == FDB_ERR_UNSUPPORTED);  // bit 0 on an int64 column
  CHECK(run_code(fdb_parquet_run_options{&four, 1, 0}) == FDB_ERR_INVALID && run_code(fdb_parquet_run_options{&minus, 1, 0}) == FDB_ERR_INVALID);
  CHECK(run_code(fdb_parquet_run_options{both, 2, 0}) == FDB_ERR_INVALID && run_code(fdb_parquet_run_options{nullptr, 1, 0}) == FDB_ERR_INVALID);
  const auto group_code = [&](const fdb_parquet_group_options& o, int64_t rows) { try { std::vector<PqwColumn> c = pqw_columns(in, 8, PqwSpec{&plain_opt}, &pr); pqg_plan(&o, rows, &c); } catch (const Error& e2) { return e2.code; } return (int)FDB_OK; };
  CHECK(group_code(fdb_parquet_group_options{0, 0, 0}, 8) == FDB_OK && group_code(fdb_parquet_group_options{64, 1, 0}, 64) == FDB_OK && group_code(fdb_parquet_group_options{128, 0, 0}, 0) == FDB_OK);
  CHECK(group_code(fdb_parquet_group_options{-64, 0, 0}, 8) == FDB_ERR_INVALID && group_code(fdb_parquet_group_options{63, 0, 0}, 8) == FDB_ERR_INVALID && group_code(fdb_parquet_group_options{64, 0, 0}, 64 * 32767 + 1) == FDB_ERR_INVALID);
  CHECK(group_code(fdb_parquet_group_options{0, 2, 0}, 8) == FDB_ERR_INVALID && group_code(fdb_parquet_group_options{0, -1, 0}, 8) == FDB_ERR_INVALID && group_code(fdb_parquet_group_options{0, 1, 1}, 8) == FDB_ERR_INVALID);
  CHECK(group_code(fdb_parquet_group_options{64, 0, 0}, 65) == FDB_OK && group_code(fdb_parquet_group_options{64, 1, 0}, 64 * 32767) == FDB_OK);  // several row groups, as many as an ordinal can say
  const auto string_code = [&](const fdb_parquet_string_options& o, const fdb_parquet_run_options* r) {
    try { std::vector<PqwColumn> c = pqw_columns(in, 8, PqwSpec{&plain_opt}, &pr); PqyPlan y; pqy_plan(&o, r, &c, &y); } catch (const Error& e2) { return e2.code; } return (int)FDB_OK;
  };
  CHECK(string_code(fdb_parquet_string_options{&none, 1, 0}, nullptr) == FDB_OK && string_code(fdb_parquet_string_options{nullptr, 0, 0}, nullptr) == FDB_OK);
  CHECK(string_code(fdb_parquet_string_options{&delta, 1, 0}, nullptr) == FDB_ERR_UNSUPPORTED && string_code(fdb_parquet_string_options{&two, 1, 0}, nullptr) == FDB_ERR_UNSUPPORTED);  // a form on an int64 column
  CHECK(string_code(fdb_parquet_string_options{&bad, 1, 0}, nullptr) == FDB_ERR_INVALID && string_code(fdb_parquet_string_options{&minus, 1, 0}, nullptr) == FDB_ERR_INVALID);
  CHECK(string_code(fdb_parquet_string_options{both, 2, 0}, nullptr) == FDB_ERR_INVALID && string_code(fdb_parquet_string_options{nullptr, 1, 0}, nullptr) == FDB_ERR_INVALID && string_code(fdb_parquet_string_options{&none, 1, 1}, nullptr) == FDB_ERR_INVALID);
  in[0].kind = ColKind::F64;
  CHECK(enc_code(&delta, 1) == FDB_ERR_UNSUPPORTED && bloom_code(fdb_parquet_bloom_options{&delta, 1, 0}) == FDB_OK);
  in[0].kind = ColKind::BOOL;
  CHECK(enc_code(&delta, 1) == FDB_ERR_UNSUPPORTED);
  CHECK(bloom_code(fdb_parquet_bloom_options{&delta, 1, 0}) == FDB_ERR_UNSUPPORTED && bloom_code(fdb_parquet_bloom_options{&none, 1, 0}) == FDB_OK);
  in[0].kind = ColKind::OTHER;
  CHECK(code(fdb_parquet_write_options{64, 0, nullptr}) == FDB_ERR_UNSUPPORTED);
  in[0].kind = ColKind::DICT;
  CHECK(code(fdb_parquet_write_options{64, 0, nullptr}) == FDB_ERR_INVALID);  // no dictionary
  pqw_free_bytes(nullptr);
}

int main() {
  uint64_t seed = 11;
  for (int round = 0; round < 400; round++) one_record(&seed, round);
  snappy_bodies(&seed);
  refusals();
  CHECK(g_streams > 100 && g_rle_inside > 20);  // the seeded records do hold stretches
  std::printf("asan parquet write ok\n");
  return 0;
}
