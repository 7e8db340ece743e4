// fdb_take.h — Take, Limit and the reservoir Sampler over records resident in HBM (fdb_take.cpp; kernels in fdb_take.hip).
#pragma once

#include <memory>
#include <string>
#include <vector>

#include "fdb_context.h"
#include "fdb_plan.h"
#include "fdb_record.h"
#include "fdb_reservoir.h"

namespace fdb {

// ≙ arrowutils.Take(ctx, r, indices) as limit.go:88 uses it: row indices[i] of `in` becomes row i of a new resident record with the
// same fields, types and dictionaries, whose lifetime does not depend on `in`'s. Any order, duplicates allowed; n == 0 gives a
// zero-row record of the schema. An index outside [0, rows) is FDB_ERR_INVALID before anything is launched.
std::unique_ptr<DeviceBatch> take_batch(const DeviceBatch& in, const int32_t* indices, int64_t n);
// The launch half of take_batch, for row numbers that are already on the device (the permutation of a Sort): d_rows[i] < in.rows for
// every i < n — the CALLER vouches for that, nothing is checked here —, n > 0, every column of `in` has its values. One launch on the
// scope's stream, one wait.
std::unique_ptr<DeviceBatch> take_device_rows(const DeviceBatch& in, CallScope* cs, const uint32_t* d_rows, int64_t n);

// ≙ Limiter.Callback (limit.go:63-98), its quirk included: `count` applies to EVERY record and is never decremented, so the call has no
// state. rows ≤ count: the whole record, copied device to device; count == 0: zero rows; else the first `count` rows.
std::unique_ptr<DeviceBatch> limit_batch(const DeviceBatch& in, uint64_t count);

// ≙ ReservoirSampler (sampler.go). The handle holds a K-slot reservoir record in HBM and nothing else: every row that enters is copied
// into its slot at once, no input record is referenced after push returns — so the reference's sizeLimit / materialize
// (sampler.go:228-289), which bound the bytes such references pin, have nothing to bound here. Single-threaded, like a plan.
class Sampler {
 public:
  Sampler(int64_t size, uint64_t seed, int device);
  ~Sampler();
  Sampler(const Sampler&) = delete;
  Sampler& operator=(const Sampler&) = delete;
  void push_batch(const DeviceBatch& b);
  void push(const ArrowArray* array, const ArrowSchema* schema);  // the record is staged, its buffers only borrowed
  // The reservoir as ONE record in materialize's form: the fields of the records whose rows are in it, sorted by name; a row whose
  // record lacked a field is NULL there; rows in slot order. Nothing kept: no columns, no rows.
  std::unique_ptr<DeviceBatch> finish_batch(int64_t* n_rows);
  void finish(ArrowArray* out, ArrowSchema* out_schema, int64_t* n_rows);
  int64_t size() const { return select_.size(); }

 private:
  struct Field {
    std::string name, format;
    ColKind kind = ColKind::OTHER;
    void* block = nullptr;       // [values of `cap_` slots | a validity byte per slot]
    uint8_t* valid = nullptr;
    DictUnion dict;              // kind DICT
  };
  void ensure_context();
  void grow(int64_t slots);      // room for `slots` slots in every field
  void alloc_field(Field* f, int64_t cap);  // every slot NULL
  int field_of(const DevColumn& c);  // the field of this name (type checked), or -1
  size_t width(const Field& f) const { return value_width(f.kind); }

  int device_;
  ReservoirSelect select_;
  Context* ctx_ = nullptr;
  hipStream_t stream_ = nullptr;
  int64_t cap_ = 0;              // slots allocated per field (grows up to size)
  std::vector<Field> fields_;    // in first-seen order
  std::vector<std::vector<int>> schemas_;  // distinct field sets of the records that contributed rows
  std::vector<int32_t> slot_schema_;       // per slot in use: the field set of the record its row came from
  std::vector<uint8_t> stamp_;
};

}  // namespace fdb
