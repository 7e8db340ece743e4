// ASan harness for the host side of fdb_batch_from_parquet (see asan_parquet_shim.cpp): the stub of the dictionary-decode launcher
#include <hip/hip_runtime_api.h>
#include "fdb_kernels.h"
hipError_t fdb_launch_pq_decode_dict8(const uint8_t*, const uint32_t*, const uint32_t*, const FdbPqPlainPage*, int32_t, const FdbPqRun*, int32_t, uint64_t, uint32_t, int64_t, int64_t,
                                      unsigned long long*, uint32_t*, hipStream_t) { return hipErrorNotSupported; }
