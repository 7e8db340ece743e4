"""ctypes binding of the C ABI (include/frostdb_amd.h), shaped like the reference's push operators.

``HashAggregatePlan`` stands where one chain ``PredicateFilter → HashAggregate(final=false)`` stands in
``physicalplan.Build`` (query/physicalplan/physicalplan.go:417-474) and offers the same five verbs as
``PhysicalPlan`` (physicalplan.go:24-30): ``Callback(record)``, ``Finish()``, ``SetNext(next)``, ``Draw()``,
``Close()``. pyarrow plays the role arrow-go's ``cdata`` package plays in the Go shim.

There is NO CPU fallback: if ``libfrostdb_amd.so`` is missing, or the HIP runtime reports an error, calls raise.
"""
from __future__ import annotations

import ctypes
import os
import threading
from typing import Any, Callable, List, Optional, Sequence

import pyarrow as pa

from .arrow_c import ArrowArray, ArrowSchema, ExportedBatch, import_batch
from .logicalplan import AggregationFunction, Column, Expr, expr_name, to_desc

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libfrostdb_amd.so")

FDB_OK, FDB_ERR_INVALID, FDB_ERR_UNSUPPORTED, FDB_ERR_NOT_FOUND, FDB_ERR_DEVICE, FDB_ERR_OOM, FDB_ERR_STATE = range(7)


class FdbError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"frostdb_amd error {code}: {msg}")
        self.code = code
        self.msg = msg


class UnsupportedError(FdbError):
    """≙ ErrUnsupportedBooleanExpression / ErrUnsupportedBinaryOperation / ErrUnsupportedSumType."""


_lib: Optional[ctypes.CDLL] = None


def lib() -> ctypes.CDLL:
    """Loads libfrostdb_amd.so (built in-tree by frostdb_amd.build / __graft_entry__.build). Fails loudly."""
    global _lib
    if _lib is not None:
        return _lib
    path = os.environ.get("FDB_LIB_PATH") or LIB_PATH  # (FDB_LIB_PATH: an instrumented build of the same library — tools/asan_gpu.sh)
    if not os.path.exists(path):
        raise ImportError(f"{path} is missing: run `python -m frostdb_amd.build` (hipcc, gfx950). There is no CPU fallback.")
    L = ctypes.CDLL(path)
    vp, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    P = ctypes.POINTER
    L.fdb_version.restype = ctypes.c_char_p
    L.fdb_last_error.restype = ctypes.c_char_p
    L.fdb_device_count.argtypes = [P(ctypes.c_int)]
    L.fdb_plan_create.argtypes = [vp, ctypes.c_int, P(vp)]
    L.fdb_plan_push.argtypes = [vp, vp, vp]
    L.fdb_plan_push_batch.argtypes = [vp, vp]
    L.fdb_plan_push_batches.argtypes = [vp, P(vp), i32]
    L.fdb_plan_finish.argtypes = [vp, vp, vp, P(i64)]
    L.fdb_plan_finish_next.argtypes = [vp, vp, vp, P(i64), P(i32)]
    L.fdb_plan_merge.argtypes = [vp, vp]
    L.fdb_plan_filter.argtypes = [vp, vp, vp, vp, vp, P(i64)]
    L.fdb_plan_select.argtypes = [vp, vp, vp, vp, i64, P(i64)]
    L.fdb_plan_draw.restype = ctypes.c_char_p
    L.fdb_plan_draw.argtypes = [vp]
    L.fdb_plan_last_error.restype = ctypes.c_char_p
    L.fdb_plan_last_error.argtypes = [vp]
    L.fdb_plan_close.argtypes = [vp]
    L.fdb_plan_close.restype = None
    L.fdb_plan_num_groups.argtypes = [vp, P(i64)]
    L.fdb_plan_partial_keys.argtypes = [vp, vp, vp]
    L.fdb_plan_partial_state.argtypes = [vp, i32, vp, i64]
    L.fdb_plan_agg_type.argtypes = [vp, i32, ctypes.c_char_p]
    L.fdb_plan_state_signature.argtypes = [vp, P(ctypes.c_uint64), P(i64)]
    L.fdb_plan_state_pointers.argtypes = [vp, P(vp), P(i64), P(i64)]
    L.fdb_plan_state_read.argtypes = [vp, i32, vp, i64]
    L.fdb_plan_state_write.argtypes = [vp, i32, vp, i64]
    L.fdb_batch_import.argtypes = [vp, vp, ctypes.c_int, P(vp)]
    L.fdb_batch_num_rows.restype = i64
    L.fdb_batch_num_rows.argtypes = [vp]
    L.fdb_batch_device_bytes.restype = i64
    L.fdb_batch_device_bytes.argtypes = [vp]
    L.fdb_batch_scan_cache_bytes.restype = i64
    L.fdb_batch_scan_cache_bytes.argtypes = [vp]
    L.fdb_batch_release.argtypes = [vp]
    L.fdb_batch_release.restype = None
    L.fdb_plan_stats.argtypes = [vp, P(i64), P(ctypes.c_double), P(i64), P(i64)]
    L.fdb_regex_match.argtypes = [ctypes.c_char_p, i64, ctypes.c_char_p, i64, P(i32)]
    L.fdb_parquet_stats.argtypes = [P(i64), P(ctypes.c_double), P(ctypes.c_double), P(i64), P(i64)]
    L.fdb_jit_stats.argtypes = [P(i64), P(ctypes.c_double), P(i64)]
    L.fdb_plan_merge_ms.argtypes = [vp, P(ctypes.c_double)]
    L.fdb_plan_set_timing.argtypes = [vp, i32]
    L.fdb_plan_stream.argtypes = [vp, P(vp)]
    L.fdb_plan_set_tuning.argtypes = [vp, i32, i32]
    L.fdb_plan_set_deterministic.argtypes = [vp, i32]
    L.fdb_plan_set_exact_sums.argtypes = [vp, i32]
    L.fdb_selftest_exact_sum.argtypes = [vp, i64, vp]
    L.fdb_snappy_decode_pages.argtypes = [vp, i64, vp, i32, vp, i64, ctypes.c_int, vp, P(ctypes.c_double)]
    L.fdb_lz4_decode_pages.argtypes = [vp, i64, vp, i32, vp, i64, ctypes.c_int, vp, P(ctypes.c_double)]
    L.fdb_parquet_device_pages.argtypes = [ctypes.c_int, P(i64), P(i64)]
    L.fdb_plan_state_arrays.argtypes = [vp, P(i32)]
    L.fdb_plan_state_array_op.argtypes = [vp, i32, P(i32)]
    L.fdb_plan_group_schema.argtypes = [vp, vp, vp]
    L.fdb_plan_seed_groups.argtypes = [vp, vp, vp]
    L.fdb_plan_hash_export.argtypes = [vp, vp, i32, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(i32)]
    L.fdb_plan_hash_import.argtypes = [vp, vp, ctypes.c_int64]
    L.fdb_read_ceiling.argtypes = [ctypes.c_int, ctypes.c_int64, i32, ctypes.POINTER(ctypes.c_double)]
    L.fdb_plan_last_kernel.argtypes = [vp]
    L.fdb_arrow_roundtrip.argtypes = [vp, vp, vp, vp]
    L.fdb_selftest_widen.argtypes = [vp, i32, vp, i64]
    L.fdb_selftest_scan_cache.argtypes = [vp, i64, i32, ctypes.c_int, vp, i64]
    L.fdb_selftest_scan_cache_nulls.argtypes = [vp, vp, i64, i64, i32, ctypes.c_int, vp, i64]
    L.fdb_selftest_scan_cache_packed.argtypes = [vp, vp, i64, i64, i32, ctypes.c_int, vp, i64]
    L.fdb_selftest_prefix_sums.argtypes = [i32, ctypes.c_int, vp, i64, i32, vp, i32, vp, vp]
    L.fdb_plan_explain.argtypes = [vp, ctypes.c_char_p, i64, P(i64)]
    L.fdb_plan_last_kernel.restype = ctypes.c_char_p
    L.fdb_comm_unique_id.argtypes = [vp]
    L.fdb_comm_init_rank.argtypes = [vp, i32, i32, ctypes.c_int, P(vp)]
    L.fdb_comm_init_all.argtypes = [P(ctypes.c_int), i32, P(vp)]
    L.fdb_comm_init_local.argtypes = [P(ctypes.c_int), i32, P(vp)]
    L.fdb_comm_rank.argtypes = [vp]
    L.fdb_comm_rank.restype = i32
    L.fdb_comm_size.argtypes = [vp]
    L.fdb_comm_size.restype = i32
    L.fdb_plan_push_many.argtypes = [vp, vp, vp, i32, P(i32)]
    L.fdb_plan_push_many.restype = i32
    L.fdb_comm_transport_ranks.argtypes = [vp]
    L.fdb_comm_transport_ranks.restype = i32
    L.fdb_comm_last_error.argtypes = [vp]
    L.fdb_comm_last_error.restype = ctypes.c_char_p
    L.fdb_comm_destroy.argtypes = [vp]
    L.fdb_comm_destroy.restype = None
    L.fdb_plan_allreduce.argtypes = [vp, vp, P(i32)]
    L.fdb_plan_exchange.argtypes = [vp, vp, P(vp)]
    L.fdb_live_allocations.argtypes = [P(i64), P(i64), P(i64)]
    L.fdb_plan_filter_batch.argtypes = [vp, vp, P(vp), P(i64)]
    L.fdb_plan_finish_batch.argtypes = [vp, P(vp), P(i64)]
    L.fdb_plan_filter_batches.argtypes = [vp, P(vp), i32, P(vp), P(i64)]
    L.fdb_plan_select_batch.argtypes = [vp, vp, vp, i64, P(i64)]
    L.fdb_batch_export.argtypes = [vp, vp, vp]
    L.fdb_plan_project_batch.argtypes = [vp, vp, i32, vp, P(vp)]
    L.fdb_plan_project_batches.argtypes = [vp, vp, i32, P(vp), i32, P(vp)]
    L.fdb_plan_project.argtypes = [vp, vp, i32, vp, vp, vp, vp]
    L.fdb_batch_from_parquet.argtypes = [vp, i32, i64, ctypes.c_int, P(vp)]
    L.fdb_batches_from_parquet.argtypes = [vp, i32, ctypes.c_int, P(vp)]
    L.fdb_batch_take.argtypes = [vp, vp, i64, P(vp)]
    L.fdb_batch_limit.argtypes = [vp, ctypes.c_uint64, P(vp)]
    L.fdb_sampler_create.argtypes = [i64, ctypes.c_uint64, ctypes.c_int, P(vp)]
    L.fdb_sampler_push_batch.argtypes = [vp, vp]
    L.fdb_sampler_push.argtypes = [vp, vp, vp]
    L.fdb_sampler_finish_batch.argtypes = [vp, P(vp), P(i64)]
    L.fdb_sampler_finish.argtypes = [vp, vp, vp, P(i64)]
    L.fdb_sampler_close.argtypes = [vp]
    L.fdb_sampler_close.restype = None
    L.fdb_selftest_reservoir.argtypes = [ctypes.c_uint64, i64, vp, i32, vp]
    L.fdb_batch_sort_indices.argtypes = [vp, vp, i32, vp]
    L.fdb_batch_sort.argtypes = [vp, vp, i32, P(vp)]
    L.fdb_selftest_sort_key.argtypes = [i32, ctypes.c_uint32, ctypes.c_uint64, P(ctypes.c_uint64)]
    L.fdb_sort_bench.argtypes = [vp, vp, i32, i32, i32, P(ctypes.c_double), P(ctypes.c_double), P(i32)]
    L.fdb_batches_merge.argtypes = [P(vp), i32, vp, i32, ctypes.c_uint64, P(vp)]
    L.fdb_batches_merge_named.argtypes = [P(vp), i32, vp, i32, ctypes.c_uint64, P(vp)]
    L.fdb_selftest_merge_schema.argtypes = [P(ctypes.c_char_p), P(i32), P(i32), i32, vp, i32, P(i32), P(i32), i32, P(i32), P(i32)]
    L.fdb_osync_create.argtypes = [i32, vp, i32, P(vp)]
    L.fdb_osync_push.argtypes = [vp, i32, vp, P(vp)]
    L.fdb_osync_finish.argtypes = [vp, i32, P(vp), P(i32)]
    L.fdb_osync_close.argtypes = [vp]
    L.fdb_osync_close.restype = None
    L.fdb_merge_tile_rows.argtypes = [i32]
    L.fdb_merge_tile_rows.restype = i32
    L.fdb_selftest_merge_path.argtypes = [vp, i64, vp, i64, i32, vp]
    L.fdb_merge_bench.argtypes = [P(vp), i32, vp, i32, i32, i32, P(ctypes.c_double), P(ctypes.c_double), P(ctypes.c_double), i32, P(i32), P(i32)]
    L.fdb_batch_column_name.argtypes = [vp, i32]
    L.fdb_batch_column_name.restype = ctypes.c_char_p
    L.fdb_batch_column_format.argtypes = [vp, i32]
    L.fdb_batch_column_format.restype = ctypes.c_char_p
    for suffix, takes in PARQUET_WRITE_ENTRIES + [PARQUET_WRITE_STRINGS]:
        optional_args = [vp, i32, vp, i32, vp, vp, vp, vp, vp][:takes + min(takes, 2)]  # (encodings and codecs: an array and its length)
        getattr(L, "fdb_batch_to_parquet" + suffix).argtypes = [vp, vp] + optional_args + [P(vp), P(i64)]
        getattr(L, "fdb_selftest_parquet_write" + suffix).argtypes = [vp, vp, vp] + optional_args + [P(vp), P(i64)]
    L.fdb_bytes_free.argtypes = [vp]
    L.fdb_bytes_free.restype = None
    _lib = L
    return L


def jit_stats() -> dict:
    """Kernels compiled with hiprtc by this process, the wall time of those compilations, code objects loaded from the disk cache."""
    n, ms, d = ctypes.c_int64(), ctypes.c_double(), ctypes.c_int64()
    lib().fdb_jit_stats(ctypes.byref(n), ctypes.byref(ms), ctypes.byref(d))
    return {"compiled": n.value, "compile_ms": ms.value, "disk_loads": d.value}


def regex_match(pattern, value: bytes) -> bool:
    """The library's built-in RE2-syntax engine (fdb_regex_match): unanchored match like Go's regexp.Regexp.Match. Raises FdbError
    (FDB_ERR_INVALID) for a pattern that does not compile."""
    pat = pattern.encode() if isinstance(pattern, str) else bytes(pattern)
    m = ctypes.c_int32()
    rc = lib().fdb_regex_match(pat, len(pat), value, len(value), ctypes.byref(m))
    if rc != 0:
        _raise(rc, lib().fdb_last_error().decode("utf-8", "replace"))
    return bool(m.value)


def parquet_stats() -> dict:
    """fdb_batch_from_parquet accumulated over the process: calls, host-part and device-part wall ms, bytes in and out."""
    c, h, d, fb, ob = ctypes.c_int64(), ctypes.c_double(), ctypes.c_double(), ctypes.c_int64(), ctypes.c_int64()
    lib().fdb_parquet_stats(ctypes.byref(c), ctypes.byref(h), ctypes.byref(d), ctypes.byref(fb), ctypes.byref(ob))
    return {"calls": c.value, "host_ms": h.value, "device_ms": d.value, "file_bytes": fb.value, "out_bytes": ob.value}


def parquet_device_pages(codec) -> dict:
    """Pages of one compression codec (a CompressionCodec number or name: "SNAPPY", "LZ4_RAW") that fdb_batch_from_parquet had the
    device inflate, accumulated over the process, and their uncompressed bytes."""
    codec = PARQUET_CODECS[codec.upper()] if isinstance(codec, str) else int(codec)
    n, b = ctypes.c_int64(), ctypes.c_int64()
    rc = lib().fdb_parquet_device_pages(codec, ctypes.byref(n), ctypes.byref(b))
    if rc != 0:
        _raise(rc, lib().fdb_last_error().decode("utf-8", "replace"))
    return {"pages": n.value, "bytes": b.value}


def read_ceiling(device: int = 0, nbytes: int = 1 << 31, reps: int = 5) -> float:
    """Best GB/s of a load-only streaming kernel over `nbytes` of HBM on this box (measurement aid)."""
    out = ctypes.c_double(0.0)
    rc = lib().fdb_read_ceiling(device, ctypes.c_int64(nbytes), reps, ctypes.byref(out))
    if rc != 0:
        raise FdbError(rc, lib().fdb_last_error().decode("utf-8", "replace"))
    return out.value


def explain(filter_expr: Optional[Expr], aggs: Sequence[AggregationFunction] = (), groups: Sequence[Column] = (), final_stage: bool = False,
            ordered: bool = False) -> str:
    """≙ Draw() of the operators this descriptor builds (`PredicateFilter (…) - HashAggregate (… by …)`), no device needed."""
    desc = to_desc(filter_expr, list(aggs), list(groups), final_stage, ordered=ordered)
    buf = ctypes.create_string_buffer(4096)
    need = ctypes.c_int64()
    rc = lib().fdb_plan_explain(ctypes.addressof(desc.desc), buf, len(buf), ctypes.byref(need))
    if rc != 0:
        _raise(rc, lib().fdb_last_error().decode("utf-8", "replace"))
    return buf.value.decode()


def arrow_roundtrip(record: pa.RecordBatch) -> pa.RecordBatch:
    """Host-only self-check (fdb_arrow_roundtrip): the record through the library's Arrow import and export code, no device."""
    arr, sch = ArrowArray(), ArrowSchema()
    with ExportedBatch(record) as ex:
        rc = lib().fdb_arrow_roundtrip(ctypes.addressof(ex.array), ctypes.addressof(ex.schema), ctypes.addressof(arr), ctypes.addressof(sch))
    if rc != 0:
        _raise(rc, lib().fdb_last_error().decode("utf-8", "replace"))
    return import_batch(arr, sch)


def selftest_exact_sum(values) -> float:
    """The correctly rounded exact sum of `values` (float64), computed on the host by the code the exact-sum kernels run
    (fdb_selftest_exact_sum; no device)."""
    xs = [float(v) for v in values]
    x = (ctypes.c_double * max(1, len(xs)))(*xs)
    out = ctypes.c_double()
    rc = lib().fdb_selftest_exact_sum(x, len(xs), ctypes.byref(out))
    if rc != FDB_OK:
        _raise(rc, lib().fdb_last_error().decode("utf-8", "replace"))
    return out.value


PREFIX_EXCLUSIVE_SCAN, PREFIX_FILTER_SCAN, PREFIX_STRIDED_SCAN = 0, 1, 2


def selftest_prefix_sums(kind: int, counts, option: int = 0, recs=None, device: int = 0):
    """One of the library's device prefix sums over `counts` (uint32), run as the library runs it (fdb_selftest_prefix_sums).
    PREFIX_EXCLUSIVE_SCAN: `option` 1 withholds the block-sum scratch; PREFIX_FILTER_SCAN: `recs` is the record table, (first tile,
    rows) per record, `option` 0 / 1 / 2 = levels as filter() chooses / one / two; PREFIX_STRIDED_SCAN: `option` is the stride and
    `counts` holds n x stride words. Returns (uint32 prefix array, uint64 totals: [sum], or rec_base[n_recs + 1] for the filter scan)."""
    import numpy as np
    a = np.ascontiguousarray(counts, dtype=np.uint32)
    n = len(a) // int(option) if kind == PREFIX_STRIDED_SCAN and int(option) >= 1 else len(a)
    table = np.ascontiguousarray(recs, dtype=np.int64).reshape(-1, 2) if recs is not None else None
    out = np.empty(max(n, 1), dtype=np.uint32)
    totals = np.empty(len(table) + 1 if table is not None else 1, dtype=np.uint64)
    rc = lib().fdb_selftest_prefix_sums(int(kind), int(device), a.ctypes.data if len(a) else None, n, int(option),
                                        table.ctypes.data if table is not None and len(table) else None, len(table) if table is not None else 0,
                                        out.ctypes.data, totals.ctypes.data)
    if rc != FDB_OK:
        _raise(rc, lib().fdb_last_error().decode("utf-8", "replace"))
    return out[:n], totals


def selftest_reservoir(seed: int, size: int, record_rows: Sequence[int]) -> List[int]:
    """The rows a ``ReservoirSampler(size, seed)`` ends with after records of `record_rows` rows were pushed in turn, by slot, numbered
    across the records in push order (fdb_selftest_reservoir: the library's own selection code on the host, no device)."""
    lens = [int(n) for n in record_rows]
    rows = (ctypes.c_int64 * max(1, len(lens)))(*lens)
    kept = min(int(size), sum(lens)) if size > 0 else 0
    out = (ctypes.c_int64 * max(1, kept))()
    rc = lib().fdb_selftest_reservoir(int(seed) & 0xFFFFFFFFFFFFFFFF, int(size), rows, len(lens), out)
    if rc != FDB_OK:
        _raise(rc, lib().fdb_last_error().decode("utf-8", "replace"))
    return [out[i] for i in range(kept)]


SORT_KIND_INT64, SORT_KIND_UINT64, SORT_KIND_FLOAT64 = 1, 2, 3


def selftest_sort_key(kind: int, descending: bool, raw: int) -> int:
    """The 64-bit radix-key value field the device Sort gives one non-NULL int64 / uint64 / float64 value (`raw` = its bits), in the
    given direction (fdb_selftest_sort_key: the encoding the key kernel runs, on the host, no device)."""
    out = ctypes.c_uint64()
    rc = lib().fdb_selftest_sort_key(int(kind), 1 if descending else 0, int(raw) & 0xFFFFFFFFFFFFFFFF, ctypes.byref(out))
    if rc != FDB_OK:
        _raise(rc, lib().fdb_last_error().decode("utf-8", "replace"))
    return out.value


def merge_tile_rows(words: int) -> int:
    """The output tile (rows) of the device merge kernel for a key of `words` 64-bit words (fdb_merge_tile_rows)."""
    return int(lib().fdb_merge_tile_rows(int(words)))


def selftest_merge_path(a, b, words: int):
    """The device merge's merge-path code run on the host (fdb_selftest_merge_path; no device): `a` and `b` are sorted runs of keys of
    `words` unsigned 64-bit words each (sequences of `words`-tuples, or arrays of shape (n, words)). Returns, per output row, its
    source: i for a[i], len(a) + j for b[j]. Ties go to `a`."""
    import numpy as np
    ka = np.ascontiguousarray(np.asarray(a, dtype=np.uint64).reshape(-1, int(words)))
    kb = np.ascontiguousarray(np.asarray(b, dtype=np.uint64).reshape(-1, int(words)))
    out = np.empty(max(1, len(ka) + len(kb)), dtype=np.uint32)
    rc = lib().fdb_selftest_merge_path(ka.ctypes.data if len(ka) else None, len(ka), kb.ctypes.data if len(kb) else None, len(kb), int(words), out.ctypes.data)
    if rc != FDB_OK:
        _raise(rc, lib().fdb_last_error().decode("utf-8", "replace"))
    return out[: len(ka) + len(kb)]


def selftest_merge_schema(records, order_by):
    """The schema union and column map of ``ResidentBatch.merge_named`` run on the host (fdb_selftest_merge_schema; no device).
    `records`: per record a list of ``(field name, column kind)``; `order_by` as for ``merge_named``. Returns ``(columns, n_sort, col_map)``:
    per output column the ``(record, field)`` where it is first seen, how many leading columns are sorting columns, and per record the
    position of every output column inside it (-1: the record lacks it). What the schema rules refuse raises FdbError."""
    records = [list(r) for r in records]
    flat = [(r, f, name, kind) for r, rec in enumerate(records) for f, (name, kind) in enumerate(rec)]
    names = (ctypes.c_char_p * max(1, len(flat)))(*[x[2].encode("utf-8") for x in flat])
    kinds = (ctypes.c_int32 * max(1, len(flat)))(*[int(x[3]) for x in flat])
    counts = (ctypes.c_int32 * max(1, len(records)))(*[len(r) for r in records])
    arr, n, _keep = _order_cols(order_by)
    cap = max(1, len(flat))
    out_fields = (ctypes.c_int32 * cap)()
    col_map = (ctypes.c_int32 * (cap * max(1, len(records))))()
    n_out, n_sort = ctypes.c_int32(), ctypes.c_int32()
    rc = lib().fdb_selftest_merge_schema(names, kinds, counts, len(records), arr, n, out_fields, col_map, cap, ctypes.byref(n_out), ctypes.byref(n_sort))
    if rc != 0:
        _raise(rc, lib().fdb_last_error().decode("utf-8", "replace"))
    columns = [flat[out_fields[i]][:2] for i in range(n_out.value)]
    return columns, n_sort.value, [[col_map[r * n_out.value + i] for i in range(n_out.value)] for r in range(len(records))]


class ParquetWriteOptions(ctypes.Structure):
    """fdb_parquet_write_options."""
    _fields_ = [("page_rows", ctypes.c_int32), ("n_optional", ctypes.c_int32), ("optional", ctypes.c_void_p)]


def _parquet_write_options(page_rows, optional, names):
    """`optional`: None (every column auto), a sequence with one entry per column or a dict by column name; an entry is None / -1
    (auto), False / 0 (required) or True / 1 (optional). Returns the struct and what it points at."""
    if optional is None:
        flags = []
    elif isinstance(optional, dict):
        unknown = [n for n in optional if n not in names]
        if unknown:
            _raise(FDB_ERR_INVALID, "parquet write: `optional` names no column of the record: %s" % unknown[0])
        flags = [optional.get(n) for n in names]
    else:
        flags = list(optional)
        if not flags and names:  # (an empty array would read as "every column auto" on the C side)
            _raise(FDB_ERR_INVALID, "parquet write: `optional` has 0 entries, the record %d columns" % len(names))
    arr = (ctypes.c_int8 * max(1, len(flags)))(*[-1 if f is None else int(f) for f in flags])
    return ParquetWriteOptions(int(page_rows), len(flags), ctypes.cast(arr, ctypes.c_void_p) if flags else None), arr


PARQUET_ENCODINGS = {None: 0, "plain": 0, "delta": 1}


def _parquet_encodings(encodings, names):
    """`encodings`: a sequence with one entry per column or a dict by column name; an entry is None / "plain" (as the column is
    written without it) or "delta" (DELTA_BINARY_PACKED; int64 / uint64 columns). Returns the int8 array and its length."""
    if isinstance(encodings, dict):
        unknown = [n for n in encodings if n not in names]
        if unknown:
            _raise(FDB_ERR_INVALID, "parquet write: `encodings` names no column of the record: %s" % unknown[0])
        wanted = [encodings.get(n) for n in names]
    else:
        wanted = list(encodings)
        if not wanted and names:  # (an empty array would read as "every column as ever" on the C side)
            _raise(FDB_ERR_INVALID, "parquet write: `encodings` has 0 entries, the record %d columns" % len(names))
    for e in wanted:
        if not (e is None or isinstance(e, str)) or e not in PARQUET_ENCODINGS:
            _raise(FDB_ERR_INVALID, "parquet write: unknown encoding %r (None, 'plain' or 'delta')" % (e,))
    return (ctypes.c_int8 * max(1, len(wanted)))(*[PARQUET_ENCODINGS[e] for e in wanted]), len(wanted)


PARQUET_WRITE_CODECS = {None: 0, "uncompressed": 0, "snappy": 1, "lz4": 7}  # "lz4": parquet's LZ4_RAW, the bare block


def _parquet_codecs(compression, names):
    """`compression`: "snappy" or "lz4" (every column), a sequence with one entry per column or a dict by column name; an entry is
    None / "uncompressed", "snappy" or "lz4" (LZ4_RAW). Returns the int8 array and its length."""
    if isinstance(compression, str):
        wanted = [compression] * len(names)
    elif isinstance(compression, dict):
        unknown = [n for n in compression if n not in names]
        if unknown:
            _raise(FDB_ERR_INVALID, "parquet write: `compression` names no column of the record: %s" % unknown[0])
        wanted = [compression.get(n) for n in names]
    else:
        wanted = list(compression)
        if not wanted and names:  # (an empty array would read as "every column uncompressed" on the C side)
            _raise(FDB_ERR_INVALID, "parquet write: `codecs` has 0 entries, the record %d columns" % len(names))
    for e in wanted:
        if not (e is None or isinstance(e, str)) or e not in PARQUET_WRITE_CODECS:
            _raise(FDB_ERR_INVALID, "parquet write: unknown codec %r (None, 'uncompressed', 'snappy' or 'lz4')" % (e,))
    return (ctypes.c_int8 * max(1, len(wanted)))(*[PARQUET_WRITE_CODECS[e] for e in wanted]), len(wanted)


class ParquetSortingColumn(ctypes.Structure):
    """fdb_parquet_sorting_column."""
    _fields_ = [("column", ctypes.c_int32), ("descending", ctypes.c_int8), ("nulls_first", ctypes.c_int8), ("pad", ctypes.c_int8 * 2)]


class ParquetIndexOptions(ctypes.Structure):
    """fdb_parquet_index_options."""
    _fields_ = [("statistics", ctypes.c_int32), ("index_size_limit", ctypes.c_int32), ("sorting_columns", ctypes.c_void_p), ("n_sorting_columns", ctypes.c_int32)]


PARQUET_STATISTICS = {None: 0, "chunk": 1, "page": 2}


def _parquet_index_options(statistics, index_size_limit, sorting_columns, names):
    """`statistics`: None, "chunk" (Statistics.min_value / max_value per chunk) or "page" (the same + ColumnIndex and OffsetIndex).
    `index_size_limit`: bytes a BYTE_ARRAY bound of the ColumnIndex is cut to (0 = 16). `sorting_columns`: a sequence of
    (name or index, descending=False, nulls_first=False), written as RowGroup.sorting_columns. Returns the struct and what it points
    at, or (None, None) when nothing is asked: the caller then calls what it called without these arguments."""
    if statistics is None and not index_size_limit and not sorting_columns:
        return None, None
    if not (statistics is None or isinstance(statistics, str)) or statistics not in PARQUET_STATISTICS:
        _raise(FDB_ERR_INVALID, "parquet write: unknown statistics %r (None, 'chunk' or 'page')" % (statistics,))
    if isinstance(index_size_limit, bool) or not isinstance(index_size_limit, int) or not -2**31 <= index_size_limit < 2**31:
        _raise(FDB_ERR_INVALID, "parquet write: index_size_limit is %r (0: 16, else 1 to 65536)" % (index_size_limit,))
    wanted = []
    for entry in (sorting_columns or ()):
        entry = tuple(entry) if isinstance(entry, (tuple, list)) else (entry,)
        if not 1 <= len(entry) <= 3:
            _raise(FDB_ERR_INVALID, "parquet write: a sorting column is (name or index, descending=False, nulls_first=False), got %r" % (entry,))
        col = entry[0]
        if isinstance(col, str):
            if col not in names:
                _raise(FDB_ERR_INVALID, "parquet write: `sorting_columns` names no column of the record: %s" % col)
            col = names.index(col)
        elif isinstance(col, bool) or not isinstance(col, int) or not -2**31 <= col < 2**31:
            _raise(FDB_ERR_INVALID, "parquet write: a sorting column is a name or an index, got %r" % (col,))
        wanted.append((col, 1 if len(entry) > 1 and entry[1] else 0, 1 if len(entry) > 2 and entry[2] else 0))
    arr = (ParquetSortingColumn * max(1, len(wanted)))()
    for i, (col, desc, first) in enumerate(wanted):
        arr[i].column, arr[i].descending, arr[i].nulls_first = col, desc, first
    return ParquetIndexOptions(PARQUET_STATISTICS[statistics], index_size_limit, ctypes.cast(arr, ctypes.c_void_p) if wanted else None, len(wanted)), arr


class ParquetBloomOptions(ctypes.Structure):
    """fdb_parquet_bloom_options."""
    _fields_ = [("columns", ctypes.c_void_p), ("n_columns", ctypes.c_int32), ("bits_per_value", ctypes.c_int32)]


def _parquet_bloom_options(bloom_filters, bits_per_value, names, is_bool, sorting_columns):
    """`bloom_filters`: None, a sequence of column names, a dict of name → bool, or "sorting": the `sorting_columns` that are not
    boolean (`is_bool`: per column), which is what the reference's Schema.NewWriter gives a filter — with no sorting column, none.
    `bits_per_value`: 0 (10) or 1 … 64. Returns the struct and what it points at, or (None, None) when nothing is asked: the caller
    then calls what it called without these arguments."""
    if bloom_filters is None and not bits_per_value:
        return None, None
    if isinstance(bits_per_value, bool) or not isinstance(bits_per_value, int) or not -2**31 <= bits_per_value < 2**31:
        _raise(FDB_ERR_INVALID, "parquet write: bloom filter bits_per_value is %r (0: 10, else 1 to 64)" % (bits_per_value,))
    wanted = [0] * len(names)
    if isinstance(bloom_filters, str):
        if bloom_filters != "sorting":
            _raise(FDB_ERR_INVALID, "parquet write: `bloom_filters` is a sequence of column names, a dict of name → bool or 'sorting', got %r" % (bloom_filters,))
        for entry in (sorting_columns or ()):
            col = entry[0] if isinstance(entry, (tuple, list)) else entry
            col = names.index(col) if isinstance(col, str) and col in names else col
            if isinstance(col, int) and not isinstance(col, bool) and 0 <= col < len(names) and not is_bool[col]:  # (anything else is the index options' to refuse)
                wanted[col] = 1
    else:
        chosen = [n for n, on in bloom_filters.items() if on] if isinstance(bloom_filters, dict) else list(bloom_filters or ())
        for n in (list(bloom_filters) if isinstance(bloom_filters, dict) else chosen):
            if not isinstance(n, str) or n not in names:
                _raise(FDB_ERR_INVALID, "parquet write: `bloom_filters` names no column of the record: %s" % (n,))
        for n in chosen:
            wanted[names.index(n)] = 1
    arr = (ctypes.c_int8 * max(1, len(wanted)))(*wanted)
    return ParquetBloomOptions(ctypes.cast(arr, ctypes.c_void_p) if wanted else None, len(wanted), bits_per_value), arr


class ParquetRunOptions(ctypes.Structure):
    """fdb_parquet_run_options."""
    _fields_ = [("columns", ctypes.c_void_p), ("n_columns", ctypes.c_int32), ("pad", ctypes.c_int32)]


PARQUET_RUN_STREAMS = {None: 0, False: 0, "values": 1, "levels": 2, True: 3}


def _parquet_run_options(runs, names, is_index, forms=None):
    """`runs`: None; True — every column, its definition levels and, of a dictionary / string / binary column (`is_index`: per
    column) that is not written with a string form (`forms`: per column, 0 = none), its indices; a sequence of column names (both streams of each); or a dict of name → True (both) / "values" (the
    dictionary indices) / "levels" (the definition levels) / None. Returns the struct and what it points at, or (None, None) when
    nothing is asked: the caller then calls what it called without this argument."""
    if runs is None or runs is False:
        return None, None
    if runs is True:
        wanted = [2 | (1 if ix and not (forms and forms[k]) else 0) for k, ix in enumerate(is_index)]
    elif isinstance(runs, str):
        _raise(FDB_ERR_INVALID, "parquet write: `runs` is True, a sequence of column names or a dict of name → True / 'values' / 'levels', got %r" % (runs,))
    else:
        wanted = [0] * len(names)
        for n in runs:
            if not isinstance(n, str) or n not in names:
                _raise(FDB_ERR_INVALID, "parquet write: `runs` names no column of the record: %s" % (n,))
            e = runs[n] if isinstance(runs, dict) else True
            if isinstance(e, (list, dict, set, tuple)) or e not in PARQUET_RUN_STREAMS or (not isinstance(e, (bool, str)) and e is not None):
                _raise(FDB_ERR_INVALID, "parquet write: unknown run streams %r (True, 'values', 'levels' or None)" % (e,))
            wanted[names.index(n)] = PARQUET_RUN_STREAMS[e]
    if not any(wanted):
        return None, None
    arr = (ctypes.c_int8 * max(1, len(wanted)))(*wanted)
    return ParquetRunOptions(ctypes.cast(arr, ctypes.c_void_p), len(wanted), 0), arr


class ParquetGroupOptions(ctypes.Structure):
    """fdb_parquet_group_options."""
    _fields_ = [("row_group_rows", ctypes.c_int64), ("dictionaries", ctypes.c_int32), ("pad", ctypes.c_int32)]


PARQUET_DICTIONARIES = {None: 0, "whole": 0, "used": 1}


def _parquet_group_options(row_group_rows, dictionaries):
    """`row_group_rows`: 0 (one row group) or the rows per row group, a multiple of 64; `dictionaries`: None / "whole" (every chunk
    carries the column's whole dictionary) or "used" (only the entries its non-NULL rows refer to). Returns the struct, or None when
    nothing is asked: the caller then calls what it called without these arguments."""
    if isinstance(dictionaries, (list, dict, set, tuple)) or dictionaries not in PARQUET_DICTIONARIES or isinstance(dictionaries, bool):
        _raise(FDB_ERR_INVALID, "parquet write: `dictionaries` is None, 'whole' or 'used', got %r" % (dictionaries,))
    if isinstance(row_group_rows, bool) or not isinstance(row_group_rows, int) or not -2**63 <= row_group_rows < 2**63:
        _raise(FDB_ERR_INVALID, "parquet write: row_group_rows must be a multiple of 64 (0: one row group), got %r" % (row_group_rows,))
    if row_group_rows == 0 and PARQUET_DICTIONARIES[dictionaries] == 0:
        return None
    return ParquetGroupOptions(row_group_rows, PARQUET_DICTIONARIES[dictionaries], 0)


class ParquetStringOptions(ctypes.Structure):
    """fdb_parquet_string_options."""
    _fields_ = [("forms", ctypes.c_void_p), ("n_columns", ctypes.c_int32), ("pad", ctypes.c_int32)]


PARQUET_STRING_FORMS = {None: 0, "dictionary": 0, "plain": 1, "delta_length": 2}


def _parquet_string_forms(strings, names, is_index, runs):
    """`strings`: None; "plain" or "delta_length" — every dictionary / string / binary column (`is_index`: per column) whose
    dictionary indices `runs` does not ask by name to be cut into runs; a sequence with one entry per column or a dict by column name
    of None / "dictionary" (a dictionary page and RLE_DICTIONARY pages, as without it), "plain" or "delta_length". Returns the form
    per column, or None when nothing is asked: the caller then calls what it called without this argument."""
    if strings is None:
        return None
    if isinstance(strings, str):
        if strings not in ("plain", "delta_length"):
            _raise(FDB_ERR_INVALID, "parquet write: `strings` is None, 'plain', 'delta_length', a sequence per column or a dict by name, got %r" % (strings,))
        indexed = set()   # the columns whose indices are asked for by name (anything else about `runs` is the run options' to refuse)
        if runs is not None and not isinstance(runs, (bool, str)):
            for n in runs:
                e = runs[n] if isinstance(runs, dict) else True
                if e is True or (isinstance(e, str) and e == "values"):
                    indexed.add(n)
        wanted = [strings if ix and n not in indexed else None for n, ix in zip(names, is_index)]
    elif isinstance(strings, dict):
        unknown = [n for n in strings if n not in names]
        if unknown:
            _raise(FDB_ERR_INVALID, "parquet write: `strings` names no column of the record: %s" % (unknown[0],))
        wanted = [strings.get(n) for n in names]
    else:
        wanted = list(strings)
        if len(wanted) != len(names):
            _raise(FDB_ERR_INVALID, "parquet write: `strings` has %d entries, the record %d columns" % (len(wanted), len(names)))
    for e in wanted:
        if not (e is None or isinstance(e, str)) or e not in PARQUET_STRING_FORMS:
            _raise(FDB_ERR_INVALID, "parquet write: unknown string form %r (None, 'dictionary', 'plain' or 'delta_length')" % (e,))
    forms = [PARQUET_STRING_FORMS[e] for e in wanted]
    return forms if any(forms) else None


def _take_bytes(rc, out, n) -> bytes:
    if rc != 0:
        _raise(rc, lib().fdb_last_error().decode("utf-8", "replace"))
    try:
        return ctypes.string_at(out.value, n.value)
    finally:
        lib().fdb_bytes_free(out.value)


# The writer's entry points, narrowest first: the suffix of the name, and how many of the optional arguments — encodings, codecs, index
# options, bloom options, run options, group options, in this order — it takes.
PARQUET_WRITE_ENTRIES = [("", 0), ("_encoded", 1), ("_compressed", 2), ("_indexed", 3), ("_filtered", 4), ("_runs", 5), ("_grouped", 6)]
PARQUET_WRITE_STRINGS = ("_strings", 7)  # … and the widest, which takes the string options behind them


def _parquet_write(entry, head, names, is_bool, is_index, asked) -> bytes:
    """`asked`, the options of ResidentBatch.to_parquet / selftest_parquet_write in their order, as the C structures, and the call
    through the NARROWEST of `entry`'s entry points that carries what was asked (`head`: its arguments in front of the options)."""
    page_rows, optional, encodings, compression, statistics, index_size_limit, sorting_columns, bloom_filters, bloom_bits_per_value, runs, row_group_rows, dictionaries, strings = asked
    opts, _keep = _parquet_write_options(page_rows, optional, names)
    enc, n_enc = _parquet_encodings(encodings, names) if encodings is not None else (None, 0)
    codecs, n_codecs = _parquet_codecs(compression, names) if compression is not None else (None, 0)
    index, _keep_index = _parquet_index_options(statistics, index_size_limit, sorting_columns, names)
    bloom, _keep_bloom = _parquet_bloom_options(bloom_filters, bloom_bits_per_value, names, is_bool, sorting_columns)
    forms = _parquet_string_forms(strings, names, is_index, runs)
    run_opts, _keep_runs = _parquet_run_options(runs, names, is_index, forms)
    group_opts = _parquet_group_options(row_group_rows, dictionaries)
    _keep_forms = (ctypes.c_int8 * max(1, len(names)))(*forms) if forms is not None else None
    string_opts = ParquetStringOptions(ctypes.cast(_keep_forms, ctypes.c_void_p), len(forms), 0) if forms is not None else None
    optional_args = [(ctypes.cast(enc, ctypes.c_void_p) if n_enc else None, n_enc), (ctypes.cast(codecs, ctypes.c_void_p) if n_codecs else None, n_codecs)]
    optional_args += [(ctypes.byref(struct) if struct is not None else None,) for struct in (index, bloom, run_opts, group_opts, string_opts)]
    is_asked = [encodings is not None, compression is not None, index is not None, bloom is not None, run_opts is not None, group_opts is not None, string_opts is not None]
    need = max([i + 1 for i, on in enumerate(is_asked) if on], default=0)
    suffix, takes = next(e for e in PARQUET_WRITE_ENTRIES + [PARQUET_WRITE_STRINGS] if e[1] >= need)
    out, n = ctypes.c_void_p(), ctypes.c_int64()
    rc = getattr(lib(), entry + suffix)(*head, ctypes.byref(opts), *[a for group in optional_args[:takes] for a in group], ctypes.byref(out), ctypes.byref(n))
    return _take_bytes(rc, out, n)


def selftest_parquet_write(record: pa.RecordBatch, page_rows: int = 0, optional=None, encodings=None, compression=None, statistics=None, index_size_limit: int = 0,
                           sorting_columns=None, bloom_filters=None, bloom_bits_per_value: int = 0, runs=None, row_group_rows: int = 0, dictionaries=None, strings=None) -> bytes:
    """The Parquet file ``ResidentBatch(record).to_parquet(page_rows, optional, encodings, compression, ...)`` writes, byte for byte,
    made without a device (fdb_selftest_parquet_write, with `encodings` fdb_selftest_parquet_write_encoded, with `compression`
    fdb_selftest_parquet_write_compressed — "snappy" by the host walk of fdb_pqsnappy.h, "lz4" by that of fdb_pqlz4.h —, with `statistics`, `index_size_limit` or `sorting_columns`
    fdb_selftest_parquet_write_indexed, with `bloom_filters` or `bloom_bits_per_value` fdb_selftest_parquet_write_filtered): the same
    layout, headers and footer, the kernels replaced by a host walk of the code they compile. With `runs`
    fdb_selftest_parquet_write_runs: the run passes walked as well; with `row_group_rows` or `dictionaries`
    fdb_selftest_parquet_write_grouped: the present and remap passes too; with `strings` fdb_selftest_parquet_write_strings: the
    byte survey and the byte encode pass, the by-position lookup included."""
    def is_index(t):
        t = t.value_type if pa.types.is_dictionary(t) else t
        return pa.types.is_string(t) or pa.types.is_large_string(t) or pa.types.is_binary(t) or pa.types.is_large_binary(t)
    asked = (page_rows, optional, encodings, compression, statistics, index_size_limit, sorting_columns, bloom_filters, bloom_bits_per_value, runs, row_group_rows, dictionaries, strings)
    with ExportedBatch(record) as ex:
        return _parquet_write("fdb_selftest_parquet_write", [ctypes.addressof(ex.array), ctypes.addressof(ex.schema)], list(record.schema.names),
                              [pa.types.is_boolean(f.type) for f in record.schema], [is_index(f.type) for f in record.schema], asked)


def live_allocations() -> dict:
    """Device blocks / bytes and pinned result blocks the library owns right now (0 once everything is closed and released)."""
    a, b, c = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
    lib().fdb_live_allocations(ctypes.byref(a), ctypes.byref(b), ctypes.byref(c))
    return {"device_blocks": a.value, "device_bytes": b.value, "pinned_blocks": c.value}


def local_cpus(device: int = 0):
    """The CPUs next to the GPU — sysfs ``local_cpulist`` of its PCI function, i.e. the cores of the NUMA node it hangs off — or None
    when that cannot be told. Threads that push HOST records (one per chain, like the reference's goroutines) belong there: on a
    two-socket MI355X box one chain moves 1.8 G rows/s of 65 536-row records from the GPU's socket and 1.36 from the other, eight chains on
    the other socket stop at half the link (profiles/round5_push_bench_numa_sdma.txt). ``pin_thread_near(device)`` applies it to the
    calling thread."""
    try:
        hip = ctypes.CDLL("libamdhip64.so")
        buf = ctypes.create_string_buffer(64)
        if hip.hipDeviceGetPCIBusId(buf, 64, int(device)) != 0:
            return None
        with open("/sys/bus/pci/devices/%s/local_cpulist" % buf.value.decode().lower()) as f:
            text = f.read().strip()
        cpus = set()
        for part in text.split(","):
            if "-" in part:
                a, b = part.split("-")
                cpus.update(range(int(a), int(b) + 1))
            elif part:
                cpus.add(int(part))
        return cpus or None
    except (OSError, ValueError, AttributeError):
        return None


def pin_thread_near(device: int = 0) -> bool:
    """Restricts the CALLING thread to ``local_cpus(device)`` (intersected with what it may run on). False: left as it was."""
    cpus = local_cpus(device)
    if not cpus:
        return False
    try:
        allowed = os.sched_getaffinity(0) & cpus
        if not allowed:
            return False
        os.sched_setaffinity(0, allowed)
        return True
    except (OSError, AttributeError):
        return False


def device_count() -> int:
    n = ctypes.c_int(0)
    lib().fdb_device_count(ctypes.byref(n))
    return n.value


def _raise(code: int, msg: str):
    raise (UnsupportedError if code == FDB_ERR_UNSUPPORTED else FdbError)(code, msg)


class SortCol(ctypes.Structure):
    """fdb_sort_col ≙ arrowutils.SortingColumn: column position, direction (0 ascending / 1 descending), nulls_first."""
    _fields_ = [("index", ctypes.c_int32), ("direction", ctypes.c_uint32), ("nulls_first", ctypes.c_uint32)]


class OrderCol(ctypes.Structure):
    """fdb_order_col: an order-by expression by name — ``dynamic`` != 0 matches every field called ``name.<something>`` — with the
    direction and NULL placement of every column it matches."""
    _fields_ = [("name", ctypes.c_char_p), ("dynamic", ctypes.c_int32), ("direction", ctypes.c_uint32), ("nulls_first", ctypes.c_uint32)]


def _order_cols(order_by):
    """`order_by` → (fdb_order_col array, count, what keeps its strings alive). An entry is ``Col(name)`` / ``DynCol(name)``, a bare name,
    ``(expr, descending=False, nulls_first=False)`` or a raw ``OrderCol``."""
    if isinstance(order_by, (str, Column, OrderCol)):
        order_by = [order_by]
    cols, keep = [], []
    for o in order_by:
        if isinstance(o, OrderCol):
            cols.append(o)
            continue
        o = (o,) if isinstance(o, (str, Column)) else tuple(o)
        if not 1 <= len(o) <= 3:
            raise ValueError("an order-by entry is (expr, descending=False, nulls_first=False)")
        expr = Column(o[0]) if isinstance(o[0], str) else o[0]
        if not isinstance(expr, Column):
            raise TypeError("an order-by expression is Col(name) or DynCol(name)")
        keep.append(expr.name.encode("utf-8"))
        cols.append(OrderCol(keep[-1], 1 if expr.dynamic else 0, 1 if len(o) > 1 and o[1] else 0, 1 if len(o) > 2 and o[2] else 0))
    return (OrderCol * max(1, len(cols)))(*cols), len(cols), (keep, cols)


class ParquetChunk(ctypes.Structure):
    """fdb_parquet_chunk: one column chunk of a row group, bytes as they sit in the file."""
    _fields_ = [("name", ctypes.c_char_p), ("physical_type", ctypes.c_int32), ("optional", ctypes.c_int32), ("utf8", ctypes.c_int32),
                ("codec", ctypes.c_int32), ("data", ctypes.c_void_p), ("n_bytes", ctypes.c_int64)]


PARQUET_INT64, PARQUET_DOUBLE, PARQUET_BYTE_ARRAY = 2, 5, 6
PARQUET_CODECS = {"UNCOMPRESSED": 0, "SNAPPY": 1, "GZIP": 2, "LZO": 3, "BROTLI": 4, "LZ4": 5, "ZSTD": 6, "LZ4_RAW": 7}  # parquet.thrift CompressionCodec


class ParquetRowGroup(ctypes.Structure):
    """fdb_parquet_row_group: the column chunks of one row group + its row count."""
    _fields_ = [("chunks", ctypes.c_void_p), ("n_chunks", ctypes.c_int32), ("n_rows", ctypes.c_int64)]


class ResidentBatch:
    """An Arrow record kept in HBM between queries (``fdb_batch``)."""

    @staticmethod
    def _parquet_chunks(chunks: Sequence[tuple]):
        arr = (ParquetChunk * len(chunks))()
        keep = []
        for i, (name, ptype, optional, utf8, data, *rest) in enumerate(chunks):
            codec = rest[0] if rest else 0
            codec = PARQUET_CODECS[codec.upper()] if isinstance(codec, str) else int(codec)
            if isinstance(data, tuple):      # (address, length): bytes that already sit somewhere stable, e.g. a pinned file buffer
                addr, size = data
            elif isinstance(data, bytes):    # no copy: the bytes object is kept alive for the call
                addr, size = ctypes.cast(ctypes.c_char_p(data), ctypes.c_void_p).value, len(data)
            else:
                data = bytes(data)
                addr, size = ctypes.cast(ctypes.c_char_p(data), ctypes.c_void_p).value, len(data)
            nm = name.encode()
            keep += [data, nm]
            arr[i] = ParquetChunk(nm, ptype, int(optional), 1 if utf8 else 0, codec, addr, size)  # optional: the column's max definition level (0 / 1; more = nested)
        return arr, keep

    @classmethod
    def from_parquet_many(cls, groups: Sequence[tuple], device: int = 0) -> list:
        """`groups`: (chunks, n_rows) per row group, `chunks` as for from_parquet — decoded by ONE call (fdb_batches_from_parquet):
        one copy queue for all of them, their host work side by side. Returns one ResidentBatch per row group, in order."""
        if not groups:
            return []
        rgs = (ParquetRowGroup * len(groups))()
        keep = []
        for g, (chunks, n_rows) in enumerate(groups):
            arr, k = cls._parquet_chunks(chunks)
            keep += [arr, k]
            rgs[g] = ParquetRowGroup(ctypes.addressof(arr), len(chunks), int(n_rows))
        outs = (ctypes.c_void_p * len(groups))()
        rc = lib().fdb_batches_from_parquet(rgs, len(groups), device, outs)
        if rc != 0:
            _raise(rc, lib().fdb_last_error().decode("utf-8", "replace"))
        return [cls(None, device=device, _handle=outs[g]) for g in range(len(groups))]

    @classmethod
    def from_parquet(cls, chunks: Sequence[tuple], n_rows: int, device: int = 0) -> "ResidentBatch":
        """`chunks`: (name, physical type, optional, utf8, bytes-like[, codec]) per column of ONE row group — decoded on the device
        (fdb_batch_from_parquet); `codec` is a CompressionCodec number or name (default UNCOMPRESSED). The byte buffers only need
        to stay alive for the duration of the call."""
        arr = (ParquetChunk * len(chunks))()
        keep = []
        for i, (name, ptype, optional, utf8, data, *rest) in enumerate(chunks):
            codec = rest[0] if rest else 0
            codec = PARQUET_CODECS[codec.upper()] if isinstance(codec, str) else int(codec)
            if isinstance(data, tuple):      # (address, length): bytes that already sit somewhere stable, e.g. a pinned file buffer
                addr, size = data
            elif isinstance(data, bytes):    # no copy: the bytes object is kept alive for the call
                addr, size = ctypes.cast(ctypes.c_char_p(data), ctypes.c_void_p).value, len(data)
            else:
                data = bytes(data)
                addr, size = ctypes.cast(ctypes.c_char_p(data), ctypes.c_void_p).value, len(data)
            nm = name.encode()
            keep += [data, nm]
            arr[i] = ParquetChunk(nm, ptype, int(optional), 1 if utf8 else 0, codec, addr, size)  # optional: the column's max definition level (0 / 1; more = nested)
        out = ctypes.c_void_p()
        rc = lib().fdb_batch_from_parquet(arr, len(chunks), n_rows, device, ctypes.byref(out))
        if rc != 0:
            _raise(rc, lib().fdb_last_error().decode("utf-8", "replace"))
        return cls(None, device=device, _handle=out.value)

    def __init__(self, batch: Optional[pa.RecordBatch], device: int = 0, _handle=None):
        if _handle is not None:  # a batch the library made itself (fdb_plan_filter_batch)
            self.handle, self.device = _handle, device
            return
        out = ctypes.c_void_p()
        with ExportedBatch(batch) as ex:
            rc = lib().fdb_batch_import(ctypes.addressof(ex.array), ctypes.addressof(ex.schema), device, ctypes.byref(out))
        if rc != 0:
            _raise(rc, lib().fdb_last_error().decode("utf-8", "replace"))
        self.handle = out.value
        self.device = device

    def to_arrow(self) -> pa.RecordBatch:
        """The resident record copied back to the host as Arrow (fdb_batch_export)."""
        arr, sch = ArrowArray(), ArrowSchema()
        rc = lib().fdb_batch_export(self.handle, ctypes.addressof(arr), ctypes.addressof(sch))
        if rc != 0:
            _raise(rc, lib().fdb_last_error().decode("utf-8", "replace"))
        return import_batch(arr, sch)

    def take(self, indices) -> "ResidentBatch":
        """≙ arrowutils.Take: row ``indices[i]`` of this record as row i of a new resident record (fdb_batch_take). int32 indices in any
        order, duplicates allowed; one outside the record raises FdbError(FDB_ERR_INVALID)."""
        import numpy as np
        idx = np.ascontiguousarray(np.asarray(indices, dtype=np.int64))
        if idx.size and (idx.min() < -(1 << 31) or idx.max() >= (1 << 31)):
            _raise(FDB_ERR_INVALID, "take: index does not fit int32")
        idx = idx.astype(np.int32)
        out = ctypes.c_void_p()
        rc = lib().fdb_batch_take(self.handle, idx.ctypes.data if idx.size else None, int(idx.size), ctypes.byref(out))
        if rc != 0:
            _raise(rc, lib().fdb_last_error().decode("utf-8", "replace"))
        return ResidentBatch(None, device=self.device, _handle=out.value)

    @property
    def column_names(self) -> List[str]:
        """The names of the record's columns, in order (fdb_batch_column_name)."""
        names, k = [], 0
        while True:
            nm = lib().fdb_batch_column_name(self.handle, k)
            if nm is None:
                return names
            names.append(nm.decode("utf-8", "replace"))
            k += 1

    @property
    def column_formats(self) -> List[str]:
        """The Arrow format strings of the record's columns, in order (fdb_batch_column_format)."""
        formats, k = [], 0
        while True:
            f = lib().fdb_batch_column_format(self.handle, k)
            if f is None:
                return formats
            formats.append(f.decode("utf-8", "replace"))
            k += 1

    def _sort_cols(self, columns):
        """`columns` → an fdb_sort_col array. A column is ``(name_or_index, descending=False, nulls_first=False)`` or a bare name /
        index; a name the record lacks (or has twice) raises KeyError before the library is called. A raw descriptor —
        ``SortCol(index, direction, nulls_first)`` — is passed through unchecked."""
        if isinstance(columns, (str, int, SortCol)):
            columns = [columns]
        names = None
        cols = []
        for c in columns:
            if isinstance(c, SortCol):
                cols.append(c)
                continue
            c = (c,) if isinstance(c, (str, int)) else tuple(c)
            if not 1 <= len(c) <= 3:
                raise ValueError("a sorting column is (name_or_index, descending=False, nulls_first=False)")
            key, descending, nulls_first = c[0], (len(c) > 1 and bool(c[1])), (len(c) > 2 and bool(c[2]))
            if isinstance(key, str):
                if names is None:
                    names = self.column_names
                if names.count(key) != 1:
                    raise KeyError("sort: the record has %s column named %r" % ("no" if key not in names else "more than one", key))
                key = names.index(key)
            cols.append(SortCol(int(key), 1 if descending else 0, 1 if nulls_first else 0))
        return (SortCol * max(1, len(cols)))(*cols), len(cols)

    def sort_indices(self, columns):
        """≙ arrowutils.SortRecord: the int32 permutation p with row p[i] of this record = row i of the sorted record
        (fdb_batch_sort_indices). Stable. `columns`: see ``sort``."""
        import numpy as np
        arr, n = self._sort_cols(columns)
        out = np.empty(max(1, self.num_rows), dtype=np.int32)
        rc = lib().fdb_batch_sort_indices(self.handle, arr, n, out.ctypes.data)
        if rc != 0:
            _raise(rc, lib().fdb_last_error().decode("utf-8", "replace"))
        return out[: self.num_rows]

    def sort_bench(self, columns, reps: int = 7, warmup: int = 2) -> dict:
        """Measurement aid (fdb_sort_bench): median device ms of the sort's key kernels + radix passes, and of bare radix sorts with
        the same pass count and bit widths."""
        arr, n = self._sort_cols(columns)
        a, b, k = ctypes.c_double(), ctypes.c_double(), ctypes.c_int32()
        rc = lib().fdb_sort_bench(self.handle, arr, n, int(reps), int(warmup), ctypes.byref(a), ctypes.byref(b), ctypes.byref(k))
        if rc != 0:
            _raise(rc, lib().fdb_last_error().decode("utf-8", "replace"))
        return {"sort_ms": a.value, "bare_sort_ms": b.value, "passes": k.value}

    def sort(self, columns) -> "ResidentBatch":
        """≙ SortRecord + Take without the indices leaving HBM: this record's rows in the order of `columns`, as a new resident record
        (fdb_batch_sort). A column is ``(name_or_index, descending=False, nulls_first=False)`` or a bare name; compared left to right;
        NULLs after a column's values unless nulls_first, whatever the direction; float64 as Go's cmp.Compare (NaNs equal, below -Inf);
        strings by their bytes; rows equal on every column keep their order."""
        arr, n = self._sort_cols(columns)
        out = ctypes.c_void_p()
        rc = lib().fdb_batch_sort(self.handle, arr, n, ctypes.byref(out))
        if rc != 0:
            _raise(rc, lib().fdb_last_error().decode("utf-8", "replace"))
        return ResidentBatch(None, device=self.device, _handle=out.value)

    @staticmethod
    def _merge_args(records, columns):
        records = list(records)
        handles = (ctypes.c_void_p * max(1, len(records)))(*[r.handle for r in records])
        if records:
            arr, n = records[0]._sort_cols(columns)
        else:
            arr, n = (SortCol * 1)(), 0
        return records, handles, arr, n

    @staticmethod
    def merge(records, columns, limit: int = 0) -> "ResidentBatch":
        """≙ arrowutils.MergeRecords: the rows of `records` — resident records of one schema, each already ordered by `columns` (as for
        ``sort``: names or indices, resolved against the first record) — as ONE new resident record in that order, at most `limit` rows
        when limit > 0 (fdb_batches_merge). Stable: equal rows come out in record order, then row order. An input that is not
        ordered raises FdbError(FDB_ERR_INVALID) naming the record and the row."""
        records, handles, arr, n = ResidentBatch._merge_args(records, columns)
        out = ctypes.c_void_p()
        rc = lib().fdb_batches_merge(handles, len(records), arr, n, int(limit), ctypes.byref(out))
        if rc != 0:
            _raise(rc, lib().fdb_last_error().decode("utf-8", "replace"))
        return ResidentBatch(None, device=records[0].device, _handle=out.value)

    @staticmethod
    def merge_named(records, order_by, limit: int = 0) -> "ResidentBatch":
        """≙ OrderedSynchronizer.ensureSameSchema + MergeRecords: ``merge`` for records whose field lists differ
        (fdb_batches_merge_named). `order_by`: ``Col(name)`` / ``DynCol(name)`` — a dynamic expression stands for every matching column,
        in name order — or ``(expr, descending, nulls_first)``. The result has the sorting columns first, then every other field in
        first-seen order; a record's rows are NULL in the columns it lacks."""
        records = list(records)
        handles = (ctypes.c_void_p * max(1, len(records)))(*[r.handle for r in records])
        arr, n, _keep = _order_cols(order_by)
        out = ctypes.c_void_p()
        rc = lib().fdb_batches_merge_named(handles, len(records), arr, n, int(limit), ctypes.byref(out))
        if rc != 0:
            _raise(rc, lib().fdb_last_error().decode("utf-8", "replace"))
        return ResidentBatch(None, device=records[0].device, _handle=out.value)

    @staticmethod
    def merge_bench(records, columns, reps: int = 7, warmup: int = 2) -> dict:
        """Measurement aid (fdb_merge_bench): median device ms of the merge's key kernels + order check + rounds, of its gather, and of
        every round alone."""
        records, handles, arr, n = ResidentBatch._merge_args(records, columns)
        a, b, k, w = ctypes.c_double(), ctypes.c_double(), ctypes.c_int32(), ctypes.c_int32()
        rounds = (ctypes.c_double * 32)()
        rc = lib().fdb_merge_bench(handles, len(records), arr, n, int(reps), int(warmup), ctypes.byref(a), ctypes.byref(b), rounds, 32, ctypes.byref(k), ctypes.byref(w))
        if rc != 0:
            _raise(rc, lib().fdb_last_error().decode("utf-8", "replace"))
        return {"merge_ms": a.value, "gather_ms": b.value, "round_ms": [rounds[i] for i in range(min(k.value, 32))], "words": w.value}

    def to_parquet(self, page_rows: int = 0, optional=None, encodings=None, compression=None, statistics=None, index_size_limit: int = 0, sorting_columns=None,
                   bloom_filters=None, bloom_bits_per_value: int = 0, runs=None, row_group_rows: int = 0, dictionaries=None, strings=None) -> bytes:
        """≙ pqarrow.RecordsToFile for one record: this resident record as one complete Parquet file (one row group, data pages V1 of
        `page_rows` rows, 0 = 65 536), its payloads encoded on the device (fdb_batch_to_parquet). `optional`: None, a
        sequence per column or a dict by name of None (auto: optional iff the column holds NULLs or is a dictionary / string column),
        False (required; refused for a column with NULLs) or True. `encodings`: None, a sequence per column or a dict by name of
        None / "plain" (as without it) or "delta": an int64 / uint64 column written DELTA_BINARY_PACKED, its deltas, widths and pages
        made on the device (fdb_batch_to_parquet_encoded) — what sorted timestamps ask for. `compression`: None (UNCOMPRESSED),
        "snappy" (every column), a sequence per column or a dict by name of None / "uncompressed" / "snappy": every page of such a
        column — dictionary page and data pages — is written as a Snappy block, compressed on the device in fragments of 32 KiB
        (fdb_batch_to_parquet_compressed), and only the compressed file crosses the link; for the length of the call the device holds
        about three times the file body. DELTA and SNAPPY go together. "lz4" in place of "snappy": the pages are LZ4_RAW blocks
        (ColumnMetaData.codec 7, the bare block without a preamble), found by the same match search, one block per page; SNAPPY,
        LZ4_RAW and uncompressed columns may stand side by side in one file. `statistics`: None, "chunk" — Statistics.min_value / max_value
        per column chunk and FileMetaData.column_orders, the bounds found by one more pass on the device — or "page": the same and the
        Parquet page index (ColumnIndex and OffsetIndex per column, between the pages and the footer), which FrostDB's own scan prunes
        row groups with; `index_size_limit`: the bytes a string bound of the ColumnIndex is cut to (0 = 16); `sorting_columns`: a
        sequence of (name or index, descending=False, nulls_first=False) written as RowGroup.sorting_columns — metadata only, the rows
        are not checked (fdb_batch_to_parquet_indexed). Without these three the call is what it was. `bloom_filters`: None, a sequence
        of column names, a dict of name → bool, or "sorting" — the `sorting_columns` that are not boolean, what the reference's
        Schema.NewWriter does: each such column gets a split-block bloom filter (XXH64 of the value's PLAIN bytes) of
        `bloom_bits_per_value` bits per non-NULL row (0 = 10; a dictionary column: per entry, when those are fewer), its bits set on the
        device by one more pass, written after the pages and named by ColumnMetaData.bloom_filter_offset / _length — what FrostDB's
        scan asks first for `=` (fdb_batch_to_parquet_filtered). A boolean column is refused; an unknown name is FDB_ERR_INVALID.
        Without these two the call is what it was. `runs`: None; True — every column; a sequence of column names; or a dict of
        name → True / "values" / "levels" / None: the pages' dictionary indices ("values") and definition levels ("levels") are cut
        into RLE and bit-packed runs instead of one bit-packed run each (the rule: include/frostdb_amd.h) — what a record sorted by
        its label columns asks for, where a label column is long stretches of one index and a dynamic column long stretches of NULL;
        sized and written on the device by two more passes (fdb_batch_to_parquet_runs). No page gets longer. "values" on a column
        that has no dictionary is refused (True skips such columns). Without it the call is what it was. `dictionaries`: None /
        "whole" — every chunk carries the column's whole dictionary — or "used": the dictionary page of a dictionary / string column
        holds only the entries a non-NULL row refers to, in entry order, and the indices are re-keyed to their rank among those and
        packed at that width — what a record asks for after filter(), take, limit, a sampler or a merge over a dictionary union;
        found and re-keyed on the device by two more passes (fdb_batch_to_parquet_grouped). `row_group_rows` (≙ WithRowGroupSize;
        here a multiple of 64): 0 (one row group), or the rows per row group — the last one shorter —, each group with its own pages,
        statistics, page index, bloom filters and (with "used") dictionaries; from_parquet_many reads them back in one call.
        Without these two the call is what it was. `strings`: None; "plain" or "delta_length" — every dictionary / string / binary
        column; a sequence per column or a dict by name of None / "dictionary" / "plain" / "delta_length": such a column's chunk has
        no dictionary page, its pages hold the non-NULL values themselves — PLAIN (length and bytes per value: FrostDB's own default
        for a string column) or DELTA_LENGTH_BYTE_ARRAY (the lengths DELTA_BINARY_PACKED, then the bytes) — what a column of mostly
        distinct values asks for; sized by a byte survey and gathered from the entries by a byte encode pass on the device
        (fdb_batch_to_parquet_strings). The bare string skips the columns that cannot take it — other kinds, and those whose
        dictionary indices `runs` asks for by name — and `runs=True` leaves the indices of a column with a form alone; an explicit
        entry that cannot be honoured is refused. `dictionaries="used"` has no effect on such a column. Without it the call is what
        it was."""
        asked = (page_rows, optional, encodings, compression, statistics, index_size_limit, sorting_columns, bloom_filters, bloom_bits_per_value, runs, row_group_rows, dictionaries, strings)
        return _parquet_write("fdb_batch_to_parquet", [self.handle], self.column_names, [f == "b" for f in self.column_formats],
                              [f not in ("l", "L", "g", "b") for f in self.column_formats], asked)

    @property
    def num_rows(self) -> int:
        return lib().fdb_batch_num_rows(self.handle)

    @property
    def device_bytes(self) -> int:
        return lib().fdb_batch_device_bytes(self.handle)

    @property
    def scan_cache_bytes(self) -> int:
        """Bytes of the narrow-index cache dense scans keep beside the record (not part of `device_bytes`; 0 until such a scan)."""
        return lib().fdb_batch_scan_cache_bytes(self.handle)

    def close(self) -> None:
        if getattr(self, "handle", None):
            lib().fdb_batch_release(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class PreparedRun:
    """The pointer tables of a run of exported host records (fdb_plan_push_many's arguments), built once."""

    def __init__(self, exported: Sequence["ExportedBatch"]):
        self.keep = list(exported)
        self.n = len(self.keep)
        self.arrs = (ctypes.c_void_p * self.n)(*[ctypes.addressof(e.array) for e in self.keep])
        self.schs = (ctypes.c_void_p * self.n)(*[ctypes.addressof(e.schema) for e in self.keep])

    def __len__(self) -> int:
        return self.n


class HashAggregatePlan:
    """One fused ``PredicateFilter → HashAggregate`` chain on one GPU."""

    def __init__(self, filter_expr: Optional[Expr], aggs: Sequence[AggregationFunction] = (),
                 groups: Sequence[Column] = (), device: int = 0, final_stage: bool = False, desc=None, regex=None, ordered: bool = False):
        """`desc`: a descriptor built once with `to_desc(filter_expr, aggs, groups, final_stage)` and shared by every chain /
        execution of the same query (≙ the logical plan being built once and `physicalplan.Build` instantiating N chains).
        `regex`: the host application's regex engine (`logicalplan.regex_matcher`), else std::regex."""
        self._desc = desc if desc is not None else to_desc(filter_expr, list(aggs), list(groups), final_stage, regex=regex, ordered=ordered)
        self.aggs = list(aggs)
        self._ctor = (filter_expr, list(aggs), list(groups), device, final_stage, self._desc)
        out = ctypes.c_void_p()
        rc = lib().fdb_plan_create(ctypes.addressof(self._desc.desc), device, ctypes.byref(out))
        if rc != 0:
            _raise(rc, lib().fdb_last_error().decode("utf-8", "replace"))
        self.handle = out.value
        self.device = device
        self._next: Optional[Callable[[pa.RecordBatch], None]] = None
        self._next_finish: Optional[Callable[[], None]] = None

    @classmethod
    def _adopt(cls, handle: int, proto: "HashAggregatePlan") -> "HashAggregatePlan":
        """Wraps a plan handle the library created itself (the shard of fdb_plan_exchange) with `proto`'s descriptor."""
        self = cls.__new__(cls)
        self._desc = proto._desc
        self.aggs = list(proto.aggs)
        self._ctor = proto._ctor
        self.handle = handle
        self.device = proto.device
        self._next = None
        self._next_finish = None
        return self

    def _check(self, rc: int) -> None:
        if rc != 0:
            _raise(rc, lib().fdb_plan_last_error(self.handle).decode("utf-8", "replace"))

    def clone_empty(self) -> "HashAggregatePlan":
        """A fresh plan with the same descriptor on the same device (no state)."""
        f, a, g, d, fs, desc = self._ctor
        return HashAggregatePlan(f, a, g, device=d, final_stage=fs, desc=desc)

    # ---- PhysicalPlan verbs --------------------------------------------------------------------------
    def Callback(self, record) -> None:
        if isinstance(record, ResidentBatch):
            self._check(lib().fdb_plan_push_batch(self.handle, record.handle))
            return
        with ExportedBatch(record) as ex:
            self._check(lib().fdb_plan_push(self.handle, ctypes.addressof(ex.array), ctypes.addressof(ex.schema)))

    def CallbackExported(self, ex: "ExportedBatch") -> None:
        """Callback for a host record whose C-data export the caller keeps (fdb_plan_push only borrows the structs, so one export
        can be pushed any number of times — measurement loops keep pyarrow's export cost out of the timed region)."""
        self._check(lib().fdb_plan_push(self.handle, ctypes.addressof(ex.array), ctypes.addressof(ex.schema)))

    def CallbackExportedMany(self, exported: Sequence["ExportedBatch"]) -> None:
        """fdb_plan_push_many: the Callbacks of a run of host records in ONE call into the library (a thread that drives a chain this
        way holds the interpreter lock once per run, not once per record)."""
        n = len(exported)
        arrs = (ctypes.c_void_p * n)(*[ctypes.addressof(e.array) for e in exported])
        schs = (ctypes.c_void_p * n)(*[ctypes.addressof(e.schema) for e in exported])
        done = ctypes.c_int32()
        self._check(lib().fdb_plan_push_many(self.handle, arrs, schs, n, ctypes.byref(done)))

    def CallbackPrepared(self, run: "PreparedRun") -> None:
        """fdb_plan_push_many over pointer tables built beforehand (PreparedRun): the call itself is ONE entry into the library and holds the
        interpreter lock for microseconds — what a goroutine of the Go shim does (its C arrays are built by that goroutine, concurrently with
        the others; here building them per call would serialise N chain threads on the interpreter lock: 0.3 ms per chain and 1 024 records)."""
        done = ctypes.c_int32()
        self._check(lib().fdb_plan_push_many(self.handle, run.arrs, run.schs, run.n, ctypes.byref(done)))

    def CallbackResident(self, records: Sequence[ResidentBatch]) -> None:
        """Callback for several HBM-resident records at once: one fused kernel launch over all of them."""
        arr = (ctypes.c_void_p * len(records))(*[r.handle for r in records])
        self._check(lib().fdb_plan_push_batches(self.handle, arr, len(records)))

    def Finish(self) -> pa.RecordBatch:
        arr, sch = ArrowArray(), ArrowSchema()
        n = ctypes.c_int64()
        self._check(lib().fdb_plan_finish(self.handle, ctypes.addressof(arr), ctypes.addressof(sch), ctypes.byref(n)))
        rec = import_batch(arr, sch)
        if self._next is not None:  # ≙ next.Callback(record) for every aggregate, then next.Finish() (aggregate.go:617-626, :540)
            if rec.num_rows:
                self._next(rec)
            while True:
                more = self.FinishNext()
                if more is None:
                    break
                self._next(more)
            if self._next_finish is not None:
                self._next_finish()
        return rec

    def FinishNext(self) -> Optional[pa.RecordBatch]:
        """The next record of a Finish that emitted several (a plain string / binary key column that would pass 2 GiB in one record starts a
        new one, aggregate.go:426-468); None when there is none left."""
        arr, sch = ArrowArray(), ArrowSchema()
        n, emitted = ctypes.c_int64(), ctypes.c_int32()
        self._check(lib().fdb_plan_finish_next(self.handle, ctypes.addressof(arr), ctypes.addressof(sch), ctypes.byref(n), ctypes.byref(emitted)))
        return import_batch(arr, sch) if emitted.value else None

    def FinishAll(self) -> List[pa.RecordBatch]:
        """≙ Finish as the next operator sees it: every record it emits, in order."""
        recs = [self.Finish()] if self._next is None else []
        if self._next is not None:
            raise FdbError(1, "FinishAll: the plan has a next operator (SetNext): Finish hands it the records")
        while True:
            more = self.FinishNext()
            if more is None:
                return recs
            recs.append(more)

    def FinishResident(self) -> "ResidentBatch":
        """≙ Finish for a device-side consumer (fdb_plan_finish_batch): the result record stays in HBM."""
        out, n = ctypes.c_void_p(), ctypes.c_int64()
        self._check(lib().fdb_plan_finish_batch(self.handle, ctypes.byref(out), ctypes.byref(n)))
        return ResidentBatch(None, device=self.device, _handle=out.value)

    def SetNext(self, callback: Callable[[pa.RecordBatch], None], finish: Optional[Callable[[], None]] = None) -> None:
        self._next, self._next_finish = callback, finish

    def Draw(self) -> str:
        return lib().fdb_plan_draw(self.handle).decode()

    def Close(self) -> None:
        if getattr(self, "handle", None):
            lib().fdb_plan_close(self.handle)
            self.handle = None

    # ---- beyond the interface ---------------------------------------------------------------------------
    def Merge(self, other: "HashAggregatePlan") -> None:
        """≙ Synchronizer + final-stage HashAggregate on one device."""
        self._check(lib().fdb_plan_merge(self.handle, other.handle))

    def Select(self, record: pa.RecordBatch):
        import numpy as np
        idx = np.zeros(max(record.num_rows, 1), dtype=np.uint32)
        n = ctypes.c_int64()
        with ExportedBatch(record) as ex:
            self._check(lib().fdb_plan_select(self.handle, ctypes.addressof(ex.array), ctypes.addressof(ex.schema),
                                              idx.ctypes.data, idx.size, ctypes.byref(n)))
        return idx[: n.value].copy()

    def Filter(self, record: pa.RecordBatch) -> Optional[pa.RecordBatch]:
        """≙ filter(): compacted record, or None when no row qualifies (filter.go:264-266)."""
        arr, sch = ArrowArray(), ArrowSchema()
        n = ctypes.c_int64()
        with ExportedBatch(record) as ex:
            self._check(lib().fdb_plan_filter(self.handle, ctypes.addressof(ex.array), ctypes.addressof(ex.schema),
                                              ctypes.addressof(arr), ctypes.addressof(sch), ctypes.byref(n)))
        if n.value == 0:
            return None
        return import_batch(arr, sch)

    def FilterResident(self, record: "ResidentBatch") -> "ResidentBatch":
        """≙ filter() on a record resident in HBM: the compacted record, resident too (zero rows when nothing qualifies)."""
        out, n = ctypes.c_void_p(), ctypes.c_int64()
        self._check(lib().fdb_plan_filter_batch(self.handle, record.handle, ctypes.byref(out), ctypes.byref(n)))
        return ResidentBatch(None, device=self.device, _handle=out.value)

    def FilterResidentMany(self, records: Sequence["ResidentBatch"]) -> List["ResidentBatch"]:
        """≙ filter() over several resident records at once (fdb_plan_filter_batches): one launch sequence for all of them."""
        n = len(records)
        arr = (ctypes.c_void_p * n)(*[r.handle for r in records])
        outs = (ctypes.c_void_p * n)()
        counts = (ctypes.c_int64 * n)()
        self._check(lib().fdb_plan_filter_batches(self.handle, arr, n, outs, counts))
        return [ResidentBatch(None, device=self.device, _handle=outs[i]) for i in range(n)]

    def SelectResident(self, record: "ResidentBatch", dev_ptr: int, capacity: int) -> int:
        """Selection vector of a resident record into a DEVICE buffer (uint32 × capacity ≥ rows); returns the number selected."""
        n = ctypes.c_int64()
        self._check(lib().fdb_plan_select_batch(self.handle, record.handle, ctypes.c_void_p(dev_ptr), capacity, ctypes.byref(n)))
        return n.value

    def num_groups(self) -> int:
        n = ctypes.c_int64()
        self._check(lib().fdb_plan_num_groups(self.handle, ctypes.byref(n)))
        return n.value

    def partial_keys(self) -> pa.RecordBatch:
        arr, sch = ArrowArray(), ArrowSchema()
        self._check(lib().fdb_plan_partial_keys(self.handle, ctypes.addressof(arr), ctypes.addressof(sch)))
        return import_batch(arr, sch)

    # ---- hash-partitioned exchange of high-cardinality partial tables (see include/frostdb_amd.h) -------------------
    def group_schema(self) -> pa.RecordBatch:
        """Zero-row record: dictionary columns carry this plan's distinct key values, plus one column per typed aggregate."""
        arr, sch = ArrowArray(), ArrowSchema()
        self._check(lib().fdb_plan_group_schema(self.handle, ctypes.addressof(arr), ctypes.addressof(sch)))
        return import_batch(arr, sch)

    def seed_groups(self, schema_record: pa.RecordBatch) -> None:
        with ExportedBatch(schema_record) as ex:
            self._check(lib().fdb_plan_seed_groups(self.handle, ctypes.addressof(ex.array), ctypes.addressof(ex.schema)))

    def hash_export(self, layout: "HashAggregatePlan", n_parts: int):
        """(device pointer, rows per partition, bytes per row): this plan's groups re-keyed for `layout`, packed by
        destination partition. The buffer belongs to this plan until its next push or Close."""
        ptr, rw = ctypes.c_void_p(), ctypes.c_int32()
        counts = (ctypes.c_int64 * n_parts)()
        self._check(lib().fdb_plan_hash_export(self.handle, layout.handle, n_parts, ctypes.byref(ptr), counts, ctypes.byref(rw)))
        return ptr.value or 0, list(counts), rw.value * 4

    def hash_import(self, dev_ptr: int, n_rows: int) -> None:
        self._check(lib().fdb_plan_hash_import(self.handle, ctypes.c_void_p(dev_ptr), n_rows))

    def state_array_ops(self) -> List[int]:
        """Merge operation of every table array (0 unused, 1 int sum, 2 float64 sum, 3 int min, 4 int max); array 0 = row counts."""
        n = ctypes.c_int32()
        self._check(lib().fdb_plan_state_arrays(self.handle, ctypes.byref(n)))
        ops = []
        for a in range(n.value):
            op = ctypes.c_int32()
            self._check(lib().fdb_plan_state_array_op(self.handle, a, ctypes.byref(op)))
            ops.append(op.value)
        return ops

    def agg_format(self, agg: int) -> str:
        c = ctypes.create_string_buffer(2)
        self._check(lib().fdb_plan_agg_type(self.handle, agg, c))
        return c.value.decode() or "l"

    def partial_state_into(self, agg: int, dst_ptr: int, capacity_bytes: int) -> None:
        """Copies aggregation `agg`'s partial column (n_groups × 8 B) to a host or device pointer."""
        self._check(lib().fdb_plan_partial_state(self.handle, agg, dst_ptr, capacity_bytes))

    def state_signature(self):
        """(layout signature, n_slots) of the plan's table — see fdb_plan_state_signature."""
        sig, n = ctypes.c_uint64(), ctypes.c_int64()
        self._check(lib().fdb_plan_state_signature(self.handle, ctypes.byref(sig), ctypes.byref(n)))
        return sig.value, n.value

    def state_pointers(self):
        """(device address of array 0, stride between arrays in elements, n_slots) — zero-copy view of the dense table."""
        base, stride, n = ctypes.c_void_p(), ctypes.c_int64(), ctypes.c_int64()
        self._check(lib().fdb_plan_state_pointers(self.handle, ctypes.byref(base), ctypes.byref(stride), ctypes.byref(n)))
        return base.value or 0, stride.value, n.value

    def stream_ptr(self) -> int:
        s = ctypes.c_void_p()
        self._check(lib().fdb_plan_stream(self.handle, ctypes.byref(s)))
        return s.value or 0

    def state_read(self, array: int, dst_ptr: int, capacity_bytes: int) -> None:
        self._check(lib().fdb_plan_state_read(self.handle, array, dst_ptr, capacity_bytes))

    def state_write(self, array: int, src_ptr: int, nbytes: int) -> None:
        self._check(lib().fdb_plan_state_write(self.handle, array, src_ptr, nbytes))

    def set_timing(self, enabled: bool) -> None:
        lib().fdb_plan_set_timing(self.handle, 1 if enabled else 0)

    def set_tuning(self, rows_per_thread: int = 8, grid_blocks: int = 0) -> None:
        lib().fdb_plan_set_tuning(self.handle, rows_per_thread, grid_blocks)

    def set_deterministic(self, enabled: bool = True) -> None:
        """Reproducible float64 sums (fdb_plan_set_deterministic): the same pushes give the same bits on every run."""
        self._check(lib().fdb_plan_set_deterministic(self.handle, 1 if enabled else 0))

    def set_exact_sums(self, enabled: bool = True) -> None:
        """Exact float64 sums (fdb_plan_set_exact_sums): every float64 SUM is the correctly rounded exact sum of the group's values,
        whatever the row order, record split or merge order. Only before the first push / merge; FdbError(FDB_ERR_STATE) after."""
        self._check(lib().fdb_plan_set_exact_sums(self.handle, 1 if enabled else 0))

    def last_kernel(self) -> str:
        """Name of the scan kernel the latest push launched (``fdb_plan_kernel`` = run-time specialised)."""
        return (lib().fdb_plan_last_kernel(self.handle) or b"").decode()

    def stats(self) -> dict:
        b, ms, n, r = ctypes.c_int64(), ctypes.c_double(), ctypes.c_int64(), ctypes.c_int64()
        lib().fdb_plan_stats(self.handle, ctypes.byref(b), ctypes.byref(ms), ctypes.byref(n), ctypes.byref(r))
        mm = ctypes.c_double()
        lib().fdb_plan_merge_ms(self.handle, ctypes.byref(mm))
        return {"algorithmic_bytes": b.value, "kernel_ms": ms.value, "launches": n.value, "rows": r.value, "merge_ms": mm.value}

    def __del__(self):
        try:
            self.Close()
        except Exception:
            pass


class ProjectCol(ctypes.Structure):
    """fdb_project_col: one item of a Projection's output list."""
    _fields_ = [("kind", ctypes.c_int32), ("_pad", ctypes.c_int32), ("name", ctypes.c_char_p)]


PROJECT_COLUMN, PROJECT_DYNAMIC, PROJECT_COMPUTED, PROJECT_ALL = 0, 1, 2, 3


class Projection:
    """≙ physicalplan.Projection (project.go:906-943) on one GPU: `exprs` is the output list — ``Col(x)`` passes the first field of that
    name through (a record without it contributes nothing), ``DynCol(x)`` every field under ``x.``, anything else is computed on the
    device under its Name() / alias. With `filter_expr` the same plan also answers FilterResident (``PredicateFilter → Projection``)."""

    def __init__(self, exprs: Sequence[Any], filter_expr: Optional[Expr] = None, device: int = 0):
        self.exprs = list(exprs)
        computed = [e for e in self.exprs if not isinstance(e, Column)]
        self._desc = to_desc(filter_expr, [], [], projections=computed)
        self._names = []
        items = (ProjectCol * max(1, len(self.exprs)))()
        for i, e in enumerate(self.exprs):
            nm = expr_name(e).encode()
            self._names.append(nm)
            items[i].kind = (PROJECT_DYNAMIC if e.dynamic else PROJECT_COLUMN) if isinstance(e, Column) else PROJECT_COMPUTED
            items[i].name = nm
        self._items, self._n_items = items, len(self.exprs)
        out = ctypes.c_void_p()
        rc = lib().fdb_plan_create(ctypes.addressof(self._desc.desc), device, ctypes.byref(out))
        if rc != 0:
            _raise(rc, lib().fdb_last_error().decode("utf-8", "replace"))
        self.handle = out.value
        self.device = device

    def _check(self, rc: int) -> None:
        if rc != 0:
            _raise(rc, lib().fdb_plan_last_error(self.handle).decode("utf-8", "replace"))

    def Callback(self, record: pa.RecordBatch) -> pa.RecordBatch:
        """Host record in, host record out (fdb_plan_project)."""
        arr, sch = ArrowArray(), ArrowSchema()
        with ExportedBatch(record) as ex:
            self._check(lib().fdb_plan_project(self.handle, self._items, self._n_items, ctypes.addressof(ex.array), ctypes.addressof(ex.schema),
                                               ctypes.addressof(arr), ctypes.addressof(sch)))
        return import_batch(arr, sch)

    def ProjectResident(self, rb: "ResidentBatch") -> "ResidentBatch":
        out = ctypes.c_void_p()
        self._check(lib().fdb_plan_project_batch(self.handle, self._items, self._n_items, rb.handle, ctypes.byref(out)))
        return ResidentBatch(None, device=self.device, _handle=out.value)

    def ProjectResidentMany(self, rbs: Sequence["ResidentBatch"]) -> List["ResidentBatch"]:
        """Every record of a scan: one launch for all computed fields (fdb_plan_project_batches)."""
        n = len(rbs)
        arr = (ctypes.c_void_p * max(1, n))(*[r.handle for r in rbs])
        outs = (ctypes.c_void_p * max(1, n))()
        self._check(lib().fdb_plan_project_batches(self.handle, self._items, self._n_items, arr, n, outs))
        return [ResidentBatch(None, device=self.device, _handle=outs[i]) for i in range(n)]

    def FilterResident(self, rb: "ResidentBatch") -> "ResidentBatch":
        """The plan's PredicateFilter on a resident record (fdb_plan_filter_batch); feed the result to ProjectResident."""
        out, n = ctypes.c_void_p(), ctypes.c_int64()
        self._check(lib().fdb_plan_filter_batch(self.handle, rb.handle, ctypes.byref(out), ctypes.byref(n)))
        return ResidentBatch(None, device=self.device, _handle=out.value)

    def set_timing(self, enabled: bool) -> None:
        lib().fdb_plan_set_timing(self.handle, 1 if enabled else 0)

    def stats(self) -> dict:
        b, ms, n, r = ctypes.c_int64(), ctypes.c_double(), ctypes.c_int64(), ctypes.c_int64()
        lib().fdb_plan_stats(self.handle, ctypes.byref(b), ctypes.byref(ms), ctypes.byref(n), ctypes.byref(r))
        return {"algorithmic_bytes": b.value, "kernel_ms": ms.value, "launches": n.value, "rows": r.value}

    def last_kernel(self) -> str:
        return (lib().fdb_plan_last_kernel(self.handle) or b"").decode()

    def Close(self) -> None:
        if getattr(self, "handle", None):
            lib().fdb_plan_close(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.Close()
        except Exception:
            pass


class Limiter:
    """≙ physicalplan.Limiter (limit.go): the first `count` rows of EVERY record — the reference never decrements its count, so a
    Limiter has no state and nothing to close."""

    def __init__(self, count: int, device: int = 0):
        if count < 0:
            count += 1 << 64  # (limit.go:36: uint64(v.Value))
        self.count = int(count)
        self.device = device

    def CallbackResident(self, rb: "ResidentBatch") -> "ResidentBatch":
        out = ctypes.c_void_p()
        rc = lib().fdb_batch_limit(rb.handle, self.count, ctypes.byref(out))
        if rc != 0:
            _raise(rc, lib().fdb_last_error().decode("utf-8", "replace"))
        return ResidentBatch(None, device=rb.device, _handle=out.value)

    def Callback(self, record: pa.RecordBatch) -> pa.RecordBatch:
        """Host record in, host record out: staged, limited on the device, exported."""
        rb = ResidentBatch(record, device=self.device)
        try:
            out = self.CallbackResident(rb)
            try:
                return out.to_arrow()
            finally:
                out.close()
        finally:
            rb.close()

    def Draw(self) -> str:
        return "Limit(%d)" % self.count


class ReservoirSampler:
    """≙ physicalplan.ReservoirSampler (sampler.go) on one GPU: up to `size` rows of everything pushed, chosen by Algorithm L with the
    generator include/frostdb_amd.h documents (`seed`). The reservoir is a record in HBM; Finish always gives ONE record (the
    reference's materialize form). Splitting `size` over the chains of a query is the caller's job."""

    def __init__(self, size: int, seed: int, device: int = 0):
        self.size = int(size)
        self.device = device
        out = ctypes.c_void_p()
        rc = lib().fdb_sampler_create(self.size, int(seed) & 0xFFFFFFFFFFFFFFFF, device, ctypes.byref(out))
        if rc != 0:
            _raise(rc, lib().fdb_last_error().decode("utf-8", "replace"))
        self.handle = out.value

    def _check(self, rc: int) -> None:
        if rc != 0:
            _raise(rc, lib().fdb_last_error().decode("utf-8", "replace"))

    def Callback(self, record: pa.RecordBatch) -> None:
        with ExportedBatch(record) as ex:
            self._check(lib().fdb_sampler_push(self.handle, ctypes.addressof(ex.array), ctypes.addressof(ex.schema)))

    def CallbackResident(self, rb: "ResidentBatch") -> None:
        self._check(lib().fdb_sampler_push_batch(self.handle, rb.handle))

    def Finish(self) -> pa.RecordBatch:
        arr, sch = ArrowArray(), ArrowSchema()
        n = ctypes.c_int64()
        self._check(lib().fdb_sampler_finish(self.handle, ctypes.addressof(arr), ctypes.addressof(sch), ctypes.byref(n)))
        return import_batch(arr, sch)

    def FinishResident(self) -> "ResidentBatch":
        out, n = ctypes.c_void_p(), ctypes.c_int64()
        self._check(lib().fdb_sampler_finish_batch(self.handle, ctypes.byref(out), ctypes.byref(n)))
        return ResidentBatch(None, device=self.device, _handle=out.value)

    def Draw(self) -> str:
        return "Reservoir Sampler (%d)" % self.size

    def Close(self) -> None:
        if getattr(self, "handle", None):
            lib().fdb_sampler_close(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.Close()
        except Exception:
            pass


class OrderedSynchronizer:
    """≙ physicalplan.OrderedSynchronizer (ordered_synchronizer.go) over resident records, without the blocking: `inputs` chains each
    contribute at most one record to a round; the call that completes a round — the push of the last running input, or the Finish that
    leaves only waiting inputs — returns the round's records merged by `order_by` (``ResidentBatch.merge_named``), every other call
    returns None. Parked records are referenced here until their round is merged. Safe to call from several threads."""

    def __init__(self, inputs: int, order_by):
        self.inputs = int(inputs)
        self._order, n, self._keep = _order_cols(order_by)
        self._parked = {}
        self._device = 0
        self._lock = threading.Lock()  # call and bookkeeping are one step (the library serialises the calls anyway: it merges under its mutex)
        out = ctypes.c_void_p()
        rc = lib().fdb_osync_create(self.inputs, self._order, n, ctypes.byref(out))
        if rc != 0:
            _raise(rc, lib().fdb_last_error().decode("utf-8", "replace"))
        self.handle = out.value

    def _merged(self, rc: int, out) -> Optional["ResidentBatch"]:
        if rc != 0:  # (what a failed round parked stays referenced until the next round is merged: longer than needed, never shorter)
            _raise(rc, lib().fdb_last_error().decode("utf-8", "replace"))
        if not out.value:
            return None
        self._parked.clear()  # the round is merged: its records are the callers' again
        return ResidentBatch(None, device=self._device, _handle=out.value)

    def Callback(self, input: int, rb: "ResidentBatch") -> Optional["ResidentBatch"]:
        out = ctypes.c_void_p()
        with self._lock:
            rc = lib().fdb_osync_push(self.handle, int(input), rb.handle, ctypes.byref(out))
            if rc == 0 and not out.value:
                self._parked[int(input)] = rb
            self._device = rb.device
            return self._merged(rc, out)

    def Finish(self, input: int):
        """→ (the merged record of the round this call completed, or None; True when the last input has finished)"""
        out, done = ctypes.c_void_p(), ctypes.c_int32()
        with self._lock:
            rc = lib().fdb_osync_finish(self.handle, int(input), ctypes.byref(out), ctypes.byref(done))
            return self._merged(rc, out), bool(done.value)

    def Draw(self) -> str:
        return "OrderedSynchronizer"

    def Close(self) -> None:
        if getattr(self, "handle", None):
            lib().fdb_osync_close(self.handle)
            self.handle = None
        self._parked = {}

    def __del__(self):
        try:
            self.Close()
        except Exception:
            pass


def execute(records: Sequence, filter_expr: Optional[Expr], aggs: Sequence[AggregationFunction],
            groups: Sequence[Column], device: int = 0) -> pa.RecordBatch:
    """The engine-level shape of the path: scan `records` through one GPU chain and return the final record."""
    plan = HashAggregatePlan(filter_expr, aggs, groups, device=device)
    try:
        for r in records:
            plan.Callback(r)
        return plan.Finish()
    finally:
        plan.Close()


def snappy_decode_pages(pages: "list[bytes]", sizes: "list[int]", device: int = 0):
    """Snappy-compressed pages → their bytes, inflated on the device (fdb_snappy_decode_pages; tests and measurement);
    device < 0: by the library's host decoder, without a GPU (the same status codes but 6). Returns (list of bytes — None for a page the decoder refused —, list of status codes, kernel milliseconds)."""
    return _decode_pages(lib().fdb_snappy_decode_pages, pages, sizes, device)


def lz4_decode_pages(pages: "list[bytes]", sizes: "list[int]", device: int = 0):
    """LZ4 blocks (Parquet's LZ4_RAW pages) → their bytes, inflated on the device (fdb_lz4_decode_pages; tests and measurement);
    device < 0: by the library's built-in host decoder, without a GPU. Returns what snappy_decode_pages returns."""
    return _decode_pages(lib().fdb_lz4_decode_pages, pages, sizes, device)


def _decode_pages(entry, pages, sizes, device):
    import numpy as np
    n = len(pages)
    src = b"".join(pages)
    table = np.zeros((n, 3), dtype=np.uint64)  # src_off, dst_off, (src_len | dst_len << 32)
    so = do = 0
    for i, (p, z) in enumerate(zip(pages, sizes)):
        table[i] = (so, do, len(p) | (int(z) << 32))
        so += len(p); do += int(z)
    dst = np.zeros(max(do, 1), dtype=np.uint8)
    status = np.zeros(max(n, 1), dtype=np.uint32)
    ms = ctypes.c_double(0.0)
    srcb = np.frombuffer(src, dtype=np.uint8) if src else np.zeros(1, dtype=np.uint8)
    rc = entry(srcb.ctypes.data, len(src), table.ctypes.data, n, dst.ctypes.data, do, device, status.ctypes.data, ctypes.byref(ms))
    if rc != FDB_OK:
        _raise(rc, (lib().fdb_last_error() or b"").decode("utf-8", "replace"))
    out, at = [], 0
    for i, z in enumerate(sizes):
        out.append(bytes(dst[at:at + int(z)]) if status[i] == 0 else None)
        at += int(z)
    return out, [int(x) for x in status[:n]], ms.value
