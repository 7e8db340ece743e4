"""Dictionary-encoded INT64 / DOUBLE Parquet columns decoded on the device (pq_decode_dict8_kernel) against pyarrow's reader of the
same bytes — the method of tests/test_gpu_parquet.py, with a comparison that leaves no row out: the uint64 VIEW of every valid row
(NaN payloads, −0.0 and subnormals included) and the NULL position of every row. The expectation is what pyarrow READS.

The dictionary sits in LDS up to FDB_PQ_DICT_LDS_ENTRIES = 4 096 entries (fdb_kernels.h) and is read from global memory above that;
both placements are covered."""
import io

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq
import pytest

from frostdb_amd.logicalplan import Col, Count, Max, Min, Sum
from tests.parquet_util import row_group_chunks, write_parquet
from tests.test_gpu_parity import assert_same_result, run_oracle
from tests.util import arrow_to_pydict

pytestmark = pytest.mark.gpu

FDB_PQ_DICT_LDS_ENTRIES = 4096
SPECIAL_DOUBLES = np.array([0.0, -0.0, np.nan, np.inf, -np.inf, 1.5, 5e-324])


@pytest.fixture(scope="module")
def pp():
    from frostdb_amd import physicalplan
    assert physicalplan.device_count() >= 1
    return physicalplan


def raw64(arr: pa.Array):
    """(uint64 view of the values, validity) of an 8-byte Arrow column, straight from its buffers."""
    assert arr.type in (pa.int64(), pa.uint64(), pa.float64()), arr.type
    n = len(arr)
    vals = np.frombuffer(arr.buffers()[1], dtype=np.uint64, count=n, offset=arr.offset * 8) if n else np.zeros(0, np.uint64)
    valid = ~np.asarray(arr.is_null()) if n else np.zeros(0, bool)
    return vals, valid


def numeric_columns_equal_pyarrow(rb, data, rg, rows, names=None):
    got = rb.to_arrow()
    want = pq.ParquetFile(io.BytesIO(data)).read_row_group(rg)
    assert got.num_rows == want.num_rows == rows
    assert got.schema.names == want.schema.names
    checked = 0
    for name in want.schema.names:
        w = want.column(name).combine_chunks()
        if w.type not in (pa.int64(), pa.uint64(), pa.float64()):
            continue
        if names is not None and name not in names:
            continue
        g = got.column(name)
        g = g.combine_chunks() if isinstance(g, pa.ChunkedArray) else g
        assert g.type == w.type, (name, g.type, w.type)
        gv, gok = raw64(g)
        wv, wok = raw64(w)
        assert np.array_equal(gok, wok), name                  # the NULL position of every row
        assert np.array_equal(gv[gok], wv[wok]), name          # the bits of every valid row
        checked += 1
    assert checked > 0
    return want


def decode_and_compare(pp, data, rg=0, names=None):
    chunks, rows = row_group_chunks(data, rg)
    rb = pp.ResidentBatch.from_parquet(chunks, rows)
    try:
        return numeric_columns_equal_pyarrow(rb, data, rg, rows, names)
    finally:
        rb.close()


def numeric_chunks_have_dictionaries(data, names):
    md = pq.ParquetFile(io.BytesIO(data)).metadata
    for rg in range(md.num_row_groups):
        for j in range(md.row_group(rg).num_columns):
            col = md.row_group(rg).column(j)
            if col.path_in_schema in names:
                assert col.has_dictionary_page and "RLE_DICTIONARY" in col.encodings, (col.path_in_schema, col.encodings)
    return md


def edge_table(rng, n):
    doubles500 = rng.normal(size=500)
    return pa.table({
        "opt100": pa.array(rng.integers(-10**15, 10**15, 100)[rng.integers(0, 100, n)], mask=rng.random(n) < 0.1),
        "runs": pa.array(np.repeat(rng.integers(-10**6, 10**6, n // 100 + 1), 100)[:n].astype(np.int64)),
        "const": pa.array(np.full(n, -42, dtype=np.int64)),
        "none": pa.array([None] * n, type=pa.int64()),
        "big": pa.array((rng.integers(0, 37, n).astype(np.uint64) * np.uint64(3)) + np.uint64(2**63 + 5)),
        "special": pa.array(SPECIAL_DOUBLES[rng.integers(0, len(SPECIAL_DOUBLES), n)]),
        "d500": pa.array(doubles500[rng.integers(0, 500, n)], mask=rng.random(n) < 0.07),
    }, schema=pa.schema([pa.field("opt100", pa.int64()), pa.field("runs", pa.int64(), nullable=False), pa.field("const", pa.int64(), nullable=False),
                         pa.field("none", pa.int64()), pa.field("big", pa.uint64(), nullable=False), pa.field("special", pa.float64(), nullable=False),
                         pa.field("d500", pa.float64())]))


EDGE_NAMES = ("opt100", "runs", "const", "none", "big", "special", "d500")


@pytest.mark.parametrize("version", ["1.0", "2.0"])
@pytest.mark.parametrize("n", [1, 31, 32, 33, 1000, 65_537, 400_003])
def test_dictionary_encoded_numeric_columns_are_bit_identical_to_pyarrow(pp, n, version):
    """Low-cardinality optional INT64, RLE runs, a constant column (bit width 0), an all-NULL column, uint64 above 2^63, the special
    doubles (±0, NaN, ±Inf, the smallest subnormal) and 500 distinct doubles with NULLs; small pages, so a chunk has many."""
    rng = np.random.default_rng(n)
    data = write_parquet(edge_table(rng, n), use_dictionary=True, data_page_version=version, data_page_size=4096 if n < 100_000 else 8192)
    numeric_chunks_have_dictionaries(data, EDGE_NAMES)
    decode_and_compare(pp, data)


@pytest.mark.parametrize("limit", [16 * 1024, None], ids=["limit16k", "default_limit"])
def test_fallback_to_plain_pages_inside_a_chunk(pp, limit):
    """200 000 random int64 over the full range: the writer gives up on its dictionary half way through the chunk and goes on with
    PLAIN pages — one chunk, both kinds of page, one kernel."""
    rng = np.random.default_rng(7)
    n = 200_000
    t = pa.table({"wild": pa.array(rng.integers(-2**63, 2**63 - 1, n, dtype=np.int64)),
                  "wild_opt": pa.array(rng.integers(-2**63, 2**63 - 1, n, dtype=np.int64), mask=rng.random(n) < 0.2)},
                 schema=pa.schema([pa.field("wild", pa.int64(), nullable=False), pa.field("wild_opt", pa.int64())]))
    kw = dict(dictionary_pagesize_limit=limit) if limit else {}
    data = write_parquet(t, use_dictionary=True, data_page_size=64 * 1024, **kw)
    if limit:
        col = numeric_chunks_have_dictionaries(data, ("wild", "wild_opt")).row_group(0).column(0)
        # more than a dictionary page plus indices of any width up to 32 bits could take: PLAIN pages exist
        assert col.total_compressed_size > limit + 4 * n, col.total_compressed_size
    decode_and_compare(pp, data)
    for codec, version in (("SNAPPY", "1.0"), ("ZSTD", "2.0")):
        decode_and_compare(pp, write_parquet(t, use_dictionary=True, data_page_size=64 * 1024, compression=codec, data_page_version=version, **kw))


@pytest.mark.parametrize("distinct", [5, FDB_PQ_DICT_LDS_ENTRIES - 96, FDB_PQ_DICT_LDS_ENTRIES, FDB_PQ_DICT_LDS_ENTRIES + 1, 60_000])
def test_both_dictionary_placements(pp, distinct):
    """The dictionary in LDS (≤ FDB_PQ_DICT_LDS_ENTRIES = 4 096 entries) and in global memory (above it; 60 000 distinct doubles need
    the writer's dictionary page limit raised to 2 MiB) — same assertions, and the threshold itself from both sides."""
    rng = np.random.default_rng(distinct)
    n = 300_000
    vals = rng.normal(size=distinct)
    ints = rng.integers(-2**62, 2**62, distinct)
    pick = np.concatenate([np.arange(distinct), rng.integers(0, distinct, n - distinct)])  # every entry occurs
    rng.shuffle(pick)
    t = pa.table({"d": pa.array(vals[pick], mask=rng.random(n) < 0.05), "i": pa.array(ints[pick])},
                 schema=pa.schema([pa.field("d", pa.float64()), pa.field("i", pa.int64(), nullable=False)]))
    data = write_parquet(t, use_dictionary=True, dictionary_pagesize_limit=2 << 20, data_page_size=32 * 1024, row_group_size=n)
    md = numeric_chunks_have_dictionaries(data, ("d", "i"))
    assert set(md.row_group(0).column(1).encodings) <= {"PLAIN", "RLE", "RLE_DICTIONARY"}
    # no fallback: dictionary page + 17-bit indices is far less than 8 bytes per row
    assert md.row_group(0).column(1).total_compressed_size < 8 * distinct + 3 * n + 65_536
    decode_and_compare(pp, data)


@pytest.mark.parametrize("version", ["1.0", "2.0"])
@pytest.mark.parametrize("codec", ["SNAPPY", "GZIP", "ZSTD", "LZ4"])
def test_compressed_dictionary_encoded_chunks(pp, codec, version):
    """The dictionary page is inflated into the chunk's image with the data pages; offsets then point into the image. Two row groups,
    one per call and both through one call."""
    rng = np.random.default_rng(len(codec) + len(version))
    data = write_parquet(edge_table(rng, 120_001), use_dictionary=True, compression=codec, data_page_version=version, data_page_size=16 * 1024, row_group_size=70_000)
    numeric_chunks_have_dictionaries(data, EDGE_NAMES)
    groups = [row_group_chunks(data, rg) for rg in range(2)]
    for rg in range(2):
        assert {c[5] for c in groups[rg][0]} == {codec}
        decode_and_compare(pp, data, rg)
    rbs = pp.ResidentBatch.from_parquet_many(groups)
    try:
        for rg, rb in enumerate(rbs):
            numeric_columns_equal_pyarrow(rb, data, rg, groups[rg][1])
    finally:
        for rb in rbs:
            rb.close()


def test_the_decoded_batch_feeds_the_aggregate_like_a_plain_one(pp):
    """cfg 2's query shape over the dictionary-encoded file = the oracle over pyarrow's reading of it = the same query over the same
    table written with PLAIN numeric pages (bit for bit: counts, MIN / MAX, int64 sums; float64 sums within the suite's 1e-9)."""
    rng = np.random.default_rng(11)
    n = 300_000
    paths = [b"/api/v1/p%04d" % i for i in range(300)]
    t = pa.table({
        "labels.code": pa.array([None if rng.random() < 0.01 else c for c in np.array([b"200", b"404", b"500"], dtype=object)[rng.integers(0, 3, n)]], type=pa.binary()),
        "labels.path": pa.array([None if m else paths[i] for i, m in zip(rng.integers(0, 300, n), rng.random(n) < 0.02)], type=pa.binary()),
        "latency": pa.array(rng.integers(0, 2_000, n).astype(np.int64) * 250, mask=rng.random(n) < 0.03),
        "value": pa.array(np.round(rng.uniform(0, 1000, n), 1), mask=rng.random(n) < 0.05),
    })
    filt = Col("labels.code") == "200"
    aggs, groups = [Sum(Col("value")), Count(Col("value")), Min(Col("latency")), Max(Col("latency")), Sum(Col("latency"))], [Col("labels.path")]
    cols = ["labels.path", "sum(value)", "count(value)", "min(latency)", "max(latency)", "sum(latency)"]

    def query(data):
        plan = pp.HashAggregatePlan(filt, aggs, groups)
        keep = []
        try:
            keep = pp.ResidentBatch.from_parquet_many([row_group_chunks(data, rg) for rg in range(3)])
            plan.CallbackResident(keep)
            return arrow_to_pydict(plan.Finish())
        finally:
            plan.Close()
            for k in keep:
                k.close()

    as_dict = write_parquet(t, use_dictionary=True, row_group_size=100_000)
    as_plain = write_parquet(t, row_group_size=100_000)
    numeric_chunks_have_dictionaries(as_dict, ("latency", "value"))
    md = pq.ParquetFile(io.BytesIO(as_plain)).metadata.row_group(0)
    assert not any(md.column(j).has_dictionary_page for j in range(md.num_columns) if md.column(j).path_in_schema in ("latency", "value"))
    got, plain = query(as_dict), query(as_plain)
    recs = [pq.ParquetFile(io.BytesIO(as_dict)).read_row_group(rg).to_batches()[0] for rg in range(3)]
    assert_same_result(got, run_oracle(recs, filt, aggs, groups), cols, float_cols={"sum(value)"})
    assert_same_result(got, plain, cols, float_cols={"sum(value)"})


def test_an_index_beyond_the_dictionary_is_an_error_code(pp):
    """Uncompressed V1 chunk, a dictionary of 5 entries (bit width 3), the values cycle so that every index run is bit-packed: one
    byte of the last run set to 0xFF holds at least two whole 3-bit indices = 7 ≥ 5. The kernel compares every index with the
    dictionary's length before it addresses anything, writes 0 and raises the call's flag: FDB_ERR_INVALID naming the column, and the
    next well-formed call on the device works."""
    n = 4096
    five = np.array([10, -20, 30, -40, 2**62], dtype=np.int64)
    t = pa.table({"ok": pa.array(np.arange(n, dtype=np.int64) % 3), "victim": pa.array(five[np.arange(n) % 5])},
                 schema=pa.schema([pa.field("ok", pa.int64(), nullable=False), pa.field("victim", pa.int64(), nullable=False)]))
    data = write_parquet(t, use_dictionary=True, data_page_version="1.0")
    md = numeric_chunks_have_dictionaries(data, ("ok", "victim")).row_group(0).column(1)
    assert md.compression == "UNCOMPRESSED" and md.data_page_offset - md.dictionary_page_offset >= 5 * 8
    chunks, rows = row_group_chunks(data, 0)
    decode_and_compare(pp, data)
    nm, ty, opt, u8, b, cd = chunks[1]
    assert nm == "victim" and len(b) > 5 * 8 + n * 3 // 8
    hurt = bytearray(b)
    hurt[-2] = 0xFF
    with pytest.raises(pp.FdbError) as e:
        pp.ResidentBatch.from_parquet([chunks[0], (nm, ty, opt, u8, bytes(hurt), cd)], rows)
    assert e.value.code == pp.FDB_ERR_INVALID and "victim" in str(e.value), str(e.value)
    with pytest.raises(pp.FdbError) as e:
        pp.ResidentBatch.from_parquet_many([(chunks, rows), ([chunks[0], (nm, ty, opt, u8, bytes(hurt), cd)], rows)])
    assert e.value.code == pp.FDB_ERR_INVALID and "victim" in str(e.value), str(e.value)
    decode_and_compare(pp, data)


def test_nothing_is_left_allocated(pp):
    import gc
    gc.collect()
    assert pp.live_allocations()["device_blocks"] == 0
