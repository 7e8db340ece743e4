"""Dictionary-encoded INT64 / DOUBLE column chunks (what every stock Parquet writer produces by default, and what a FrostDB schema
gets with ENCODING_RLE_DICTIONARY on a numeric column, dynparquet/schema.go:531-560) are parsed on the host before a device is
touched: a well-formed file gets as far as the device call (FDB_ERR_DEVICE on a box without a GPU, a batch on one with), a damaged
chunk is FDB_ERR_INVALID, and what the path does not decode stays FDB_ERR_UNSUPPORTED."""
import io

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq
import pytest

from tests.parquet_util import row_group_chunks, write_parquet

NUMERIC = ("status", "runs", "seq", "ratio", "wild")


def numeric_table(n, seed=1):
    rng = np.random.default_rng(seed)
    return pa.table({
        "labels.a": pa.array([None if i % 9 == 0 else b"v%d" % (i % 13) for i in range(n)], type=pa.binary()),
        "status": pa.array(rng.choice([200, 201, 204, 301, 404, 500, 503], n).astype(np.int64), mask=rng.random(n) < 0.1),  # low cardinality, optional
        "runs": pa.array(np.repeat(np.arange(n // 100 + 1, dtype=np.int64) * 15_000, 100)[:n]),                                # long runs, required
        "seq": pa.array(rng.integers(0, 50, n).astype(np.uint64) + np.uint64(2**63)),                                          # uint64
        "ratio": pa.array(rng.choice([0.0, 0.25, 0.5, 1.5, 99.0], n), mask=rng.random(n) < 0.05),                              # few doubles
        "wild": pa.array(rng.integers(-2**63, 2**63 - 1, n, dtype=np.int64)),                                                  # high cardinality
    }, schema=pa.schema([pa.field("labels.a", pa.binary()), pa.field("status", pa.int64()), pa.field("runs", pa.int64(), nullable=False),
                         pa.field("seq", pa.uint64(), nullable=False), pa.field("ratio", pa.float64()), pa.field("wild", pa.int64(), nullable=False)]))


def assert_numeric_chunks_are_dictionary_encoded(data):
    md = pq.ParquetFile(io.BytesIO(data)).metadata
    for rg in range(md.num_row_groups):
        for j in range(md.row_group(rg).num_columns):
            col = md.row_group(rg).column(j)
            if col.path_in_schema in NUMERIC:
                assert col.has_dictionary_page and "RLE_DICTIONARY" in col.encodings, (col.path_in_schema, col.encodings)
    return md


def parses(pp, call):
    """The parser accepts the input: a batch where there is a GPU, FDB_ERR_DEVICE where there is none — never a parser verdict."""
    if pp.device_count() == 0:
        with pytest.raises(pp.FdbError) as e:
            call()
        assert e.value.code == pp.FDB_ERR_DEVICE, str(e.value)
        return
    out = call()
    for rb in (out if isinstance(out, list) else [out]):
        rb.close()


@pytest.mark.parametrize("kw", [dict(), dict(dictionary_pagesize_limit=16 * 1024), dict(data_page_version="2.0"), dict(compression="SNAPPY"),
                                dict(compression="ZSTD", data_page_version="2.0"), dict(compression="SNAPPY", dictionary_pagesize_limit=16 * 1024)],
                         ids=["plain", "fallback", "v2", "snappy", "zstd_v2", "snappy_fallback"])
def test_dictionary_encoded_numeric_chunks_get_past_the_parser(kw):
    from frostdb_amd import physicalplan as pp
    n = 20_000
    data = write_parquet(numeric_table(n), use_dictionary=True, data_page_size=8 * 1024, row_group_size=12_000, **kw)
    md = assert_numeric_chunks_are_dictionary_encoded(data)
    assert md.num_row_groups == 2
    if "dictionary_pagesize_limit" in kw:  # 12 000 distinct int64 values do not fit a 16 KiB dictionary: PLAIN pages follow the indexed ones
        wild = [md.row_group(0).column(j) for j in range(md.row_group(0).num_columns) if md.row_group(0).column(j).path_in_schema == "wild"][0]
        assert "PLAIN" in wild.encodings and wild.total_uncompressed_size > 16 * 1024 + 4 * 12_000
    groups = [row_group_chunks(data, rg) for rg in range(2)]
    for chunks, rows in groups:
        parses(pp, lambda: pp.ResidentBatch.from_parquet(chunks, rows))
    parses(pp, lambda: pp.ResidentBatch.from_parquet_many(groups))


def test_damaged_numeric_dictionary_chunks_are_invalid_not_a_crash():
    from frostdb_amd import physicalplan as pp
    n = 5_000
    for kw in (dict(), dict(compression="SNAPPY")):
        data = write_parquet(numeric_table(n), use_dictionary=True, data_page_size=4 * 1024, **kw)
        assert_numeric_chunks_are_dictionary_encoded(data)
        chunks, rows = row_group_chunks(data, 0)
        col_md = {pq.ParquetFile(io.BytesIO(data)).metadata.row_group(0).column(j).path_in_schema: pq.ParquetFile(io.BytesIO(data)).metadata.row_group(0).column(j)
                  for j in range(len(chunks))}
        for victim in ("status", "ratio", "wild"):
            m = col_md[victim]
            dict_page_bytes = m.data_page_offset - m.dictionary_page_offset  # header + body of the dictionary page
            assert 8 < dict_page_bytes < m.total_compressed_size
            for what, cut in (("inside the dictionary page", lambda b: b[:dict_page_bytes // 2]), ("dictionary page cut away", lambda b: b[dict_page_bytes:])):
                hurt = [(nm, ty, opt, u8, cut(b) if nm == victim else b, cd) for nm, ty, opt, u8, b, cd in chunks]
                with pytest.raises(pp.FdbError) as e:
                    pp.ResidentBatch.from_parquet(hurt, rows)
                assert e.value.code == pp.FDB_ERR_INVALID, (kw, victim, what, str(e.value))
                with pytest.raises(pp.FdbError) as e:
                    pp.ResidentBatch.from_parquet_many([(chunks, rows), (hurt, rows)])
                assert e.value.code == pp.FDB_ERR_INVALID, (kw, victim, what, str(e.value))


def test_what_stays_refused_stays_refused():
    """DELTA_BINARY_PACKED pages next to pages of another encoding in one chunk: no writer here produces that, but a page chain is
    self-describing, so the chunks of two files laid end to end are such a chunk (first half dictionary-encoded or PLAIN, second half
    DELTA_BINARY_PACKED, and the other way round). A dictionary page on a BOOLEAN chunk and INT32 / FLOAT columns stay refused too."""
    from frostdb_amd import physicalplan as pp
    n = 4_000
    rng = np.random.default_rng(3)
    col = pa.table({"x": pa.array(rng.integers(0, 40, n).astype(np.int64))}, schema=pa.schema([pa.field("x", pa.int64(), nullable=False)]))
    one = lambda **kw: row_group_chunks(write_parquet(col, data_page_size=2048, **kw), 0)[0][0]  # noqa: E731
    as_dict, as_plain, as_delta = one(use_dictionary=True), one(), one(use_dictionary=False, column_encoding={"x": "DELTA_BINARY_PACKED"})
    for first, second in ((as_dict, as_delta), (as_delta, as_dict), (as_plain, as_delta), (as_delta, as_plain)):
        glued = (first[0], first[1], first[2], first[3], first[4] + second[4], first[5])
        with pytest.raises(pp.FdbError) as e:
            pp.ResidentBatch.from_parquet([glued], 2 * n)
        assert e.value.code == pp.FDB_ERR_UNSUPPORTED, str(e.value)
    # … while dictionary-indexed pages followed by PLAIN ones (a writer's fallback) are one decodable chunk
    glued = (as_dict[0], as_dict[1], as_dict[2], as_dict[3], as_dict[4] + as_plain[4], as_dict[5])
    parses(pp, lambda: pp.ResidentBatch.from_parquet([glued], 2 * n))
    flags = pa.table({"flag": pa.array(rng.random(n) < 0.5)})
    data = write_parquet(flags, use_dictionary=True)
    chunks, rows = row_group_chunks(data, 0)
    if pq.ParquetFile(io.BytesIO(data)).metadata.row_group(0).column(0).has_dictionary_page:  # (pyarrow never dictionary-encodes BOOLEAN; kept for writers that do)
        with pytest.raises(pp.FdbError) as e:
            pp.ResidentBatch.from_parquet(chunks, rows)
        assert e.value.code == pp.FDB_ERR_UNSUPPORTED
    # a BOOLEAN chunk that starts with (someone else's) dictionary page
    with pytest.raises(pp.FdbError) as e:
        pp.ResidentBatch.from_parquet([("flag", 0, chunks[0][2], False, as_dict[4][:as_dict_dictionary_bytes(col)] + chunks[0][4], "UNCOMPRESSED")], rows)
    assert e.value.code == pp.FDB_ERR_UNSUPPORTED, str(e.value)
    odd = pa.table({"i32": pa.array(rng.integers(0, 9, n).astype(np.int32)), "f32": pa.array(rng.choice([0.5, 1.5], n).astype(np.float32))})
    for name in ("i32", "f32"):
        bad, rows = row_group_chunks(write_parquet(odd.select([name]), use_dictionary=True), 0)
        with pytest.raises(pp.FdbError) as e:
            pp.ResidentBatch.from_parquet(bad, rows)
        assert e.value.code == pp.FDB_ERR_UNSUPPORTED, (name, str(e.value))


def as_dict_dictionary_bytes(col):
    m = pq.ParquetFile(io.BytesIO(write_parquet(col, data_page_size=2048, use_dictionary=True))).metadata.row_group(0).column(0)
    return m.data_page_offset - m.dictionary_page_offset
