"""The hand-laid Parquet pages of tests/parquet_pages.py, before any of them goes to a device: pyarrow's reader — which knows nothing
of the builder — reads every case's file back to exactly the values and NULLs the case was built from (so the bytes are valid
Parquet and mean what the builder says), and the library's host walk (page headers, run headers, DELTA block headers) accepts every
chunk: a batch where there is a GPU, FDB_ERR_DEVICE where there is none, never a parser verdict. Two malformed chunks are refused by
both."""
import io

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq
import pytest

from tests import parquet_pages as P
from tests.test_gpu_parquet_numeric_dict import raw64
from tests.test_parquet_numeric_dict_cpu import parses

FAMILIES = sorted(P.FAMILIES)


def same_column(got, want, cid):
    """Row for row: the NULL positions, and the bits (8-byte types), bytes (strings) or values (booleans) of every valid row."""
    got = got.combine_chunks() if isinstance(got, pa.ChunkedArray) else got
    if pa.types.is_dictionary(got.type):
        got = got.dictionary_decode()
    assert len(got) == len(want), cid
    if want.type in (pa.int64(), pa.uint64(), pa.float64()):
        assert got.type == want.type, (cid, got.type, want.type)
        gv, gok = raw64(got)
        wv, wok = raw64(want)
        assert np.array_equal(gok, wok), f"{cid}: NULL positions differ, first at row {int(np.flatnonzero(gok != wok)[0])}"
        bad = np.flatnonzero((gv != wv) & wok)
        assert len(bad) == 0, f"{cid}: {len(bad)} rows differ, first at row {int(bad[0])}: {int(gv[bad[0]]):#018x} for {int(wv[bad[0]]):#018x}"
    elif pa.types.is_boolean(want.type):
        assert got.type == want.type and np.array_equal(np.asarray(got.is_null()), np.asarray(want.is_null())), cid
        assert got.equals(want), cid
    else:
        assert np.array_equal(np.asarray(got.is_null()), np.asarray(want.is_null())), cid
        assert got.cast(pa.binary()).equals(want.cast(pa.binary())), cid


@pytest.mark.parametrize("family", FAMILIES)
def test_pyarrow_reads_every_case_back_to_what_it_was_built_from(family):
    seen = set()
    for c in P.cases(family):
        assert c.id not in seen and c.id.startswith(family + "/"), c.id
        seen.add(c.id)
        table = pq.ParquetFile(io.BytesIO(c.file)).read_row_group(0)
        assert table.num_rows == c.rows == len(c.expect) and table.schema.names == [c.chunk[0]], c.id
        got = table.column(0).combine_chunks()
        assert got.type == c.expect.type, (c.id, got.type, c.expect.type)
        same_column(got, c.expect, c.id)
    assert seen


@pytest.mark.parametrize("family", FAMILIES)
def test_the_host_walk_accepts_every_case(family):
    from frostdb_amd import physicalplan as pp
    cs = P.cases(family)
    for c in cs:
        parses(pp, lambda: pp.ResidentBatch.from_parquet([c.chunk], c.rows))
    small = [c for c in cs if c.rows < 100_000]
    for a in range(0, len(small), 3):
        parses(pp, lambda: pp.ResidentBatch.from_parquet_many([([c.chunk], c.rows) for c in small[a:a + 3]]))
    for c in cs:
        if c.rows >= 100_000:
            parses(pp, lambda: pp.ResidentBatch.from_parquet_many([([c.chunk], c.rows)]))


def test_the_case_list_is_what_the_families_promise():
    count = {f: len(P.cases(f)) for f in P.FAMILIES}
    assert count == {"delta_widths": 65 + 5 * 8 + 3, "delta_shapes": 26, "dict8_widths": 33 * 4 + 6, "dict8_shapes": 7, "string_widths": 64,
                     "levels": 42, "booleans": 28, "v2_uncompressed": 4, "grid_stride": 2}, count
    again = P.FAMILIES["levels"]()
    assert all(a.chunk == b.chunk and a.file == b.file for a, b in zip(again, P.cases("levels")))  # seeded: the same bytes every time


def test_malformed_pages_are_refused_by_pyarrow_and_by_the_library():
    from frostdb_amd import physicalplan as pp
    good = P.cases("delta_shapes")[2]
    for cid, chunk, rows, dictionary_bytes in P.refusals():
        with pytest.raises((OSError, pa.ArrowException)):
            pq.ParquetFile(io.BytesIO(P.file_of(chunk, rows, dictionary_bytes))).read_row_group(0)
        with pytest.raises(pp.FdbError) as e:
            pp.ResidentBatch.from_parquet([chunk], rows)
        assert e.value.code == pp.FDB_ERR_INVALID, (cid, str(e.value))
        with pytest.raises(pp.FdbError) as e:
            pp.ResidentBatch.from_parquet_many([([good.chunk], good.rows), ([chunk], rows)])
        assert e.value.code == pp.FDB_ERR_INVALID, (cid, str(e.value))
        parses(pp, lambda: pp.ResidentBatch.from_parquet([good.chunk], good.rows))  # the next well-formed call works
