"""The Parquet decode kernels (pq_validity_kernel, pq_decode_kernel, pq_decode_dict8_kernel, pq_delta_kernel) on the hand-laid pages
of tests/parquet_pages.py: DELTA miniblocks of every width and geometry, dictionary indices at every declared width, run and page
shapes no stock writer produces, chunks larger than one launch's grid. The expectation is what pyarrow's READER makes of the same
bytes (tests/test_parquet_pages_cpu.py has already held the builder to it): the NULL position of every row, the uint64 view of every
valid 8-byte value (the DOUBLE cases carry NaN payloads, −0.0 and subnormals), the bytes of every string, the value of every boolean.
No tolerance, no row left out."""
import functools
import io

import pyarrow.parquet as pq
import pytest

from tests import parquet_pages as P
from tests.test_parquet_pages_cpu import same_column

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pp():
    from frostdb_amd import physicalplan
    assert physicalplan.device_count() >= 1
    return physicalplan


@functools.lru_cache(maxsize=None)
def pyarrow_reads(cid, family):
    c = {c.id: c for c in P.cases(family)}[cid]
    return pq.ParquetFile(io.BytesIO(c.file)).read_row_group(0).column(0).combine_chunks()


def batch_equals_pyarrow(rb, c, family):
    got = rb.to_arrow()
    assert got.num_rows == c.rows and got.schema.names == [c.chunk[0]], c.id
    same_column(got.column(0), pyarrow_reads(c.id, family), c.id)


@pytest.mark.parametrize("family", sorted(P.FAMILIES))
def test_every_case_decodes_to_what_pyarrow_reads(pp, family):
    for c in P.cases(family):
        rb = pp.ResidentBatch.from_parquet([c.chunk], c.rows)
        try:
            batch_equals_pyarrow(rb, c, family)
        finally:
            rb.close()


@pytest.mark.parametrize("family", P.MANY_FAMILIES)
def test_three_cases_as_three_row_groups_of_one_call(pp, family):
    cs = P.cases(family)
    for a in range(0, len(cs), 3):
        rbs = pp.ResidentBatch.from_parquet_many([([c.chunk], c.rows) for c in cs[a:a + 3]])
        try:
            assert len(rbs) == len(cs[a:a + 3])
            for rb, c in zip(rbs, cs[a:a + 3]):
                batch_equals_pyarrow(rb, c, family)
        finally:
            for rb in rbs:
                rb.close()


def test_nothing_is_left_allocated(pp):
    import gc
    gc.collect()
    assert pp.live_allocations()["device_blocks"] == 0
