"""LZ4_RAW pages of literals are inflated on the device (fdb_parquet.cpp plan_chunk → lz4_decode_kernel), everything else on the host
as before: the files of tests/test_gpu_parquet.py::test_literal_snappy_pages_are_inflated_on_the_device written with codec 7, counted
page by page against fdb_parquet_device_pages."""
import numpy as np
import pyarrow as pa
import pytest

from tests import lz4_cases
from tests.parquet_util import row_group_chunks, write_parquet

pytestmark = pytest.mark.gpu

LZ4_RAW, SNAPPY = 7, 1


@pytest.fixture(scope="module")
def pp():
    from frostdb_amd import physicalplan
    assert physicalplan.device_count() >= 1
    return physicalplan


def _chunks(data, rg):
    """row_group_chunks with the codec the FOOTER names (pyarrow's metadata API says "LZ4" for codec 5 and codec 7 alike)"""
    chunks, rows = row_group_chunks(data, rg)
    return [c[:5] + ("LZ4_RAW",) for c in chunks], rows


def _equals(got: pa.RecordBatch, want: pa.Table):
    assert got.schema.names == want.schema.names and got.num_rows == want.num_rows
    for name in want.schema.names:
        g, w = got.column(name), want.column(name).combine_chunks()  # (a resident batch exports one record batch: plain arrays)
        if pa.types.is_dictionary(g.type):
            g = g.dictionary_decode()
        assert np.array_equal(np.asarray(g.is_null()), np.asarray(w.is_null())), name
        if pa.types.is_binary(w.type):
            assert g.cast(pa.binary()).equals(w), name
        else:  # bit for bit where a value is present
            ok = ~np.asarray(w.is_null())
            gv, wv = g.to_numpy(zero_copy_only=False), w.to_numpy(zero_copy_only=False)
            assert np.array_equal(np.asarray(gv)[ok].view(np.int64), np.asarray(wv)[ok].view(np.int64)), name


@pytest.mark.parametrize("version", ["1.0", "2.0"])
def test_literal_lz4_raw_pages_are_inflated_on_the_device(pp, version, monkeypatch):
    """Random int64 / float64 values do not compress: their 1 MiB PLAIN pages are a few LZ4 sequences each and meet the gate (V1 and V2,
    required and optional — V1: the definition levels sit inside the compressed body, the host inflates just them); the int64 ramp of
    `timestamp` compresses to a half and stays on the host, like the dictionary indices of `labels.path`. Bit-identical to pyarrow's
    reader and to the all-host path; the device's page counter rises by exactly the pages that meet the gate."""
    rng = np.random.default_rng(77)
    n = 700_000

    def runs(v):  # 4 % of the values in runs of 80 equal ones: a page of literal stretches with a match between them, ≈ 0.96 of its plain size
        v = v.copy()
        for i in range(0, len(v) - 80, 2000):
            v[i:i + 80] = v[i]
        return v
    t = pa.table({
        "labels.path": pa.array([b"/p%03d" % i for i in rng.integers(0, 300, n)], type=pa.binary()),
        "timestamp": pa.array(1_700_000_000_000 + np.arange(n, dtype=np.int64) * 15),          # compressible: stays on the host
        "noise_req": pa.array(rng.integers(-2**62, 2**62, n)),                                    # one sequence of literals per page, required
        "noise_opt": pa.array(runs(rng.integers(-2**62, 2**62, n)), mask=rng.random(n) < 0.1),   # 10 % NULLs (bit-packed levels)
        "value": pa.array(runs(rng.uniform(0, 1000, n)), mask=rng.random(n) < 0.001),            # rare NULLs (RLE + bit-packed levels)
        "value_req": pa.array(runs(rng.uniform(0, 1000, n))),
    }, schema=pa.schema([pa.field("labels.path", pa.binary()), pa.field("timestamp", pa.int64(), nullable=False), pa.field("noise_req", pa.int64(), nullable=False),
                         pa.field("noise_opt", pa.int64()), pa.field("value", pa.float64()), pa.field("value_req", pa.float64(), nullable=False)]))
    data = write_parquet(t, compression="LZ4_RAW", data_page_version=version, data_page_size=1 << 20, row_group_size=400_000)
    assert set(lz4_cases.footer_codecs(data)) == {LZ4_RAW}
    for rg in range(2):
        chunks, rows = _chunks(data, rg)
        want = lz4_cases.read_row_group(data, rg)
        gate = {c[0]: lz4_cases.pages_for_the_device(c[4], c[1]) for c in chunks}  # per column: the body sizes of the pages that meet the gate
        assert gate["timestamp"] == [] and gate["labels.path"] == [], gate
        assert all(len(gate[k]) > 0 for k in ("noise_opt", "value", "value_req")), gate
        # (pure noise grows under LZ4: a V1 page carries it compressed all the same, a V2 page says "not compressed" and is copied as it is)
        assert (len(gate["noise_req"]) > 0) == (version == "1.0"), gate
        monkeypatch.delenv("FDB_PARQUET_HOST_INFLATE", raising=False)
        before, snappy_before = pp.parquet_device_pages(LZ4_RAW), pp.parquet_device_pages(SNAPPY)
        rb = pp.ResidentBatch.from_parquet(chunks, rows)
        dev = rb.to_arrow()
        rb.close()
        after = pp.parquet_device_pages("LZ4_RAW")
        assert after["pages"] - before["pages"] == sum(len(v) for v in gate.values()), (gate, before, after)
        assert after["bytes"] - before["bytes"] == sum(sum(v) for v in gate.values())
        assert pp.parquet_device_pages(SNAPPY) == snappy_before
        _equals(dev, want)
        monkeypatch.setenv("FDB_PARQUET_HOST_INFLATE", "1")
        rb2 = pp.ResidentBatch.from_parquet(chunks, rows)
        host = rb2.to_arrow()
        rb2.close()
        assert pp.parquet_device_pages(LZ4_RAW) == after  # every page on the host this time
        assert host.equals(dev)
    # both row groups by one call
    monkeypatch.delenv("FDB_PARQUET_HOST_INFLATE", raising=False)
    before = pp.parquet_device_pages(LZ4_RAW)
    groups = [_chunks(data, rg) for rg in range(2)]
    rbs = pp.ResidentBatch.from_parquet_many(groups)
    for rg, rb in enumerate(rbs):
        _equals(rb.to_arrow(), lz4_cases.read_row_group(data, rg))
        rb.close()
    assert pp.parquet_device_pages(LZ4_RAW)["pages"] - before["pages"] == sum(len(lz4_cases.pages_for_the_device(c[4], c[1])) for ch, _ in groups for c in ch)
    assert pp.live_allocations()["device_blocks"] == 0


def test_snappy_pages_are_counted_too(pp, monkeypatch):
    monkeypatch.delenv("FDB_PARQUET_HOST_INFLATE", raising=False)
    rng = np.random.default_rng(4)
    n = 100_000
    t = pa.table({"value": pa.array(rng.uniform(0, 1000, n))}, schema=pa.schema([pa.field("value", pa.float64(), nullable=False)]))
    data = write_parquet(t, compression="SNAPPY", data_page_size=256 << 10)
    chunks, rows = row_group_chunks(data, 0)
    want = len(lz4_cases.pages_for_the_device(chunks[0][4], chunks[0][1]))
    assert want > 0
    before, lz4_before = pp.parquet_device_pages(SNAPPY), pp.parquet_device_pages(LZ4_RAW)
    rb = pp.ResidentBatch.from_parquet(chunks, rows)
    assert rb.to_arrow().column("value").to_numpy().tobytes() == t.column("value").to_numpy().tobytes()
    rb.close()
    after = pp.parquet_device_pages(SNAPPY)
    assert after["pages"] - before["pages"] == want and after["bytes"] - before["bytes"] == n * 8
    assert pp.parquet_device_pages(LZ4_RAW) == lz4_before


def _literal_page(raw: bytes, at: int, far: int, length: int = 64) -> bytes:
    """raw as two sequences: literals up to `at`, a match of `length` bytes from `far` bytes back, the rest as literals"""
    return lz4_cases.seq(raw[:at], length, far) + lz4_cases.seq(raw[at + length:])


@pytest.mark.parametrize("far", [65_535, lz4_cases.RING_REACH + 1, lz4_cases.RING_REACH])
def test_lz4_pages_with_matches_from_far_back_take_the_host_path(pp, far, monkeypatch):
    """A legal LZ4 page whose one match reaches further back than the 64 KiB ring of the device's decoder keeps (offset > 65 472; LZ4
    offsets go up to 65 535): plan_chunk's token walk leaves it to the host and the row group loads, bit-identical to the values the page
    was built from. At 65 472 itself the page goes to the device."""
    monkeypatch.delenv("FDB_PARQUET_HOST_INFLATE", raising=False)
    rng = np.random.default_rng(5)
    n = 60_000                                      # 480 000 bytes of PLAIN doubles: they do not compress
    raw = bytearray(rng.uniform(0, 1000, n).tobytes())
    at = 300_000
    raw[at:at + 64] = raw[at - far:at - far + 64]
    raw = bytes(raw)
    body = _literal_page(raw, at, far)
    assert pa.Codec("lz4_raw").decompress(body, decompressed_size=len(raw), asbytes=True) == raw  # (the page is what the test thinks it is)
    chunk = lz4_cases.page_header_v1(n, len(raw), len(body)) + body
    assert len(lz4_cases.pages_for_the_device(chunk, 5)) == 1  # (sizes alone would send it to the device)
    before = pp.parquet_device_pages(LZ4_RAW)
    rb = pp.ResidentBatch.from_parquet([("value", 5, 0, False, chunk, "LZ4_RAW")], n)
    got = rb.to_arrow().column("value").to_numpy(zero_copy_only=False)
    rb.close()
    assert got.tobytes() == raw
    assert pp.parquet_device_pages(LZ4_RAW)["pages"] - before["pages"] == (1 if far <= lz4_cases.RING_REACH else 0)
    assert pp.live_allocations()["device_blocks"] == 0


def test_a_corrupt_literal_lz4_page_is_invalid_and_leaves_nothing_behind(pp, monkeypatch):
    """A page of literals whose token walk is sound (so it goes to the device) but whose match points before the page's first byte: the
    device's verdict comes back as FDB_ERR_INVALID, no batch, no device allocation."""
    monkeypatch.delenv("FDB_PARQUET_HOST_INFLATE", raising=False)
    rng = np.random.default_rng(6)
    n = 60_000
    raw = rng.uniform(0, 1000, n).tobytes()
    body = lz4_cases.seq(raw[:1000], 64, 1001) + lz4_cases.seq(raw[1064:])  # offset 1001 with 1000 bytes of output
    chunk = lz4_cases.page_header_v1(n, len(raw), len(body)) + body
    good = lz4_cases.page_header_v1(n, len(raw), len(_literal_page(raw, 1000, 1000))) + _literal_page(raw, 1000, 1000)
    before = pp.parquet_device_pages(LZ4_RAW)
    with pytest.raises(pp.FdbError) as e:
        pp.ResidentBatch.from_parquet([("fine", 5, 0, False, good, "LZ4_RAW"), ("value", 5, 0, False, chunk, "LZ4_RAW")], n)
    assert e.value.code == pp.FDB_ERR_INVALID and "corrupt LZ4 page in column value" in str(e.value), str(e.value)
    assert pp.parquet_device_pages(LZ4_RAW) == before  # a call that failed counts nothing
    assert pp.live_allocations()["device_blocks"] == 0
    # the same page on the host's threads: refused there too
    monkeypatch.setenv("FDB_PARQUET_HOST_INFLATE", "1")
    with pytest.raises(pp.FdbError) as e:
        pp.ResidentBatch.from_parquet([("value", 5, 0, False, chunk, "LZ4_RAW")], n)
    assert e.value.code == pp.FDB_ERR_INVALID and "corrupt LZ4 page" in str(e.value)
    assert pp.live_allocations()["device_blocks"] == 0
