"""The library's built-in LZ4 block decoder (fdb_codec.cpp lz4_raw, reached through fdb_lz4_decode_pages with device < 0: no GPU is
touched), and the Parquet path's use of it where liblz4 is not installed ($FDB_PARQUET_BUILTIN_LZ4 hides it): bit-identical to pyarrow's
lz4_raw codec on compressor output and on hand-made streams that only the format allows; damaged pages refused one by one."""
import os
import subprocess
import sys

import numpy as np
import pyarrow as pa
import pytest

from tests import lz4_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def pp():
    from frostdb_amd import physicalplan
    return physicalplan


def test_host_lz4_equals_the_codec(pp):
    codec = pa.Codec("lz4_raw")
    plain = lz4_cases.payloads()
    comp = [codec.compress(p, asbytes=True) for p in plain]
    out, status, ms = pp.lz4_decode_pages(comp, [len(p) for p in plain], device=-1)
    assert status == [0] * len(plain), status
    assert ms == 0.0
    for i, (a, b) in enumerate(zip(out, plain)):
        assert a == b, (i, len(b))
    for i, (c, p) in enumerate(zip(comp, plain)):  # every page alone, too
        o, st, _ = pp.lz4_decode_pages([c], [len(p)], device=-1)
        assert st == [0] and o[0] == p, i


def test_host_lz4_hand_made_sequences(pp):
    """Lengths that end exactly on a 255 boundary, patterns of period 1 … 9 longer than 64 bytes, a match whose source ends where its
    destination starts, offset 65 535 — the host decoder takes all of them (the device leaves the last kind to it)."""
    cases = lz4_cases.hand_made()
    lz4_cases.check_hand_made(cases)
    assert any(far for *_, far in cases)
    out, status, _ = pp.lz4_decode_pages([c for _, c, _, _ in cases], [len(p) for _, _, p, _ in cases], device=-1)
    assert status == [0] * len(cases), [n for (n, *_), s in zip(cases, status) if s]
    for (name, _, plain, _), got in zip(cases, out):
        assert got == plain, name
    for name, c, p, _ in cases:
        o, st, _ = pp.lz4_decode_pages([c], [len(p)], device=-1)
        assert st == [0] and o[0] == p, name


def test_host_lz4_refuses_damaged_pages_one_by_one(pp):
    c, plain = lz4_cases.good()
    bad = lz4_cases.damaged()
    pages, sizes = [c], [len(plain)]
    for _, stream, announced, _ in bad:
        pages += [stream, c]; sizes += [announced, len(plain)]
    out, status, _ = pp.lz4_decode_pages(pages, sizes, device=-1)
    assert all(s == 0 and o == plain for s, o in zip(status[0::2], out[0::2])), status
    for (name, _, _, codes), s, o in zip(bad, status[1::2], out[1::2]):  # the codes the device's decoder gives: what failed first
        assert s in codes and o is None, (name, s)


def test_pages_outside_the_buffers_are_an_error_not_a_read(pp):
    import ctypes
    src = np.frombuffer(lz4_cases.seq(b"0123456789abcdef"), dtype=np.uint8).copy()
    dst = np.zeros(16, dtype=np.uint8)
    status = np.zeros(1, dtype=np.uint32)
    for so, do, sl, dl in ((0, 0, len(src) + 1, 16), (0, 0, len(src), 17), (2, 0, len(src) - 1, 16), (0, 1, len(src), 16)):
        table = np.array([[so, do, sl | (dl << 32)]], dtype=np.uint64)
        rc = pp.lib().fdb_lz4_decode_pages(src.ctypes.data, len(src), table.ctypes.data, 1, dst.ctypes.data, 16, -1, status.ctypes.data, ctypes.byref(ctypes.c_double()))
        assert rc == pp.FDB_ERR_INVALID, (so, do, sl, dl)


def test_device_page_counter_starts_per_codec(pp):
    for codec in (1, 7, "SNAPPY", "LZ4_RAW"):
        got = pp.parquet_device_pages(codec)
        assert set(got) == {"pages", "bytes"} and got["pages"] >= 0
    with pytest.raises(pp.FdbError) as e:
        pp.parquet_device_pages(8)
    assert e.value.code == pp.FDB_ERR_INVALID


_PARQUET_CHILD = r"""
import io, sys
import numpy as np, pyarrow as pa, pyarrow.parquet as pq
from frostdb_amd import physicalplan as pp
from tests import lz4_cases
from tests.parquet_util import row_group_chunks, write_parquet

def verdict(chunks, rows):
    # a batch where there is a GPU, FDB_ERR_DEVICE where there is none: the host part (headers, inflate, parse) is done by then
    try:
        rb = pp.ResidentBatch.from_parquet(chunks, rows)
    except pp.FdbError as e:
        return e.code, str(e), None
    t = rb.to_arrow(); rb.close()
    return 0, "", t

def same(got, data):  # a resident batch exports one record batch; pyarrow's reader a table
    want = lz4_cases.read_row_group(data, 0)
    assert got.schema.names == want.schema.names
    for name in want.schema.names:
        assert got.column(name).to_pylist() == want.column(name).to_pylist(), name

rng = np.random.default_rng(2)
n = 30_000
t = pa.table({"ts": pa.array(1_700_000_000_000 + np.arange(n, dtype=np.int64) * 15), "idx": pa.array(rng.integers(0, 5, n)),
              "value": pa.array(np.round(rng.uniform(0, 10, n), 1), mask=rng.random(n) < 0.1)})
for version in ("1.0", "2.0"):
    data = write_parquet(t, compression="LZ4_RAW", data_page_version=version, data_page_size=16 << 10)
    assert set(lz4_cases.footer_codecs(data)) == {7}
    chunks, rows = row_group_chunks(data, 0)
    chunks = [c[:5] + ("LZ4_RAW",) for c in chunks]
    code, msg, got = verdict(chunks, rows)
    assert code in (0, pp.FDB_ERR_DEVICE), (code, msg)
    if got is not None:
        same(got, data)
    # the same pages behind Hadoop's frames (the deprecated codec 5): [uncompressed size BE32][compressed size BE32][block], here two per page
    codec = pa.Codec("lz4_raw")
    if version == "1.0":
        vals = t.column("ts").to_numpy().tobytes()
        half = len(vals) // 2 // 8 * 8
        body = b"".join(len(p).to_bytes(4, "big") + len(c).to_bytes(4, "big") + c for p in (vals[:half], vals[half:]) for c in [codec.compress(p, asbytes=True)])
        chunk = lz4_cases.page_header_v1(n, len(vals), len(body)) + body
        code, msg, got = verdict([("ts", 2, 0, False, chunk, "LZ4")], n)
        assert code in (0, pp.FDB_ERR_DEVICE), (code, msg)
        if got is not None:
            assert got.column("ts").to_numpy().tobytes() == vals
    # a damaged page is the parser's to refuse, whichever decoder inflates it
    bad = []
    for c in chunks:
        if c[0] == "ts":
            pg = lz4_cases.chunk_pages(c[4])[0]
            b = bytearray(c[4])
            b[pg["at"] + pg["prefix"]] = 0x0F  # the page now starts with a match: nothing to copy from
            c = c[:4] + (bytes(b), c[5])
        bad.append(c)
    code, msg, _ = verdict(bad, rows)
    assert code == pp.FDB_ERR_INVALID and "corrupt LZ4 page" in msg, (code, msg)
# pages of literals big enough for the device: the host walks their tokens (lz4_device_ok) and inflates only the definition levels at the
# head of a V1 page (lz4_prefix) before the device is asked for
big = pa.table({"noise": pa.array(rng.integers(-2**62, 2**62, 60_000), mask=rng.random(60_000) < 0.1)})
for version in ("1.0", "2.0"):
    data = write_parquet(big, compression="LZ4_RAW", data_page_version=version, data_page_size=256 << 10)
    chunks, rows = row_group_chunks(data, 0)
    chunks = [c[:5] + ("LZ4_RAW",) for c in chunks]
    code, msg, got = verdict(chunks, rows)
    assert code in (0, pp.FDB_ERR_DEVICE), (code, msg)
    if got is not None:
        same(got, data)
# which decoder inflates: a block that ENDS IN A MATCH is fine by the format's definition and by the built-in decoder, and refused by
# LZ4_decompress_safe (it wants the last 5 bytes to be literals) — so the switch is seen to hide liblz4, and its absence to use it
import ctypes, os
vals = np.arange(4000, dtype=np.int64).tobytes()
vals = vals[:-64] + vals[-64 - 2048:-2048]      # the last 64 bytes repeat those 2 048 bytes before them
body = lz4_cases.seq(vals[:-64], 64, 2048)      # … and are a match, with nothing behind it
chunk = lz4_cases.page_header_v1(4000, len(vals), len(body)) + body
code, msg, got = verdict([("ts", 2, 0, False, chunk, "LZ4_RAW")], 4000)
try:
    ctypes.CDLL("liblz4.so.1"); have_liblz4 = True
except OSError:
    have_liblz4 = False
if os.environ.get("FDB_PARQUET_BUILTIN_LZ4") or not have_liblz4:
    assert code in (0, pp.FDB_ERR_DEVICE), (code, msg)
    if got is not None:
        assert got.column("ts").to_numpy().tobytes() == vals
else:
    assert code == pp.FDB_ERR_INVALID and "corrupt LZ4 page" in msg, (code, msg)
print("ok")
"""


@pytest.mark.parametrize("builtin", [False, True], ids=["liblz4_if_installed", "builtin_decoder"])
def test_parquet_lz4_pages_do_not_need_liblz4(builtin):
    """LZ4_RAW and Hadoop-framed LZ4 chunks get through the host part (and decode, where there is a GPU) with liblz4 hidden from the
    library: no FDB_ERR_UNSUPPORTED any more. The switch is read once per process, so each case is a process of its own."""
    env = dict(os.environ)
    env.pop("FDB_PARQUET_BUILTIN_LZ4", None)
    if builtin:
        env["FDB_PARQUET_BUILTIN_LZ4"] = "1"
    r = subprocess.run([sys.executable, "-c", _PARQUET_CHILD], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr
