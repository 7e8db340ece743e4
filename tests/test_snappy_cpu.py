"""The library's host Snappy block decoder (fdb_codec.cpp snappy_block, reached through fdb_snappy_decode_pages with device < 0: no GPU is
touched): bit-identical to pyarrow's snappy codec on compressor output and on hand-made streams that only the format allows; damaged
pages refused one by one, with the device decoder's codes."""
import ctypes

import numpy as np
import pyarrow as pa
import pytest

from tests import snappy_cases


@pytest.fixture(scope="module")
def pp():
    from frostdb_amd import physicalplan
    return physicalplan


def test_host_snappy_equals_the_codec(pp):
    codec = pa.Codec("snappy")
    plain = snappy_cases.payloads()
    comp = [codec.compress(p, asbytes=True) for p in plain]
    out, status, ms = pp.snappy_decode_pages(comp, [len(p) for p in plain], device=-1)
    assert status == [0] * len(plain), status
    assert ms == 0.0
    for i, (a, b) in enumerate(zip(out, plain)):
        assert a == b, (i, len(b))
    for i, (c, p) in enumerate(zip(comp, plain)):  # every page alone, too
        o, st, _ = pp.snappy_decode_pages([c], [len(p)], device=-1)
        assert st == [0] and o[0] == p, i


def test_host_snappy_hand_made_elements(pp):
    """Every offset form, a 4-byte literal length, patterns of period 1 … 9, and copies from further back than the device's ring
    reaches: the host decoder takes all of them."""
    cases = snappy_cases.hand_made()
    codec = pa.Codec("snappy")
    for name, stream, plain, _ in cases:  # the hand-made streams are Snappy
        assert codec.decompress(stream, decompressed_size=len(plain), asbytes=True) == plain, name
    assert sum(far for *_, far in cases) == 2
    out, status, _ = pp.snappy_decode_pages([c for _, c, _, _ in cases], [len(p) for _, _, p, _ in cases], device=-1)
    assert status == [0] * len(cases), [n for (n, *_), s in zip(cases, status) if s]
    for (name, _, plain, _), got in zip(cases, out):
        assert got == plain, name
    for name, c, p, _ in cases:
        o, st, _ = pp.snappy_decode_pages([c], [len(p)], device=-1)
        assert st == [0] and o[0] == p, name


def test_host_snappy_refuses_damaged_pages_one_by_one(pp):
    c, plain = snappy_cases.good()
    bad = snappy_cases.damaged()
    pages, sizes = [c], [len(plain)]
    for _, stream, announced, _ in bad:
        pages += [stream, c]; sizes += [announced, len(plain)]
    out, status, _ = pp.snappy_decode_pages(pages, sizes, device=-1)
    assert all(s == 0 and o == plain for s, o in zip(status[0::2], out[0::2])), status
    for (name, _, _, codes), s, o in zip(bad, status[1::2], out[1::2]):  # the codes the device's decoder gives: what failed first
        assert s in codes and o is None, (name, s)


def test_pages_outside_the_buffers_are_an_error_not_a_read(pp):
    src = np.frombuffer(snappy_cases.varint(16) + snappy_cases.lit(b"0123456789abcdef"), dtype=np.uint8).copy()
    dst = np.zeros(16, dtype=np.uint8)
    status = np.zeros(1, dtype=np.uint32)
    for so, do, sl, dl in ((0, 0, len(src) + 1, 16), (0, 0, len(src), 17), (2, 0, len(src) - 1, 16), (0, 1, len(src), 16)):
        table = np.array([[so, do, sl | (dl << 32)]], dtype=np.uint64)
        rc = pp.lib().fdb_snappy_decode_pages(src.ctypes.data, len(src), table.ctypes.data, 1, dst.ctypes.data, 16, -1, status.ctypes.data, ctypes.byref(ctypes.c_double()))
        assert rc == pp.FDB_ERR_INVALID, (so, do, sl, dl)
