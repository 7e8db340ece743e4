"""The narrow-index cache's bytes (frostdb_amd/csrc/fdb_record.h, scan_cache_position): the builder kernel, run through
fdb_selftest_scan_cache over a caller's uint32 array, against the position formula restated here in numpy.

With F = rows // 1024 * 1024, row i < F sits at element 1024 b + 16 l + 4 u + r (1 byte per index) or 1024 b + 512 (u // 2) + 8 l +
4 (u % 2) + r (2 bytes), where b = i // 1024, j = i % 1024, u = j // 256, l = (j % 256) // 4, r = j % 4; rows i >= F stay at element i;
behind the last row the buffer holds zeros up to the end of its last 16-byte vector.

No row threshold applies to the builder itself, so the rows are the smallest at which a permutation can go wrong: around a 16-byte
vector, a sub-step of 256 rows, one and two blocks of 1 024 rows, and a partial block behind three full ones. Row i holds
(7 i + 3) mod 251 / 65 521: distinct over the whole array at 2 bytes, and at 1 byte equal only between rows a multiple of 251 apart —
a prime, so no stride of the layout (4, 16, 256, 1 024 and their sums below 251) takes an element to a place that wants its value."""
import ctypes

import numpy as np
import pytest

from frostdb_amd import physicalplan as pp

pytestmark = pytest.mark.gpu

ROWS = [1, 15, 16, 17, 255, 1023, 1024, 1025, 2047, 2048, 3 * 1024 + 513]


def position(i: np.ndarray, rows: int, width: int) -> np.ndarray:
    full = rows // 1024 * 1024
    b, j = i // 1024, i % 1024
    u, l, r = j // 256, (j % 256) // 4, j % 4
    at = 1024 * b + 16 * l + 4 * u + r if width == 1 else 1024 * b + 512 * (u // 2) + 8 * l + 4 * (u % 2) + r
    return np.where(i < full, at, i)


def build(indices: np.ndarray, width: int) -> np.ndarray:
    rows = len(indices)
    out = np.full((rows * width + 15) // 16 * 16, 0xAB, dtype=np.uint8)
    L = pp.lib()
    rc = L.fdb_selftest_scan_cache(indices.ctypes.data, rows, width, 0, out.ctypes.data, len(out))
    assert rc == 0, L.fdb_last_error().decode("utf-8", "replace")
    return out.view(np.uint8 if width == 1 else np.uint16)


@pytest.mark.parametrize("width", [1, 2])
@pytest.mark.parametrize("rows", ROWS)
def test_builder_against_the_position_formula(rows, width):
    modulus = 251 if width == 1 else 65521
    i = np.arange(rows, dtype=np.int64)
    # (the upper bits are cut by the builder: they must not reach the cache)
    indices = ((i * 7 + 3) % modulus).astype(np.uint32) | np.uint32(0x5A000000 if width == 1 else 0x5A5A0000)
    got = build(indices, width)
    want = np.zeros(len(got), dtype=got.dtype)
    at = position(i, rows, width)
    assert np.array_equal(np.sort(at), i)  # a permutation of the rows
    want[at] = (i * 7 + 3) % modulus
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:8]
    assert not got[rows:].any()  # zeros behind the last row


def test_bad_arguments():
    L = pp.lib()
    src, out = np.zeros(16, dtype=np.uint32), np.zeros(64, dtype=np.uint8)
    assert L.fdb_selftest_scan_cache(src.ctypes.data, 16, 4, 0, out.ctypes.data, 64) == pp.FDB_ERR_INVALID  # no cache at 4 bytes
    assert L.fdb_selftest_scan_cache(src.ctypes.data, 16, 1, 0, out.ctypes.data, 32) == pp.FDB_ERR_INVALID  # out_bytes is not rows x width rounded up to 16
    assert L.fdb_selftest_scan_cache(None, 16, 1, 0, out.ctypes.data, 16) == pp.FDB_ERR_INVALID
