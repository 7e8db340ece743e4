"""Snappy blocks for the decoders' tests (tests/test_snappy_cpu.py: the host decoder; tests/test_gpu_snappy.py: snappy_decode_kernel):
payloads that pyarrow's snappy codec compresses, hand-made streams that no compressor emits but the format allows, damaged pages. The
counterpart of tests/lz4_cases.py."""
import numpy as np
import pyarrow as pa

from tests.lz4_cases import RING_REACH  # the furthest back a copy may reach on the device: the two decoders share the ring


def payloads():
    rng = np.random.default_rng(11)
    out = [b"", b"x", b"ab" * 3, bytes(range(60)), bytes(range(61)), bytes(rng.integers(0, 256, 59, dtype=np.uint8)), bytes(rng.integers(0, 256, 300, dtype=np.uint8)),
           bytes(rng.integers(0, 256, 70_000, dtype=np.uint8)),             # incompressible: literals with 2- and 3-byte lengths
           bytes(rng.integers(0, 256, 1 << 20, dtype=np.uint8)),            # 1 MiB of noise (a DOUBLE page of random values looks like this)
           b"\x00" * 100_000, b"\x07" * 17, b"abc" * 50_000, b"0123456" * 9_999, bytes(range(256)) * 300,  # patterns of period 1, 3, 7, 256
           np.arange(200_000, dtype=np.int64).tobytes(),                     # a timestamp-like column: long matches at offset 8 … 64
           (1_700_000_000_000 + 15_000 * (np.arange(131_072) // 7)).astype(np.int64).tobytes(),
           rng.integers(0, 6, 500_000).astype(np.uint32).tobytes(),         # dictionary indices: short matches, short literals
           b" ".join(b"/api/v1/p%04d" % rng.integers(0, 1000) for _ in range(40_000))]
    big = bytearray(rng.integers(0, 256, 300_000, dtype=np.uint8).tobytes())
    big[200_000:260_000] = big[0:60_000]  # a match 200 000 bytes back: 4-byte (or 2-byte, fragment-local) offsets
    out.append(bytes(big))
    return out


def varint(n):
    b = bytearray()
    while True:
        b.append((n & 0x7F) | (0x80 if n > 0x7F else 0))
        n >>= 7
        if not n:
            return bytes(b)


def lit(data, nbytes=None):
    l = len(data) - 1
    if nbytes is None and l < 60:
        return bytes([l << 2]) + data
    nb = nbytes or (1 if l < 256 else 2 if l < 65536 else 3)
    return bytes([(59 + nb) << 2]) + l.to_bytes(nb, "little") + data


def copy4(length, off):
    return bytes([((length - 1) << 2) | 3]) + off.to_bytes(4, "little")


def copy2(length, off):
    return bytes([((length - 1) << 2) | 2]) + off.to_bytes(2, "little")


def copy1(length, off):
    return bytes([((off >> 8) << 5) | ((length - 4) << 2) | 1, off & 0xFF])


def hand_made():
    """[(name, stream, plain, far)] — streams no compressor emits but the format allows: a copy with a 4-byte offset, a literal with a
    4-byte length, a pattern copy of 64 bytes with offset 1 … 9, a copy whose source ends exactly where the destination starts. `far`:
    a copy reaches further back than the device's ring keeps (legal Snappy: the host decodes it, the device answers 6)."""
    cases = []
    seed = bytes(range(1, 10))
    for off in range(1, 10):
        body = lit(seed) + copy2(64, off) + copy2(64, off) + copy1(11, off) + copy4(33, off)
        want = bytearray(seed)
        for ln in (64, 64, 11, 33):
            for _ in range(ln):
                want.append(want[-off])
        cases.append((f"pattern_{off}", varint(len(want)) + body, bytes(want), False))
    data = bytes(np.random.default_rng(3).integers(0, 256, 1000, dtype=np.uint8))
    cases.append(("adjacent_1000", varint(2000) + lit(data, nbytes=4) + copy4(64, 1000) + copy2(64, 1000) + copy4(64, 1000) * 13 + copy2(40, 1000), data + data, False))
    noise = bytes(np.random.default_rng(4).integers(0, 256, 65_600, dtype=np.uint8))
    assert 65_500 > RING_REACH
    for name, far_copy in (("far_copy4", copy4(64, 65_500)), ("far_copy2", copy2(64, 65_500))):
        cases.append((name, varint(65_664) + lit(noise) + far_copy, noise + noise[100:164], True))
    return cases


def good():
    plain = np.arange(50_000, dtype=np.int64).tobytes()
    return pa.Codec("snappy").compress(plain, asbytes=True), plain


def damaged():
    """[(name, stream, announced size, status codes that name the damage)] — every one refused; the good page they sit between is `good()`."""
    c, plain = good()
    preamble = 1 if c[0] < 0x80 else 2 if c[1] < 0x80 else 3
    return [("bad_len", bytes([c[0] ^ 1]) + c[1:], len(plain), (1,)),          # another length in the preamble
            ("truncated", c[:len(c) // 2], len(plain), (2, 5)),
            ("bad_offset", c[:1 + preamble] + bytes([0x02 | (10 << 2), 0xFF, 0xFF]) + c[8:], len(plain), (4,))]  # a copy from before the page's first byte
