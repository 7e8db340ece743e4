"""Snappy pages inflated on the device (fdb_snappy_decode_pages, snappy_decode_kernel): bit-identical to pyarrow's codec on payloads
that exercise every element kind — literals with 1 … 4 length bytes, copies with 1-, 2- and 4-byte offsets, overlapping patterns of
every short period, empty and one-byte pages — many pages per launch, and damaged pages refused one by one without touching the others."""
import numpy as np
import pyarrow as pa
import pytest

from tests import snappy_cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pp():
    from frostdb_amd import build
    build.build()
    from frostdb_amd import physicalplan
    return physicalplan


def test_device_snappy_equals_the_codec(pp):
    codec = pa.Codec("snappy")
    plain = snappy_cases.payloads()
    comp = [codec.compress(p, asbytes=True) for p in plain]
    out, status, ms = pp.snappy_decode_pages(comp, [len(p) for p in plain])
    assert status == [0] * len(plain), status
    for i, (a, b) in enumerate(zip(out, plain)):
        assert a == b, (i, len(b))
    # every page alone, too (page offsets and the window refill at other alignments)
    for i, (c, p) in enumerate(zip(comp, plain)):
        o, st, _ = pp.snappy_decode_pages([c], [len(p)])
        assert st == [0] and o[0] == p, i


def test_device_snappy_hand_made_elements(pp):
    """Streams no compressor emits but the format allows (snappy_cases.hand_made); a copy from beyond the ring's reach is legal Snappy
    that the ring cannot serve: said so with status 6, not decoded wrongly, and decoded by the host path in the same process."""
    cases = snappy_cases.hand_made()
    assert sum(far for *_, far in cases) == 2
    comp, sizes = [c for _, c, _, _ in cases], [len(p) for _, _, p, _ in cases]
    out, status, _ = pp.snappy_decode_pages(comp, sizes)
    for (name, _, plain, far), st, got in zip(cases, status, out):
        if far:
            assert st == 6 and got is None, (name, st)
        else:
            assert st == 0 and got == plain, (name, st)
    host, hstatus, _ = pp.snappy_decode_pages(comp, sizes, device=-1)
    assert hstatus == [0] * len(cases) and host == [p for _, _, p, _ in cases]


def test_device_snappy_refuses_damaged_pages_one_by_one(pp):
    c, plain = snappy_cases.good()
    bad = snappy_cases.damaged()
    pages, sizes = [c], [len(plain)]
    for _, stream, announced, _ in bad:
        pages += [stream, c]; sizes += [announced, len(plain)]
    out, status, _ = pp.snappy_decode_pages(pages, sizes)
    assert all(s == 0 and o == plain for s, o in zip(status[0::2], out[0::2])), status
    for (name, _, _, codes), s, o in zip(bad, status[1::2], out[1::2]):
        assert s in codes and o is None, (name, s)
    for name, stream, announced, codes in bad:  # and alone
        o, st, _ = pp.snappy_decode_pages([stream], [announced])
        assert st[0] in codes and o[0] is None, (name, st)


def test_device_snappy_rate(pp, capsys):
    """What a launch over a row group's pages reaches (reported, loosely bounded): 240 pages of 1 MiB — a third noise (DOUBLE values),
    a third a DELTA-friendly int64 column, a third dictionary indices."""
    codec = pa.Codec("snappy")
    rng = np.random.default_rng(1)
    plain = []
    for k in range(240):
        if k % 3 == 0:
            plain.append(rng.uniform(0, 1000, 131_072).tobytes())
        elif k % 3 == 1:
            plain.append((1_700_000_000_000 + 15_000 * (np.arange(131_072) // 7 + k)).astype(np.int64).tobytes())
        else:
            plain.append(rng.integers(0, 6, 262_144).astype(np.uint32).tobytes())
    comp = [codec.compress(p, asbytes=True) for p in plain]
    out, status, ms = pp.snappy_decode_pages(comp, [len(p) for p in plain])
    assert status == [0] * 240 and out == plain
    out, status, ms = pp.snappy_decode_pages(comp, [len(p) for p in plain])
    gb = sum(len(p) for p in plain) / 1e9
    with capsys.disabled():
        print(f"\n[snappy] 240 pages, {sum(len(c) for c in comp) / 1e6:.0f} MB -> {gb * 1e3:.0f} MB in {ms:.3f} ms = {gb / (ms * 1e-3):.1f} GB/s of output")
        for kind, name in enumerate(("noise (float64 values)", "int64 timestamps", "dictionary indices")):
            cs, ps = comp[kind::3], plain[kind::3]
            pp.snappy_decode_pages(cs, [len(p) for p in ps])
            _, st, ms_k = pp.snappy_decode_pages(cs, [len(p) for p in ps])
            assert st == [0] * len(cs)
            print(f"[snappy]   80 pages of {name}: {sum(len(c) for c in cs) / 1e6:.1f} MB -> {sum(len(p) for p in ps) / 1e6:.0f} MB in {ms_k:.3f} ms"
                  f" = {sum(len(p) for p in ps) / 1e9 / (ms_k * 1e-3):.1f} GB/s of output, {sum(len(p) for p in ps) / len(ps) / 1e6 / (ms_k * 1e-3):.0f} MB/s per page")
    assert ms < 200.0
