"""LZ4 blocks inflated on the device (fdb_lz4_decode_pages, lz4_decode_kernel): bit-identical to pyarrow's lz4_raw codec and to the
library's host decoder on compressor output and on hand-made streams that only the format allows — lengths that end on a 255 boundary,
patterns shorter than the 64 bytes a wave copies at a time, matches from as far back as the ring reaches — many pages per launch and
each alone; damaged pages refused one by one without touching the others; a match from beyond the ring's reach answered with status 6."""
import numpy as np
import pyarrow as pa
import pytest

from tests import lz4_cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pp():
    from frostdb_amd import build
    build.build()
    from frostdb_amd import physicalplan
    return physicalplan


def test_device_lz4_equals_the_codec(pp):
    codec = pa.Codec("lz4_raw")
    plain = lz4_cases.payloads()
    comp = [codec.compress(p, asbytes=True) for p in plain]
    # (liblz4 uses the format's whole 65 535-byte window: a page with a match from beyond the ring's reach is legal, is the host's in the
    # Parquet path, and is answered with 6 here — which pages those are is read off the streams, not off the decoder)
    want = [6 if lz4_cases.max_offset(c) > lz4_cases.RING_REACH else 0 for c in comp]
    # (the one page of these that liblz4 gives such a match is the text; the noise, the ramps and the match 60 000 bytes back are the device's)
    assert [i for i, w in enumerate(want) if w] in ([], [len(plain) - 2]), want
    assert want[8] == 0 and len(plain[8]) == 1 << 20 and want[-1] == 0 and lz4_cases.max_offset(comp[-1]) == 60_000
    out, status, ms = pp.lz4_decode_pages(comp, [len(p) for p in plain])
    assert status == want, (status, want)
    for i, (a, b) in enumerate(zip(out, plain)):
        assert a == (b if want[i] == 0 else None), (i, len(b))
    host, hstatus, _ = pp.lz4_decode_pages(comp, [len(p) for p in plain], device=-1)
    assert hstatus == [0] * len(plain) and host == plain
    # every page alone, too (page offsets and the window refill at other alignments)
    for i, (c, p) in enumerate(zip(comp, plain)):
        o, st, _ = pp.lz4_decode_pages([c], [len(p)])
        assert st == [want[i]] and o[0] == (p if want[i] == 0 else None), i


def test_device_lz4_hand_made_sequences(pp):
    cases = lz4_cases.hand_made()
    lz4_cases.check_hand_made(cases)
    out, status, _ = pp.lz4_decode_pages([c for _, c, _, _ in cases], [len(p) for _, _, p, _ in cases])
    for (name, _, plain, far), st, got in zip(cases, status, out):
        if far:  # legal LZ4 that the ring cannot serve: said so, not decoded wrongly
            assert st == 6 and got is None, (name, st)
        else:
            assert st == 0 and got == plain, (name, st)
    for name, c, p, far in cases:
        o, st, _ = pp.lz4_decode_pages([c], [len(p)])
        assert (st == [6] and o[0] is None) if far else (st == [0] and o[0] == p), (name, st)


def test_device_lz4_refuses_damaged_pages_one_by_one(pp):
    c, plain = lz4_cases.good()
    bad = lz4_cases.damaged()
    pages, sizes = [c], [len(plain)]
    for _, stream, announced, _ in bad:
        pages += [stream, c]; sizes += [announced, len(plain)]
    out, status, _ = pp.lz4_decode_pages(pages, sizes)
    assert all(s == 0 and o == plain for s, o in zip(status[0::2], out[0::2])), status
    for (name, _, _, codes), s, o in zip(bad, status[1::2], out[1::2]):
        assert s in codes and o is None, (name, s)
    for name, stream, announced, codes in bad:  # and alone
        o, st, _ = pp.lz4_decode_pages([stream], [announced])
        assert st[0] in codes and o[0] is None, (name, st)


def test_device_lz4_rate(pp, capsys):
    """What a launch over a row group's pages reaches (reported, loosely bounded — the bound is test_device_snappy_rate's, a guard against
    a hang-like slowdown): 240 pages of 1 MiB — a third noise (DOUBLE values), a third a DELTA-friendly int64 column, a third dictionary
    indices — and, in the same process, snappy_decode_kernel on the same plain pages."""
    rng = np.random.default_rng(1)
    plain = []
    for k in range(240):
        if k % 3 == 0:
            plain.append(rng.uniform(0, 1000, 131_072).tobytes())
        elif k % 3 == 1:
            plain.append((1_700_000_000_000 + 15_000 * (np.arange(131_072) // 7 + k)).astype(np.int64).tobytes())
        else:
            plain.append(rng.integers(0, 6, 262_144).astype(np.uint32).tobytes())
    sizes = [len(p) for p in plain]
    comp = {name: [pa.Codec(name).compress(p, asbytes=True) for p in plain] for name in ("lz4_raw", "snappy")}
    decode = {"lz4_raw": pp.lz4_decode_pages, "snappy": pp.snappy_decode_pages}
    out, status, ms = pp.lz4_decode_pages(comp["lz4_raw"], sizes)
    assert status == [0] * 240 and out == plain
    out, status, ms = pp.lz4_decode_pages(comp["lz4_raw"], sizes)
    gb = sum(sizes) / 1e9
    with capsys.disabled():
        print(f"\n[lz4] 240 pages, {sum(len(c) for c in comp['lz4_raw']) / 1e6:.0f} MB -> {gb * 1e3:.0f} MB in {ms:.3f} ms = {gb / (ms * 1e-3):.1f} GB/s of output")
        for kind, name in enumerate(("noise (float64 values)", "int64 timestamps", "dictionary indices")):
            for codec in ("lz4_raw", "snappy"):
                cs, ps = comp[codec][kind::3], plain[kind::3]
                decode[codec](cs, [len(p) for p in ps])
                times = []
                for _ in range(7):
                    _, st, ms_k = decode[codec](cs, [len(p) for p in ps])
                    assert st == [0] * len(cs)
                    times.append(ms_k)
                times.sort()
                nb = sum(len(p) for p in ps)
                print(f"[{codec}]   80 pages of {name}: {sum(len(c) for c in cs) / 1e6:.1f} MB -> {nb / 1e6:.0f} MB, median of 7 {times[3]:.3f} ms (min {times[0]:.3f}, max {times[6]:.3f})"
                      f" = {nb / 1e9 / (times[3] * 1e-3):.1f} GB/s of output, {nb / len(ps) / 1e6 / (times[3] * 1e-3):.0f} MB/s per page")
    assert ms < 200.0
