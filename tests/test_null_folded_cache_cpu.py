"""The null-folded narrow-index cache (frostdb_amd/csrc/fdb_record.h), without a GPU.

1. Which columns are folded is a pure function of (dictionary entries, NULL count, rows); tools/scan_cache_dump.cpp prints it. The rules,
   from which every row of the table below is worked out by hand:
     * a record below 2^20 rows has no cache at all (width 4);
     * the width is 1 byte up to 256 entries, 2 up to 65 536, else 4 (no cache);
     * a cached column is folded iff it holds a NULL and its entry count S itself fits the width: S <= 255 at 1 byte, S <= 65 535 at 2;
       a NULL row then holds S.
   So 256 and 65 536 entries keep their widths and are never folded, and a column without NULLs never is.

2. What the scan kernel of bench.py's headline (`labels.code == '200'`, SUM(value) GROUP BY labels.path; a 1-byte filter column, a
   2-byte group column, one float64 column) looks like once neither dictionary slot has a bitmap: the straight-line head of a full
   1 024-row block holds 3 index loads + 4 x 2 value loads = 11 vector loads, all of 16 bytes, and no byte load; the kernel has no scratch
   and spills nothing. Its VGPR count is printed beside that of the shape with both bitmaps (81 to 85 with the compilers seen so far;
   72 against 81 when this test was written)."""
import os
import re
import subprocess

import pytest

from tests.test_jit_quad_isa_cpu import compile_asm, placement
from tests.test_jit_sources_cpu import ROOT, jit_dump  # noqa: F401  (the fixture builds tools/jit_dump.cpp)

T = 1 << 20

# (entries, nulls, rows) -> (width, folded, index of a NULL row)
FOLD_TABLE = [
    ((5, 1, T), (1, True, 5)),                # the headline's labels.code: 5 codes and NULLs
    ((1024, 7, T + 3), (2, True, 1024)),      # … and labels.path
    ((5, 0, T), (1, False, None)),            # no NULL, no bitmap: nothing to fold
    ((5, 1, T - 1), (4, False, None)),        # below the row threshold there is no cache
    ((0, T, T), (1, True, 0)),                # every row NULL over an empty dictionary: NULL is index 0
    ((1, 1, T), (1, True, 1)),
    ((254, 3, T), (1, True, 254)),
    ((255, 3, T), (1, True, 255)),            # the last 1-byte size with room for S
    ((256, 3, T), (1, False, None)),          # 256 entries fill the byte: width 1 still, the bitmap stays
    ((257, 3, T), (2, True, 257)),
    ((65534, 3, T), (2, True, 65534)),
    ((65535, 3, T), (2, True, 65535)),        # the last 2-byte size with room for S
    ((65535, 0, T), (2, False, None)),
    ((65536, 3, T), (2, False, None)),        # fills 16 bits
    ((65537, 3, T), (4, False, None)),        # too large for a cache
    ((65536, 3, T - 1), (4, False, None)),
    ((255, 2 * T, 2 * T), (1, True, 255)),    # every row NULL
]


def build_tool(out_dir, sanitize):
    exe = str(out_dir / ("scan_cache_dump_asan" if sanitize else "scan_cache_dump"))
    flags = ["-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"] if sanitize else ["-O1"]
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror"] + flags + ["-DFDB_RECORD_HOST_ONLY", "-I", os.path.join(ROOT, "frostdb_amd", "csrc"),
                           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tools", "scan_cache_dump.cpp"), "-o", exe])
    return exe


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_fold_predicate_against_the_table(tmp_path, sanitize):
    """The stand-alone tool, also as its own program under AddressSanitizer and UBSan (host code only: it touches no device)."""
    exe = build_tool(tmp_path, sanitize)
    args = ["%d:%d:%d" % case for case, _ in FOLD_TABLE]
    lines = subprocess.run([exe, "fold"] + args, check=True, capture_output=True, text=True).stdout.splitlines()
    assert len(lines) == len(FOLD_TABLE)
    for (case, (width, folded, null_index)), line in zip(FOLD_TABLE, lines):
        want = "width=%d folded=%d null_index=%s" % (width, int(folded), null_index if folded else "-")
        assert line == want, (case, line, want)
    # positions, by hand for 2 051 rows (two full blocks and 3 rows): row 4 is lane 1's first row of sub-step 0, row 256 lane 0's first of
    # sub-step 1, row 1 027 lane 0's fourth row of block 1, row 2 049 lies in the partial block and stays where it is
    at1 = subprocess.run([exe, "at", "2051", "1", "0", "4", "256", "1027", "2049"], check=True, capture_output=True, text=True).stdout.split()
    assert at1 == ["0", "16", "4", "1027", "2049"]
    at2 = subprocess.run([exe, "at", "2051", "2", "0", "4", "256", "512", "1027", "2049"], check=True, capture_output=True, text=True).stdout.split()
    assert at2 == ["0", "8", "4", "512", "1027", "2049"]
    assert subprocess.run([exe, "fold", "5:9:3"], capture_output=True).returncode == 2  # more NULLs than rows


def test_headline_shape_without_bitmaps(jit_dump):  # noqa: F811
    exe, out = jit_dump
    args = ["plan", "lds", "narrow", "256", "sum"]
    src = subprocess.run([exe] + args + ["nonull"], check=True, capture_output=True, text=True).stdout
    with_bitmaps = subprocess.run([exe] + args, check=True, capture_output=True, text=True).stdout
    assert "ldv(" in with_bitmaps.split("extern \"C\"")[-1] and "ldv(" not in src.split("extern \"C\"")[-1]  # no bitmap is read, in the block or in the tail
    asm, log = compile_asm(src, str(out / "headline_nonull.hip"))
    _, log_b = compile_asm(with_bitmaps, str(out / "headline_bitmaps.hip"))
    x4, ub, other, waits = placement(asm)
    vgprs, vgprs_b = re.findall(r" VGPRs: (\d+)", log)[:1], re.findall(r" VGPRs: (\d+)", log_b)[:1]
    print("headline without bitmaps: %d 16-byte loads and %d byte loads before the first branch, waits vmcnt %s, VGPRs %s (with both bitmaps: %s)" % (x4, ub, waits, vgprs, vgprs_b))
    assert (x4, ub) == (3 + 4 * 2, 0) and not other, (x4, ub, other)
    assert not re.search(r"global_load_(u|s)byte", asm)  # … nor anywhere else in the kernel
    for what in ("ScratchSize [bytes/lane]", "SGPRs Spill", "VGPRs Spill"):
        lines = [ln for ln in log.splitlines() if what in ln]
        assert lines and all(re.search(re.escape(what) + r": 0\b", ln) for ln in lines), lines
