"""The one description of the narrow-index cache's forms (frostdb_amd/csrc/fdb_record.h, ScanForm), without a GPU: tools/scan_cache_dump.cpp,
plain and as its own program under AddressSanitizer and UBSan, held to tables written by hand.
  * the table: five forms — 1 and 2 bytes, 4 (the uint32 column itself), H (4 bits), T (12 bits) — with their codes, bits per index, largest
    index, bytes per 1 024-row block, whether a partial block occupies a whole frame, and the rows a record must have;
  * a launch reads a column at the first form of its first part that every part offers: the same packed form in all parts, else the same
    byte form in all parts, else 4;
  * a buffer's size is what the two old formulas gave: align_up(rows x width + 256, 256) for the byte forms, whole frames + 256 rounded up
    to 256 for the packed ones;
  * a column's packed candidate folds NULL into the index exactly when its byte candidate does, so "does any candidate fold" can be asked
    before a launch has chosen a form."""
import subprocess

import pytest

from tests.test_null_folded_cache_cpu import build_tool

M = 1 << 20

# code, name, bits per index, largest index, bytes per 1 024-row block, whole frames, minimum rows
TABLE = [
    (1, "1", 8, 255, 1024, 0, M),
    (2, "2", 16, 65535, 2048, 0, M),
    (4, "4", 32, 4294967295, 4096, 0, 0),
    (5, "H", 4, 15, 512, 1, 4 * M),
    (6, "T", 12, 4095, 1536, 1, 4 * M),
]

# parts as (entries, nulls, rows) -> the form of the launch
COMMON = [
    ([(15, 0, 4 * M), (300, 0, 4 * M)], "4"),      # H and T, 1 and 2 bytes: nothing in common
    ([(15, 0, 4 * M), (15, 0, 4 * M - 1)], "1"),   # the second part is a row short of the packed forms
    ([(15, 0, 4 * M), (12, 3, 8 * M)], "H"),
    ([(300, 0, 4 * M), (4000, 5, 4 * M)], "T"),
    ([(4096, 3, 4 * M), (300, 0, 4 * M)], "2"),    # 4 096 entries and NULL do not fit 12 bits
    ([(16, 3, 4 * M), (10, 0, 4 * M)], "1"),       # 16 entries and NULL do not fit 4 bits
    ([(70000, 0, 4 * M)], "4"),
    ([(15, 0, M - 1)], "4"),                       # below every threshold
    ([(200, 0, M), (300, 0, M)], "4"),             # 1 byte and 2 bytes
]


def up(n):
    return (n + 255) // 256 * 256


def old_slot(form, rows):
    """The two sizing formulas as they were before there was one, restated."""
    if form in ("1", "2", "4"):
        return up(rows * int(form) + 256)
    return up((rows + 1023) // 1024 * (512 if form == "H" else 1536) + 256)


def run(exe, *args):
    return subprocess.run([exe] + [str(a) for a in args], check=True, capture_output=True, text=True).stdout.splitlines()


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_table_common_form_slots_and_fold_agreement(tmp_path, sanitize):
    exe = build_tool(tmp_path, sanitize)
    assert run(exe, "table") == ["code=%d name=%s bits=%d max_index=%d block_bytes=%d framed=%d min_rows=%d" % row for row in TABLE]
    for parts, want in COMMON:
        assert run(exe, "common", *["%d:%d:%d" % p for p in parts]) == [want], (parts, want)
    rows_of = (1, 1023, 1024, 1025, 2051, 4 * M)
    sized = run(exe, "table", *rows_of)  # the table's rows, scan_form_slot of each row count behind every one
    assert [line.split()[:7] for line in sized] == [line.split() for line in run(exe, "table")]
    for row, line in zip(TABLE, sized):
        assert line.split()[7:] == [str(old_slot(row[1], rows)) for rows in rows_of], line
    # every candidate list ends in 4, which never folds; a packed candidate and a byte candidate of one column agree on folding
    cases = [(e, n, r) for e in (0, 1, 15, 16, 17, 255, 256, 257, 4095, 4096, 4097, 65535, 65536, 65537) for n in (0, 3) for r in (M - 1, M, 4 * M - 1, 4 * M)]
    lines = run(exe, "forms", *["%d:%d:%d" % c for c in cases])
    assert len(lines) == len(cases)
    both = 0
    for case, line in zip(cases, lines):
        forms = [tuple(f.split(":")) for f in line.split()]
        assert forms[-1] == ("4", "0") and 1 <= len(forms) <= 3, (case, line)
        packed = [f for f in forms if f[0] in "HT"]
        byte = [f for f in forms if f[0] in "12"]
        assert len(packed) <= 1 and len(byte) <= 1 and forms == packed + byte + [("4", "0")], (case, line)
        if packed and byte:
            both += 1
            assert packed[0][1] == byte[0][1] == ("1" if case[1] else "0"), (case, line)
    # by hand: at 4 Mi rows, H beside 1 byte for 0, 1, 15 entries (and 16 without NULLs), T beside 2 bytes for 257, 4 095 (and 4 096 without NULLs)
    assert both == 2 * 3 + 1 + 2 * 2 + 1
    assert subprocess.run([exe, "common", "5:9:3"], capture_output=True).returncode == 2  # more NULLs than rows
    assert subprocess.run([exe, "table", "0"], capture_output=True).returncode == 2
