"""The packed forms of the narrow-index cache (frostdb_amd/csrc/fdb_record.h), without a GPU: tools/scan_cache_dump.cpp, plain and as its
own program under AddressSanitizer and UBSan, held to tables worked out by hand from the rule:
  * packed forms are for records of at least 4 Mi rows; below, a record is scanned as before (1 byte up to 256 entries, 2 up to 65 536);
  * H (4 bits) where entries + (nulls > 0) <= 16; else 1 byte where entries <= 256; else T (12 bits) where entries + (nulls > 0) <= 4 096;
    else 2 bytes where entries <= 65 536; else none (4);
  * a packed buffer of a column with NULLs is always folded, NULL being index S = entries; the byte forms fold where S fits the width;
  * a packed buffer is whole frames, one per 1 024-row block — 512 B (H) or 1 024 B of low bytes + 512 B of nibbles (T) — + 256, rounded up
    to 256; a byte buffer is align_up(rows x width + 256, 256)."""
import subprocess

import pytest

from tests.test_null_folded_cache_cpu import build_tool

M = 1 << 20


def up(n):
    return (n + 255) // 256 * 256


def hbytes(rows):
    return up((rows + 1023) // 1024 * 512 + 256)


def tbytes(rows):
    return up((rows + 1023) // 1024 * 1536 + 256)


def byte_form(entries, nulls, rows):
    w = 1 if entries <= 256 else 2 if entries <= 65536 else 4
    if w == 4:
        return ("4", False, 0)
    return (str(w), nulls and entries < (1 << (8 * w)), up(rows * w + 256))


# entries -> (without NULLs, with NULLs) at 4 Mi rows and above, by hand: H / T, folded with NULLs always; the rest as the byte forms
PACKED = {
    0: ("H", "H"), 1: ("H", "H"), 14: ("H", "H"), 15: ("H", "H"), 16: ("H", "1"), 17: ("1", "1"), 255: ("1", "1"), 256: ("1", "1"),
    257: ("T", "T"), 4094: ("T", "T"), 4095: ("T", "T"), 4096: ("T", "2"), 4097: ("2", "2"), 65535: ("2", "2"),
}


def table():
    rows_of = (4 * M - 1, 4 * M, 8 * M)
    cases = []
    for rows in rows_of:
        for entries, forms in PACKED.items():
            for nulls in (0, 3):
                form = forms[1 if nulls else 0] if rows >= 4 * M else byte_form(entries, nulls, rows)[0]
                if form == "H":
                    want = ("H", bool(nulls), hbytes(rows))
                elif form == "T":
                    want = ("T", bool(nulls), tbytes(rows))
                else:
                    want = byte_form(entries, nulls, rows)
                    assert want[0] == form
                cases.append(((entries, nulls, rows), want))
    return cases


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_form_rule_positions_and_sizes(tmp_path, sanitize):
    exe = build_tool(tmp_path, sanitize)
    cases = table()
    assert len(cases) == 14 * 2 * 3
    lines = subprocess.run([exe, "form"] + ["%d:%d:%d" % c for c, _ in cases], check=True, capture_output=True, text=True).stdout.splitlines()
    assert len(lines) == len(cases)
    for (case, (form, folded, nbytes)), line in zip(cases, lines):
        want = "form=%s folded=%d null_index=%s bytes=%d" % (form, int(folded), case[0] if folded else "-", nbytes)
        assert line == want, (case, line, want)
    # a few spelt out: 16 entries fill the nibble, so with NULLs the column falls to the 1-byte form, which folds it (S = 16 fits a byte);
    # 4 096 with NULLs falls to 2 bytes; one row short of 4 Mi nothing is packed
    spelt = subprocess.run([exe, "form", "16:3:%d" % (4 * M), "4096:3:%d" % (4 * M), "5:1:%d" % (4 * M - 1), "1024:0:%d" % (4 * M)], check=True, capture_output=True, text=True).stdout.splitlines()
    assert spelt == ["form=1 folded=1 null_index=16 bytes=%d" % (4 * M + 256), "form=2 folded=1 null_index=4096 bytes=%d" % (8 * M + 256),
                     "form=1 folded=1 null_index=5 bytes=%d" % up(4 * M - 1 + 256), "form=T folded=0 null_index=- bytes=%d" % (4096 * 1536 + 256)]
    # positions, by hand for 2 051 rows (two full blocks and 3 rows; frames of 512 / 1 536 bytes):
    #   row 0: lane 0, sub-step 0, r 0: element 0 -> byte 0, nibble 0 (byte 0, shift 0)
    #   row 4: lane 1's first row of sub-step 0: element 16 -> byte 16, nibble 16 = byte 8 of the plane, shift 0
    #   row 256: lane 0's first row of sub-step 1: element 4 -> byte 4, nibble 4 = byte 2, shift 0
    #   row 1 027: block 1, lane 0, sub-step 0, r 3: element 3 -> byte 3, nibble 3 = byte 1, shift 4; H frame at 512 (-> 513), T frame at 1 536 (-> 1 539; nibbles at + 1 024 -> 2 561)
    #   row 2 049: the partial block (block 2), row 1 of it, in row order: byte 1, nibble 1 = byte 0, shift 4; H frame at 1 024, T frame at 3 072
    ath = subprocess.run([exe, "pat", "2051", "H", "0", "4", "256", "1027", "2049"], check=True, capture_output=True, text=True).stdout.splitlines()
    assert ath == ["- 0 0", "- 8 0", "- 2 0", "- 513 4", "- 1024 4"]
    att = subprocess.run([exe, "pat", "2051", "T", "0", "4", "256", "1027", "2049"], check=True, capture_output=True, text=True).stdout.splitlines()
    assert att == ["0 1024 0", "16 1032 0", "4 1026 0", "1539 2561 4", "3073 4096 4"]
    # the buffers of those 2 051 rows hold three frames each (the threshold is the launch's business, not the size formula's)
    assert hbytes(2051) == 1792 and tbytes(2051) == 4864
    assert subprocess.run([exe, "pat", "2051", "B", "0"], capture_output=True).returncode == 2
    assert subprocess.run([exe, "form", "5:9:3"], capture_output=True).returncode == 2  # more NULLs than rows
