"""The host-only half of the resident record's layout contract (frostdb_amd/csrc/fdb_record.h), without a GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_layout_arithmetic_is_clean_under_address_sanitizer():
    """tools/asan_record.sh: slot alignment, disjointness, tail pad and totals of random column lists, the equivalence of the three
    bitmap-size forms, and finish_column for every kind, in a stand-alone program built with -fsanitize=address,undefined (no GPU, not
    inside python)."""
    r = subprocess.run(["bash", os.path.join(ROOT, "tools", "asan_record.sh")], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    assert "asan record ok" in r.stdout
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
