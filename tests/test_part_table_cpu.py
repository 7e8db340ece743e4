"""The host side of the packed part table (frostdb_amd/csrc/fdb_jit.h: jit_part_fields, jit_pack_parts), without a GPU:
tools/part_table_dump.cpp builds argument blocks by hand for three shapes and prints each shape's field list, W and the packed words.
They are held to values worked out by hand from that file's blocks, W is compared with the stride the emitted kernel uses, and the
tool is built and run a second time, stand-alone, under AddressSanitizer and UBSan (host code only: nothing here touches a GPU)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = [os.path.join(ROOT, "tools", "part_table_dump.cpp"), os.path.join(ROOT, "frostdb_amd", "csrc", "fdb_jitgen.cpp")]
FLAGS = ["g++", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROOT, "frostdb_amd", "csrc"), "-I", os.path.join(ROOT, "include"), "-I", "/opt/rocm/include"]


def parse(text):
    shapes, cur = {}, None
    for ln in text.splitlines():
        m = re.match(r"shape (\w+) key=(\S+) records=(\d+) W=(\d+)", ln)
        if m:
            cur = shapes[m.group(1)] = {"key": m.group(2), "W": int(m.group(4)), "fields": [], "records": []}
            continue
        m = re.match(r"  field (.*) bits=(\d+) word=(\d+) shift=(\d+)", ln)
        if m:
            cur["fields"].append((m.group(1), int(m.group(2)), int(m.group(3)), int(m.group(4))))
            continue
        m = re.match(r"  record \d+: (.*)", ln)
        if m:
            cur["records"].append([int(w, 16) for w in m.group(1).split()])
    return shapes


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    if not os.path.exists("/opt/rocm/include/hip/hip_runtime_api.h"):
        pytest.skip("no HIP headers on this host")
    exe = str(tmp_path_factory.mktemp("ptab") / "part_table_dump")
    subprocess.check_call(FLAGS + SRC + ["-o", exe])
    return exe


@pytest.fixture(scope="module")
def dump(tool):
    return parse(subprocess.run([tool], check=True, capture_output=True, text=True).stdout)


def test_headline_fields_and_words(dump):
    s = dump["headline"]
    assert s["key"].startswith("b256l1c0t0r0h0uqp|") and s["W"] == 11
    # three 64-bit range words, three column pointers (no bitmaps), the truth bits, then 32-bit fields paired in list order
    assert s["fields"] == [("tile_end", 64, 0, 0), ("tile_begin", 64, 1, 0), ("n_rows", 64, 2, 0), ("c4[0].values", 64, 3, 0), ("c4[1].values", 64, 4, 0),
                           ("c8[0].values", 64, 5, 0), ("[0] leaf.lit", 64, 6, 0), ("[0] leaf.lut_len", 32, 7, 0), ("[0] gcol.lut", 64, 8, 0), ("[0] gcol.stride", 32, 7, 32),
                           ("[0] gcol.lut_lds", 32, 9, 0), ("[0] gcol.lut_len", 32, 9, 32), ("lut_class", 32, 10, 0)]
    assert s["records"] == [
        [6104, 0, 25000000, 0x7F0000001000, 0x7F0000002000, 0x7F0000003000, 0x25, (1 << 32) | 7, 0x7E0000000040, (1025 << 32) | 0, 0],
        [6361, 6104, 1048577, 0x7F0100001000, 0x7F0100002000, 0x7F0100003000, 0x25, (1 << 32) | 7, 0x7E0000000040, (1025 << 32) | 0, 0],
    ]


def test_two_phase_fields_and_words(dump):
    s = dump["two_phase"]
    assert s["W"] == 15 and "|v1w1||v2w2|v0v0|" in s["key"]  # the group column's bitmap: in some records
    names = [f[0] for f in s["fields"]]
    assert names == ["tile_end", "tile_begin", "n_rows", "c4[0].values", "c4[0].validity", "l4[0].values", "l4[0].validity", "l8[0].values", "l8[1].values",
                     "[0] leaf.lut", "[0] leaf.lut_len", "[0] leaf.lut_lds", "[1] leaf.op", "[0] gcol.lut", "[0] gcol.stride", "[0] gcol.lut_lds", "[0] gcol.lut_len", "lut_class"]
    assert [(f[2], f[3]) for f in s["fields"][9:]] == [(9, 0), (10, 0), (10, 32), (11, 0), (12, 0), (11, 32), (13, 0), (13, 32), (14, 0)]
    r0, r1, r2 = s["records"]
    assert r0 == [256, 0, 1 << 20, 0x10000, 0x20000, 0x30000, 0, 0x50000, 0x60000, 0x70000, 200, (1 << 32) | 1, 0x70100, (300 << 32) | 208, 0]
    assert r1 == [513, 256, (1 << 20) + 1, 0x11000, 0x21000, 0x31000, 0x40000, 0x51000, 0x61000, 0x70000, 200, (1 << 32) | 1, 0x70100, (301 << 32) | 208, 0]
    assert r2 == [770, 513, (1 << 20) + 2, 0x12000, 0x22000, 0x32000, 0, 0x52000, 0x62000, 0x70800, 200, (1 << 32) | 1, 0x70900, (302 << 32) | 208, 1]


def test_computed_fields_and_words(dump):
    s = dump["computed"]
    # a compare leaf brings its literal only; a group LUT outside LDS neither offset nor length; the expression's literal node; the class fills the stride's word
    assert s["fields"] == [("tile_end", 64, 0, 0), ("tile_begin", 64, 1, 0), ("n_rows", 64, 2, 0), ("c4[0].values", 64, 3, 0), ("c8[0].values", 64, 4, 0),
                           ("[0] leaf.lit", 64, 5, 0), ("[0] gcol.lut", 64, 6, 0), ("[0] gcol.stride", 32, 7, 0), ("[1] expr.lit", 64, 8, 0), ("lut_class", 32, 7, 32)]
    assert s["W"] == 9 and s["records"] == [[1221, 0, 5000000, 0xA000, 0xB000, 0x4059000000000000, 0xC000, 7, 0x3FE0000000000000]]


def test_emitted_stride_is_the_packers(tool, dump):
    for k, name in enumerate(["headline", "two_phase", "computed"]):
        src = subprocess.run([tool, "source", str(k)], check=True, capture_output=True, text=True).stdout
        strides = set(re.findall(r"\(size_t\)(?:np|part) \* (\d+)", src))
        assert strides == {str(dump[name]["W"])}, (name, strides)
        assert len(re.findall(r"\bw\d+ = pw\[\d+\]", src)) == dump[name]["W"]


def test_stand_alone_under_sanitizers(tool, dump, tmp_path):
    san = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    # whether this toolchain has the sanitizers' runtimes at all is asked of a trivial program; the tool's own build must then succeed
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    p = subprocess.run(["g++"] + san + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True)
    if p.returncode != 0 or subprocess.run([str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("this toolchain has no sanitizer runtimes")
    exe = str(tmp_path / "part_table_dump_san")
    r = subprocess.run(FLAGS + san + SRC + ["-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "ERROR" not in out.stderr and "runtime error" not in out.stderr, out.stderr[-2000:]
    assert parse(out.stdout) == dump
    for k in range(3):
        src = subprocess.run([exe, "source", str(k)], capture_output=True, text=True)
        assert src.returncode == 0 and "runtime error" not in src.stderr and "fdb_plan_kernel" in src.stdout, src.stderr[-2000:]
