"""The generated dense scan over packed index caches (frostdb_amd/csrc/fdb_record.h: form H, 4 bits per index; form T, 12 bits as a byte
plane and a nibble plane), without a GPU.

  isa     bench.py's headline shape (`labels.code == '200'`, SUM(value) GROUP BY labels.path) with `code` at H and `path` at T, compiled for
          gfx950: the straight-line head of a full 1 024-row block holds 11 vector loads — 9 of 16 bytes (path's low bytes + 4 x 2 of value)
          and 2 of 8 bytes (the two nibble words) —, all in front of the first branch; no byte or short load sits in the block path; no
          scratch and no spills; the VGPR count is printed beside that of the byte-form shape.
  text    the source of the packed shapes below is pinned by SHA-256 (tests/golden/jit_packed_digests.json; FDB_WRITE_JIT_DIGESTS=1 rewrites
          it), and the two existing golden files (tests/golden/jit_source_digests.json, jit_part_table_digests.json) are reproduced unchanged."""
import hashlib
import json
import os
import re
import subprocess

import pytest

from tests.jit_corpus import CORPUS
from tests.jit_corpus_part_table import PART_TABLE
from tests.test_jit_quad_isa_cpu import compile_asm
from tests.test_jit_sources_cpu import ROOT, jit_dump  # noqa: F401  (the fixture builds tools/jit_dump.cpp)

DIGESTS = os.path.join(ROOT, "tests", "golden", "jit_packed_digests.json")
PART_DIGESTS = os.path.join(ROOT, "tests", "golden", "jit_part_table_digests.json")
SOURCE_DIGESTS = os.path.join(ROOT, "tests", "golden", "jit_source_digests.json")

# (name, jit_dump arguments): `packed` in the place of `narrow`
PACKED = [
    ("headline_packed", ["plan", "lds", "packed", "256", "sum", "nonull"]),
    ("headline_packed_ptab", ["plan", "lds", "packed", "256", "sum", "nonull", "ptab"]),
    ("headline_packed_bitmaps", ["plan", "lds", "packed", "256", "sum"]),
    ("two_phase_packed", ["plan", "two", "packed", "256"]),
    ("wave_tables_packed", ["plan", "wave", "packed", "256"]),
    ("cfg3_packed", ["plan", "two", "packed", "256", "cfg3"]),
]


def block_head(asm):
    """(lines, begin, end, tail): the kernel's instructions and labels; the full-block path's head, lines[begin:end], from behind the branch
    that chooses between a full and a partial block to the first branch behind the path's loads; and the index of the label that branch
    jumps to, where the partial block's path begins. The full-block path is told by the 8-byte load of form T's nibble plane, 1 KiB behind
    the frame's low bytes: only a full block has it."""
    lines = [ln.strip() for ln in asm.splitlines()]
    lines = [ln for ln in lines if ln and not ln.startswith((";", "//")) and (not ln.startswith(".") or re.match(r"\.LBB\d+_\d+:", ln))]
    marks = [i for i, ln in enumerate(lines) if re.match(r"global_load_dwordx2 .*offset:1024 nt$", ln)]
    assert len(marks) == 1, marks
    choose = max(i for i in range(marks[0]) if lines[i].startswith("s_cbranch_"))
    end = min(i for i in range(marks[0], len(lines)) if lines[i].startswith("s_cbranch_"))
    assert not any(ln.startswith(".LBB") for ln in lines[choose:end]), lines[choose:end]  # straight-line: no label inside
    target = lines[choose].split()[-1] + ":"
    tail = [i for i, ln in enumerate(lines) if ln.split()[0] == target]
    assert len(tail) == 1 and tail[0] > end, (lines[choose], tail)
    return lines, choose + 1, end, tail[0]


def test_headline_shape_at_h_and_t(jit_dump):  # noqa: F811
    exe, out = jit_dump
    src = subprocess.run([exe] + PACKED[0][1], check=True, capture_output=True, text=True).stdout
    bytes_src = subprocess.run([exe, "plan", "lds", "narrow", "256", "sum", "nonull"], check=True, capture_output=True, text=True).stdout
    asm, log = compile_asm(src, str(out / "headline_packed.hip"))
    _, log_b = compile_asm(bytes_src, str(out / "headline_bytes.hip"))
    lines, begin, end, tail = block_head(asm)
    loads = [ln.split()[0] for ln in lines[begin:end] if ln.startswith("global_load")]
    vgprs, vgprs_b = re.findall(r" VGPRs: (\d+)", log)[:1], re.findall(r" VGPRs: (\d+)", log_b)[:1]
    print("headline at H / T: loads before the first branch %s, VGPRs %s (byte forms: %s)" % (sorted(loads), vgprs, vgprs_b))
    assert sorted(loads) == ["global_load_dwordx2"] * 2 + ["global_load_dwordx4"] * 9, loads
    # No byte or short load in the block path. The whole kernel holds exactly the partial block's two 2-byte nibble loads (one of H, one of
    # T) and no byte load, and both sit behind the label the full-or-partial branch jumps to: had one been sunk into a sub-step of the full
    # block, the kernel would hold a third, or one in front of that label.
    small = [i for i, ln in enumerate(lines) if re.match(r"global_load_(u|s)(byte|short)", ln)]
    assert [lines[i].split()[0] for i in small] == ["global_load_ushort"] * 2, [lines[i] for i in small]
    assert min(small) > tail, (small, tail)
    # … and every other load of the full-block path sits in its head: between the head's end and that label nothing is loaded
    assert not [ln for ln in lines[end:tail] if ln.startswith("global_load")], [ln for ln in lines[end:tail] if ln.startswith("global_load")]
    for what in ("ScratchSize [bytes/lane]", "SGPRs Spill", "VGPRs Spill"):
        found = [ln for ln in log.splitlines() if what in ln]
        assert found and all(re.search(re.escape(what) + r": 0\b", ln) for ln in found), found


def test_packed_sources_are_the_recorded_ones_and_the_old_ones_did_not_move(jit_dump):  # noqa: F811
    exe, _ = jit_dump
    got = {name: hashlib.sha256(subprocess.run([exe] + args, check=True, capture_output=True, text=True).stdout.encode()).hexdigest() for name, args in PACKED}
    if os.environ.get("FDB_WRITE_JIT_DIGESTS"):
        with open(DIGESTS, "w") as f:
            json.dump(got, f, indent=1, sort_keys=True)
            f.write("\n")
    with open(DIGESTS) as f:
        want = json.load(f)
    assert got == want, sorted(n for n in got if got[n] != want.get(n))
    # every shape of tests/jit_corpus.py generates what tests/golden/jit_source_digests.json recorded before the packed forms
    with open(SOURCE_DIGESTS) as f:
        pinned = json.load(f)
    assert sorted(pinned) == sorted(name for name, _ in CORPUS)
    for name, args in CORPUS:
        assert hashlib.sha256(subprocess.run([exe] + args, check=True, capture_output=True).stdout).hexdigest() == pinned[name], name
    # the byte-form shapes with the part table generate what tests/golden/jit_part_table_digests.json recorded before the packed forms
    with open(PART_DIGESTS) as f:
        old = json.load(f)
    for name, args in PART_TABLE:
        text = subprocess.run([exe] + args + ["ptab"], check=True, capture_output=True, text=True).stdout
        assert hashlib.sha256(text.encode()).hexdigest() == old[name]["sha256"], name
        assert "ldblock8" not in text and "idxTx4" not in text, name
