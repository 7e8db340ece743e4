"""fdb_plan_kernel with the packed part table on (JitShape::part_table; tools/jit_dump.cpp `ptab`), checked without a GPU.

  text        the source of every shape of tests/jit_corpus_part_table.py is pinned by SHA-256 (tests/golden/jit_part_table_digests.json;
              FDB_WRITE_JIT_DIGESTS=1 rewrites the file, the compiled figures included). With the table off the generator prints what it
              printed before: that is tests/test_jit_source_identity_cpu.py, whose digests this change leaves alone.
  record entry  the kernel has no FdbScanArgs array: its only FdbScanArgs is `c`, by value, and the tile loop takes every per-record value
              from `ptab`, W words apart, W being what the packer uses (tools/part_table_dump.cpp checks that side).
  compiled    each shape compiles for gfx950 without scratch; its VGPR count is recorded beside that of its twin without the table, and
              may not exceed it by more than 4 (the table's words replace the structure's fields one for one, so the record entry needs
              no more registers than before; 4 is slack for the allocator).
  scalar loads  the table's words reach the kernel through scalar loads, and no vector load is added over the twin's.
  block loads the headline's full-block path still issues its 3 index and 8 value loads, 16 bytes each, before its first branch
              (tests/test_jit_quad_isa_cpu.py's check, on the part-table source)."""
import hashlib
import json
import os
import re
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

from tests.jit_corpus_part_table import PART_TABLE
from tests.test_jit_quad_isa_cpu import KEEP_ALIVE, compile_asm, placement
from tests.test_jit_sources_cpu import ROOT, jit_dump  # noqa: F401  (the fixture builds tools/jit_dump.cpp)

DIGESTS = os.path.join(ROOT, "tests", "golden", "jit_part_table_digests.json")


@pytest.fixture(scope="module")
def built(jit_dump):  # noqa: F811
    """name → (source with the table, compile log, source without, compile log, assembly with the table, assembly without)"""
    exe, out = jit_dump

    def one(shape):
        name, args = shape
        on = subprocess.run([exe] + args + ["ptab"], check=True, capture_output=True, text=True).stdout
        off = subprocess.run([exe] + args, check=True, capture_output=True, text=True).stdout
        asm_on, log_on = compile_asm(on, str(out / ("ptab_" + name + ".hip")))
        asm_off, log_off = compile_asm(off, str(out / ("ptab_" + name + "_off.hip")))
        return name, (on, log_on, off, log_off, asm_on, asm_off)

    with ThreadPoolExecutor(max_workers=min(len(PART_TABLE), os.cpu_count() or 4, 16)) as ex:
        return dict(ex.map(one, PART_TABLE))


def vgprs(log):
    return int(re.search(r" VGPRs: (\d+)", log).group(1))


def test_sources_are_the_recorded_ones(built):
    got = {name: {"sha256": hashlib.sha256(b[0].encode()).hexdigest(), "vgprs": vgprs(b[1]), "vgprs_without_table": vgprs(b[3])} for name, b in built.items()}
    if os.environ.get("FDB_WRITE_JIT_DIGESTS"):
        with open(DIGESTS, "w") as f:
            json.dump(got, f, indent=1, sort_keys=True)
            f.write("\n")
    with open(DIGESTS) as f:
        want = json.load(f)
    assert sorted(want) == sorted(got)
    for name in sorted(got):
        print("%s: %d VGPRs with the table, %d without (recorded %d, %d)" % (name, got[name]["vgprs"], got[name]["vgprs_without_table"], want[name]["vgprs"], want[name]["vgprs_without_table"]))
    changed = sorted(name for name in got if got[name]["sha256"] != want[name]["sha256"])
    assert not changed, "the generated part-table source of %s changed" % ", ".join(changed)


@pytest.mark.parametrize("name", [n for n, _ in PART_TABLE])
def test_compiles_without_scratch_and_needs_no_more_registers(built, name):
    _, log_on, _, log_off, _, _ = built[name]
    for log in (log_on, log_off):
        scratch = [ln for ln in log.splitlines() if "ScratchSize" in ln]
        assert scratch and all("ScratchSize [bytes/lane]: 0" in ln for ln in scratch), scratch
    assert vgprs(log_on) <= vgprs(log_off) + 4, (vgprs(log_on), vgprs(log_off))


@pytest.mark.parametrize("name", [n for n, _ in PART_TABLE])
def test_record_entry_reads_the_table_only(built, name):
    on, _, off, _, _, _ = built[name]
    assert "const FdbScanArgs* __restrict__ parts" in off and "parts[" in off  # (the twin is the kernel this one replaces)
    assert "FdbScanArgs*" not in on and "FdbScanArgs&" not in on and "const FdbScanArgs c)" in on  # the by-value block, and no other
    assert "const unsigned long long* __restrict__ ptab" in on
    loop = on[on.index("for (long long tile = blockIdx.x;"):]
    assert not re.search(r"\bparts\b|\bpa\b", loop)
    strides = set(re.findall(r"\(size_t\)(?:np|part) \* (\d+)", loop))
    assert len(strides) == 1, strides  # the walk and the field reads agree on W
    W = int(strides.pop())
    assert [int(w) for w in re.findall(r"\bw(\d+) = pw\[\d+\]", loop)] == list(range(W))  # every word of the record, once
    used = {int(w) for w in re.findall(r"\(s(\d+)(?: >> 32)?\);", loop)}
    assert used == set(range(W)), (used, W)  # … and none that no field needs
    # pointers and tile bounds come back as scalars
    assert len(re.findall(r"\bs(\d+) = ptw\(w\d+\)", loop)) == W and "__builtin_amdgcn_readfirstlane" in on


@pytest.mark.parametrize("name", [n for n, _ in PART_TABLE])
def test_table_is_read_with_scalar_loads(built, name):
    """The table is read from global memory (no LDS copy): every lane of a wave reads the same words, and the compiler must see that —
    the record's W words arrive through wide scalar loads (8 or 16 dwords at a time; no shape here has W < 9), the kernel has no LDS
    store of table words in front of its loop, and no vector load is added over the twin's (the column loads are the only `nt` ones)."""
    on, _, _, _, asm_on, asm_off = built[name]
    assert not re.search(r"\blpt\b|\bptab_off\b", on)  # no LDS copy, no offset argument
    assert re.search(r"^\s*s_load_dwordx(8|16) ", asm_on, re.M), name
    plain = lambda asm: [ln for ln in asm.splitlines() if re.match(r"\s*global_load_dword", ln) and not ln.rstrip().endswith(" nt")]  # noqa: E731
    assert len(plain(asm_on)) <= len(plain(asm_off)), (len(plain(asm_on)), len(plain(asm_off)))


def test_headline_block_loads_leave_before_the_first_branch(built):
    for name in ("headline", "headline_nonull"):
        on, log, _, _, asm, _ = built[name]
        assert len(KEEP_ALIVE.findall(on)) == 1
        x4, ub, other, waits = placement(asm)
        want_ub = 8 if name == "headline" else 0  # a validity byte per dictionary column and sub-step, where the slots have bitmaps
        print("%s: %d 16-byte loads, %d validity bytes before the first branch, waits vmcnt %s" % (name, x4, ub, waits))
        assert (x4, ub) == (11, want_ub) and not other, (name, x4, ub, other)
        assert waits and waits[-1] > 0, (name, waits)
