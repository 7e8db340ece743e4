"""Where the loads of a quad shape's full 1 024-row block end up in the COMPILED kernel — checked without a GPU, on the assembly hipcc
produces with the options hiprtc gets. The generated source issues every load that does not wait for `sel` in front of sub-step 0
(Gen::block_loads), but the optimiser sinks a load whose only uses sit behind the first data-dependent branch below that branch: without
the keep-alive statement at the end of block_loads, sub-step 0's group validity byte and its two 16-byte value loads were issued behind
`has == 0` and waited for at once — a second memory round trip per block. Three properties per shape:

  load placement   the straight-line code that holds the block's 16-byte index loads, up to its first branch, holds every early load of the
                   block: single-phase shapes 3 index + 4 x 2 value loads (global_load_dwordx4) and 4 x 2 validity bytes
                   (global_load_ubyte); the two-phase shape what its slots say (late slots stay behind `sel`, which is their design);
  counted wait     the last wait for memory in front of that branch leaves loads in flight (vmcnt > 0);
  no scratch.

The test is its own negative control: the same source without the keep-alive statement must miss the first property wherever sub-step 0
has a load the filter does not read (every single-phase shape)."""
import os
import re
import subprocess

import pytest

from tests.jit_corpus import QUAD_ISA
from tests.test_jit_sources_cpu import HIPCC, ROOT, jit_dump  # noqa: F401  (the fixture builds tools/jit_dump.cpp)

# (name, jit_dump arguments, two_phase)
SHAPES = [(n, a, a[1] == "two") for n, a in QUAD_ISA]

KEEP_ALIVE = re.compile(r'^ *asm volatile\("" :: "v"\(.*\);\n', re.M)


def expected_loads(two_phase):
    """(16-byte loads, validity bytes) of a full block that do not wait for `sel`, from the slots tools/jit_dump.cpp gives the shape."""
    if two_phase:
        # early: the 1-byte filter column (1 index load, a validity byte per sub-step); the late 2-byte group column's 2 index loads
        # leave early as well. Its validity and the two late 8-byte columns wait for `sel`.
        return 1 + 2, 4
    # the 1-byte filter column, the 2-byte group column, one 8-byte column (2 loads per sub-step); a validity byte per dictionary column and sub-step
    return 1 + 2 + 4 * 2, 4 * 2


def compile_asm(src, path):
    with open(path, "w") as f:
        f.write(src)
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-munsafe-fp-atomics", "-DFDB_DEVICE_ONLY=1", "-include", "hip/hip_runtime.h",
                        "-I", os.path.join(ROOT, "frostdb_amd", "csrc"), "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-S", path, "-o", path + ".s"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    with open(path + ".s") as f:
        return f.read(), r.stderr


def full_block_head(asm):
    """The instructions from the first 16-byte non-temporal load of the full-block path to the first branch behind it. The path is
    told by the group column's second index load, 1 KiB behind the first: only a full block has it."""
    lines = [ln.strip() for ln in asm.splitlines()]
    lines = [ln for ln in lines if ln and not ln.startswith((";", ".", "//"))]
    marks = [i for i, ln in enumerate(lines) if re.match(r"global_load_dwordx4 .*offset:1024 nt$", ln)]
    assert len(marks) == 1, marks
    begin = max(i for i in range(marks[0]) if lines[i].startswith("s_cbranch_")) + 1
    end = min(i for i in range(marks[0], len(lines)) if lines[i].startswith("s_cbranch_"))
    head = lines[begin:end]
    first = min(i for i, ln in enumerate(head) if re.match(r"global_load_dwordx4 .* nt$", ln))
    assert not any(ln.startswith("global_load") for ln in head[:first]), head[:first]
    return head[first:]


def placement(asm):
    head = full_block_head(asm)
    x4 = sum(1 for ln in head if ln.startswith("global_load_dwordx4 "))
    ub = sum(1 for ln in head if ln.startswith("global_load_ubyte "))
    other = [ln for ln in head if ln.startswith("global_load") and not ln.startswith(("global_load_dwordx4 ", "global_load_ubyte "))]
    waits = [int(m.group(1)) for ln in head if ln.startswith("s_waitcnt") for m in [re.search(r"vmcnt\((\d+)\)", ln)] if m]
    return x4, ub, other, waits


@pytest.mark.parametrize("name,args,two_phase", SHAPES, ids=[s[0] for s in SHAPES])
def test_full_block_loads_leave_before_the_first_branch(jit_dump, name, args, two_phase):  # noqa: F811
    exe, out = jit_dump
    src = subprocess.run([exe] + args, check=True, capture_output=True, text=True).stdout
    assert len(KEEP_ALIVE.findall(src)) == 1, name
    want = expected_loads(two_phase)
    asm, log = compile_asm(src, str(out / (name + "_isa.hip")))
    x4, ub, other, waits = placement(asm)
    vgprs = re.findall(r" VGPRs: (\d+)", log)
    print("%s: %d 16-byte loads and %d validity bytes before the first branch (want %d, %d), waits vmcnt %s, %s VGPRs" % (name, x4, ub, want[0], want[1], waits, vgprs[:1]))
    assert (x4, ub) == want and not other, (name, x4, ub, other)
    assert waits and waits[-1] > 0, (name, waits)
    scratch = [ln for ln in log.splitlines() if "ScratchSize" in ln]
    assert scratch and all("ScratchSize [bytes/lane]: 0" in ln for ln in scratch), scratch
    # negative control: without the keep-alive the optimiser sinks sub-step 0's group validity byte and value loads below the branch
    if not two_phase:
        asm0, _ = compile_asm(KEEP_ALIVE.sub("", src), str(out / (name + "_isa_sunk.hip")))
        x4_0, ub_0, _, _ = placement(asm0)
        print("%s without the keep-alive: %d 16-byte loads and %d validity bytes before the first branch" % (name, x4_0, ub_0))
        assert (x4_0, ub_0) != want and x4_0 <= want[0] and ub_0 < want[1], (name, x4_0, ub_0)
