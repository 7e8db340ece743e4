"""The quad form of the dense plan kernel (JitShape::quad: a launch with a narrow slot) compiles for gfx950 — checked without a GPU, like
tests/test_jit_narrow_sources_cpu.py, whose three shapes are dumped here with the flag set, plus the same single-phase shape at 256 and
at 512 threads per workgroup. A wave's full 1 024-row block reads its narrow slots with 16-byte loads of the wave-interleaved cache
(fdb_record.h, scan_cache_position): one per lane for the 1-byte filter column, two for the 2-byte group column; the record's last,
partial block keeps the direct loads at row-order offsets. None may spill to scratch memory. The VGPR count of each shape goes to the
test's log (pytest -s, or the captured output of a failure): the geometry table in DESIGN.md §3 quotes it."""
import os
import re
import subprocess

import pytest

from tests.jit_corpus import QUAD
from tests.test_jit_sources_cpu import HIPCC, ROOT, jit_dump  # noqa: F401  (the fixture builds tools/jit_dump.cpp)

# (name, jit_dump arguments, threads per workgroup: what the tool gives the variant, or the fourth argument)
SHAPES = [(name, args, int(args[3]) if len(args) > 3 else 256 if args[1] == "wave" else 512) for name, args in QUAD]


@pytest.mark.parametrize("name,args,block", SHAPES, ids=[s[0] for s in SHAPES])
def test_quad_plan_kernels_compile_for_gfx950(jit_dump, name, args, block):  # noqa: F811
    exe, out = jit_dump
    src = subprocess.run([exe] + args, check=True, capture_output=True, text=True).stdout
    assert "__launch_bounds__(%d) void fdb_plan_kernel(" % block in src, name
    body = src[src.index("void fdb_plan_kernel("):]
    group_reg = "l4_0" if args[1] == "two" else "e4_1"
    # the unit of work: block x 16 rows, a wave's block of 1 024 inside it
    assert "const long long wb = (tile - tile_begin) * %dLL + (long long)wave * 1024;" % (block * 16) in body, name
    # a full block: the 16-byte index loads, one at 1 byte per index, two 1 KiB apart at 2
    assert "const u32x4 Q_e4_0 = ldblock(P_e4_0_v + (size_t)wb, lane * 16u);" in body, name
    assert ("const u32x4 Q_%sa = ldblock(P_%s_v + (size_t)wb * 2, lane * 16u), Q_%sb = ldblock(P_%s_v + (size_t)wb * 2 + 1024, lane * 16u);" % ((group_reg,) * 4)) in body, name
    assert body.count("ldblock(") == 3, name
    assert "const u32x4 e4_0 = idx1x4(dword_of(Q_e4_0, u));" in body, name
    # a partial block: the direct loads, once each
    assert body.count("ld1x4(") == 1 and body.count("ld2x4(") == 1 and "ld4(" not in body, name
    # the barriers stay in the record-entry code, in front of the wave-uniform branch
    loop = body[body.index("const long long wb = "):]
    loop = loop[:loop.index("\n  }\n")]  # … to the end of the grid-stride loop
    assert "if (wb + 1024 <= n_rows) {" in loop and "#pragma unroll 1" in loop and "__syncthreads" not in loop, name
    path = str(out / (name + ".hip"))
    with open(path, "w") as f:
        f.write(src)
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-munsafe-fp-atomics", "-DFDB_DEVICE_ONLY=1", "-include", "hip/hip_runtime.h",
                        "-I", os.path.join(ROOT, "frostdb_amd", "csrc"), "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", path, "-o", path + ".o"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    scratch = [ln for ln in r.stderr.splitlines() if "ScratchSize" in ln]
    assert scratch and all("ScratchSize [bytes/lane]: 0" in ln for ln in scratch), scratch
    vgprs = re.findall(r" VGPRs: (\d+)", r.stderr)
    assert vgprs, r.stderr[-2000:]
    print("%s: %s VGPRs, %d threads per workgroup" % (name, vgprs[0], block))
