"""The dense plan kernel with narrow index slots compiles for gfx950 — checked without a GPU, like tests/test_jit_sources_cpu.py: a 1-byte
filter slot plus a 2-byte group slot (the records' narrow-index caches, fdb_record.h), single-phase, two-phase and with per-wave tables.
The sources must hold the narrow loads, and none may spill to scratch memory."""
import os
import subprocess

import pytest

from tests.jit_corpus import NARROW
from tests.test_jit_sources_cpu import HIPCC, ROOT, jit_dump  # noqa: F401  (the fixture builds tools/jit_dump.cpp)

SHAPES = NARROW


@pytest.mark.parametrize("name,args", SHAPES, ids=[s[0] for s in SHAPES])
def test_narrow_plan_kernels_compile_for_gfx950(jit_dump, name, args):  # noqa: F811
    exe, out = jit_dump
    src = subprocess.run([exe] + args, check=True, capture_output=True, text=True).stdout
    wide = subprocess.run([exe] + args[:2], check=True, capture_output=True, text=True).stdout
    assert "void fdb_plan_kernel(" in src
    body = src[src.index("void fdb_plan_kernel("):]
    assert " = ld1x4(P_e4_0_v + tile_off1, lane_off1);" in body, name
    group_reg = "l4_0" if args[1] == "two" else "e4_1"
    assert " = ld2x4(P_%s_v + tile_off2, lane_off2);" % group_reg in body, name
    assert "ld4(" not in body, name  # both dictionary slots are narrow
    wide_body = wide[wide.index("void fdb_plan_kernel("):]
    assert "ld1x4(" not in wide_body and "ld2x4(" not in wide_body and wide_body.count("ld4(") == 2, name  # the 4-byte shape is what it was
    path = str(out / (name + ".hip"))
    with open(path, "w") as f:
        f.write(src)
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-munsafe-fp-atomics", "-DFDB_DEVICE_ONLY=1", "-include", "hip/hip_runtime.h",
                        "-I", os.path.join(ROOT, "frostdb_amd", "csrc"), "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", path, "-o", path + ".o"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    scratch = [ln for ln in r.stderr.splitlines() if "ScratchSize" in ln]
    assert scratch and all("ScratchSize [bytes/lane]: 0" in ln for ln in scratch), scratch
