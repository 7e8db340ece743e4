"""The exact-sum variant of the run-time generated hash kernel (fdb_jitgen.cpp, JitHashShape::exact: limb adds through fdb_exact_add_wave
after the tile's probes) compiles for gfx950 without spilling — checked here, without a GPU, with the options hiprtc gets."""
import glob
import os
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

from tests.jit_corpus import EXACT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

SHAPES = EXACT


def test_exact_hash_kernels_compile_for_gfx950(tmp_path):
    from frostdb_amd import build
    lib = build.build()
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc on this host")
    objs = sorted(glob.glob(os.path.join(os.path.dirname(lib), "csrc", "*.o")))
    assert objs, "frostdb_amd/csrc/*.o missing: build.build() keeps them next to the sources"
    exe = str(tmp_path / "jit_dump")
    subprocess.check_call(["g++", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROOT, "frostdb_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                           "-I", "/opt/rocm/include", os.path.join(ROOT, "tools", "jit_dump.cpp")] + objs +
                          ["-L/opt/rocm/lib", "-lamdhip64", "-lhiprtc", "-ldl", "-lpthread", "-lz", "-Wl,-rpath,/opt/rocm/lib", "-o", exe])

    def one(shape):
        name, args = shape
        src = subprocess.run([exe] + args, check=True, capture_output=True, text=True).stdout
        assert "void fdb_hash_kernel(" in src and "fdb_exact_add_wave(" in src, name
        path = str(tmp_path / (name + ".hip"))
        with open(path, "w") as f:
            f.write(src)
        r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-munsafe-fp-atomics", "-DFDB_DEVICE_ONLY=1", "-include", "hip/hip_runtime.h",
                            "-I", os.path.join(ROOT, "frostdb_amd", "csrc"), "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", path, "-o", path + ".o"],
                           capture_output=True, text=True)
        scratch = [ln for ln in r.stderr.splitlines() if "ScratchSize" in ln]
        return name, r.returncode, r.stderr if r.returncode else "", scratch

    with ThreadPoolExecutor(max_workers=len(SHAPES)) as ex:
        results = list(ex.map(one, SHAPES))
    failed = [(n, err[-2000:]) for n, rc, err, _ in results if rc != 0]
    assert not failed, failed
    spilled = [(n, s) for n, _, _, s in results if s and not all("ScratchSize [bytes/lane]: 0" in ln for ln in s)]
    assert not spilled, spilled
