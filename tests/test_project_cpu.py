"""The Projection operator without a GPU: the C ABI's new struct and symbols, and the kernels fdb_jitgen.cpp generates for the expression
sets of tests/test_gpu_project.py's differential test — compiled offline for gfx950 the way test_jit_sources_cpu.py does it for the
other generated kernels (a source that does not compile, or spills, would only show on the GPU box)."""
import ctypes
import glob
import os
import re
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

from tests.jit_corpus import PROJECT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def _c_sizeof(tmp_path, type_name: str) -> dict:
    """sizeof / offsets of `type_name` as the C compiler sees include/frostdb_amd.h."""
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "frostdb_amd.h"\n'
                   'int main(void) { printf("%zu %zu %zu\\n", sizeof(' + type_name + '), offsetof(' + type_name + ', kind), offsetof(' + type_name + ', name)); return 0; }\n')
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    size, off_kind, off_name = (int(x) for x in subprocess.check_output([str(exe)]).split())
    return {"size": size, "kind": off_kind, "name": off_name}


def test_project_col_matches_ctypes_mirror(tmp_path):
    from frostdb_amd.physicalplan import ProjectCol
    c = _c_sizeof(tmp_path, "fdb_project_col")
    assert c["size"] == ctypes.sizeof(ProjectCol) == 16
    assert c["kind"] == ProjectCol.kind.offset == 0
    assert c["name"] == ProjectCol.name.offset == 8


def test_project_symbols_are_exported():
    from frostdb_amd import build
    lib = ctypes.CDLL(build.build())
    for sym in ("fdb_plan_project_batch", "fdb_plan_project_batches", "fdb_plan_project"):
        assert hasattr(lib, sym), sym
    # …and in the header, with the prototypes the issue fixes
    text = open(os.path.join(ROOT, "include", "frostdb_amd.h")).read()
    for sym in ("fdb_plan_project_batch(", "fdb_plan_project_batches(", "fdb_plan_project("):
        assert "FDB_API int " + sym in text, sym


def test_filter_only_descriptor_with_projections_is_valid():
    """A plan with n_aggs == 0, n_groups == 0 and n_projections > 0 (what physicalplan.Projection creates): the descriptor carries the
    computed expressions under their Name() / alias and nothing else."""
    from frostdb_amd.logicalplan import Col, Literal, AliasExpr, to_desc
    exprs = [Col("value") * Col("timestamp"), (Col("a") / Col("b")).Alias("q"), AliasExpr(Literal(7), "seven"), Col("a").Alias("aa")]
    d = to_desc(None, [], [], projections=exprs).desc
    assert (d.n_aggs, d.n_groups, d.n_filter) == (0, 0, 0)
    assert [d.projections[i].name.decode() for i in range(d.n_projections)] == ["value * timestamp", "q", "seven", "aa"]
    assert d.projections[2].n_nodes == 1 and d.projections[2].nodes[0].kind == 1  # a literal root
    assert d.projections[3].n_nodes == 1 and d.projections[3].nodes[0].kind == 0  # an aliased column


@pytest.fixture(scope="module")
def jit_dump(tmp_path_factory):
    from frostdb_amd import build
    lib = build.build()
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc on this host")
    out = tmp_path_factory.mktemp("jit_project")
    exe = str(out / "jit_dump")
    objs = sorted(glob.glob(os.path.join(os.path.dirname(lib), "csrc", "*.o")))
    assert objs, "frostdb_amd/csrc/*.o missing: build.build() keeps them next to the sources"
    subprocess.check_call(["g++", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROOT, "frostdb_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                           "-I", "/opt/rocm/include", os.path.join(ROOT, "tools", "jit_dump.cpp")] + objs +
                          ["-L/opt/rocm/lib", "-lamdhip64", "-lhiprtc", "-ldl", "-lpthread", "-lz", "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    return exe, out


def test_project_kernels_compile_for_gfx950_without_scratch(jit_dump):
    exe, out = jit_dump

    def one(shape):
        name, args = shape
        src = subprocess.run([exe] + args, check=True, capture_output=True, text=True).stdout
        assert "void fdb_project_kernel(" in src, name
        path = str(out / (name + ".hip"))
        with open(path, "w") as f:
            f.write(src)
        r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-munsafe-fp-atomics", "-DFDB_DEVICE_ONLY=1", "-include", "hip/hip_runtime.h",
                            "-I", os.path.join(ROOT, "frostdb_amd", "csrc"), "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", path, "-o", path + ".o"],
                           capture_output=True, text=True)
        usage = [ln.split("remark: ")[-1].replace(" [-Rpass-analysis=kernel-resource-usage]", "") for ln in r.stderr.splitlines() if "remark:" in ln and ("ScratchSize" in ln or "VGPRs:" in ln or "SGPRs:" in ln or "LDS Size" in ln or "Spill" in ln)]
        return name, r.returncode, r.stderr if r.returncode else "", usage

    with ThreadPoolExecutor(max_workers=min(len(PROJECT), os.cpu_count() or 4)) as ex:
        results = list(ex.map(one, PROJECT))
    failed = [(n, err[-2000:]) for n, rc, err, _ in results if rc != 0]
    assert not failed, failed
    for name, _, _, usage in results:
        print(name, "|", " | ".join(u.strip() for u in usage))
        scratch = [u for u in usage if "ScratchSize" in u]
        assert scratch and all("ScratchSize [bytes/lane]: 0" in u for u in scratch), (name, usage)
        assert all(re.search(r"Spill: 0\b", u) for u in usage if "Spill" in u), (name, usage)
