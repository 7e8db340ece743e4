"""CPU-side checks of Take / Limit / the reservoir Sampler: the entry points exist, the library's row selection equals the Python
restatement (tests/sampler_oracle.py) draw for draw and is uniform, the kernels of fdb_take.hip compile for gfx950 without scratch, and
the host-only half runs clean under AddressSanitizer as a stand-alone program. No GPU is touched."""
import os
import re
import subprocess

import pytest

from tests import sampler_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

ENTRY_POINTS = ["fdb_batch_take", "fdb_batch_limit", "fdb_sampler_create", "fdb_sampler_push_batch", "fdb_sampler_push", "fdb_sampler_finish_batch",
                "fdb_sampler_finish", "fdb_sampler_close", "fdb_selftest_reservoir"]
# (K, rows of the records pushed in turn)
SHAPES = [(5, [7, 1, 12]), (3, [3, 5000]), (64, [1, 64, 65, 1000]), (1, [1, 1, 1, 1, 1, 1]), (4, [4, 5]), (10, [4, 5]), (0, [4, 5]), (5, [0, 7, 0, 13])]


def test_entry_points_are_in_library_header_and_exports_map():
    import fnmatch
    from frostdb_amd import physicalplan as pp
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "frostdb_amd.h")).read(), flags=re.S)
    version_script = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "frostdb_amd", "csrc", "exports.map")).read(), flags=re.S)
    patterns = re.findall(r"global:\s*([^;]+);", version_script)
    assert patterns
    L = pp.lib()
    for name in ENTRY_POINTS:
        assert hasattr(L, name), name
        assert re.search(r"^FDB_API (?:int|void) %s\(" % name, header, flags=re.M), name
        assert any(fnmatch.fnmatchcase(name, p.strip()) for p in patterns), name
    for cls in ("Limiter", "ReservoirSampler"):
        assert hasattr(pp, cls)
    assert hasattr(pp.ResidentBatch, "take")
    assert pp.Limiter(7).Draw() == "Limit(7)"


@pytest.mark.parametrize("size,lens", SHAPES, ids=[f"K{k}-{'_'.join(map(str, l))}" for k, l in SHAPES])
def test_selection_equals_the_restatement(size, lens):
    from frostdb_amd.physicalplan import selftest_reservoir
    total = sum(lens)
    for seed in range(200):
        got = selftest_reservoir(seed, size, lens)
        assert got == sampler_oracle.sample(seed, size, lens), (seed, size, lens)
        assert len(got) == min(size, total)
        assert len(set(got)) == len(got) and all(0 <= r < total for r in got), (seed, got)


def test_selection_is_uniform():
    """K = 5 of the 20 rows of records [7, 1, 12], seeds 0 … 3999: every row is kept 1000 times in expectation, binomial sd
    sqrt(4000 · ¼ · ¾) = 27.4; each count must lie within 6 sd (1000 ± 165). The restatement alone is 1.7 sd off at worst on these
    seeds and the library equals it (test above), so the bound has room for nothing but a broken selection."""
    from frostdb_amd.physicalplan import selftest_reservoir
    counts = [0] * 20
    for seed in range(4000):
        for r in selftest_reservoir(seed, 5, [7, 1, 12]):
            counts[r] += 1
    print("kept per row:", counts)
    assert sum(counts) == 4000 * 5
    assert all(abs(c - 1000) <= 165 for c in counts), counts


def test_selection_refuses_bad_arguments():
    from frostdb_amd import physicalplan as pp
    with pytest.raises(pp.FdbError) as e:
        pp.selftest_reservoir(1, -1, [3])
    assert e.value.code == pp.FDB_ERR_INVALID
    with pytest.raises(pp.FdbError) as e:
        pp.selftest_reservoir(1, 2, [3, -4])
    assert e.value.code == pp.FDB_ERR_INVALID


def test_take_kernels_compile_for_gfx950_without_scratch(tmp_path):
    """The ahead-of-time kernels of fdb_take.hip, compiled offline for gfx950: the compiler's resource report shows both kernels, no
    scratch and no spills."""
    src = os.path.join(ROOT, "frostdb_amd", "csrc", "fdb_take.hip")
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-munsafe-fp-atomics", "-I", os.path.join(ROOT, "frostdb_amd", "csrc"),
                        "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", str(tmp_path / "fdb_take.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    remarks = [ln.split("remark: ")[-1].replace(" [-Rpass-analysis=kernel-resource-usage]", "").strip() for ln in r.stderr.splitlines() if "remark:" in ln]
    names = [u for u in remarks if u.startswith("Function Name:")]
    print(" | ".join(remarks))
    assert any("take_kernel" in u for u in names) and any("scatter_kernel" in u for u in names), names
    scratch = [u for u in remarks if "ScratchSize" in u]
    assert len(scratch) == len(names) and all("ScratchSize [bytes/lane]: 0" in u for u in scratch), remarks
    spills = [u for u in remarks if "Spill" in u]
    assert spills and all(re.search(r"Spill: 0\b", u) for u in spills), remarks


def test_host_code_is_clean_under_address_sanitizer():
    """tools/asan_sampler.sh: the selection, the dictionary union / translation tables and the index validation in a stand-alone
    program built with -fsanitize=address,undefined (no GPU, not inside python)."""
    r = subprocess.run(["bash", os.path.join(ROOT, "tools", "asan_sampler.sh")], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    assert "asan sampler ok" in r.stdout
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
