"""The text of every generated kernel is pinned: tests/golden/jit_source_digests.json holds the SHA-256 of the source tools/jit_dump.cpp
prints for each shape of tests/jit_corpus.py. A compiled kernel depends on nothing but that text (the process cache is keyed by the
shape, the disk cache by the source), so a change of the generator (fdb_jitgen.cpp) that leaves every digest alone changes no
behaviour, no register allocation and no cache entry — and one that means to change a kernel says which shapes it changed:

    FDB_WRITE_JIT_DIGESTS=1 python -m pytest tests/test_jit_source_identity_cpu.py

rewrites the file from the sources of this tree. No GPU is touched and nothing is compiled for one."""
import hashlib
import json
import os
import subprocess
from concurrent.futures import ThreadPoolExecutor

from tests.jit_corpus import CORPUS
from tests.test_jit_sources_cpu import ROOT, jit_dump  # noqa: F401  (the fixture builds tools/jit_dump.cpp)

DIGESTS = os.path.join(ROOT, "tests", "golden", "jit_source_digests.json")


def test_generated_sources_are_the_recorded_ones(jit_dump):  # noqa: F811
    exe, out = jit_dump

    def one(shape):
        name, args = shape
        first = subprocess.run([exe] + args, check=True, capture_output=True).stdout
        again = subprocess.run([exe] + args, check=True, capture_output=True).stdout
        assert first == again and len(first) > 1000, name  # deterministic, and a kernel
        return name, first

    with ThreadPoolExecutor(max_workers=min(len(CORPUS), os.cpu_count() or 4, 16)) as ex:
        sources = dict(ex.map(one, CORPUS))
    got = {name: hashlib.sha256(src).hexdigest() for name, src in sources.items()}
    if os.environ.get("FDB_WRITE_JIT_DIGESTS"):
        with open(DIGESTS, "w") as f:
            json.dump(got, f, indent=1, sort_keys=True)
            f.write("\n")
    with open(DIGESTS) as f:
        want = json.load(f)
    assert sorted(want) == sorted(got), (sorted(set(want) - set(got)), sorted(set(got) - set(want)))
    changed = sorted(name for name in got if got[name] != want[name])
    for name in changed:  # what the generator prints now, for a diff against the parent's
        with open(str(out / (name + ".changed.hip")), "wb") as f:
            f.write(sources[name])
    assert not changed, "the generated source of %s changed (new text: %s/<shape>.changed.hip)" % (", ".join(changed), out)
