"""Writes tests/golden/go_reference.json: what tests/test_go_shim_cpu.py needs to know about the FrostDB tree the Go drop-in targets,
as data only (no source text), so that the suite does not need that tree.

  python tools/gen_go_reference_fixture.py <frostdb checkout>

- ``physicalplan_names`` / ``logicalplan_names``: the top-level identifiers (type / func / var / const, grouped const / var blocks
  included) of query/physicalplan and query/logicalplan, test files excluded;
- ``physicalplan_go``: query/physicalplan/physicalplan.go as a SHA-256 prefix per line (what the Build patch's hunks must match,
  at fuzz 0), the bracket counts of its code (comments and literals blanked) and how often the strings the patch test looks for
  occur in it.
"""
import hashlib
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests.test_go_shim_cpu import PP_MARKERS, go_code, line_hash  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "go_reference.json")


def defined(pkg_dir):
    names = set()
    for fn in sorted(os.listdir(pkg_dir)):
        if fn.endswith(".go") and not fn.endswith("_test.go"):
            text = open(os.path.join(pkg_dir, fn)).read()
            names |= set(re.findall(r"^(?:type|func|var|const) (\w+)", text, flags=re.M))
            for block in re.findall(r"^(?:const|var) \((.*?)^\)", text, flags=re.M | re.S):
                names |= set(re.findall(r"^\t(\w+)", block, flags=re.M))
    return sorted(names)


def main(ref):
    pp_go = open(os.path.join(ref, "query", "physicalplan", "physicalplan.go")).read()
    code = go_code(pp_go)
    fixture = {
        "physicalplan_names": defined(os.path.join(ref, "query", "physicalplan")),
        "logicalplan_names": defined(os.path.join(ref, "query", "logicalplan")),
        "physicalplan_go": {
            "line_sha256_16": [line_hash(ln) for ln in pp_go.split("\n")],
            "code_brackets": {c: code.count(c) for c in "{}()"},
            "markers": {m: pp_go.count(m) for m in PP_MARKERS},
        },
    }
    with open(OUT, "w") as f:
        json.dump(fixture, f, indent=0)
        f.write("\n")
    print(OUT)


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
