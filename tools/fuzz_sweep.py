#!/usr/bin/env python
"""Extended fuzz sweep (GPU box): the plan-vs-oracle fuzzers of tests/test_gpu_fuzz.py and the edge-value cases of
tests/test_gpu_edges_fuzz.py (every composition mode) over seeds the suite does not hold.
   python tools/fuzz_sweep.py [first seed = 1000] [count = 300]     — prints the seeds that disagree (none expected)."""
import os, sys, traceback
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pytest
from frostdb_amd import comm as fcomm
from frostdb_amd import physicalplan as pp
from tests import test_gpu_edges_fuzz as E
from tests import test_gpu_fuzz as F

first = int(sys.argv[1]) if len(sys.argv) > 1 else 1000
count = int(sys.argv[2]) if len(sys.argv) > 2 else 300
cases = [(F.test_fuzz_plan_vs_oracle.__name__, lambda seed, mp: F.test_fuzz_plan_vs_oracle(pp, seed, mp)),
         (F.test_fuzz_plain_strings_and_bools_vs_oracle.__name__, lambda seed, mp: F.test_fuzz_plain_strings_and_bools_vs_oracle(pp, seed))]
cases += [(f"edges_{m}", lambda seed, mp, m=m: E.edge_case(pp, fcomm, m, seed, mp)) for m in E.MODES]
bad, n = [], 0
for seed in range(first, first + count):
    for name, fn in cases:
        if name.startswith("edges_") and E.MODES[seed % len(E.MODES)] != name[6:]:
            continue  # (one edge mode per seed, as in the suite)
        mp = pytest.MonkeyPatch()
        n += 1
        try:
            fn(seed, mp)
        except Exception as e:  # noqa: BLE001
            bad.append((name, seed))
            traceback.print_exc(limit=3)
            if isinstance(e, pp.FdbError) and e.code in (pp.FDB_ERR_DEVICE, pp.FDB_ERR_OOM):
                mp.undo()  # a faulted device or exhausted memory: nothing after it would mean anything — stop here
                print(f"stopped at {name} seed {seed}: {e}")
                sys.exit(1)
        finally:
            mp.undo()
print(f"seeds {first} … {first + count - 1}: {n} cases, {len(bad)} disagree {bad}")
