"""bench.py's plain run end to end on the device, at a small size: one JSON line whose ms_per_step times the --steps steps, nothing of
--full, and --dump-outputs writing the last timed step's result — checked here against the numpy restatement of the query over the
same seeded records."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.timeout(600)
def test_plain_run_times_the_headline_and_dumps_its_result(tmp_path):
    rows, batch, steps = 4_000_000, 1_000_000, 3
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--rows", str(rows), "--batch-rows", str(batch),
                        "--steps", str(steps), "--warmup", "1", "--dump-outputs", str(tmp_path / "out")],
                       capture_output=True, text=True, timeout=550, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, p.stdout
    line = json.loads(lines[0])
    assert line["steps"] == steps and line["ms_per_step"] > 0 and line["unit"] == "rows/s" and line["higher_is_better"] is True
    assert math.isclose(line["value"], rows / (line["ms_per_step"] * 1e-3), rel_tol=1e-6)
    assert "other_configs" not in line and line["cpu_baseline"] is None and line["checked"] is None
    assert line["roofline"]["measured_read_ceiling"] is None and line["roofline"]["kernel"] == "fdb_plan_kernel"

    import bench
    from frostdb_amd import synth
    exp_sum, exp_cnt = None, None
    for i in range(rows // batch):
        s, c = bench.expected_cfg2(synth.prometheus_chunk(0, i, batch, row_base=i * batch))
        exp_sum, exp_cnt = (s, c) if exp_sum is None else (exp_sum + s, exp_cnt + c)
    names = synth.PATHS + [None]
    present = sorted((i for i in range(len(names)) if exp_cnt[i] > 0), key=lambda i: (names[i] is None, names[i] or b""))
    out = {f: np.load(tmp_path / "out" / f) for f in os.listdir(tmp_path / "out")}
    assert set(out) == {"labels.path.npy", "sum_value.npy", "num_rows.npy"} and all(a.dtype == np.float64 for a in out.values())
    assert out["num_rows.npy"].tolist() == [len(present)]
    n_keys = sum(names[i] is not None for i in present)
    assert out["labels.path.npy"].tolist() == list(range(n_keys)) + [-1.0] * (len(present) - n_keys)
    assert np.allclose(out["sum_value.npy"], exp_sum[present], rtol=1e-9, atol=0.0)
