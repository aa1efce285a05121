"""bench.py's plain one-GPU run with the real env: a lean result line, and `--dump-outputs` writing the same last-step
outputs from two runs with the same arguments (what lets two builds be compared output for output)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

NAMES = ("observation", "reward", "discount", "step_type")


@pytest.mark.gpu
@pytest.mark.timeout(600)
def test_plain_run_dumps_identical_outputs(tmp_path):
    runs = []
    for name in ("a", "b"):
        out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "12", "--warmup", "3",
                              "--envs-per-gpu", "1024", "--dump-outputs", str(tmp_path / name)],
                             capture_output=True, text=True, timeout=280)
        assert out.returncode == 0, out.stderr[-2000:]
        lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 1
        d = json.loads(lines[0])
        assert d["steps"] == 12 and d["ms_per_step"] > 0 and d["value"] > 0 and d["unit"] == "env-steps/s" and d["dtype"] == "f32"
        assert not {"roofline", "async_groups", "capacity", "cpu_baseline"} & set(d)
        runs.append({n: np.load(tmp_path / name / (n + ".npy")) for n in NAMES})
    a, b = runs
    assert a["observation"].shape == (1024, 104) and all(a[n].shape == (1024,) for n in NAMES[1:])
    assert np.isfinite(a["observation"]).all() and np.isfinite(a["reward"]).all()
    for n in NAMES:
        np.testing.assert_array_equal(a[n], b[n], err_msg=n)
