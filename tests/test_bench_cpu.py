"""bench.py without a GPU: the plain run's result line and `--dump-outputs`, on the N>1 control flow rehearsed with gloo and
the stand-in env (FLYBODY_BENCH_FAKE), and the seeded row sample that keeps a large dump within its limit."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

NAMES = ("observation", "reward", "discount", "step_type")


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _fake_bench(*extra):
    env = dict(os.environ, FLYBODY_BENCH_FAKE="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "7", "--warmup", "2",
           "--envs-per-gpu", "64", *extra]
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=280)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


@pytest.mark.timeout(600)
def test_plain_run_is_lean_and_dumps_the_last_step(tmp_path):
    runs = []
    for name in ("a", "b"):
        d = _fake_bench("--dump-outputs", str(tmp_path / name))
        for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
            assert k in d, k
        assert d["steps"] == 7 and d["ms_per_step"] > 0 and d["higher_is_better"] is True
        assert not {"roofline", "async_groups", "capacity", "cpu_baseline"} & set(d)
        runs.append({n: np.load(tmp_path / name / (n + ".npy")) for n in NAMES})
    a, b = runs
    assert a["observation"].shape == (128, 104) and all(a[n].shape == (128,) for n in NAMES[1:])
    for n in NAMES:
        assert a[n].dtype == np.float32
        np.testing.assert_array_equal(a[n], b[n], err_msg=n)  # same arguments, same inputs, same outputs


def test_dump_outputs_keeps_a_fixed_sample_within_the_limit(tmp_path, monkeypatch):
    import bench

    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 4000)
    rows = np.arange(100)
    arrays = {"observation": np.repeat(rows[:, None], 10, 1), "reward": rows, "step_type": rows.astype(np.int32)}
    for name in ("a", "b"):
        bench.dump_outputs(str(tmp_path / name), arrays)
    a = {n: np.load(tmp_path / "a" / (n + ".npy")) for n in arrays}
    assert sum(x.nbytes for x in a.values()) <= 4000 and len(a["reward"]) > 0
    picked = np.load(tmp_path / "a" / "sample_rows.npy")
    for n, x in a.items():
        assert x.dtype == np.float32
        np.testing.assert_array_equal(x.reshape(len(x), -1)[:, 0], picked, err_msg=n)  # every array keeps the same rows
        np.testing.assert_array_equal(x, np.load(tmp_path / "b" / (n + ".npy")), err_msg=n)
