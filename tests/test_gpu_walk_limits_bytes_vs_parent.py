"""The joint-limit kernel of the free-root walking fly returns, byte for byte, what the library of the commit before the constraint
solve moved into csrc/row_newton.hpp returned (tests/golden/walk_limits_parent_digest.npz, recorded on an MI355X by
tools/record_walk_limits_digest.py in a checkout of that commit; its hash is in the file).  The batch of 32 states - set C, four
states with 36 ... 48 limits, two with 70 (overflow), two without any - and its controls are read from the file; four runs (all forces
on / only the limits, 1 / 10 substeps) are replayed on the current library.  The ints and the first four envs are kept whole, the
other envs' float rows as one 16-byte digest each (see the tool).  The file is never re-recorded from the code under test.
Run with `-m gpu` on an MI355X."""
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(GOLDEN, "walk_limits_parent_digest.npz")


@pytest.fixture(scope="module")
def recorder():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import record_walk_limits_digest
    finally:
        sys.path.pop(0)
    return record_walk_limits_digest


@pytest.fixture(scope="module")
def parent():
    with np.load(FIXTURE) as f:
        return {k: f[k] for k in f.files}


def test_fixture_covers_the_cases(recorder, parent):
    R = recorder
    assert len(str(parent["commit"])) == 40
    assert R.B == 32 and R.RAW_ROWS == 4 and R.BIG_COUNTS == [36, 40, 44, 48] and R.OVER_COUNTS == [70, 70]
    assert R.RUNS == {"lim_n1": (64 | 512, 1), "lim_n10": (64 | 512, 10), "only_n1": (64 | 512 | 61, 1), "only_n10": (64 | 512 | 61, 10)}
    names = {f"{r}_{k}_{w}" for r in R.RUNS for k in R.FLOATS for w in ("raw", "digest")} | {f"{r}_{k}" for r in R.RUNS for k in R.INTS}
    assert set(parent) == names | {"in_qpos", "in_qvel", "in_act", "in_ctrl", "commit"}
    assert os.path.getsize(FIXTURE) <= 256 * 1024
    assert parent["in_qpos"].shape == (32, 109) and parent["in_qvel"].shape == (32, 108) and parent["in_ctrl"].shape == (32, 59)
    assert parent["in_qpos"].dtype == np.float64 and parent["in_ctrl"].dtype == np.float32
    C, big, over, clamped = (R.GROUPS[k] for k in ("C", "big", "over", "clamped"))
    for r in R.RUNS:
        ints, val = parent[f"{r}_ints"], parent[f"{r}_validity"]
        assert ints.shape == (32, 8) and val.shape == (32, 4) and ints.dtype == np.int32 and val.dtype == np.int32
        for k in R.FLOATS:
            assert parent[f"{r}_{k}_raw"].shape[0] == 4 and parent[f"{r}_{k}_digest"].shape == (28, 16)
            assert np.isfinite(parent[f"{r}_{k}_raw"]).all()
        # bit value 2 on exactly the two overflow envs, in the validity column and in task-state int 7
        assert (val[:, 0] == 2).nonzero()[0].tolist() == [28, 29] and not val[:28].any() and not val[30:].any() and not val[:, 1:].any()
        assert np.array_equal(ints[:, 7], val[:, 0])
    for r in ("lim_n1", "only_n1"):
        rows, iters = parent[f"{r}_ints"][:, 4], parent[f"{r}_ints"][:, 6]
        # one substep: the rows are the pushed hinges, so every case and every instantiation of the solver (8, 16, 32, 48 rows) is there
        assert rows[C].tolist() == [1, 2, 3, 4, 6, 8, 12, 16, 20, 24, 28, 32] * 2
        assert rows[big].tolist() == [36, 40, 44, 48] and rows[over].tolist() == [48, 48] and rows[clamped].tolist() == [0, 0]
        for lo, hi in ((1, 8), (9, 16), (17, 32), (33, 48)):
            assert ((rows >= lo) & (rows <= hi)).any(), (lo, hi)
        assert (iters[clamped] == 0).all() and iters[:30].any()  # no row, no solve
    # only the limits act, from the first substep: the stopping scale is ~0 and the solver runs to its cap of 20 (int 6 is the LAST
    # substep's count, and after ten substeps the velocity-dependent forces have given the scale a size again)
    assert (parent["only_n1_ints"][:, 6] == 20).sum() >= 2
    assert max(int(parent[f"{r}_ints"][:, 6].max()) for r in R.RUNS) == 20


@pytest.mark.parametrize("name", ["lim_n1", "lim_n10", "only_n1", "only_n10"])
def test_run_is_byte_identical_to_the_parent(recorder, parent, name):
    got = recorder.run(parent, name)
    bad = []
    for k, v in got.items():
        want = parent[k]
        first = 4 if k.endswith("_digest") else 0  # env row of the entry's first row
        if v.dtype != want.dtype or v.shape != want.shape:
            bad.append(f"{k}: {v.dtype}{v.shape} against {want.dtype}{want.shape}")
        elif v.tobytes() != want.tobytes():
            n = v.shape[0]
            rows = np.nonzero((v.view(np.uint8).reshape(n, -1) != want.view(np.uint8).reshape(n, -1)).any(axis=1))[0] + first
            bad.append(f"{k}: env rows {rows.tolist()} differ ({len(rows)} of {n})")
    assert not bad, "\n".join(bad)
