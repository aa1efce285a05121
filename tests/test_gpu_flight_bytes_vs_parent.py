"""The flight step kernel returns, byte for byte, what the library of the commit before the lane-address rematerialisation returned
(tests/golden/flight_parent_digest.npz, recorded on an MI355X by tools/record_flight_digest.py in a checkout of that commit; its hash is
in the file).  The rollouts - B = 130 and 5, contact capacities 6 and 12, 40 control steps of full-range actions with one `reset_envs`
after step 20 - pass through mouth-part contacts on every step, second-pass collision calls, joint limits, the stage-1 carry-over and
both reset paths.  The B = 130 entries are one 16-byte digest per env row, the B = 5 entries the arrays themselves (see the tool).
Run with `-m gpu` on an MI355X."""
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(GOLDEN, "flight_parent_digest.npz")


@pytest.fixture(scope="module")
def recorder():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import record_flight_digest
    finally:
        sys.path.pop(0)
    return record_flight_digest


@pytest.fixture(scope="module")
def parent():
    with np.load(FIXTURE) as f:
        return {k: f[k] for k in f.files}


def test_fixture_covers_the_cases(recorder, parent):
    assert len(str(parent["commit"])) == 40
    assert recorder.BATCHES == (130, 5) and recorder.CAPACITIES == (6, 12) and recorder.STEPS == 40
    assert recorder.KEEP == (10, 20, 21, 30, 40) and recorder.RESET_AFTER == 20
    tags = [f"step{k}" for k in recorder.KEEP] + ["reset_envs"]
    names = {f"b{B}_c{cap}_{t}_{w}" for B in (130, 5) for cap in (6, 12) for t in tags for w in ("observation", "reward", "discount", "step_type")}
    names |= {f"b{B}_c{cap}_final_{w}" for B in (130, 5) for cap in (6, 12) for w in ("qpos", "qvel")}
    assert set(parent) == names | {"commit"}
    assert os.path.getsize(FIXTURE) <= 256 * 1024
    # the B = 5 rollouts are kept whole: episodes run (MID rows), the masked envs restart (FIRST rows) and the others do not
    m = recorder.reset_mask(5)
    for cap in (6, 12):
        st = parent[f"b5_c{cap}_reset_envs_step_type"][:, 0]
        assert (st[m] == 0).all() and (st[~m] == parent[f"b5_c{cap}_step20_step_type"][~m, 0]).all()


@pytest.mark.parametrize("capacity", [6, 12])
@pytest.mark.parametrize("B", [130, 5])
def test_rollout_is_byte_identical_to_the_parent(recorder, parent, B, capacity):
    got = recorder.rollout(B, capacity)
    bad = []
    for k, v in got.items():
        want = parent[f"b{B}_c{capacity}_{k}"]
        if v.dtype != want.dtype or v.shape != want.shape:
            bad.append(f"{k}: {v.dtype}{v.shape} against {want.dtype}{want.shape}")
        elif v.tobytes() != want.tobytes():
            rows = np.nonzero((v.view(np.uint8).reshape(B, -1) != want.view(np.uint8).reshape(B, -1)).any(axis=1))[0]
            bad.append(f"{k}: env rows {rows.tolist()[:20]} differ ({len(rows)} of {B})")
    assert not bad, "\n".join(bad)
