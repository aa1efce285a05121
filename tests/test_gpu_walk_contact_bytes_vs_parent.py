"""The contact kernels of the free-root walking fly - `floor_step`, `floor_self_step`, `imitation_floor_step`, `imitation_self_step` - return,
byte for byte, what the library of the commit before `floor_forces` / `self_forces` became one `contact_forces` and `floor_sense` /
`self_sense` one sensor pass returned (tests/golden/walk_contact_parent_digest.npz, recorded on an MI355X by
tools/record_walk_contact_digest.py in a checkout of that commit; its hash is in the file).  The batch of 32 states, its controls and
the actions of the env runs are read from the file; eight physics runs (floor / self handle; all forces for 1 and 10 substeps,
FFE_NO_NOSLIP and FFE_NO_FLUID | FFE_NO_ADHESION for 1) and two env runs (a reset and three steps, without and with the fly's own
contacts) are replayed on the current library.  The ints and the first four envs are kept whole, the other envs' float rows as one
16-byte digest each (see the tool).  The file is never re-recorded from the code under test.  Run with `-m gpu` on an MI355X."""
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(GOLDEN, "walk_contact_parent_digest.npz")
sys.path.insert(0, os.path.join(ROOT, "tools"))
try:
    import record_walk_contact_digest as R
finally:
    sys.path.pop(0)


@pytest.fixture(scope="module")
def parent():
    with np.load(FIXTURE) as f:
        return {k: f[k] for k in f.files}


def test_fixture_covers_the_cases(parent):
    """Read from the parent's recorded ints alone."""
    assert len(str(parent["commit"])) == 40 and os.path.getsize(FIXTURE) <= 256 * 1024
    assert R.B == 32 and R.RAW_ROWS == 4 and len(R.RUNS) == 10
    assert parent["in_qpos"].shape == (32, 109) and parent["in_qvel"].shape == (32, 108) and parent["in_act"].shape == (32, 59)
    assert parent["in_ctrl"].shape == (32, 59) and parent["in_actions"].shape == (3, 32, 59)
    for k, v in parent.items():
        if k.endswith("_raw"):
            assert v.shape[0] == 4 and np.isfinite(v).all() and parent[k[:-4] + "_digest"].shape == (28, 16), k
    far, hover = R.GROUPS["far"], R.GROUPS["hover"]
    for name, (self_contacts, _, nsteps) in R.PHYSICS_RUNS.items():
        ints, val = parent[f"{name}_ints"], parent[f"{name}_validity"]
        assert ints.shape == (32, 8) and val.shape == (32, 4) and ints.dtype == np.int32 and val.dtype == np.int32
        ncon, nself, nlim = ints[:, 5], ints[:, 3], ints[:, 4]
        assert np.array_equal(ints[:, 7], val[:, 0]) and not val[:, 1:].any() and not ints[:, :3].any()
        if not self_contacts:
            assert not ncon[far].any() and not nself.any()  # the far envs: no floor in reach
            if nsteps == 1:
                assert ((ncon == 0) & (nlim > 0))[hover].any()  # in reach, no contact: the cone solver with no cone block
        else:
            # (the counts are the last substep's: after ten, a contact of the stored state may have opened)
            assert (nsteps > 1 or (nself > 0).all()) and (nself > 0).sum() >= 24 and (ncon > nself).any() and np.array_equal(ncon[far], nself[far])
        if nsteps == 1:  # one substep: the rows are those of the stored states, a pushed hinge is one row
            rows = R.row_counts(parent, name)
            for lo, hi in R.ROW_CLASSES:
                assert ((rows >= lo) & (rows <= hi)).any(), (name, lo, hi, rows.tolist())
            fits = (val[:, 0] & 2) == 0  # (more rows than RMAX: the limit rows beyond are dropped)
            want = np.array([0, 0] + [R.HOVER_PUSHED] * 4 + [0] * 6 + R.PUSH_COUNTS)
            pinned = np.r_[hover, R.GROUPS["pushed"]]
            assert (nlim[pinned] <= want[pinned]).all() and np.array_equal(nlim[pinned][fits[pinned]], want[pinned][fits[pinned]])
        assert ints[:, 6].any()
    for name, self_contacts in R.ENV_RUNS.items():
        ints = parent[f"{name}_ints"]
        assert (ints[:, 0] == np.arange(32) % 3).all() and (ints[:, 5] > 0).any()
        assert not parent[f"{name}_reset_step_type"].any() and (parent[f"{name}_step_step_type"] == 1).any()


@pytest.mark.parametrize("name", R.RUNS)
def test_run_is_byte_identical_to_the_parent(parent, name):
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    got = R.run(parent, name)
    assert set(got) == {k for k in parent if k.startswith(name + "_")}
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
