"""The walk_on_ball kernel returns, byte for byte, what the library of the commit before its `self_collide` / `convex_collide` and the
walker's `self_prim_collide` / `self_convex_collide` became `prim_pairs` / `convex_pairs` of csrc/self_pairs.hpp returned
(tests/golden/ball_parent_digest.npz, recorded on an MI355X by tools/record_ball_digest.py in a checkout of that commit; its hash is in
the file).  The batch of 32 states, its controls and the actions of the env run are read from the file; three physics runs (all forces
for 1 and 10 substeps, FFE_NO_NOSLIP | FFE_NO_ADHESION for 1) and one env run (a reset and three steps) are replayed on the current
library.  The ints and the first four envs are kept whole, the other envs' float rows as one 16-byte digest each (see the tool).  The
file is never re-recorded from the code under test.  Run with `-m gpu` on an MI355X."""
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(GOLDEN, "ball_parent_digest.npz")
sys.path.insert(0, os.path.join(ROOT, "tools"))
try:
    import record_ball_digest as R
finally:
    sys.path.pop(0)


@pytest.fixture(scope="module")
def parent():
    with np.load(FIXTURE) as f:
        return {k: f[k] for k in f.files}


def test_fixture_covers_the_cases(parent):
    """Read from the parent's recorded ints alone."""
    assert len(str(parent["commit"])) == 40 and os.path.getsize(FIXTURE) <= 256 * 1024
    assert R.B == 32 and R.RAW_ROWS == 4 and len(R.RUNS) == 4
    assert parent["in_qpos"].shape == (32, 106) and parent["in_qvel"].shape == (32, 105) and parent["in_act"].shape == (32, 59)
    assert parent["in_ctrl"].shape == (32, 59) and parent["in_actions"].shape == (3, 32, 59)
    for k, v in parent.items():
        if k.endswith("_raw"):
            assert v.shape[0] == 4 and np.isfinite(v).all() and parent[k[:-4] + "_digest"].shape == (28, 16), k
    touching, over = R.GROUPS["fly_fly"], slice(R.GROUPS["primitive"].start, R.GROUPS["convex"].stop)
    assert (touching.start, touching.stop, over.start, over.stop) == (0, 20, 20, 32)
    more, iters = False, False
    for name, (_, nsteps) in R.PHYSICS_RUNS.items():
        ints, val = parent[f"{name}_ints"], parent[f"{name}_validity"]
        assert ints.shape == (32, 8) and val.shape == (32, 4) and ints.dtype == np.int32 and val.dtype == np.int32
        if nsteps == 1:
            assert (ints[over, 7] & 1).all(), (name, ints[:, 7].tolist())         # more than 16 contacts in every forced pose
        assert not (ints[touching, 7] & 1).any(), (name, ints[:, 7].tolist())     # and in none of the touching ones
        assert (ints[touching, 3] > 0).all(), (name, ints[:, 3].tolist())         # nself: the fly touches itself in every one of them
        more |= bool((ints[:, 5] > ints[:, 3]).any())                             # ball contacts are present
        iters |= bool(ints[:, 6].any())
    assert more and iters
    assert not parent["env_reset_step_type"].any() and (parent["env_step_step_type"] == 1).all()


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
