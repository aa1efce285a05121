"""State sets shared by tests/test_walk_limits_cpu.py and tests/test_gpu_walk_limits.py (generated once per session on the CPU with the
float64 oracle; the oracle always runs with FFE_NO_CONTACT and never sees FFE_WALK_JOINT_LIMITS).

  A  the 24 states of tests/test_gpu_walk_physics.py (the construction is copied, not imported): (qpos, qvel, act) sampled every 3
     control steps along an `OracleWalkEnv` rollout, actions uniform +-0.6, full physics.
  C  24 states built from A: every limited hinge clamped to at least 1e-3 rad inside its range, then n hinges - chosen with
     RandomState(7) without replacement - pushed uniform(1e-3, 0.05) rad past their lower or upper bound (probability 1/2 each);
     n runs over [1, 2, 3, 4, 6, 8, 12, 16, 20, 24, 28, 32] twice.  Velocities and activations are A's.
  clamped(A)  A with every limited hinge at least 1e-3 rad inside its range.
  pushed(A, n, seed)  as C with the same n for every state (the overflow test uses n = 70)."""
import functools
import os

import numpy as np

from conftest import ROOT

ASSETS = os.path.join(ROOT, "flybody_amd", "assets")
WALK_BLOB = os.path.join(ASSETS, "fly_walk.ffmb")
NO_FLUID, NO_LIMIT, NO_DAMPER, NO_SPRING, NO_GRAVITY, NO_ACTUATION, NO_CONTACT, WALK_JOINT_LIMITS = 1, 2, 4, 8, 16, 32, 64, 512
C_COUNTS = [1, 2, 3, 4, 6, 8, 12, 16, 20, 24, 28, 32] * 2


@functools.lru_cache(maxsize=1)
def _hinges():
    from flybody_amd.model.blob import read_blob

    t = read_blob(WALK_BLOB)
    lim = np.asarray(t["jnt_limited"]).astype(bool).ravel()
    rng = np.asarray(t["jnt_range"]).reshape(-1, 2)
    jt, qadr = np.asarray(t["jnt_type"]).ravel(), np.asarray(t["jnt_qposadr"]).ravel()
    hl = np.where(lim & (jt == 3))[0]
    assert len(hl) == 102
    return hl, rng, qadr


def clamp_inside(q):
    hl, rng, qadr = _hinges()
    q = q.copy()
    q[qadr[hl]] = np.minimum(np.maximum(q[qadr[hl]], rng[hl, 0] + 1e-3), rng[hl, 1] - 1e-3)
    return q


def pushed(states, counts, seed):
    hl, rng, qadr = _hinges()
    rs = np.random.RandomState(seed)
    out = []
    for (q, v, a), n in zip(states, counts):
        q = clamp_inside(q)
        for j in rs.choice(hl, n, replace=False):
            lo, hi = rng[j]
            e = rs.uniform(1e-3, 0.05)
            q[qadr[j]] = lo - e if rs.rand() < 0.5 else hi + e
        out.append((q, v.copy(), a.copy()))
    return out


@functools.lru_cache(maxsize=1)
def sets():
    """(oracle model, A, C)"""
    from flybody_amd.tasks import walking as W
    from oracle import oracle as O

    view = W.WalkModelView()
    refs = W.WalkRefSet(W.synthetic_snippets(view, n=1, length=200))
    m = O.OracleModel(WALK_BLOB)
    env = O.OracleWalkEnv(m, refs, view.mocap_jnt, view.mocap_site, (view.retract_qadr, view.retract_val), terminal_com_dist=float("inf"))
    env.force_next(0)
    env.reset()
    rs = np.random.RandomState(5)
    A = []
    for _ in range(24):
        for _ in range(3):
            st, _, _, _ = env.step(rs.uniform(-0.6, 0.6, env.naction))
            assert st == 1  # MID: the rollout stays inside one episode
        d = env.data
        A.append((d.qpos.copy(), d.qvel.copy(), d.act.copy()))
    C = pushed(A, C_COUNTS, 7)
    return m, A, C


def oracle_advance(m, state, ctrl, nsteps, flags, trace=None):
    """step1; (step2; step1) x nsteps, exactly as tests/test_gpu_walk_physics.py::_oracle_advance.  `flags` never carry
    WALK_JOINT_LIMITS.  `trace`, a list, receives nefc of every substep taken (the rows its constraint stage instantiated)."""
    from oracle import oracle as O

    assert not flags & WALK_JOINT_LIMITS
    d = O.OracleData(m)
    m.set_flags(flags)
    d.qpos[:], d.qvel[:], d.act[:] = state
    d.ctrl[:] = ctrl
    d.step1()
    for _ in range(nsteps):
        d.step2()
        if trace is not None:
            trace.append(d.nefc)
        d.step1()
    m.set_flags(0)
    return d.qpos.copy(), d.qvel.copy(), d.act.copy()
