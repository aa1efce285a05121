"""State sets shared by tests/test_walk_floor_cpu.py and tests/test_gpu_walk_floor.py (generated once per session on the CPU with the
float64 oracle).

The oracle always collides the fly's own pairs too, and the floor kernel does not.  So both sides run on a temporary copy of
fly_walk.ffmb whose collision bits leave the floor pairs alone: geom_contype = 1, geom_conaffinity = 0 on every fly geom and 0 / 1 on the
floor (`floor_only_blob`).  On it the oracle's pair list drops from 2 336 pairs to the 48 (floor, sphere / capsule) pairs.

  F06  24 states (qpos, qvel, act) sampled every 3 control steps along an `OracleWalkEnv` rollout on that blob, actions uniform +-0.6,
       RandomState(5), full physics (the construction of set A of tests/walk_limit_sets.py)
  F10  the same with actions uniform +-1.0"""
import functools
import os
import tempfile

import numpy as np

from conftest import ROOT

ASSETS = os.path.join(ROOT, "flybody_amd", "assets")
WALK_BLOB = os.path.join(ASSETS, "fly_walk.ffmb")
NO_FLUID, NO_LIMIT, NO_DAMPER, NO_SPRING, NO_GRAVITY, NO_ACTUATION, NO_CONTACT, NO_NOSLIP, NO_ADHESION = 1, 2, 4, 8, 16, 32, 64, 128, 256
WALK_JOINT_LIMITS, WALK_EPISODES, WALK_FLOOR = 512, 1024, 2048
FLOOR = NO_CONTACT | WALK_JOINT_LIMITS | WALK_FLOOR
ORACLE_MASK = NO_FLUID | NO_DAMPER | NO_SPRING | NO_GRAVITY | NO_ACTUATION | NO_NOSLIP | NO_ADHESION  # what the oracle is shown of a device flag set
BAND = 2e-6  # cm: a state is left out when a candidate pair comes this close to a switching distance (the tethered test's band)

_keep = []


@functools.lru_cache(maxsize=1)
def floor_only_blob():
    """Path of the temporary blob (kept for the session)."""
    from flybody_amd.model.blob import read_blob, write_blob

    t = read_blob(WALK_BLOB)
    body, ty = np.asarray(t["geom_bodyid"]).ravel(), np.asarray(t["geom_type"]).ravel()
    ct, ca = np.asarray(t["geom_contype"]).copy(), np.asarray(t["geom_conaffinity"]).copy()
    floor = (body == 0) & (ty == 0)
    assert floor.sum() == 1
    ct.ravel()[:] = np.where(floor, 0, 1)
    ca.ravel()[:] = np.where(floor, 1, 0)
    t = dict(t)
    t["geom_contype"], t["geom_conaffinity"] = ct, ca
    d = tempfile.TemporaryDirectory(prefix="walk_floor_")
    _keep.append(d)
    path = os.path.join(d.name, "fly_walk_flooronly.ffmb")
    write_blob(path, t)
    return path


@functools.lru_cache(maxsize=1)
def model():
    from oracle import oracle as O

    m = O.OracleModel(floor_only_blob())
    assert m.npair == 48, m.npair
    return m


def _rollout(amp):
    from flybody_amd.tasks import walking as W
    from oracle import oracle as O

    view = W.WalkModelView()
    refs = W.WalkRefSet(W.synthetic_snippets(view, n=1, length=200))
    m = model()
    env = O.OracleWalkEnv(m, refs, view.mocap_jnt, view.mocap_site, (view.retract_qadr, view.retract_val), terminal_com_dist=float("inf"))
    env.force_next(0)
    env.reset()
    rs = np.random.RandomState(5)
    out = []
    for _ in range(24):
        for _ in range(3):
            st, _, _, _ = env.step(rs.uniform(-amp, amp, env.naction))
            assert st == 1  # MID: the rollout stays inside one episode
        d = env.data
        out.append((d.qpos.copy(), d.qvel.copy(), d.act.copy()))
    return out


@functools.lru_cache(maxsize=1)
def sets():
    """(oracle model, F06, F10)"""
    return model(), _rollout(0.6), _rollout(1.0)


@functools.lru_cache(maxsize=1)
def reset_pose():
    """qpos of the reset pose of clip 0 (what `OracleWalkEnv.reset` starts from)."""
    from flybody_amd.tasks import walking as W
    from oracle import oracle as O

    view = W.WalkModelView()
    refs = W.WalkRefSet(W.synthetic_snippets(view, n=1, length=200))
    env = O.OracleWalkEnv(model(), refs, view.mocap_jnt, view.mocap_site, (view.retract_qadr, view.retract_val), terminal_com_dist=float("inf"))
    env.force_next(0)
    env.reset()
    return env.data.qpos.copy()


def oracle_advance(m, state, ctrl, nsteps, flags, trace=None):
    """step1; (step2; step1) x nsteps as tests/walk_limit_sets.py::oracle_advance, contacts on.  `flags`: force switches, NO_NOSLIP,
    NO_ADHESION only.  `trace`, a list, receives (ncon, nefc) of every substep taken.  Returns (qpos, qvel, act, closest approach of a
    candidate pair to a switching distance over the substeps taken)."""
    from oracle import oracle as O

    assert not flags & ~ORACLE_MASK
    d = O.OracleData(m)
    m.set_flags(flags)
    d.qpos[:], d.qvel[:], d.act[:] = state
    d.ctrl[:] = ctrl
    d.step1()
    d.contact_hist(reset=True)
    for _ in range(nsteps):
        d.step2()  # (its velocity stage records how close the collision of the step1 before it came to a switch)
        if trace is not None:
            trace.append((d.ncon, d.nefc))
        d.step1()
    gap = d.contact_hist(reset=True)[1]
    m.set_flags(0)
    return d.qpos.copy(), d.qvel.copy(), d.act.copy(), gap
