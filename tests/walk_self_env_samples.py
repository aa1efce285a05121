"""Teacher-forced samples shared by tests/test_walk_self_env_cpu.py and tests/test_gpu_walk_self_env.py (generated once per session on the
CPU with the float64 oracle, on the SHIPPED blob): one control step of the walk_imitation environment on the floor with the fly's own
contacts (FFE_WALK_EPISODES | FFE_WALK_FLOOR | FFE_WALK_SELF).

A rollout of the env on the shipped blob, sampled as tests/test_gpu_walk_floor_env.py samples the floor-only one, comes within BAND of
a switching distance too often (9 / 5 / 7 of 24 under the three flag sets).  So the states are given, not rolled out: state i of a
set of tests/walk_self_sets.py (R10: 24 states of a +-1.0 rollout; XS: the 12 crafted poses where floor and fly-fly rows mix) is forced
into an oracle env that was reset on clip i % 3 and advanced SAMPLE_STEPS[(i // 3) % 8] zero-action steps (so that the step counter, and
with it the reference the reward reads, differs from sample to sample), and one step follows with action i of `actions(seed, 24, 0.5)`.
The device env is brought to the same (clip, step), given the same state and stepped with the same action.

SEEDS holds, per flag set, the action seed with which at most 6 of the 24 R10 samples (3 of the 12 XS samples) fall inside the band;
tests/test_walk_self_env_cpu.py asserts that with the oracle alone."""
import numpy as np

import walk_self_sets as S
from walk_self_sets import NO_ADHESION, NO_FLUID, NO_NOSLIP

SAMPLE_STEPS = (0, 2, 4, 7, 10, 14, 19, 27)  # tests/test_gpu_walk_episode.py
FLAG_SETS = [(0, "all"), (NO_NOSLIP, "no_noslip"), (NO_FLUID | NO_ADHESION, "no_fluid_no_adhesion")]
SEEDS = {("R10", 0): 21, ("R10", NO_NOSLIP): 21, ("R10", NO_FLUID | NO_ADHESION): 11, ("XS", 0): 21}
LEFT_OUT_CAP = {"R10": 6, "XS": 3}  # the project's: a quarter of the set
_cache = {}


def actions(seed, n, amplitude):
    """tests/test_gpu_walk_episode.py::actions (restated: that module needs a GPU's fixtures)"""
    rs = np.random.RandomState(seed)
    return [(amplitude * rs.uniform(-1.0, 1.0, 59)).astype(np.float32) for _ in range(n)]


def world():
    """(view, refs): tests/test_gpu_walk_episode.py::world"""
    from flybody_amd.tasks import walking as W

    if "world" not in _cache:
        view = W.WalkModelView()
        _cache["world"] = (view, W.WalkRefSet(W.synthetic_snippets(view, n=3, length=100)))
    return _cache["world"]


def make_oracle(flags=0, refs=None, **kw):
    """An oracle env on the shipped blob, on a model of its own (the flags live in the model)."""
    from oracle import oracle as O

    view, wrefs = world()
    m = O.OracleModel(S.WALK_BLOB)
    assert m.npair == 2336
    m.set_flags(flags)
    return O.OracleWalkEnv(m, refs or wrefs, view.mocap_jnt, view.mocap_site, (view.retract_qadr, view.retract_val), **kw)


def last_substep_counts(state, ctrl, flags):
    """(ncon_matter, the fly-fly contacts among them, the fly-fly contacts with a row) of the tenth substep of a control step from `state`."""
    from oracle import oracle as O

    m = S.model()
    d = O.OracleData(m)
    m.set_flags(flags)
    try:
        d.qpos[:], d.qvel[:], d.act[:] = state[:3]
        d.ctrl[:] = ctrl
        d.step1()
        for k in range(10):
            d.step2()
            if k == 9:  # (step2 solves on the contact list of the step1 before it and leaves the list alone)
                out = (d.ncon_matter, S._matter_self(m, d), sum(1 for r in S.fly_fly(d.contacts()) if int(r[4]) >= 0))
            d.step1()
    finally:
        m.set_flags(0)
    return out


def forced_samples(which, flags, seed=None):
    """[dict(clip, step, state, action, st, reward, discount, obs, gap, ncon, nself, self_rows)] for the states of set `which`, and the
    oracle's observation layout."""
    seed = SEEDS[(which, flags)] if seed is None else seed
    key = (which, flags, seed)
    if key in _cache:
        return _cache[key]
    states = {"R10": S.r10, "XS": S.x_standing}[which]()
    acts = actions(seed, 24, 0.5)
    out = []
    for i, s in enumerate(states):
        o = make_oracle(flags, terminal_com_dist=np.inf)
        clip, step = i % 3, SAMPLE_STEPS[(i // 3) % 8]
        o.force_next(clip)
        o.reset()
        for _ in range(step):
            assert o.step(np.zeros(59))[0] == 1
        d = o.data
        d.qpos[:], d.qvel[:], d.act[:] = s[:3]
        d.step1()
        d.contact_hist(reset=True)
        state = (d.qpos.copy(), d.qvel.copy(), d.act.copy())
        res = o.step(acts[i])
        gap = d.contact_hist(reset=True)[1]
        ncon, nself, rows = last_substep_counts(state, d.ctrl.copy(), flags)
        out.append(dict(clip=clip, step=step, state=state, action=acts[i], st=res[0], reward=res[1], discount=res[2], obs=res[3].copy(), gap=gap,
                        ncon=ncon, nself=nself, self_rows=rows))
        layout = o.LAYOUT
    _cache[key] = (out, layout)
    return _cache[key]


def kept(samples):
    return [i for i, s in enumerate(samples) if s["gap"] >= S.BAND]
