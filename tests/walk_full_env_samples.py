"""Shared by tests/test_walk_full_env_cpu.py and tests/test_gpu_walk_full_env.py (generated once per session on the CPU with the float64
oracle): the walk_imitation environment with every contact of the reference's task (`BatchedWalkEnv(floor_contacts=True,
self_contacts=True, floor_convex=True)`, csrc/walk_imit_full_env.hip `imitation_full_step`).

oracle/ does not restate mjc_PlaneConvex / mjc_PlaneCylinder, so three references are used:

  1. round blobs   Two copies of the shipped blob, written into a temporary directory.  On the DEVICE blob every ellipsoid keeps its type
                   and gets all three semi-axes set to its smallest one; on the ORACLE blob the same geoms are spheres of that radius.  A
                   round ellipsoid is a sphere, so the oracle's plane-sphere collider is the exact answer for the device's
                   `ellipsoid_support` path in every pose and over any number of substeps, root-only thorax rows included.  Shrinking can
                   only remove reachable pairs, so every compiled candidate list stays a superset.  The cylinders stay cylinders, and the
                   oracle does not collide them with the plane: a compared step must keep every plane-cylinder candidate outside margin +
                   CLEAR in each of its substeps (`cylinder_clearance`, from the oracle's geom frames).  ROUND samples: the eight states
                   of set B of tests/walk_floor_convex_sets.py (on its back: thorax and wings) and the four of `set_h` (on its back,
                   pitched until the shrunken head, mouth parts or a coxa are lowest) at rest, rolled on the round oracle blob with
                   zero actions; the state after ROUND_STEPS[set] control steps is a sample (28 in all), stepped once with a +-0.5 action.  (Set C
                   of that file does not serve: its coxae and mouth parts no longer reach the floor once they are round, and its abdomen
                   does within two steps.)
  2. witness       A reset row is one forward pass with one collision pass, for which a witness blob is exact
                   (walk_floor_convex_sets.witness_model).  `static_clips()`: clips whose rows repeat one fallen pose - of set A (abdomen:
                   cylinders), B and C - settled so that the pose the reset builds (the oracle's own state after a reset on the shipped
                   blob, retraction included) is inside every capacity and CLEAR of every switching distance.
  3. bridge        `bridge_states()`: sets A / B / C on the shipped blob, for the comparison of `env.step` with the bare-physics kernel
                   `floor_full_step`, which the tests of step 3d pin against the oracle substep by substep."""
import functools
import os
import shutil
import tempfile

import numpy as np

import walk_floor_convex_sets as F
import walk_self_env_samples as E
import walk_self_sets as S
from walk_self_env_samples import FLAG_SETS, SAMPLE_STEPS, actions, kept, world  # noqa: F401
from walk_self_sets import NO_ADHESION, NO_FLUID, NO_NOSLIP

CLEAR = F.CLEAR
# control steps of the zero-action rollout after which a state is sampled: inside the window where round geoms touch the floor and no
# cylinder has come near yet (tests/test_walk_full_env_cpu.py asserts both per substep of the compared step)
ROUND_STEPS = {"B": (3, 4, 5), "H": (0,)}  # (a head that rests 0.002 .. 0.008 cm deep is pushed out within a step or two: sampled at rest, while it touches)
HEAD_KINDS = ("head", "rostrum", "haustellum", "labrum", "coxa")
SEEDS = {0: 21, NO_NOSLIP: 21, NO_FLUID | NO_ADHESION: 21}  # action seeds; the CPU test asserts the band cap with the oracle alone
LEFT_OUT_CAP = 7  # the project's: a quarter of the set (28 samples)
OPEN_LOOP = (1, 21)  # samples from which case c runs four consecutive steps (cylinder-free over the window: asserted on the CPU)
OPEN_STEPS = 4
CLIP_ROWS = 100  # a static clip: future_steps = 64 leaves an episode of 35 steps
_keep = []
_cache = {}


# ------------------------------------------------------------------------------------------------ 1. round blobs
@functools.lru_cache(maxsize=1)
def ellipsoids():
    """(geom ids of the shipped blob's ellipsoids, the smallest semi-axis of each)"""
    ty = F._flat("geom_type")
    ell = np.nonzero(ty == 4)[0]
    return ell, np.asarray(F.tables()["geom_size"], dtype=np.float64)[ell].min(axis=1)


@functools.lru_cache(maxsize=1)
def round_blobs():
    """(path of the device blob, path of the oracle blob), kept for the session; fly_walk.json lies beside the device blob."""
    from flybody_amd.model.blob import write_blob

    ell, r = ellipsoids()
    dev = {k: np.array(v, copy=True) for k, v in F.tables().items()}
    ora = {k: np.array(v, copy=True) for k, v in F.tables().items()}
    dev["geom_size"][ell] = r[:, None].astype(dev["geom_size"].dtype)
    ora["geom_type"].reshape(-1)[ell] = 2
    ora["geom_size"][ell] = 0
    ora["geom_size"][ell, 0] = r.astype(ora["geom_size"].dtype)
    dr = tempfile.TemporaryDirectory(prefix="walk_full_env_")
    _keep.append(dr)
    paths = os.path.join(dr.name, "fly_walk_round.ffmb"), os.path.join(dr.name, "fly_walk_round_oracle.ffmb")
    write_blob(paths[0], dev)
    write_blob(paths[1], ora)
    shutil.copy(os.path.splitext(S.WALK_BLOB)[0] + ".json", os.path.splitext(paths[0])[0] + ".json")
    return paths


def round_model(flags=0):
    """An OracleModel of the round oracle blob, of its own (the flags live in the model)."""
    from oracle import oracle as O

    m = O.OracleModel(round_blobs()[1])
    assert m.npair == 2336 + 16, m.npair
    m.set_flags(flags)
    return m


def make_oracle(flags=0, model=None, refs=None, **kw):
    """An oracle env on the round oracle blob (or on `model`)."""
    from oracle import oracle as O

    view, wrefs = world()
    m = model or round_model(flags)
    return O.OracleWalkEnv(m, refs or wrefs, view.mocap_jnt, view.mocap_site, (view.retract_qadr, view.retract_val), **kw)


def cylinder_clearance(d):
    """Smallest (distance - margin) of a plane-cylinder candidate point at the geom frames of `d`: positive = no candidate inside the margin."""
    n, x0 = F.plane()
    size, ty = np.asarray(F.tables()["geom_size"], dtype=np.float64), F._flat("geom_type")
    clear = np.inf
    for g in F.floor_candidates((5,)):
        margin, _ = F.pair_margin(g)
        for _, dist in F.plane_cylinder(n, x0, d.geom_xpos[g], d.geom_xmat[g], size[g, 0], size[g, 1], np.inf):
            clear = min(clear, dist - margin)
    return clear


def round_floor(d):
    """[(geom, dist, pos, active)] of the oracle's floor contacts on retyped geoms."""
    ell = set(ellipsoids()[0].tolist())
    f = F.floor_geom()
    out = []
    for r in d.contacts():
        g = int(r[1]) if int(r[0]) == f else (int(r[0]) if int(r[1]) == f else -1)
        if g in ell:
            out.append((g, float(r[5]), r[6:9].copy(), not int(r[3])))
    return out


def trace_step(state, ctrl, flags, nsteps=10):
    """The substeps of a control step from `state` on the round oracle blob: per substep (ncon_matter, fly-fly among them, retyped geoms
    with an active floor contact, cylinder clearance), of the contact list each substep solves on."""
    from oracle import oracle as O

    m = round_model(flags)
    d = O.OracleData(m)
    d.qpos[:], d.qvel[:], d.act[:] = state[:3]
    d.ctrl[:] = ctrl
    d.step1()
    out = []
    for _ in range(nsteps):
        out.append((d.ncon_matter, S._matter_self(m, d), [g for g, _, _, on in round_floor(d) if on], cylinder_clearance(d)))
        d.step2()
        d.step1()
    return out


@functools.lru_cache(maxsize=1)
def set_h():
    """Four states (qpos, info) at rest on the round oracle blob: legs tucked, on its back and pitched, settled so that the lowest round
    geom sits 0.002 .. 0.008 cm below the plane; taken when a round geom of the head, the mouth parts or a coxa touches, at most 7
    contacts matter (21 rows, were they all in one block of the inertia), every cylinder stays 0.02 cm clear of its margin and no candidate is within CLEAR of a switching distance."""
    from oracle import oracle as O

    _, names, _ = S.tables()
    ell, r = ellipsoids()
    n, x0 = F.plane()
    m = round_model()
    d = O.OracleData(m)
    rng = np.random.RandomState(31)
    out = []
    for _ in range(1500):
        if len(out) == 4:
            break
        q = F.tucked(up=(0.0, 0.0, -1.0)).copy()  # (towards the belly: away from the floor on its back)
        q[3:7] = F._quat_xyz(np.pi + rng.uniform(-0.4, 0.4), rng.uniform(0.3, 1.5), rng.uniform(-3, 3))
        q[:2] = rng.uniform(-1, 1, 2)
        d.qpos[:] = q; d.qvel[:] = 0; d.act[:] = 0; d.ctrl[:] = 0
        d.forward()
        q[2] -= min(float(n @ (d.geom_xpos[g] - x0)) - rr for g, rr in zip(ell, r)) + rng.uniform(0.002, 0.008)
        d.qpos[:] = q
        d.step1()
        d.contact_hist(reset=True)
        touching = [names[g] for g, _, _, on in round_floor(d) if on]
        ok = any(k in x for x in touching for k in HEAD_KINDS) and d.ncon_matter <= 7 and cylinder_clearance(d) >= 0.02
        if not ok:
            continue
        d.step2(); d.step1()
        if d.contact_hist(reset=True)[1] < CLEAR:
            continue
        out.append((q, touching))
    assert len(out) == 4, len(out)
    return out


def _round_states(which):
    return [s[0] for s in (F.get("B") if which == "B" else set_h())]


def round_samples(flags, seed=None):
    """([dict(clip, step, state, action, st, reward, discount, obs, gap, ncon, nself, nconvex, geoms, cyl, trace)], layout): 28 samples."""
    seed = SEEDS[flags] if seed is None else seed
    key = ("round", flags, seed)
    if key in _cache:
        return _cache[key]
    acts = actions(seed, 28, 0.5)
    out = []
    for which in ("B", "H"):
        for i, q0 in enumerate(_round_states(which)):
            clip = i % 3
            roll = make_oracle(0, terminal_com_dist=np.inf)  # the rollout itself runs with every force on
            roll.force_next(clip)
            roll.reset()
            d = roll.data
            d.qpos[:] = q0; d.qvel[:] = 0; d.act[:] = 0
            d.step1()
            states = {0: (d.qpos.copy(), d.qvel.copy(), d.act.copy())}
            for k in range(1, max(ROUND_STEPS[which]) + 1):
                assert roll.step(np.zeros(59))[0] == 1
                states[k] = (d.qpos.copy(), d.qvel.copy(), d.act.copy())
            for k in ROUND_STEPS[which]:
                o = make_oracle(flags, terminal_com_dist=np.inf)
                o.force_next(clip)
                o.reset()
                for _ in range(k):
                    assert o.step(np.zeros(59))[0] == 1
                d2 = o.data
                d2.qpos[:], d2.qvel[:], d2.act[:] = states[k]
                d2.step1()
                d2.contact_hist(reset=True)
                state = (d2.qpos.copy(), d2.qvel.copy(), d2.act.copy())
                a = acts[len(out)]
                res = o.step(a)
                gap = d2.contact_hist(reset=True)[1]
                tr = trace_step(state, d2.ctrl.copy(), flags)
                out.append(dict(set=which, clip=clip, step=k, state=state, action=a, st=res[0], reward=res[1], discount=res[2], obs=res[3].copy(),
                                gap=gap, ncon=tr[-1][0], nself=tr[-1][1], nconvex=len(tr[-1][2]), geoms=sorted({g for t in tr for g in t[2]}),
                                cyl=min(t[3] for t in tr), trace=tr, after=(d2.qpos.copy(), d2.qvel.copy(), d2.act.copy())))
                layout = o.LAYOUT
    _cache[key] = (out, layout)
    return _cache[key]


def open_loop(flags=0):
    """Case c: [per start sample: [dict(action, st, reward, discount, obs, ncon, nself, nconvex, cyl, gap) per step]] for OPEN_STEPS
    consecutive steps from the samples OPEN_LOOP, the first of which is the sample's own step."""
    key = ("open", flags)
    if key in _cache:
        return _cache[key]
    samples, _ = round_samples(flags)
    runs = []
    for i in OPEN_LOOP:
        s = samples[i]
        o = make_oracle(flags, terminal_com_dist=np.inf)
        o.force_next(s["clip"])
        o.reset()
        for _ in range(s["step"]):
            assert o.step(np.zeros(59))[0] == 1
        d = o.data
        d.qpos[:], d.qvel[:], d.act[:] = s["state"]
        d.step1()
        acts = [s["action"]] + actions(300 + i, OPEN_STEPS - 1, 0.5)
        run = []
        for a in acts:
            state = (d.qpos.copy(), d.qvel.copy(), d.act.copy())
            d.contact_hist(reset=True)
            res = o.step(a)
            gap = d.contact_hist(reset=True)[1]
            tr = trace_step(state, d.ctrl.copy(), flags)
            run.append(dict(action=a, st=res[0], reward=res[1], discount=res[2], obs=res[3].copy(), ncon=tr[-1][0], nself=tr[-1][1],
                            nconvex=len(tr[-1][2]), cyl=min(t[3] for t in tr), gap=gap))
        runs.append(run)
    _cache[key] = runs
    return runs


# ------------------------------------------------------------------------------------------------ 2. static fallen clips, witness spheres
def _row(view, qpos):
    return np.concatenate([qpos[:7], qpos[view.mocap_qadr]])


def _static_snippet(view, row):
    from flybody_amd.tasks import walking as W

    ft = W.walker_features(view, view.full_qpos(row), np.zeros(view.nv))
    J = len(view.mocap_jnt)
    return {"qpos": np.tile(row, (CLIP_ROWS, 1)), "qvel": np.zeros((CLIP_ROWS, 6 + J)), "root2site": np.tile(ft["root2site"], (CLIP_ROWS, 1, 1)),
            "joint_quat": np.tile(ft["joint_quat"][1:], (CLIP_ROWS, 1, 1))}


@functools.lru_cache(maxsize=1)
def static_clips():
    """(WalkRefSet of static clips, [dict(set, pose, contacts, ncon0, nself0)]): two poses of each of the sets A, B, C.  A clip's pose is
    what a reset builds from its row - qpos0, the root, the tracked joints, the retracted wings - so the set's state is rebuilt that way
    and settled again; it is taken when `walk_floor_convex_sets._accept` takes it (every capacity, CLEAR of every switching distance)."""
    from flybody_amd.tasks import walking as W

    view = world()[0]
    ty = F._flat("geom_type")
    rows, info = [], []
    for which in ("A", "B", "C"):
        got = 0
        for s in F.get(which):
            for depth in (0.004, 0.008, 0.012):
                pose = F._settle(view.full_qpos(_row(view, s[0])), depth)
                ok, keep, _ = F._accept(pose)
                if ok and (which != "A" or any(ty[c[0]] == 5 for c in keep)):
                    break
            else:
                continue
            rows.append(_row(view, pose))
            info.append(dict(set=which, pose=pose, contacts=keep))
            got += 1
            if got == 2:
                break
        assert got == 2, (which, got)
    refs = W.WalkRefSet([_static_snippet(view, r) for r in rows])
    return refs, info


def reset_pose(refs, clip):
    """The oracle's own state after a reset on clip `clip` of `refs` on the shipped blob."""
    o = E.make_oracle(0, refs=refs)
    o.force_next(clip)
    o.reset()
    return o.data.qpos.copy()


def witness_reset(refs, clip, pad):
    """(st, reward, discount, obs, ncon_matter, fly-fly among them, restated contacts, layout) of a reset on clip `clip` of `refs` by an
    oracle env on the witness blob of the pose that reset builds."""
    pose = reset_pose(refs, clip)
    con, clear = F.restated(pose)
    keep = F.matter(con)
    assert len(keep) == len(con) and clear >= CLEAR
    m, _ = F.witness_model(pose, keep)
    o = make_oracle(0, model=m, refs=refs)
    o.set_pad_first_obs(pad)
    o.force_next(clip)
    st, r, disc, obs = o.reset()
    assert np.array_equal(o.data.qpos, pose)
    return st, r, disc, obs, o.data.ncon_matter, S._matter_self(m, o.data), keep, o.LAYOUT, o


# ------------------------------------------------------------------------------------------------ 3. the bridge
@functools.lru_cache(maxsize=1)
def bridge_states():
    """[(set, qpos, qvel, act)]: sets A, B, C (24 states)."""
    return [(w, s[0], s[1], s[2]) for w in ("A", "B", "C") for s in F.get(w)]


def applied_ctrl(action):
    """The ctrl the environment applies for a raw action (the oracle env's own `apply_action`)."""
    o = E.make_oracle(0, terminal_com_dist=np.inf)
    o.force_next(0)
    o.reset()
    assert o.step(action)[0] == 1
    return o.data.ctrl.copy()
