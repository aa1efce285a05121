"""GPU parity tests of the floor plane against the walking fly's ellipsoids and cylinders (csrc/walk_full_env.hip `floor_full_step`,
through `BatchedWalkPhysics(floor_contacts=True, self_contacts=True, floor_convex=True)` and the C ABI).
Run with `-m gpu` on an MI355X.  One wavefront is one env; no batch here exceeds 130.

The float64 oracle does not restate the two colliders, so a fallen state is compared with the oracle on its WITNESS blob
(tests/walk_floor_convex_sets.py): the shipped blob plus one small sphere per plane-ellipsoid / plane-cylinder contact, placed so that the
oracle's plane-sphere contact has exactly the wanted distance, position and pair parameters.  The device runs on the shipped blob with
the bit.  A witness is valid for the collision pass of its own state, so the oracle comparisons are one substep, teacher-forced.
State sets A / B / C of that file (fallen: on the abdomen, on the back, on coxae and mouth parts) and R10 / XL / XS of
tests/walk_self_sets.py (standing and lifted: no plane-ellipsoid / plane-cylinder contact).

Bounds per error group (the groups of tests/test_gpu_walk_limits.py): CAP1 of that file on the fallen sets; on R10 / XL / XS the bounds
of tests/test_gpu_walk_self.py.  The reference is always the oracle."""
import numpy as np
import pytest

import walk_floor_convex_sets as F
import walk_self_sets as S
from test_gpu_walk_floor import CAP1, CAP10, LADDER, _assert_bounds, _ctrls, _errors, _gpu_advance, _kept  # noqa: F401
from test_gpu_walk_self import ONE_MEASURED as SELF_MEASURED
from walk_floor_convex_sets import FULL, WALK_FLOOR_CONVEX
from walk_self_sets import NO_FLUID, SELF, WALK_SELF

pytestmark = pytest.mark.gpu
NO_GRAVITY, NO_ACTUATION, WALK_EPISODES, NO_LIMIT, NO_CONTACT, WALK_JOINT_LIMITS, WALK_FLOOR = 16, 32, 1024, 2, 64, 512, 2048
# Worst one-substep errors per set over the three flag sets of LADDER, measured on the MI355X against the oracle on the witness blobs
# (relative to max(1, max |ref| of the group) on the velocity groups); no state is left out.  Int 5 (2 ... 7 on A, 1 ... 11 on B, 2 ... 9
# on C) equals the oracle's `ncon_matter` on the witness blob and real 2 (1 ... 6, 1 ... 5, 2 ... 4) the restated count on every state;
# real 1 is within 7.1e-8 cm of the smaller minimum; the solver took at most 12 iterations.  Recorded, not a bound: the bound is CAP1.
#   A  hinge_qpos 1.824e-7, root_pos 1.587e-8, root_quat 1.362e-7, act 2.704e-8, root_lin 2.810e-5, root_ang 3.945e-5, hinge_vel 9.315e-6
#   B  hinge_qpos 5.976e-7, root_pos 5.679e-9, root_quat 1.957e-7, act 2.642e-8, root_lin 2.841e-5, root_ang 1.109e-4, hinge_vel 2.616e-5
#   C  hinge_qpos 3.391e-7, root_pos 2.362e-8, root_quat 1.006e-7, act 2.703e-8, root_lin 5.516e-5, root_ang 7.115e-5, hinge_vel 1.738e-5
ONE_MEASURED = {
    "A": {"hinge_qpos": 1.83e-7, "root_pos": 1.59e-8, "root_quat": 1.37e-7, "act": 2.8e-8, "root_lin": 2.9e-5, "root_ang": 4.0e-5, "hinge_vel": 9.4e-6},
    "B": {"hinge_qpos": 6.0e-7, "root_pos": 5.7e-9, "root_quat": 2.0e-7, "act": 2.7e-8, "root_lin": 2.9e-5, "root_ang": 1.11e-4, "hinge_vel": 2.7e-5},
    "C": {"hinge_qpos": 3.4e-7, "root_pos": 2.4e-8, "root_quat": 1.01e-7, "act": 2.8e-8, "root_lin": 5.6e-5, "root_ang": 7.2e-5, "hinge_vel": 1.74e-5},
}


@pytest.fixture(scope="module")
def torch_mod():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def _advance(torch, states, ctrls, nsteps, flags, **kw):
    return _gpu_advance(torch, states, ctrls, nsteps, flags, blob=S.WALK_BLOB, **kw)


@pytest.mark.parametrize("which", ["A", "B", "C"])
@pytest.mark.parametrize("extra,name", LADDER)
def test_one_substep_teacher_forced(torch_mod, which, extra, name):
    """One substep from every state of the set against the oracle on the state's witness blob: every error group within CAP1; int 5 is
    the oracle's `ncon_matter` on the witness blob, real 2 the restated plane-ellipsoid / plane-cylinder contacts, real 1 the smaller of
    the oracle's and the restatement's smallest distance within 2e-6 cm; no overflow bit."""
    states = F.get(which)
    ctrls = _ctrls(len(states))
    trace, ref = [], []
    for s, c in zip(states, ctrls):
        ref.append(F.oracle_advance(s, c.astype(np.float64), 1, extra, trace=trace))
    q, v, a, ints, reals, info = _advance(torch_mod, states, ctrls, 1, FULL | extra)
    assert np.isfinite(q).all() and np.isfinite(v).all()
    keep = _kept(ref, f"{which} {name}")
    assert len(keep) == len(states)  # (the sets are built clear of every switching distance)
    e = _errors(q, v, a, ref, keep)
    print(f"one substep [{which} {name}]: " + " ".join(f"{k} {x:.3e}" for k, x in e.items()) + f" solver iterations max {ints[:, 6].max()} "
          f"contacts {ints[:, 5].tolist()} fly-fly {ints[:, 3].tolist()} plane-convex {reals[:, 2].tolist()} limit rows {ints[:, 4].tolist()} "
          f"bits {ints[:, 7].tolist()} nefc {[t['nefc'] for t in trace]}")
    print(f"per state [{which} {name}] worst velocity error: " + " ".join(f"{max(_errors(q, v, a, ref, [i])[k] for k in ('root_lin', 'root_ang', 'hinge_vel')):.1e}" for i in keep))
    print(f"smallest distance [{which} {name}]: worst difference {max(abs(reals[i, 1] - trace[i]['mind']) for i in keep):.3e}")
    assert ints[:, 5].tolist() == [t["ncon_matter"] for t in trace], (ints[:, 5].tolist(), trace)
    assert reals[:, 2].tolist() == [t["nconvex"] for t in trace], (reals[:, 2].tolist(), trace)
    assert max(t["nconvex"] for t in trace) >= 2
    for i in keep:
        assert abs(reals[i, 1] - trace[i]["mind"]) <= 2e-6, (i, reals[i, 1], trace[i])
    assert not ints[:, 7].any() and not info.any() and not ints[:, [0, 1, 2]].any()
    for k in CAP1:
        assert e[k] <= CAP1[k], (which, name, k, e[k], CAP1[k])


@pytest.mark.parametrize("which", ["R10", "XL", "XS"])
def test_no_plane_convex_contact_no_new_physics(torch_mod, which):
    """R10 / XL / XS have no plane-ellipsoid / plane-cylinder contact: the new handle meets the oracle bounds of
    tests/test_gpu_walk_self.py on the shipped blob, with the oracle's counts and a new count of 0.  (It is another kernel: bit identity
    with `floor_self_step` is not asked for.)"""
    m = S.model()
    states = {"R10": S.r10, "XL": S.x_lifted, "XS": S.x_standing}[which]()
    ctrls = _ctrls(len(states))
    trace, ref = [], []
    for s, c in zip(states, ctrls):
        tr = []
        ref.append(S.oracle_advance(m, s, c.astype(np.float64), 1, 0, trace=tr))
        trace.append(tr[0])
    q, v, a, ints, reals, info = _advance(torch_mod, states, ctrls, 1, FULL)
    keep = _kept(ref, f"{which} all")
    e = _errors(q, v, a, ref, keep)
    print(f"one substep without a plane-convex contact [{which}]: " + " ".join(f"{k} {x:.3e}" for k, x in e.items()))
    assert ints[keep, 5].tolist() == [trace[i][0] for i in keep] and ints[keep, 3].tolist() == [trace[i][1] for i in keep]
    assert not reals[:, 2].any() and not ints[:, 7].any() and not info.any()
    _assert_bounds(e, SELF_MEASURED[which], CAP1, which)


def test_without_the_bit_the_contacts_are_missed(torch_mod):
    """Set B on the parent handle (FFE_WALK_SELF without the bit): fewer contacts and a smaller sum of normal forces on every state."""
    states = F.get("B")
    ctrls = _ctrls(len(states))
    new = _advance(torch_mod, states, ctrls, 1, FULL)
    old = _advance(torch_mod, states, ctrls, 1, SELF)
    print(f"with the bit: contacts {new[3][:, 5].tolist()} normal forces {new[4][:, 0].tolist()}; without: {old[3][:, 5].tolist()} {old[4][:, 0].tolist()}")
    assert (old[3][:, 5] < new[3][:, 5]).all() and (old[4][:, 0] < new[4][:, 0]).all() and not old[4][:, 2].any()


def test_root_only_rows(torch_mod):
    """A state of B in which the thorax ellipsoids alone touch the floor, at rest, gravity and actuation off: the contact rows have the
    root entries J_r = (p x e, e) alone, so the hinges feel the contact only through Y.  One substep against the float64 witness run,
    every group within CAP1; and the root's momentum: the total linear momentum along the plane's normal after the substep (the oracle
    evaluates it from the device's state; every other force is internal or zero at rest) is h x real 0, the ratio within CAP1's root_lin."""
    from oracle import oracle as O

    names = S.tables()[1]
    pick = [s for s in F.get("B") if s[3][1] == 0 and all("thorax" in names[c[0]] for c in F.restated(s[0])[0])]
    assert pick
    states = [(s[0], np.zeros(108), np.zeros(59)) for s in pick]
    zero = [np.zeros(59, dtype=np.float32)] * len(states)
    flags = NO_GRAVITY | NO_ACTUATION | NO_FLUID
    trace, ref = [], []
    for s in states:
        ref.append(F.oracle_advance(s, np.zeros(59), 1, flags, trace=trace))
    q, v, a, ints, reals, info = _advance(torch_mod, states, zero, 1, FULL | flags)
    e = _errors(q, v, a, ref, list(range(len(states))))
    print("root-only rows: " + " ".join(f"{k} {x:.3e}" for k, x in e.items()) + f" contacts {ints[:, 5].tolist()} plane-convex {reals[:, 2].tolist()}")
    assert (ints[:, 5] == reals[:, 2]).all() and (reals[:, 2] >= 1).all() and not ints[:, 3].any()
    for k in CAP1:
        assert e[k] <= CAP1[k], (k, e[k])
    m = S.model()
    d = O.OracleData(m)
    n, _ = F.plane()
    for i in range(len(states)):
        # (the new velocity at the pose it was formed in: qvel+ = qvel + h qacc belongs to the configuration before the integration)
        d.qpos[:], d.qvel[:], d.act[:] = states[i][0], v[i], a[i]
        d.ctrl[:] = 0
        d.forward()
        lin, _ = d.momentum()
        impulse = m.timestep * reals[i, 0]
        print(f"root-only rows state {i}: p.n {float(lin @ n):.6e} h x normal force {impulse:.6e} max |hinge vel| {np.abs(v[i, 6:]).max():.3e}")
        assert impulse > 0 and abs(float(lin @ n) / impulse - 1.0) <= CAP1["root_lin"]


@pytest.mark.parametrize("which", ["A", "B"])
def test_ten_substeps_open_loop(torch_mod, which):
    """Ten substeps from every state, at rest (a state's random velocity may point into the floor): finite, no overflow, and the
    smallest distance does not fall below the first substep's (the floor pushes the fly out).  No oracle here: a witness blob is valid
    for the collision pass of its own state only."""
    states = [(s[0], np.zeros(108), np.zeros(59)) for s in F.get(which)]
    zero = [np.zeros(59, dtype=np.float32)] * len(states)
    one = _advance(torch_mod, states, zero, 1, FULL)
    ten = _advance(torch_mod, states, zero, 10, FULL)
    print(f"ten substeps [{which}]: smallest distance first {one[4][:, 1].tolist()} tenth {ten[4][:, 1].tolist()} contacts {ten[3][:, 5].tolist()}")
    for x in ten[:3] + (ten[4],):
        assert np.isfinite(x).all()
    assert np.abs(ten[1]).max() < 1e4 and not ten[5].any()
    assert (ten[4][:, 1] >= one[4][:, 1] - 2e-6).all()


def _belly_down():
    from flybody_amd.model.blob import read_blob

    q0 = np.asarray(read_blob(S.WALK_BLOB)["qpos0"], dtype=np.float64).ravel().copy()
    q0[2] = 0.05
    return (q0, np.zeros(108), np.zeros(59))


def test_overflow_stays_finite(torch_mod):
    """qpos0 with the root at z = 0.05 cm, belly down: far more floor contacts of both kinds than slots.  The 16 deepest are kept, the env
    is flagged with bit value 1 and a control step stays finite; fallen states in the same batch are not flagged."""
    low = _belly_down()
    d = F.forward(low[0])
    con = F.restated(low[0], d)[0]
    assert d.ncon_matter + len(con) > 16 and len(con) >= 4
    states = [low] * 2 + [s[:3] for s in F.get("B")[:4]]
    zero = [np.zeros(59, dtype=np.float32)] * len(states)
    q, v, a, ints, reals, info = _advance(torch_mod, states, zero, 1, FULL)
    print(f"overflow, first substep: contacts {ints[:, 5].tolist()} fly-fly {ints[:, 3].tolist()} plane-convex {reals[:, 2].tolist()} validity {info[:, 0].tolist()}"
          f" smallest distance {reals[:2, 1].tolist()}")
    assert (ints[:2, 5] == 16).all() and (info[:2, 0] & 1).all() and np.isfinite(v).all()
    # the deepest of both kinds: the smallest distance over the oracle's floor contacts and the restated ones is among the kept
    deepest = min([r[5] for r in F.floor_rows(d.contacts())] + [c[2] for c in con])
    assert np.abs(reals[:2, 1] - deepest).max() <= 2e-6
    q, v, a, ints, reals, info = _advance(torch_mod, states, zero, 10, FULL)
    assert np.isfinite(q).all() and np.isfinite(v).all() and np.isfinite(a).all() and np.isfinite(reals).all()
    assert np.abs(v).max() < 1e6
    assert (info[:2, 0] & 1).all() and (ints[:2, 7] & 1).all() and (ints[:2, 5] == 16).all()
    assert not info[2:, 0].any() and not ints[2:, 7].any() and not info[:, 1:].any()


def test_overflow_keeps_the_deepest_of_both_kinds(torch_mod):
    """Two belly-down states with tucked legs whose 16 deepest floor contacts are of both kinds and leave out contacts of both kinds (in
    the second the primitive pass overflows by itself first): 16 contacts kept, bit value 1, and the number of plane-ellipsoid /
    plane-cylinder contacts among them is the number among the 16 deepest of the oracle's floor contacts and the restated ones."""
    states = F.overflow_mixed()
    want = [F.deepest_sixteen(s[0]) for s in states]
    assert all(0 < w[0] < 16 < w[1] for w in want), want
    zero = [np.zeros(59, dtype=np.float32)] * len(states)
    q, v, a, ints, reals, info = _advance(torch_mod, states, zero, 1, FULL)
    print(f"mixed overflow: contacts {ints[:, 5].tolist()} fly-fly {ints[:, 3].tolist()} plane-convex {reals[:, 2].tolist()} wanted {want} validity {info[:, 0].tolist()}")
    assert (ints[:, 5] == 16).all() and not ints[:, 3].any() and (info[:, 0] & 1).all() and np.isfinite(v).all()
    assert reals[:, 2].tolist() == [w[0] for w in want]
    assert np.abs(reals[:, 1] - np.array([w[2] for w in want])).max() <= 2e-6


def test_a_launch_depends_on_its_state_alone(torch_mod):
    """State B after the handle has run state A gives the bits of B on a fresh handle: nothing is kept from launch to launch."""
    import torch

    from flybody_amd.batched_env import BatchedWalkPhysics

    first, second = [s[:3] for s in F.get("A")[:6]], [s[:3] for s in F.get("B")[:6]]
    ctrl = _ctrls(6, seed=12)
    fresh = _advance(torch_mod, second, ctrl, 10, FULL)
    env = BatchedWalkPhysics(batch_size=6, floor_contacts=True, self_contacts=True, floor_convex=True)
    t = lambda rows, k, dt=torch.float64: torch.tensor(np.stack([r[k] for r in rows]), dtype=dt, device="cuda")
    c = torch.tensor(np.stack(ctrl), dtype=torch.float32, device="cuda")
    for st in (first, second):
        env.set_state(t(st, 0), t(st, 1))
        env.set_act(t(st, 2))
        env.physics_step(c, 10)
    q, v = env.get_state()
    a = env.get_act()
    ints, reals = env.get_task_state()
    torch.cuda.synchronize()
    for x, y in zip((q, v, a, ints, reals), fresh):
        assert np.array_equal(x.cpu().numpy(), y)
    env.close()


def test_rows_do_not_depend_on_their_batch(torch_mod):
    """Four states alone (B = 1 each) and at rows 0, 63, 64 and 129 of a batch of 130 whose other rows hold another state."""
    A, B, C = F.get("A"), F.get("B"), F.get("C")
    four, ctrls = [A[6][:3], B[0][:3], C[7][:3], _belly_down()], _ctrls(4, seed=8)
    alone = [_advance(torch_mod, [s], [c], 3, FULL) for s, c in zip(four, ctrls)]
    out = _advance(torch_mod, four, ctrls, 3, FULL, batch=130, rows=[0, 63, 64, 129], filler=(A[1][:3], _ctrls(1, seed=9)[0]))
    for i, one in enumerate(alone):
        for x, y in zip(out, one):
            assert np.array_equal(x[i], y[0]), i


def test_protocol(torch_mod):
    """The keywords and the flag set that create the handle, the sets refused with a text naming the bit, the calls the handle refuses,
    and the zeros of a fresh handle."""
    from flybody_amd import _capi
    from flybody_amd.batched_env import FFE_WALK_FLOOR_CONVEX, BatchedWalkPhysics

    torch = torch_mod
    L = _capi.lib()
    assert FFE_WALK_FLOOR_CONVEX == WALK_FLOOR_CONVEX == 32768
    for kw in ({}, {"floor_contacts": True}):
        with pytest.raises(ValueError, match="floor_convex"):
            BatchedWalkPhysics(batch_size=1, floor_convex=True, **kw)
    env = BatchedWalkPhysics(batch_size=4, floor_contacts=True, self_contacts=True, floor_convex=True)
    assert env.physics_flags == FULL
    other = BatchedWalkPhysics(batch_size=1, floor_contacts=True, self_contacts=True, floor_convex=True, physics_flags=NO_FLUID | 128 | 256,
                               blob_path=S.WALK_BLOB)
    assert other.physics_flags == FULL | NO_FLUID | 128 | 256
    other.close()
    ints, reals = env.get_task_state()
    info = torch.ones(4, 4, dtype=torch.int32, device="cuda")
    assert L.ffe_get_validity(env._h, info.data_ptr(), env._stream()) == 0
    torch.cuda.synchronize()
    assert not ints.cpu().numpy().any() and not reals.cpu().numpy().any() and not info.cpu().numpy().any()
    z = torch.zeros(4, 59, dtype=torch.float32, device="cuda")
    obs, rew, st = torch.zeros(4, 8, device="cuda"), torch.zeros(4, device="cuda"), torch.zeros(4, dtype=torch.int32, device="cuda")
    p = lambda x: x.data_ptr()
    calls = {
        "ffe_reset": lambda: L.ffe_reset(env._h, p(obs), p(rew), p(rew), p(st), env._stream()),
        "ffe_step": lambda: L.ffe_step(env._h, p(z), p(obs), p(rew), p(rew), p(st), env._stream()),
    }
    for name, call in calls.items():
        assert call() < 0, name
        assert b"not available on a walk physics handle" in L.ffe_last_error(env._h), name
    env.physics_step(z, 1)  # still usable
    torch.cuda.synchronize()
    assert np.isfinite(env.get_state()[0].cpu().numpy()).all()
    env.close()
    C = WALK_FLOOR_CONVEX
    for bad in (C, NO_CONTACT | C, S.FLOOR | C, SELF | C | NO_LIMIT, SELF | C | WALK_EPISODES, SELF | C | WALK_EPISODES | 8192,
                NO_CONTACT | NO_LIMIT | C, NO_CONTACT | WALK_JOINT_LIMITS | C, NO_CONTACT | WALK_JOINT_LIMITS | WALK_SELF | C, FULL | 16384):
        with pytest.raises(RuntimeError, match="FFE_WALK_FLOOR_CONVEX"):
            BatchedWalkPhysics(batch_size=1, physics_flags=bad)
    # without the new bit the pinned refusals stay
    with pytest.raises(RuntimeError, match="FFE_WALK_SELF"):
        BatchedWalkPhysics(batch_size=1, physics_flags=SELF | 16384)
