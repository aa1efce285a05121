"""GPU parity tests of the floor contacts of the free-root walking-fly physics (csrc/walk_env.hip `floor_step`, through
`BatchedWalkPhysics(floor_contacts=True)` and the C ABI) against the float64 oracle on identical inputs.
Run with `-m gpu` on an MI355X.  One wavefront is one env; no batch here exceeds 130.

Both sides run on the floor-only copy of the walk blob of tests/walk_floor_sets.py (the oracle would otherwise collide the fly's own
pairs too); state sets F06 / F10 of that file.  A state is left out of a comparison only when the oracle's `contact_hist` reports a
candidate pair within 2e-6 cm of a switching distance during the substeps compared, at most 3 of 24 per set.

Bounds per error group (the groups of tests/test_gpu_walk_limits.py): min(3 x the worst value measured on the MI355X, CAP1 / CAP10 of
that file)."""
import numpy as np
import pytest

import walk_floor_sets as S
from walk_floor_sets import FLOOR, NO_ADHESION, NO_CONTACT, NO_FLUID, NO_LIMIT, NO_NOSLIP, WALK_EPISODES, WALK_FLOOR, WALK_JOINT_LIMITS

pytestmark = pytest.mark.gpu
LIM = NO_CONTACT | WALK_JOINT_LIMITS
# caps: tests/test_gpu_walk_limits.py (1.5e-4 on velocities is also tests/test_gpu_ball.py's bound for one substep of cone contacts)
CAP1 = {"hinge_qpos": 2e-6, "root_pos": 2e-6, "root_quat": 2e-6, "act": 1e-6, "root_lin": 1.5e-4, "root_ang": 1.5e-4, "hinge_vel": 1.5e-4}
CAP10 = {"hinge_qpos": 2e-5, "root_pos": 2e-5, "root_quat": 2e-5, "act": 1e-6, "root_lin": 1e-2, "root_ang": 1e-2, "hinge_vel": 1e-2}
# Worst one-substep errors over F06 + F10 and the three flag sets, measured on the MI355X against the oracle (relative to
# max(1, max |ref| of the group) on the velocity groups): hinge_qpos 1.160e-7 (F06 no_fluid_no_adhesion), root_pos 1.474e-9, root_quat
# 8.878e-8, act 4.047e-8, root_lin 7.060e-6 (F10 all), root_ang 1.292e-4 (F10 no_fluid_no_adhesion; the other five cases 1.8e-5 ...
# 7.8e-5), hinge_vel 3.644e-5.  The solver took at most 7 iterations.  One state of F06 is left out (2e-6 cm band), none of F10.
ONE_MEASURED = {"hinge_qpos": 1.17e-7, "root_pos": 1.48e-9, "root_quat": 8.9e-8, "act": 4.1e-8, "root_lin": 7.1e-6, "root_ang": 1.3e-4,
                "hinge_vel": 3.7e-5}
# Ten substeps open loop on F06, measured the same way (3 of 24 states left out): hinge_qpos 5.224e-7, root_pos 1.819e-8, root_quat
# 1.614e-7, act 3.955e-8, root_lin 1.917e-5, root_ang 8.927e-5, hinge_vel 1.551e-5.
TEN_MEASURED = {"hinge_qpos": 5.3e-7, "root_pos": 1.9e-8, "root_quat": 1.7e-7, "act": 4.0e-8, "root_lin": 2.0e-5, "root_ang": 9.0e-5,
                "hinge_vel": 1.6e-5}


@pytest.fixture(scope="module")
def torch_mod():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def _ctrls(n, seed=11):
    rs = np.random.RandomState(seed)
    return [rs.uniform(-0.5, 0.5, 59).astype(np.float32) for _ in range(n)]


def _gpu_advance(torch, states, ctrls, nsteps, flags, batch=None, rows=None, filler=None, blob=None, calls=1):
    """Advances `states` on the device (tests/test_gpu_walk_limits.py::_gpu_advance with the blob, the reals and `calls` launches of
    `nsteps` substeps each)."""
    from flybody_amd import _capi
    from flybody_amd.batched_env import BatchedWalkPhysics

    n = len(states)
    batch = batch or n
    rows = list(range(n)) if rows is None else list(rows)
    if filler is not None:
        states, ctrls = list(states) + [filler[0]], list(ctrls) + [filler[1]]
    pick = [n] * batch
    for k, r in enumerate(rows):
        pick[r] = k
    env = BatchedWalkPhysics(batch_size=batch, physics_flags=flags, blob_path=blob or S.floor_only_blob())
    qpos = torch.tensor(np.stack([states[k][0] for k in pick]), dtype=torch.float64, device="cuda")
    qvel = torch.tensor(np.stack([states[k][1] for k in pick]), dtype=torch.float64, device="cuda")
    act = torch.tensor(np.stack([states[k][2] for k in pick]), dtype=torch.float64, device="cuda")
    env.set_state(qpos, qvel)
    env.set_act(act)
    ctrl = torch.tensor(np.stack([ctrls[k] for k in pick]), dtype=torch.float32, device="cuda")
    for _ in range(calls):
        env.physics_step(ctrl, nsteps)
    q, v = env.get_state()
    a = env.get_act()
    ints, reals = env.get_task_state()
    info = torch.full((batch, 4), -1, dtype=torch.int32, device="cuda")
    assert _capi.lib().ffe_get_validity(env._h, info.data_ptr(), env._stream()) == 0
    torch.cuda.synchronize()
    out = (q.cpu().numpy()[rows], v.cpu().numpy()[rows], a.cpu().numpy()[rows], ints.cpu().numpy()[rows], reals.cpu().numpy()[rows],
           info.cpu().numpy()[rows])
    env.close()
    return out


def _errors(q, v, a, ref, keep):
    """Worst error per group over the kept states (tests/test_gpu_walk_limits.py::_errors)."""
    e = {k: 0.0 for k in CAP1}

    def rel(x, r):
        return float(np.abs(x - r).max() / max(1.0, np.abs(r).max()))

    for i in keep:
        rq, rv, ra = ref[i][:3]
        e["hinge_qpos"] = max(e["hinge_qpos"], float(np.abs(q[i, 7:] - rq[7:]).max()))
        e["root_pos"] = max(e["root_pos"], float(np.abs(q[i, :3] - rq[:3]).max()))
        sgn = 1.0 if np.dot(q[i, 3:7], rq[3:7]) >= 0 else -1.0
        e["root_quat"] = max(e["root_quat"], float(np.abs(sgn * q[i, 3:7] - rq[3:7]).max()))
        e["act"] = max(e["act"], float(np.abs(a[i] - ra).max()))
        e["root_lin"] = max(e["root_lin"], rel(v[i, :3], rv[:3]))
        e["root_ang"] = max(e["root_ang"], rel(v[i, 3:6], rv[3:6]))
        e["hinge_vel"] = max(e["hinge_vel"], rel(v[i, 6:], rv[6:]))
    return e


def _kept(ref, name):
    keep = [i for i, r in enumerate(ref) if r[3] >= S.BAND]
    print(f"{name}: {len(ref) - len(keep)} of {len(ref)} states within {S.BAND:g} cm of a switching distance are left out")
    assert len(ref) - len(keep) <= 3
    return keep


def _assert_bounds(e, measured, cap, name):
    assert measured is not None, "the measured errors have not been recorded"
    for k in cap:
        assert e[k] <= min(3 * measured[k], cap[k]), (name, k, e[k], measured[k], cap[k])


LADDER = [(0, "all"), (NO_NOSLIP, "no_noslip"), (NO_FLUID | NO_ADHESION, "no_fluid_no_adhesion")]


@pytest.mark.parametrize("which", ["F06", "F10"])
@pytest.mark.parametrize("extra,name", LADDER)
def test_one_substep_teacher_forced(torch_mod, which, extra, name):
    """One substep from every state of the set; task-state int 5 is the oracle's contact count on every state."""
    m, F06, F10 = S.sets()
    states = F06 if which == "F06" else F10
    ctrls = _ctrls(len(states))
    ncon, nefc, ref = [], [], []
    for s, c in zip(states, ctrls):
        tr = []
        ref.append(S.oracle_advance(m, s, c.astype(np.float64), 1, extra, trace=tr))
        ncon.append(tr[0][0])
        nefc.append(tr[0][1])
    assert 2 <= min(ncon) and max(ncon) <= 6 and 7 <= min(nefc) and max(nefc) <= 18, (ncon, nefc)
    q, v, a, ints, reals, info = _gpu_advance(torch_mod, states, ctrls, 1, FLOOR | extra)
    assert np.isfinite(q).all() and np.isfinite(v).all()
    keep = _kept(ref, f"{which} {name}")
    e = _errors(q, v, a, ref, keep)
    print(f"one substep [{which} {name}]: " + " ".join(f"{k} {x:.3e}" for k, x in e.items()) + f" solver iterations max {ints[:, 6].max()} "
          f"contacts {ints[:, 5].tolist()} limit rows {ints[:, 4].tolist()}")
    assert ints[keep, 5].tolist() == [ncon[i] for i in keep], (ints[:, 5].tolist(), ncon)
    assert not ints[:, 7].any() and not info.any() and not ints[:, [0, 1, 2, 3]].any()
    _assert_bounds(e, ONE_MEASURED, CAP1, name)


def test_ten_substeps_open_loop(torch_mod):
    m, F06, _ = S.sets()
    ctrls = _ctrls(len(F06), seed=3)
    ref = [S.oracle_advance(m, s, c.astype(np.float64), 10, 0) for s, c in zip(F06, ctrls)]
    q, v, a, ints, reals, info = _gpu_advance(torch_mod, F06, ctrls, 10, FLOOR)
    keep = _kept(ref, "ten substeps F06")
    e = _errors(q, v, a, ref, keep)
    print("ten substeps F06: " + " ".join(f"{k} {x:.3e}" for k, x in e.items()))
    assert not info.any()
    _assert_bounds(e, TEN_MEASURED, CAP10, "ten")


def test_a_standing_fly_is_carried(torch_mod):
    """The oracle's own known answer (tests/test_oracle_walk.py): from the reset pose of clip 0 with zero ctrl, after 60 control steps
    the fly still stands on at least 3 contacts whose normal forces add up to its weight."""
    from flybody_amd.model.blob import read_blob

    qpos = S.reset_pose()
    state = (qpos, np.zeros(108), np.zeros(59))
    q, v, a, ints, reals, info = _gpu_advance(torch_mod, [state] * 2, [np.zeros(59, dtype=np.float32)] * 2, 10, FLOOR, calls=60)
    weight = float(np.sum(read_blob(S.WALK_BLOB)["body_mass"])) * 981.0
    print(f"standing fly: z {q[0, 2]:.5f} contacts {ints[0, 5]} normal force {reals[0, 0]:.4f} (weight {weight:.4f}) smallest distance {reals[0, 1]:.3e} "
          f"limit rows {ints[0, 4]} validity {info[0, 0]}")
    assert np.array_equal(q[0], q[1])
    assert 0.10 < q[0, 2] < 0.14
    assert ints[0, 5] >= 3
    assert abs(reals[0, 0] - weight) < 0.05 * weight, (reals[0, 0], weight)
    assert reals[0, 1] > -2e-3


def test_no_floor_in_reach_no_difference(torch_mod):
    """F06 lifted to z = 1 cm, 10 substeps: the floor handle and a limits handle give the same bits (every state has limit rows on the
    way).  While the root is higher over the plane than any geom can reach, a floor substep is the limits kernel's own code."""
    _, F06, _ = S.sets()
    states = []
    for q, v, a in F06:
        q = q.copy()
        q[2] = 1.0
        states.append((q, v, a))
    ctrls = _ctrls(len(states), seed=5)
    qf, vf, af, fints, freals, finfo = _gpu_advance(torch_mod, states, ctrls, 10, FLOOR)
    ql, vl, al, lints, _, linfo = _gpu_advance(torch_mod, states, ctrls, 10, LIM)
    bad = [i for i in range(len(states)) if not (np.array_equal(qf[i], ql[i]) and np.array_equal(vf[i], vl[i]) and np.array_equal(af[i], al[i]))]
    print(f"no floor in reach: {len(bad)} of {len(states)} states differ {bad}; max |dq| {np.abs(qf - ql).max():.3e} |dv| {np.abs(vf - vl).max():.3e}; "
          f"limit rows {lints[:, 4].tolist()} iterations floor {fints[:, 6].tolist()} limits {lints[:, 6].tolist()}")
    assert not fints[:, 5].any() and not freals.any()
    assert np.array_equal(qf, ql) and np.array_equal(vf, vl) and np.array_equal(af, al)
    assert np.array_equal(fints, lints) and np.array_equal(finfo, linfo)


def test_committed_blob_and_floor_only_blob_give_the_same_bits(torch_mod):
    _, F06, _ = S.sets()
    ctrls = _ctrls(len(F06), seed=7)
    a = _gpu_advance(torch_mod, F06, ctrls, 10, FLOOR)
    b = _gpu_advance(torch_mod, F06, ctrls, 10, FLOOR, blob=S.WALK_BLOB)
    assert a[3][:, 5].min() >= 1
    for x, y in zip(a, b):
        assert np.array_equal(x, y)


def test_overflow_stays_finite(torch_mod):
    """qpos0 with the root at z = 0.05 cm (the oracle has 77 contacts and 231 rows there): one control step stays finite and the env is
    flagged with bit value 1.  Int 5 equals the capacity after the first substep of that control step, where it is read: the fly is
    pushed out so fast (the oracle: 77, 77, 76, 75, 63, 59, 51, 42, 30 and 10 contacts in the ten substeps, 53 cm/s at the end) that the
    tenth substep has fewer contacts than slots on the device too (15).  F06's envs in the same batch are not flagged."""
    from flybody_amd.model.blob import read_blob

    _, F06, _ = S.sets()
    q0 = np.asarray(read_blob(S.WALK_BLOB)["qpos0"], dtype=np.float64).ravel().copy()
    q0[2] = 0.05
    low = (q0, np.zeros(108), np.zeros(59))
    states = [low] * 2 + F06[:4]
    zero = [np.zeros(59, dtype=np.float32)] * len(states)
    q, v, a, ints, reals, info = _gpu_advance(torch_mod, states, zero, 1, FLOOR)
    print(f"overflow, first substep: contacts {ints[:, 5].tolist()} validity {info[:, 0].tolist()}")
    assert (ints[:2, 5] == 16).all() and (info[:2, 0] & 1).all() and np.isfinite(v).all()
    q, v, a, ints, reals, info = _gpu_advance(torch_mod, states, zero, 10, FLOOR)
    print(f"overflow, one control step: max |qvel| {np.abs(v[:2]).max():.3e} contacts {ints[:, 5].tolist()} validity {info[:, 0].tolist()} "
          f"normal force {reals[:2, 0].tolist()}")
    assert np.isfinite(q).all() and np.isfinite(v).all() and np.isfinite(a).all() and np.isfinite(reals).all()
    assert np.abs(v).max() < 1e6
    assert (info[:2, 0] & 1).all() and (ints[:2, 7] & 1).all()
    assert not info[2:, 0].any() and not ints[2:, 7].any() and not info[:, 1:].any()


def test_rows_do_not_depend_on_their_batch(torch_mod):
    """Four of F10's states alone (B = 1 each) and at rows 0, 63, 64 and 129 of a batch of 130 whose other rows hold another state."""
    _, F06, F10 = S.sets()
    four, ctrls = [F10[3], F10[8], F10[11], F10[22]], _ctrls(4, seed=8)
    alone = [_gpu_advance(torch_mod, [s], [c], 3, FLOOR) for s, c in zip(four, ctrls)]
    out = _gpu_advance(torch_mod, four, ctrls, 3, FLOOR, batch=130, rows=[0, 63, 64, 129], filler=(F06[5], _ctrls(1, seed=9)[0]))
    for i, one in enumerate(alone):
        for x, y in zip(out, one):
            assert np.array_equal(x[i], y[0]), i


def test_protocol(torch_mod):
    """The keyword and the flag sets that create a floor handle, the ones that are refused with a text naming the bit, the calls the
    handle refuses, and the zeros of a fresh handle."""
    import ctypes as C

    from flybody_amd import _capi
    from flybody_amd.batched_env import FFE_WALK_FLOOR, BatchedWalkPhysics

    torch = torch_mod
    L = _capi.lib()
    assert FFE_WALK_FLOOR == WALK_FLOOR
    env = BatchedWalkPhysics(batch_size=4, floor_contacts=True)
    assert env.physics_flags == FLOOR
    other = BatchedWalkPhysics(batch_size=1, floor_contacts=True, physics_flags=NO_FLUID | NO_NOSLIP | NO_ADHESION)
    assert other.physics_flags == FLOOR | NO_FLUID | NO_NOSLIP | NO_ADHESION
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
    for bad in (FLOOR | WALK_EPISODES, FLOOR | NO_LIMIT, NO_CONTACT | WALK_FLOOR, WALK_FLOOR, WALK_JOINT_LIMITS | WALK_FLOOR,
                NO_CONTACT | NO_LIMIT | WALK_FLOOR):
        with pytest.raises(RuntimeError, match="FFE_WALK_FLOOR"):
            BatchedWalkPhysics(batch_size=1, physics_flags=bad)
    # without the bit: today's texts
    with pytest.raises(RuntimeError, match="floor contacts and joint limits are not built yet: physics_flags must contain FFE_NO_CONTACT \\| FFE_NO_LIMIT"):
        BatchedWalkPhysics(batch_size=1, physics_flags=0)
    with pytest.raises(RuntimeError, match="floor contacts and joint limits are not built.*FFE_WALK_JOINT_LIMITS"):
        BatchedWalkPhysics(batch_size=1, physics_flags=WALK_JOINT_LIMITS)
