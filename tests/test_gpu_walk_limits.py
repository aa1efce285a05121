"""GPU parity tests of the joint-limit rows of the free-root walking-fly physics (csrc/walk_env.hip, `walk_limits_kernel`, through
`BatchedWalkPhysics(joint_limits=True)` and the C ABI) against the float64 oracle on identical inputs.
Run with `-m gpu` on an MI355X.  One wavefront is one env, so no batch here exceeds 130.  The oracle runs with FFE_NO_CONTACT (and the
force switches of the case); FFE_WALK_JOINT_LIMITS is never passed to it.

State sets: tests/walk_limit_sets.py (A: 24 rollout states, 15 of them with one or two limits instantiated; C: A with 1 ... 32 hinges
pushed 1e-3 ... 0.05 rad out of range).  No state is excluded from any comparison.

Bounds: CAP1 / CAP10 of tests/test_gpu_walk_physics.py per error group; for the three velocity groups of the one-substep test and for the
recoil test 3x the worst value measured on the MI355X (the *_MEASURED constants below), never more than the cap."""
import numpy as np
import pytest

import walk_limit_sets as S
from walk_limit_sets import NO_ACTUATION, NO_CONTACT, NO_DAMPER, NO_FLUID, NO_GRAVITY, NO_LIMIT, NO_SPRING, WALK_JOINT_LIMITS

pytestmark = pytest.mark.gpu
LIM = NO_CONTACT | WALK_JOINT_LIMITS
PLAIN = NO_CONTACT | NO_LIMIT
ONLY_LIMITS = NO_FLUID | NO_GRAVITY | NO_ACTUATION | NO_SPRING | NO_DAMPER
# caps: tests/test_gpu_walk_physics.py (tests/test_gpu_ball.py's "smooth" / "limits" rungs and its ten-substep bounds)
CAP1 = {"hinge_qpos": 2e-6, "root_pos": 2e-6, "root_quat": 2e-6, "act": 1e-6, "root_lin": 1.5e-4, "root_ang": 1.5e-4, "hinge_vel": 1.5e-4}
CAP10 = {"hinge_qpos": 2e-5, "root_pos": 2e-5, "root_quat": 2e-5, "act": 1e-6, "root_lin": 1e-2, "root_ang": 1e-2, "hinge_vel": 1e-2}
# Worst one-substep errors over sets A + C and the three flag sets, measured on the MI355X against the oracle (relative to
# max(1, max |ref| of the group)): root_lin 7.598e-7 (limits), root_ang 1.042e-5 (no_fluid), hinge_vel 8.516e-6 (limits); the other
# groups: hinge_qpos 2.152e-7, root_pos 1.523e-10, root_quat 8.441e-8, act 2.700e-8.  The solver took at most 2 iterations with the
# smooth forces on; with every force off its stopping scale is ~0 and it runs to rounding (20).  The test asserts 3x the three
# velocity groups, never above CAP1.
MEASURED1 = {"root_lin": 7.6e-7, "root_ang": 1.05e-5, "hinge_vel": 8.6e-6}
# Recoil from rest (set C, 5 substeps, only the limits act): worst error of the root's linear / angular velocity relative to that
# group's own max |ref| (a kernel without the rank-6 root term of G reads 1.0): measured 2.354e-6 and 1.553e-5.  Asserted at 3x, never
# above 1e-2.
RECOIL_LIN_MEASURED, RECOIL_ANG_MEASURED = 2.4e-6, 1.56e-5
# Ten substeps, measured (worst of A and C): hinge_qpos 6.2e-7, root_pos 2.7e-9, root_quat 8.4e-8, act 8.2e-8, root_lin 2.1e-6,
# root_ang 3.4e-5, hinge_vel 2.9e-5 - all far inside CAP10.

@pytest.fixture(scope="module")
def torch_mod():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def _ctrls(n, seed=11):
    rs = np.random.RandomState(seed)
    return [rs.uniform(-0.5, 0.5, 59).astype(np.float32) for _ in range(n)]


def _gpu_advance(torch, states, ctrls, nsteps, flags, batch=None, rows=None, filler=None):
    """Advances `states` on the device (tests/test_gpu_walk_physics.py::_gpu_advance, copied); also returns the task-state ints and the
    validity rows read after the call."""
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
    env = BatchedWalkPhysics(batch_size=batch, physics_flags=flags)
    qpos = torch.tensor(np.stack([states[k][0] for k in pick]), dtype=torch.float64, device="cuda")
    qvel = torch.tensor(np.stack([states[k][1] for k in pick]), dtype=torch.float64, device="cuda")
    act = torch.tensor(np.stack([states[k][2] for k in pick]), dtype=torch.float64, device="cuda")
    env.set_state(qpos, qvel)
    env.set_act(act)
    env.physics_step(torch.tensor(np.stack([ctrls[k] for k in pick]), dtype=torch.float32, device="cuda"), nsteps)
    q, v = env.get_state()
    a = env.get_act()
    ints, reals = env.get_task_state()
    info = torch.full((batch, 4), -1, dtype=torch.int32, device="cuda")
    assert _capi.lib().ffe_get_validity(env._h, info.data_ptr(), env._stream()) == 0
    torch.cuda.synchronize()
    assert not reals.cpu().numpy().any()
    out = q.cpu().numpy()[rows], v.cpu().numpy()[rows], a.cpu().numpy()[rows], ints.cpu().numpy()[rows], info.cpu().numpy()[rows]
    env.close()
    return out


def _errors(q, v, a, ref):
    """Worst error per group over the states (tests/test_gpu_walk_physics.py::_errors, copied).  Velocity groups: max |err| /
    max(1, max |ref| of that group), each group on its own."""
    e = {k: 0.0 for k in CAP1}

    def rel(x, r):
        return float(np.abs(x - r).max() / max(1.0, np.abs(r).max()))

    for i, (rq, rv, ra) in enumerate(ref):
        e["hinge_qpos"] = max(e["hinge_qpos"], float(np.abs(q[i, 7:] - rq[7:]).max()))
        e["root_pos"] = max(e["root_pos"], float(np.abs(q[i, :3] - rq[:3]).max()))
        sgn = 1.0 if np.dot(q[i, 3:7], rq[3:7]) >= 0 else -1.0
        e["root_quat"] = max(e["root_quat"], float(np.abs(sgn * q[i, 3:7] - rq[3:7]).max()))
        e["act"] = max(e["act"], float(np.abs(a[i] - ra).max()))
        e["root_lin"] = max(e["root_lin"], rel(v[i, :3], rv[:3]))
        e["root_ang"] = max(e["root_ang"], rel(v[i, 3:6], rv[3:6]))
        e["hinge_vel"] = max(e["hinge_vel"], rel(v[i, 6:], rv[6:]))
    return e


LADDER = [(0, "limits"), (NO_FLUID, "no_fluid"), (ONLY_LIMITS, "only_limits")]


@pytest.mark.parametrize("extra,name", LADDER)
def test_one_substep_teacher_forced(torch_mod, extra, name):
    """One substep from sets A + C.  Task-state int 4 is the oracle's nefc on every state and int 7 is 0."""
    m, A, C = S.sets()
    states = A + C
    ctrls = _ctrls(len(states))
    nefc, ref = [], []
    for s, c in zip(states, ctrls):
        tr = []
        ref.append(S.oracle_advance(m, s, c.astype(np.float64), 1, NO_CONTACT | extra, trace=tr))
        nefc.append(tr[0])
    assert nefc[24:] == S.C_COUNTS and sum(1 for n in nefc[:24] if n > 0) >= 12 and max(nefc[:24]) <= 2
    q, v, a, ints, info = _gpu_advance(torch_mod, states, ctrls, 1, LIM | extra)
    assert np.isfinite(q).all() and np.isfinite(v).all()
    e = _errors(q, v, a, ref)
    print(f"one substep [{name}] A + C: " + " ".join(f"{k} {x:.3e}" for k, x in e.items()) + f" solver iterations max {ints[:, 6].max()}")
    assert ints[:, 4].tolist() == nefc, (ints[:, 4].tolist(), nefc)
    assert not ints[:, 7].any() and not info.any() and not ints[:, [0, 1, 2, 3, 5]].any()
    for k in CAP1:
        assert e[k] < CAP1[k], (name, k, e[k])
    assert MEASURED1 is not None, "the measured one-substep errors have not been recorded"
    for k in ("root_lin", "root_ang", "hinge_vel"):
        assert 3 * MEASURED1[k] <= CAP1[k]
        assert e[k] <= 3 * MEASURED1[k], (name, k, e[k])


def test_recoil_from_rest(torch_mod):
    """Set C's poses at rest, every force but the limits off, 5 substeps: a limit force on a hinge makes the free thorax recoil, and
    the only path from the one to the other is the rank-6 root term of G (and M_rj in the Euler solve).  The root's velocities are
    compared relative to their own size (the oracle: 2.7e-5 ... 0.109 cm/s and 0.0024 ... 4.4 rad/s; the hinges 4.8 ... 19 rad/s)."""
    m, _, C = S.sets()
    states = [(q, np.zeros_like(v), np.zeros_like(a)) for q, v, a in C]
    zero = [np.zeros(59, dtype=np.float32)] * len(states)
    ref = [S.oracle_advance(m, s, np.zeros(59), 5, NO_CONTACT | ONLY_LIMITS) for s in states]
    q, v, a, ints, info = _gpu_advance(torch_mod, states, zero, 5, LIM | ONLY_LIMITS)
    lin = max(float(np.abs(v[i, :3] - r[1][:3]).max() / np.abs(r[1][:3]).max()) for i, r in enumerate(ref))
    ang = max(float(np.abs(v[i, 3:6] - r[1][3:6]).max() / np.abs(r[1][3:6]).max()) for i, r in enumerate(ref))
    rl, ra = [float(np.abs(r[1][:3]).max()) for r in ref], [float(np.abs(r[1][3:6]).max()) for r in ref]
    hv = [float(np.abs(v[i, 6:]).max()) for i in range(len(states))]
    print(f"recoil: root_lin {lin:.3e} root_ang {ang:.3e} (own scale); oracle root |v| {min(rl):.3g} ... {max(rl):.3g} cm/s, |w| {min(ra):.3g} ... "
          f"{max(ra):.3g} rad/s; fastest hinge per state {min(hv):.3g} ... {max(hv):.3g} rad/s")
    assert min(rl) > 1e-5 and min(ra) > 1e-3  # the oracle's root does recoil on every state
    # at rest and out of range every row is active (aref > 0 = J a_s), so every state must move a hinge
    assert min(hv) > 1.0 and min(float(np.abs(r[1][6:]).max()) for r in ref) > 1.0
    assert lin < 1e-2 and ang < 1e-2, (lin, ang)
    assert RECOIL_LIN_MEASURED is not None and RECOIL_ANG_MEASURED is not None, "the measured recoil errors have not been recorded"
    assert 3 * RECOIL_LIN_MEASURED <= 1e-2 and 3 * RECOIL_ANG_MEASURED <= 1e-2
    assert lin <= 3 * RECOIL_LIN_MEASURED and ang <= 3 * RECOIL_ANG_MEASURED, (lin, ang)


def test_ten_substeps_open_loop(torch_mod):
    m, A, C = S.sets()
    states = A + C
    ctrls = _ctrls(len(states), seed=3)
    ref = [S.oracle_advance(m, s, c.astype(np.float64), 10, NO_CONTACT) for s, c in zip(states, ctrls)]
    q, v, a, ints, info = _gpu_advance(torch_mod, states, ctrls, 10, LIM)
    eA, eC = _errors(q[:24], v[:24], a[:24], ref[:24]), _errors(q[24:], v[24:], a[24:], ref[24:])
    print("ten substeps set A: " + " ".join(f"{k} {x:.3e}" for k, x in eA.items()))
    print("ten substeps set C: " + " ".join(f"{k} {x:.3e}" for k, x in eC.items()))
    assert not info.any()
    for k in CAP10:
        assert max(eA[k], eC[k]) < CAP10[k], (k, eA[k], eC[k])


def test_no_limit_no_difference(torch_mod):
    """Set A clamped 1e-3 rad inside every range, 3 substeps: on the states that stay free of limit rows (the oracle reports nefc == 0
    at every substep) the limits kernel and the plain kernel give the same bits."""
    m, A, _ = S.sets()
    states = [(S.clamp_inside(q), v, a) for q, v, a in A]
    ctrls = _ctrls(len(states), seed=5)
    free = []
    for i, (s, c) in enumerate(zip(states, ctrls)):
        tr = []
        S.oracle_advance(m, s, c.astype(np.float64), 3, NO_CONTACT, trace=tr)
        if not any(tr):
            free.append(i)
    print(f"no limit, no difference: {len(free)} of {len(states)} states stay free of rows")
    assert len(free) >= 12
    ql, vl, al, ints, _ = _gpu_advance(torch_mod, states, ctrls, 3, LIM)
    qp, vp, ap, pints, pinfo = _gpu_advance(torch_mod, states, ctrls, 3, PLAIN)
    assert not pints.any() and not pinfo.any()  # a plain handle keeps reporting zeros
    assert not ints[free, 4].any()
    assert np.array_equal(ql[free], qp[free]) and np.array_equal(vl[free], vp[free]) and np.array_equal(al[free], ap[free])


def test_overflow_is_flagged_and_stays_finite(torch_mod):
    """70 hinges out of range are more rows than the kernel carries (48): the rows that do not fit are dropped for the substep, the env
    is flagged with bit value 2 and one control step stays finite.  Set A's envs in the same batch are not flagged."""
    _, A, _ = S.sets()
    over = S.pushed(A[:6], [70] * 6, 9)
    states = over + A[:6]
    q, v, a, ints, info = _gpu_advance(torch_mod, states, _ctrls(len(states), seed=6), 10, LIM)
    print(f"overflow: max |qvel| {np.abs(v[:6]).max():.3e}, rows of the last substep {ints[:6, 4].tolist()}, validity {info[:, 0].tolist()}")
    assert np.isfinite(q).all() and np.isfinite(v).all() and np.isfinite(a).all()
    assert np.abs(v).max() < 1e6
    assert (info[:6, 0] & 2).all() and (ints[:6, 7] & 2).all()
    assert not info[6:, 0].any() and not ints[6:, 7].any() and not info[:, 1:].any()


def test_rows_do_not_depend_on_their_batch(torch_mod):
    """Four of set C's states alone (B = 1 each) and at rows 0, 63, 64 and 129 of a batch of 130 whose other rows hold another state."""
    _, A, C = S.sets()
    four, ctrls = [C[3], C[8], C[11], C[22]], _ctrls(4, seed=8)
    alone = [_gpu_advance(torch_mod, [s], [c], 3, LIM) for s, c in zip(four, ctrls)]
    q, v, a, ints, _ = _gpu_advance(torch_mod, four, ctrls, 3, LIM, batch=130, rows=[0, 63, 64, 129], filler=(A[5], _ctrls(1, seed=9)[0]))
    for i, (q1, v1, a1, i1, _) in enumerate(alone):
        assert np.array_equal(q[i], q1[0]) and np.array_equal(v[i], v1[0]) and np.array_equal(a[i], a1[0]) and np.array_equal(ints[i], i1[0]), i


def test_protocol(torch_mod):
    """The keyword and the flag sets that create a handle, the ones that are refused, the calls a limits handle refuses, and the zeros
    of a fresh handle."""
    import ctypes as C

    from flybody_amd import _capi
    from flybody_amd.batched_env import FFE_WALK_JOINT_LIMITS, BatchedWalkPhysics

    torch = torch_mod
    L = _capi.lib()
    assert FFE_WALK_JOINT_LIMITS == WALK_JOINT_LIMITS
    env = BatchedWalkPhysics(batch_size=4, joint_limits=True)
    assert env.physics_flags == LIM
    other = BatchedWalkPhysics(batch_size=1, joint_limits=True, physics_flags=NO_FLUID | NO_GRAVITY)
    assert other.physics_flags == LIM | NO_FLUID | NO_GRAVITY
    other.close()
    ints, reals = env.get_task_state()
    info = torch.ones(4, 4, dtype=torch.int32, device="cuda")
    assert L.ffe_get_validity(env._h, info.data_ptr(), env._stream()) == 0
    torch.cuda.synchronize()
    assert not ints.cpu().numpy().any() and not reals.cpu().numpy().any() and not info.cpu().numpy().any()
    z = torch.zeros(4, 59, dtype=torch.float32, device="cuda")
    obs, rew, st = torch.zeros(4, 8, device="cuda"), torch.zeros(4, device="cuda"), torch.zeros(4, dtype=torch.int32, device="cuda")
    ms = C.c_float()
    p = lambda x: x.data_ptr()
    calls = {
        "ffe_reset": lambda: L.ffe_reset(env._h, p(obs), p(rew), p(rew), p(st), env._stream()),
        "ffe_step": lambda: L.ffe_step(env._h, p(z), p(obs), p(rew), p(rew), p(st), env._stream()),
        "ffe_time_kernel": lambda: L.ffe_time_kernel(env._h, p(z), p(obs), p(rew), p(rew), p(st), 1, env._stream(), C.byref(ms)),
    }
    for name, call in calls.items():
        assert call() < 0, name
        assert b"not available on a walk physics handle" in L.ffe_last_error(env._h), name
    env.physics_step(z, 1)  # still usable
    torch.cuda.synchronize()
    assert np.isfinite(env.get_state()[0].cpu().numpy()).all()
    env.close()
    for bad in (NO_CONTACT | NO_LIMIT | WALK_JOINT_LIMITS, WALK_JOINT_LIMITS, WALK_JOINT_LIMITS | NO_LIMIT):
        with pytest.raises(RuntimeError, match="floor contacts and joint limits are not built.*FFE_WALK_JOINT_LIMITS"):
            BatchedWalkPhysics(batch_size=1, physics_flags=bad)
