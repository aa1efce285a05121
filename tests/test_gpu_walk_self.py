"""GPU parity tests of the walking fly's own contacts (csrc/walk_self_env.hip `floor_self_step`, through
`BatchedWalkPhysics(floor_contacts=True, self_contacts=True)` and the C ABI) against the float64 oracle on identical inputs (DESIGN.md
section 12 step 3c).  Run with `-m gpu` on an MI355X.  One wavefront is one env; no batch here exceeds 130.

Both sides run on the SHIPPED blob: the oracle collides the floor pairs and the fly's own pairs, as the device does with FFE_WALK_SELF.
State sets R10 / XL / XS of tests/walk_self_sets.py.  A state is left out of a comparison only when the oracle's `contact_hist` reports
a candidate pair within 2e-6 cm of a switching distance during the substeps compared, at most 3 per set.

Bounds per error group (the groups of tests/test_gpu_walk_limits.py): min(3 x the worst value measured on the MI355X against the oracle,
CAP1 / CAP10 of that file).  The reference is always the oracle."""
import numpy as np
import pytest

import walk_self_sets as S
from test_gpu_walk_floor import CAP1, CAP10, LADDER, _assert_bounds, _ctrls, _errors, _gpu_advance, _kept
from walk_self_sets import FLOOR, NO_FLUID, SELF, WALK_SELF

pytestmark = pytest.mark.gpu
NO_GRAVITY, WALK_EPISODES, NO_LIMIT, NO_CONTACT, WALK_JOINT_LIMITS, WALK_FLOOR = 16, 1024, 2, 64, 512, 2048
# Worst one-substep errors per set over the three flag sets of LADDER, measured on the MI355X against the oracle (relative to
# max(1, max |ref| of the group) on the velocity groups); no state of the three sets is left out (2e-6 cm band).  The contact counts
# (int 5: 4 ... 7 on R10, 1 ... 2 on XL, 5 ... 13 on XS; int 3: 0 ... 3, 1 ... 2, 1 ... 5) equal the oracle's on every state; the solver took
# at most 8 iterations.
#   R10  hinge_qpos 1.039e-7, root_pos 8.767e-10, root_quat 7.443e-8, act 4.047e-8, root_lin 4.395e-6, root_ang 7.297e-5 (no_noslip;
#        1.201e-5 all, 1.212e-5 no_fluid_no_adhesion), hinge_vel 1.365e-5
#   XL   hinge_qpos 9.653e-8, root_pos 4.076e-11, root_quat 2.343e-8, act 2.643e-8, root_lin 2.077e-7, root_ang 6.789e-6, hinge_vel 4.707e-6
#   XS   hinge_qpos 8.700e-8, root_pos 5.738e-9, root_quat 3.977e-8, act 2.775e-8, root_lin 1.241e-5, root_ang 5.696e-5, hinge_vel 9.445e-6
# No kind on XS needs more than CAP1: the 3e-4 ceiling of the tethered kernel's fly-fly test is not used.
# (With the noslip revert test of `ConeRows` instead of `ConeRowsResidual`, csrc/row_newton.hpp, R10 state 8 gave root_ang 7.245e-4 under
# FFE_NO_FLUID | FFE_NO_ADHESION and XS state 3 gave 1.858e-4 under the full set: the third sweep reverted or not by rounding.)
ONE_MEASURED = {
    "R10": {"hinge_qpos": 1.04e-7, "root_pos": 8.8e-10, "root_quat": 7.5e-8, "act": 4.1e-8, "root_lin": 4.4e-6, "root_ang": 7.3e-5, "hinge_vel": 1.37e-5},
    "XL": {"hinge_qpos": 9.7e-8, "root_pos": 4.1e-11, "root_quat": 2.4e-8, "act": 2.7e-8, "root_lin": 2.1e-7, "root_ang": 6.8e-6, "hinge_vel": 4.8e-6},
    "XS": {"hinge_qpos": 8.7e-8, "root_pos": 5.8e-9, "root_quat": 4.0e-8, "act": 2.8e-8, "root_lin": 1.25e-5, "root_ang": 5.7e-5, "hinge_vel": 9.5e-6},
}
# Ten substeps open loop on R10, measured the same way (1 of 24 states left out): hinge_qpos 3.428e-7, root_pos 8.391e-9, root_quat
# 6.659e-8, act 8.867e-8, root_lin 7.770e-6, root_ang 1.611e-5, hinge_vel 1.078e-5.
TEN_MEASURED = {"hinge_qpos": 3.5e-7, "root_pos": 8.4e-9, "root_quat": 6.7e-8, "act": 8.9e-8, "root_lin": 7.8e-6, "root_ang": 1.62e-5, "hinge_vel": 1.08e-5}


@pytest.fixture(scope="module")
def torch_mod():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def _set(which):
    return {"R10": S.r10, "XL": S.x_lifted, "XS": S.x_standing}[which]()


def _advance(torch, states, ctrls, nsteps, flags, **kw):
    return _gpu_advance(torch, states, ctrls, nsteps, flags, blob=S.WALK_BLOB, **kw)


@pytest.mark.parametrize("which", ["R10", "XL", "XS"])
@pytest.mark.parametrize("extra,name", LADDER)
def test_one_substep_teacher_forced(torch_mod, which, extra, name):
    """One substep from every state of the set; task-state int 5 is the oracle's `ncon_matter` and int 3 the fly-fly contacts among
    them on every kept state; no overflow bit."""
    m, states = S.model(), _set(which)
    ctrls = _ctrls(len(states))
    trace, ref = [], []
    for s, c in zip(states, ctrls):
        tr = []
        ref.append(S.oracle_advance(m, s, c.astype(np.float64), 1, extra, trace=tr))
        trace.append(tr[0])
    ncon, nself, nefc = [t[0] for t in trace], [t[1] for t in trace], [t[2] for t in trace]
    assert max(ncon) <= 14 and max(nefc) <= 40 and max(nself) >= 2, (ncon, nself, nefc)
    if which == "XL":
        assert ncon == nself  # lifted: the fly-fly rows are alone
    q, v, a, ints, reals, info = _advance(torch_mod, states, ctrls, 1, SELF | extra)
    assert np.isfinite(q).all() and np.isfinite(v).all()
    keep = _kept(ref, f"{which} {name}")
    e = _errors(q, v, a, ref, keep)
    print(f"one substep [{which} {name}]: " + " ".join(f"{k} {x:.3e}" for k, x in e.items()) + f" solver iterations max {ints[:, 6].max()} "
          f"contacts {ints[:, 5].tolist()} fly-fly {ints[:, 3].tolist()} limit rows {ints[:, 4].tolist()}")
    assert ints[keep, 5].tolist() == [ncon[i] for i in keep], (ints[:, 5].tolist(), ncon)
    assert ints[keep, 3].tolist() == [nself[i] for i in keep], (ints[:, 3].tolist(), nself)
    assert not ints[:, 7].any() and not info.any() and not ints[:, [0, 1, 2]].any()
    _assert_bounds(e, ONE_MEASURED[which], CAP1, f"{which} {name}")


def test_ten_substeps_open_loop(torch_mod):
    m, R10 = S.model(), S.r10()
    ctrls = _ctrls(len(R10), seed=3)
    ref = [S.oracle_advance(m, s, c.astype(np.float64), 10, 0) for s, c in zip(R10, ctrls)]
    q, v, a, ints, reals, info = _advance(torch_mod, R10, ctrls, 10, SELF)
    keep = _kept(ref, "ten substeps R10")
    e = _errors(q, v, a, ref, keep)
    print("ten substeps R10: " + " ".join(f"{k} {x:.3e}" for k, x in e.items()))
    assert not info.any()
    _assert_bounds(e, TEN_MEASURED, CAP10, "ten")


def test_without_the_bit_the_contacts_are_missed(torch_mod):
    """R10 on a plain floor handle (FFE_WALK_FLOOR without the bit): the hinge velocities differ from the oracle's by far more than the
    bound, so the comparisons above see the fly's own contacts."""
    m, R10 = S.model(), S.r10()
    ctrls = _ctrls(len(R10))
    ref = [S.oracle_advance(m, s, c.astype(np.float64), 1, 0) for s, c in zip(R10, ctrls)]
    q, v, a, ints, reals, info = _advance(torch_mod, R10, ctrls, 1, FLOOR)
    e = _errors(q, v, a, ref, _kept(ref, "plain floor handle"))
    print("plain floor handle against the oracle with the fly's own contacts: " + " ".join(f"{k} {x:.3e}" for k, x in e.items()))
    assert e["hinge_vel"] > 20 * CAP1["hinge_vel"] and not ints[:, 3].any()


def test_internal_forces_do_not_push_the_root(torch_mod):
    """XL at rest with gravity and the fluid off: every force left is internal (actuators, springs, dampers, limits, fly-fly contacts),
    so the total linear momentum p stays zero.  After one substep it is compared with sqrt(2 T m) >= |p| (T the kinetic energy, m the
    total mass; the oracle evaluates both from the device's state).  The contact forces cancel on the root whatever the solver returns
    (their rows have no root entry), so what is left is the float32 rounding of the root rows of the arrowhead solve: the condition
    number of S_m is at most 850 on walking states, 850 x 2^-24 = 5.1e-5 per solve through it, and a substep
    goes through the Y solves, the Schur complement, its factor and the back substitution: the bound is four times that, 2e-4.  A
    contact force of 1 dyn that did push the root would leave 2e-4 g cm/s, a tenth or more of sqrt(2 T m) here."""
    from flybody_amd.model.blob import read_blob
    from oracle import oracle as O

    m, XL = S.model(), S.x_lifted()
    states = [(s[0], np.zeros(108), np.zeros(59)) for s in XL]
    zero = [np.zeros(59, dtype=np.float32)] * len(states)
    q, v, a, ints, reals, info = _advance(torch_mod, states, zero, 1, SELF | NO_GRAVITY | NO_FLUID)
    mass = float(np.asarray(read_blob(S.WALK_BLOB)["body_mass"]).sum())
    d = O.OracleData(m)
    worst = 0.0
    for i in range(len(states)):
        d.qpos[:], d.qvel[:], d.act[:] = q[i], v[i], a[i]
        d.ctrl[:] = 0
        d.forward()
        lin, _ = d.momentum()
        scale = float(np.sqrt(2.0 * d.energy()[1] * mass))
        print(f"momentum state {i} ({XL[i][4]}): |p| {np.abs(lin).max():.3e} sqrt(2 T m) {scale:.3e} fly-fly contacts {ints[i, 3]} max |qvel| {np.abs(v[i]).max():.3e}")
        assert scale > 0 and np.abs(v[i, 6:]).max() > 1e-3
        worst = max(worst, float(np.abs(lin).max()) / scale)
    assert (ints[:, 3] >= 1).all() and ints[:, 5].tolist() == ints[:, 3].tolist()
    print(f"momentum: worst |p| / sqrt(2 T m) {worst:.3e}")
    assert worst <= 2e-4, worst


def test_overflow_stays_finite(torch_mod):
    """qpos0 with the root at z = 0.05 cm (the oracle has more than 77 contacts there): the floor's contacts fill the 16 slots, the env
    is flagged with bit value 1 and one control step stays finite; R10's envs in the same batch are not flagged."""
    from flybody_amd.model.blob import read_blob

    R10 = S.r10()
    q0 = np.asarray(read_blob(S.WALK_BLOB)["qpos0"], dtype=np.float64).ravel().copy()
    q0[2] = 0.05
    low = (q0, np.zeros(108), np.zeros(59))
    states = [low] * 2 + R10[:4]
    zero = [np.zeros(59, dtype=np.float32)] * len(states)
    q, v, a, ints, reals, info = _advance(torch_mod, states, zero, 1, SELF)
    print(f"overflow, first substep: contacts {ints[:, 5].tolist()} fly-fly {ints[:, 3].tolist()} validity {info[:, 0].tolist()}")
    assert (ints[:2, 5] == 16).all() and (info[:2, 0] & 1).all() and np.isfinite(v).all()
    q, v, a, ints, reals, info = _advance(torch_mod, states, zero, 10, SELF)
    assert np.isfinite(q).all() and np.isfinite(v).all() and np.isfinite(a).all() and np.isfinite(reals).all()
    assert np.abs(v).max() < 1e6
    assert (info[:2, 0] & 1).all() and (ints[:2, 7] & 1).all()
    assert not info[2:, 0].any() and not ints[2:, 7].any() and not info[:, 1:].any()


def test_a_launch_depends_on_its_state_alone(torch_mod):
    """State B after the handle has run state A gives the bits of B on a fresh handle: nothing is kept from launch to launch."""
    import torch

    from flybody_amd.batched_env import BatchedWalkPhysics

    XS, R10 = S.x_standing(), S.r10()
    A, B = XS[:6], R10[:6]
    ctrl = _ctrls(6, seed=12)
    fresh = _advance(torch_mod, B, ctrl, 10, SELF)
    env = BatchedWalkPhysics(batch_size=6, floor_contacts=True, self_contacts=True)
    t = lambda rows, k, dt=torch.float64: torch.tensor(np.stack([r[k] for r in rows]), dtype=dt, device="cuda")
    c = torch.tensor(np.stack(ctrl), dtype=torch.float32, device="cuda")
    for st in (A, B):
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
    XS, R10 = S.x_standing(), S.r10()
    four, ctrls = [XS[1], XS[4], R10[11], XS[10]], _ctrls(4, seed=8)
    alone = [_advance(torch_mod, [s], [c], 3, SELF) for s, c in zip(four, ctrls)]
    out = _advance(torch_mod, four, ctrls, 3, SELF, batch=130, rows=[0, 63, 64, 129], filler=(R10[5], _ctrls(1, seed=9)[0]))
    for i, one in enumerate(alone):
        for x, y in zip(out, one):
            assert np.array_equal(x[i], y[0]), i


def test_protocol(torch_mod):
    """The keywords and the flag set that create the handle, the sets refused with a text naming the bit, the calls the handle refuses,
    and the zeros of a fresh handle."""
    from flybody_amd import _capi
    from flybody_amd.batched_env import FFE_WALK_SELF, BatchedWalkPhysics

    torch = torch_mod
    L = _capi.lib()
    assert FFE_WALK_SELF == WALK_SELF == 4096
    with pytest.raises(ValueError, match="floor_contacts"):
        BatchedWalkPhysics(batch_size=1, self_contacts=True)
    env = BatchedWalkPhysics(batch_size=4, floor_contacts=True, self_contacts=True)
    assert env.physics_flags == SELF
    other = BatchedWalkPhysics(batch_size=1, floor_contacts=True, self_contacts=True, physics_flags=NO_FLUID | 128 | 256, blob_path=S.WALK_BLOB)
    assert other.physics_flags == SELF | NO_FLUID | 128 | 256
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
    for bad in (SELF | WALK_EPISODES, SELF | NO_LIMIT, WALK_SELF, NO_CONTACT | WALK_SELF, NO_CONTACT | WALK_JOINT_LIMITS | WALK_SELF,
                WALK_JOINT_LIMITS | WALK_FLOOR | WALK_SELF, NO_CONTACT | NO_LIMIT | WALK_SELF, NO_CONTACT | WALK_JOINT_LIMITS | WALK_EPISODES | WALK_SELF):
        with pytest.raises(RuntimeError, match="FFE_WALK_SELF"):
            BatchedWalkPhysics(batch_size=1, physics_flags=bad)
    with pytest.raises(RuntimeError, match="FFE_WALK_SELF.*does not carry"):
        BatchedWalkPhysics(batch_size=1, physics_flags=SELF | WALK_EPISODES)
    # without the new bit the pinned refusal stays
    with pytest.raises(RuntimeError, match="FFE_WALK_FLOOR"):
        BatchedWalkPhysics(batch_size=1, physics_flags=WALK_JOINT_LIMITS | WALK_FLOOR)
