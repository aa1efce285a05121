"""The error contract of the env-handle C ABI (include/flybody_env.h, "Return codes"), pinned call by call on one handle of each kind:
flight, walk_on_ball and free-root walk physics at batch 2.  Every bad call here is rejected on the host - nothing is launched with a bad
pointer - and each handle still works afterwards.  The `ffe_spec` values are literals recorded before the boundary moved into
csrc/capi.hip, and so are all codes and texts but those of the refusals that had no text before the move (a NULL argument, act get / set
on a flight handle): these got one with it.  Run with `-m gpu` on an MI355X."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_parity import torch_mod  # noqa: F401

pytestmark = pytest.mark.gpu

B = 2
H32_FLIGHT, H32_LEGS = 4.999999873689376e-05, 0.00019999999494757503  # float32(5e-5), float32(2e-4): the models' timesteps
WALK_REFUSAL = b"not available on a walk physics handle"

# ffe_spec: batch nq nv nu action_dim obs_dim nsub | physics_timestep control_timestep | off_accelerometer off_gyro off_joints_pos
# off_joints_vel off_velocimeter off_world_zaxis off_ref_displacement off_ref_root_quat n_obs_joints n_ref
SPEC = {
    "flight": (2, 43, 42, 11, 12, 104, 4, H32_FLIGHT, 0.0002, 0, 3, 6, 31, 56, 59, 62, 80, 25, 6),
    "ball": (2, 106, 105, 59, 59, 289, 10, H32_LEGS, 0.002, 0, 104, 107, 192, 283, 286, -1, -1, 85, 0),
    "walk": (2, 109, 108, 59, 59, 0, 10, H32_LEGS, 0.0019999999494757503, -1, -1, -1, -1, -1, -1, -1, -1, 0, 0),
}


def _make(kind, wb_tables, ref_traj, **kw):
    from flybody_amd.batched_env import BatchedBallEnv, BatchedFlyEnv, BatchedWalkPhysics

    if kind == "flight":
        return BatchedFlyEnv(wb_tables, *ref_traj, batch_size=B, seed=7, **kw)
    return BatchedBallEnv(batch_size=B, **kw) if kind == "ball" else BatchedWalkPhysics(batch_size=B, **kw)


class _Calls:
    """The raw entry points on one handle, with scratch device buffers of the handle's own shapes."""

    def __init__(self, torch, env):
        from flybody_amd import _capi

        self.L, self.env, self.h = _capi.lib(), env, env._h
        s = env.spec
        z = lambda *shape, dtype=torch.float32: torch.zeros(*shape, dtype=dtype, device="cuda")
        self.act, self.obs, self.rew, self.disc = z(B, s.action_dim), z(B, max(s.obs_dim, 1)), z(B), z(B)
        self.st, self.mask = z(B, dtype=torch.int32), torch.ones(B, dtype=torch.uint8, device="cuda")
        self.info = z(B + 1, 4, dtype=torch.int32)
        self.actf64 = z(B, s.nu, dtype=torch.float64)
        self.ms = C.c_float(-1.0)

    def err(self):
        return self.L.ffe_last_error(self.h)

    def step(self, act=True, obs=True):
        p = lambda t, on: t.data_ptr() if on else None
        return self.L.ffe_step(self.h, p(self.act, act), p(self.obs, obs), self.rew.data_ptr(), self.disc.data_ptr(), self.st.data_ptr(), self.env._stream())

    def reset(self):
        return self.L.ffe_reset(self.h, self.obs.data_ptr(), self.rew.data_ptr(), self.disc.data_ptr(), self.st.data_ptr(), self.env._stream())

    def reset_envs(self, mask=True):
        return self.L.ffe_reset_envs(self.h, self.mask.data_ptr() if mask else None, self.obs.data_ptr(), self.rew.data_ptr(), self.disc.data_ptr(),
                                     self.st.data_ptr(), self.env._stream())

    def validity(self, offset_bytes=0):
        return self.L.ffe_get_validity(self.h, self.info.data_ptr() + offset_bytes, self.env._stream())

    def get_act(self):
        return self.L.ffe_get_act(self.h, self.actf64.data_ptr(), self.env._stream())

    def set_act(self):
        return self.L.ffe_set_act(self.h, self.actf64.data_ptr(), self.env._stream())

    def force(self, index):
        idx, ph = (C.c_int32 * B)(*([index] * B)), (C.c_double * B)()
        return self.L.ffe_force_next_episode(self.h, idx, ph, self.env._stream())

    def timed(self, name, iters):
        self.ms = C.c_float(-1.0)
        return getattr(self.L, name)(self.h, self.act.data_ptr(), self.obs.data_ptr(), self.rew.data_ptr(), self.disc.data_ptr(), self.st.data_ptr(), iters,
                                     self.env._stream(), C.byref(self.ms))


def _refused(c, rc, code, text):
    print(f"rc {rc} (expected {code}), err {c.err()!r} (expected to contain {text!r})")
    assert rc == code and text in c.err()


def _common_refusals(c):
    # a NULL argument is refused with a text of its own: the previous call's does not stay behind
    _refused(c, c.L.ffe_get_state(c.h, None, None, c.env._stream()), -1, b"ffe_get_state: null buffer")
    _refused(c, c.L.ffe_physics_step(c.h, c.act.data_ptr(), 0, c.env._stream()), -1, b"ffe_physics_step: null ctrl or nsteps < 1")
    _refused(c, c.L.ffe_time_kernel(c.h, None, None, None, None, None, 2, c.env._stream(), None), -1, b"ffe_time_kernel: null ms or iters < 1")
    _refused(c, c.reset_envs(mask=False), -1, b"null reset mask")
    _refused(c, c.validity(offset_bytes=4), -1, b"16-byte aligned")


def _spec_tuple(env):
    from flybody_amd import _capi

    s = _capi.Spec()
    assert _capi.lib().ffe_spec(env._h, C.byref(s)) == 0
    return tuple(getattr(s, n) for n, _ in _capi.Spec._fields_)


def _destroy_then_create_again(kind, env, wb_tables, ref_traj):
    assert env._L.ffe_destroy(env._h) == 0
    env._h = None
    again = _make(kind, wb_tables, ref_traj)
    assert _spec_tuple(again) == SPEC[kind]
    again.close()


@pytest.mark.parametrize("kind", ["flight", "ball"])
def test_env_handle_contract(torch_mod, wb_tables, ref_traj, kind):
    torch = torch_mod
    env = _make(kind, wb_tables, ref_traj)
    print(kind, _spec_tuple(env))
    assert _spec_tuple(env) == SPEC[kind]
    c = _Calls(torch, env)
    if kind == "flight":
        _refused(c, c.step(obs=False), -1, b"null device buffer")
        _refused(c, c.step(act=False), -1, b"null device buffer")
        _refused(c, c.get_act(), -1, b"ffe_get_act: not available on this kind of handle")
        _refused(c, c.set_act(), -1, b"ffe_set_act: not available on this kind of handle")
        _refused(c, c.force(len(ref_traj[0])), -1, b"trajectory index out of range")
    else:
        _refused(c, c.step(obs=False), -2, b"walk_on_ball: null output buffer")
        _refused(c, c.step(act=False), -2, b"null action buffer")
        _refused(c, c.force(0), -1, b"no per-episode randomness")
    _common_refusals(c)
    # still usable
    assert c.reset() == 0 and c.step() == 0
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(x).all()) for x in env.get_state()) and bool(torch.isfinite(c.obs).all())
    for name in ("ffe_time_steps", "ffe_time_kernel"):
        assert c.timed(name, 2) == 0
        print(kind, name, c.ms.value)
        assert np.isfinite(c.ms.value) and c.ms.value > 0
    _destroy_then_create_again(kind, env, wb_tables, ref_traj)


@pytest.mark.parametrize("kind", ["flight", "ball"])
def test_time_kernel_leaves_the_trajectory_alone(torch_mod, wb_tables, ref_traj, kind):
    torch = torch_mod
    ends = []
    for timed in (True, False):
        env = _make(kind, wb_tables, ref_traj)
        c = _Calls(torch, env)
        c.act.fill_(0.05)
        assert c.reset() == 0
        if timed:
            assert c.timed("ffe_time_kernel", 2) == 0
        else:
            assert c.step() == 0 and c.step() == 0
        torch.cuda.synchronize()
        ends.append([x.clone() for x in env.get_state()] + [c.obs.clone(), c.st.clone()])
        env.close()
    assert all(torch.equal(x, y) for x, y in zip(*ends))


def test_walk_physics_handle_contract(torch_mod, wb_tables, ref_traj):
    torch = torch_mod
    env = _make("walk", wb_tables, ref_traj)
    print("walk", _spec_tuple(env))
    assert _spec_tuple(env) == SPEC["walk"]
    c = _Calls(torch, env)
    for name, call in (("ffe_reset", c.reset), ("ffe_reset_envs", c.reset_envs), ("ffe_step", c.step), ("ffe_time_steps", lambda: c.timed("ffe_time_steps", 2)),
                       ("ffe_time_kernel", lambda: c.timed("ffe_time_kernel", 2)), ("ffe_force_next_episode", lambda: c.force(0))):
        print(name, end=": ")
        _refused(c, call(), -1, WALK_REFUSAL)
    _common_refusals(c)
    # task state and validity: zero-filled
    ints = torch.ones(B, 8, dtype=torch.int32, device="cuda")
    reals = torch.ones(B, 8, dtype=torch.float64, device="cuda")
    c.info.fill_(1)
    assert c.L.ffe_get_task_state(c.h, ints.data_ptr(), reals.data_ptr(), env._stream()) == 0 and c.validity() == 0
    torch.cuda.synchronize()
    assert not ints.any() and not reals.any() and not c.info[:B].any() and bool(c.info[B].all())
    assert c.get_act() == 0 and c.set_act() == 0
    # still usable
    env.physics_step(torch.zeros(B, env.spec.nu, dtype=torch.float32, device="cuda"), 1)
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(x).all()) for x in env.get_state())
    _destroy_then_create_again("walk", env, wb_tables, ref_traj)


class _CreateSpy:
    """The library with the return codes of its create functions recorded."""

    def __init__(self, L):
        self._L, self.codes = L, []

    def __getattr__(self, name):
        f = getattr(self._L, name)
        if not name.startswith("ffe_create"):
            return f

        def call(*args):
            self.codes.append(f(*args))
            return self.codes[-1]
        return call


def test_create_refusals(torch_mod, wb_tables, ref_traj, monkeypatch):
    from flybody_amd import _capi
    from flybody_amd.batched_env import BALL_BLOB, FFE_NO_CONTACT, FFE_NO_LIMIT, FLIGHT_BLOB, WALK_BLOB, BatchedFlyEnv, BatchedWalkPhysics

    L = _capi.lib()
    blobs = {k: open(p, "rb").read() for k, p in (("flight", FLIGHT_BLOB), ("ball", BALL_BLOB), ("walk", WALK_BLOB))}
    ndev = torch_mod.cuda.device_count()

    def create(kind, task, device):
        h = C.c_void_p(1)
        blob = blobs[kind]
        if kind == "flight":
            rc = L.ffe_create_flight(blob, len(blob), task, B, device, 0, 0, C.byref(h))
        elif kind == "ball":
            rc = L.ffe_create_walk_on_ball(blob, len(blob), task, B, device, C.byref(h))
        else:
            rc = L.ffe_create_walk_physics(blob, len(blob), task, B, device, C.byref(h))
        print(kind, device, rc, L.ffe_last_error(None))
        assert h.value is None  # *out is cleared on every refusal
        return rc, L.ffe_last_error(None)

    tasks = {"flight": _capi.FlightTask(), "ball": _capi.BallTask(control_timestep=2e-3, time_limit_steps=1001),
             "walk": _capi.WalkPhysicsTask(physics_flags=FFE_NO_CONTACT | FFE_NO_LIMIT)}
    names = {"flight": b"ffe_create_flight", "ball": b"ffe_create_walk_on_ball", "walk": b"ffe_create_walk_physics"}
    for kind in ("flight", "ball", "walk"):
        assert create(kind, None, 0) == (-1, names[kind] + b": bad arguments")
        for device in (-1, ndev):
            assert create(kind, C.byref(tasks[kind]), device) == (-1, names[kind] + b": no such device")
    bad_flags = _capi.WalkPhysicsTask(physics_flags=FFE_NO_CONTACT)
    assert create("walk", C.byref(bad_flags), 0) == (-1, b"ffe_create_walk_physics: floor contacts and joint limits are not built yet: physics_flags must "
                                                         b"contain FFE_NO_CONTACT | FFE_NO_LIMIT")
    with pytest.raises(RuntimeError, match="floor contacts and joint limits are not built yet"):
        BatchedWalkPhysics(batch_size=B, physics_flags=FFE_NO_CONTACT)
    # a complete flight task with capacity 7: the constructor builds it, the code is read off the library call
    spy = _CreateSpy(L)
    monkeypatch.setattr(_capi, "_lib", spy)
    with pytest.raises(RuntimeError, match=r"ffe_create_flight: contact_capacity must be 6 or 12 \(0 = 6\), got 7"):
        BatchedFlyEnv(wb_tables, *ref_traj, batch_size=B, contact_capacity=7)
    assert spy.codes == [-1]
