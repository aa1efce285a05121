"""`BatchedFlyEnv`: the dm_env-style surface of the reference's fly environments with a leading batch
dimension, backed by the HIP library through the C ABI (include/flybody_env.h).

What it mirrors: `composer.Environment.reset/step/action_spec/observation_spec/
reward_spec/discount_spec/control_timestep` as consumed by `acme.EnvironmentLoop`
(`agents/ray_distributed_dmpo.py:314-315,399-404`).  Tensors are torch-ROCm tensors on the env's device;
PyTorch is used only for device memory and streams.
"""

from __future__ import annotations

import collections
import ctypes as C
import os

import numpy as np

from . import _capi
from .dm_types import Array, BoundedArray, StepType, TimeStep  # noqa: F401  (re-exported)
from .tasks.constants import _WING_PARAMS

_ASSETS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "assets")
FLIGHT_BLOB = os.path.join(_ASSETS, "fly_flight.ffmb")
BALL_BLOB = os.path.join(_ASSETS, "fly_ball.ffmb")
WALK_BLOB = os.path.join(_ASSETS, "fly_walk.ffmb")
FFE_NO_LIMIT, FFE_NO_CONTACT = 2, 64  # include/flybody_env.h
FFE_WALK_JOINT_LIMITS = 512  # ffe_create_walk_physics only: joint limits on (provisional opt-in, see the header)
FFE_WALK_EPISODES = 1024  # ffe_create_walk_physics only: the walk_imitation environment with the floor off (provisional opt-in)
FFE_WALK_FLOOR = 2048  # ffe_create_walk_physics only: the floor plane against the fly's sphere / capsule geoms (opt-in; bare physics, or
#                        with FFE_WALK_EPISODES the walk_imitation environment on the floor)
FFE_WALK_SELF = 4096  # ffe_create_walk_physics only: the fly's own contacts on the floor handle, bare physics or environment (provisional opt-in)
FFE_WALK_SELF_EPISODES = 8192  # ffe_create_walk_physics only: next to FFE_WALK_SELF under the environment (the three bits alone stay refused)
FFE_WALK_FLOOR_CONVEX = 32768  # ffe_create_walk_physics only: the floor against the fly's ellipsoids and cylinders, with FFE_WALK_FLOOR | FFE_WALK_SELF (bare physics or environment)


# `env.validity()`: four int32 [B] views of one [B, 4] device buffer (include/flybody_env.h, ffe_get_validity)
Validity = collections.namedtuple("Validity", ["step_bits", "episode_flagged_steps", "episode_bits", "episode_steps"])


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def time_limit_control_steps(time_limit: float, physics_timestep: float, nsub: int) -> int:
    """Control steps after which `composer.Environment` ends an episode on `physics.time() >= time_limit`.

    MuJoCo's `time` is a float64 running sum of `opt.timestep` (one addition per `mj_step`), so the count is found by
    replaying that sum, not by `round(time_limit / control_timestep)`: 12 000 additions of 5e-5 give 0.5999999999999421
    (flight, 0.6 s -> 3001 control steps) and 10 000 additions of 2e-4 give 1.9999999999998124 (walk_on_ball, 2.0 s ->
    1001)."""
    if not (time_limit > 0 and physics_timestep > 0 and nsub >= 1):
        raise ValueError("time_limit, physics_timestep and nsub must be positive")
    if time_limit / (physics_timestep * nsub) > 5e7:
        return 2**31 - 1  # effectively unlimited
    t, n = 0.0, 0
    h = float(physics_timestep)
    while t < time_limit:
        for _ in range(nsub):
            t += h
        n += 1
    return n


class EnvHandle(_capi.LibHandle):
    """One env handle of the C ABI (include/flybody_env.h) and what every kind of handle shares: `_h`, `_L`, `device`, error checking and
    `close` (`_capi.LibHandle`), the stream, the spec and the raw state accessors.  `get_act` / `set_act` exist on every kind; the library
    refuses them on a flight handle."""

    _destroy, _last_error, _error_prefix = "ffe_destroy", "ffe_last_error", "flybody_env: "

    def _open(self, batch_size: int, device: int):
        """Binds the library and the device; the subclass then creates its handle and passes it to `_adopt`."""
        import torch

        if not torch.cuda.is_available():
            raise RuntimeError(f"{type(self).__name__} needs a HIP device (MI355X); there is no CPU fallback")
        self._torch = torch
        self._L = _capi.lib()
        self.batch_size = int(batch_size)
        self.device = torch.device("cuda", device)

    def _adopt(self, what: str, rc: int, h):
        """Takes the handle a create function returned and reads its spec and action bounds."""
        self._check(rc, None, what + ": ")
        self._h = h
        self.spec = _capi.Spec()
        self._check(self._L.ffe_spec(self._h, C.byref(self.spec)))
        amin, amax = (C.c_float * self.spec.action_dim)(), (C.c_float * self.spec.action_dim)()
        self._check(self._L.ffe_action_bounds(self._h, amin, amax))
        self._action_min, self._action_max = np.array(amin[:], dtype=np.float32), np.array(amax[:], dtype=np.float32)

    def _stream(self):
        return C.c_void_p(self._torch.cuda.current_stream(self.device).cuda_stream)

    def raw_action_bounds(self):
        """(minimum, maximum) of the un-wrapped action spec (`fruitfly.py:496-526`)."""
        return self._action_min.copy(), self._action_max.copy()

    def get_state(self):
        t = self._torch
        qpos = t.empty(self.batch_size, self.spec.nq, dtype=t.float64, device=self.device)
        qvel = t.empty(self.batch_size, self.spec.nv, dtype=t.float64, device=self.device)
        self._check(self._L.ffe_get_state(self._h, qpos.data_ptr(), qvel.data_ptr(), self._stream()))
        return qpos, qvel

    def set_state(self, qpos, qvel):
        t = self._torch
        qpos = qpos.to(device=self.device, dtype=t.float64).contiguous()
        qvel = qvel.to(device=self.device, dtype=t.float64).contiguous()
        assert tuple(qpos.shape) == (self.batch_size, self.spec.nq) and tuple(qvel.shape) == (self.batch_size, self.spec.nv)
        self._check(self._L.ffe_set_state(self._h, qpos.data_ptr(), qvel.data_ptr(), self._stream()))
        t.cuda.current_stream(self.device).synchronize()

    def physics_step(self, ctrl, nsteps: int = 1):
        """`physics.set_control(ctrl)` then `nsteps` x `physics.step()` for every env, no task layer (BASELINE config 2).
        `ctrl`: float32 [B, nu] cuda tensor."""
        assert ctrl.is_cuda and ctrl.device == self.device and ctrl.dtype == self._torch.float32 and ctrl.is_contiguous() and tuple(ctrl.shape) == (self.batch_size, self.spec.nu)
        self._check(self._L.ffe_physics_step(self._h, ctrl.data_ptr(), int(nsteps), self._stream()))

    def get_task_state(self):
        t = self._torch
        ints = t.empty(self.batch_size, 8, dtype=t.int32, device=self.device)
        reals = t.empty(self.batch_size, 8, dtype=t.float64, device=self.device)
        self._check(self._L.ffe_get_task_state(self._h, ints.data_ptr(), reals.data_ptr(), self._stream()))
        return ints, reals

    def get_act(self):
        t = self._torch
        act = t.empty(self.batch_size, self.spec.nu, dtype=t.float64, device=self.device)
        self._check(self._L.ffe_get_act(self._h, act.data_ptr(), self._stream()))
        return act

    def set_act(self, act):
        t = self._torch
        act = act.to(device=self.device, dtype=t.float64).contiguous()
        assert tuple(act.shape) == (self.batch_size, self.spec.nu)
        self._check(self._L.ffe_set_act(self._h, act.data_ptr(), self._stream()))
        t.cuda.current_stream(self.device).synchronize()


class BatchedFlyEnv(EnvHandle):
    """B independent flight-imitation environments stepping in lock-step on one MI355X.

    One `step()` = one kernel launch = one control step (4 physics substeps + task) of every env.
    Envs that returned LAST reset themselves on the next `step()` and report FIRST, as dm_control's
    composer.Environment does per instance.

    **Output aliasing.**  `reset()` / `step()` return a `TimeStep` whose tensors are views of device buffers the env owns
    and overwrites on the next call: a consumer that keeps the previous timestep (acme's `observe(action, next_timestep)`
    adders do) must copy it, or construct the env with `double_buffer=True`, which alternates two buffer sets so that the
    timestep returned by call *k* stays valid until call *k + 2*."""

    task_kind = "flight_imitation"

    def __init__(self, wbpg, ref_qpos, ref_qvel=None, *, batch_size: int, device: int = 0, seed: int = 0, env_id_base: int = 0,
                 future_steps: int = 5, time_limit: float = 0.6, terminal_com_dist: float = 2.0, pad_first_obs: bool = False,
                 physics_flags: int = 0, canonical_actions: bool = False, clip_actions: bool = False, double_buffer: bool = False,
                 blob_path: str = FLIGHT_BLOB, contact_capacity: int = 6):
        """`ref_qpos` / `ref_qvel`: preprocessed reference set, either stacked arrays (N,T,7) / (N,T,6) or one
        `tasks.trajectories.RefSet` (trajectories of individual lengths).

        `contact_capacity`: simultaneous self-contacts the solver carries per env, 6 (default, the benchmarked kernel) or 12
        (a second instantiation of the step kernel: same physics up to six contacts, constraint rows for up to twelve).  The
        library rejects every other value."""
        import json

        self._open(batch_size, device)
        if isinstance(contact_capacity, bool) or int(contact_capacity) != contact_capacity:
            raise TypeError(f"contact_capacity must be an integer (6 or 12), got {contact_capacity!r}")
        self.contact_capacity = int(contact_capacity)
        with open(blob_path, "rb") as f:
            blob = f.read()
        with open(os.path.splitext(blob_path)[0] + ".json") as f:
            self._meta = json.load(f)
        from .model.blob import read_blob

        tens = read_blob(blob_path)
        # the ghost is a wingless fly on a free joint with armature 1 (`tasks/base.py:142-149`): gravity moves it by
        # g * m / (m + 1)
        wing_links = [i for i, b in enumerate(tens["link_body"]) if self._meta["body_name"][b].startswith("wing")]
        m_ghost = float(tens["link_mass"].sum() - tens["link_mass"][wing_links].sum())
        ghost_accel_z = float(tens["opt"][5]) * m_ghost / (m_ghost + 1.0)
        from .tasks.trajectories import as_refset

        refs = as_refset(ref_qpos, ref_qvel)
        self.refs = refs
        self._keep = dict(bf=_f64(wbpg.beat_freqs), off=np.ascontiguousarray(wbpg.tab_off, dtype=np.int32), traj=_f64(wbpg.traj),
                          phase=_f64(wbpg.phase), rq=refs.qpos, rv=refs.qvel, roff=refs.off)
        k = self._keep
        n, t = refs.ntraj, int(refs.lengths().max())
        h_phys = float(tens["opt"][0])
        nsub = int(round(wbpg.dt_ctrl / h_phys))
        dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
        task = _capi.FlightTask(
            wb_nfreq=len(k["bf"]), wb_beat_freqs=dp(k["bf"]), wb_tab_off=k["off"].ctypes.data_as(C.POINTER(C.c_int32)),
            wb_traj=dp(k["traj"]), wb_phase=dp(k["phase"]), wb_base_freq=wbpg.base_freq, wb_rel_range=wbpg.rel_range,
            wb_rate=wbpg.rate, wb_dt_ctrl=wbpg.dt_ctrl, ntraj=n, traj_len=t, ref_qpos=dp(k["rq"]), ref_qvel=dp(k["rv"]),
            traj_off=k["roff"].ctypes.data_as(C.POINTER(C.c_int32)),
            future_steps=future_steps, time_limit_steps=int(round(time_limit / wbpg.dt_ctrl)),
            episode_limit_steps=time_limit_control_steps(time_limit, h_phys, nsub),
            terminal_com_dist=float(terminal_com_dist), ghost_accel_z=ghost_accel_z, pad_first_obs=int(pad_first_obs),
            physics_flags=int(physics_flags), canonical_actions=int(canonical_actions), clip_actions=int(clip_actions),
            contact_capacity=self.contact_capacity)
        self.time_limit_steps = int(task.episode_limit_steps)  # control steps after which the time limit ends an episode
        h = C.c_void_p()
        rc = self._L.ffe_create_flight(blob, len(blob), C.byref(task), self.batch_size, device, seed, env_id_base, C.byref(h))
        self._adopt("ffe_create_flight", rc, h)
        self.ghost_accel_z = ghost_accel_z
        self.canonical_actions = bool(canonical_actions)
        s = self.spec
        self._alloc_outputs(double_buffer)
        j, r = s.n_obs_joints, s.n_ref
        # key order: enabled walker observables alphabetically, then the task's additions (dm_control Observables)
        self._layout = collections.OrderedDict([
            ("walker/accelerometer", (s.off_accelerometer, (3,))), ("walker/actuator_activation", (0, (0,))),
            ("walker/gyro", (s.off_gyro, (3,))), ("walker/joints_pos", (s.off_joints_pos, (j,))),
            ("walker/joints_vel", (s.off_joints_vel, (j,))), ("walker/velocimeter", (s.off_velocimeter, (3,))),
            ("walker/world_zaxis", (s.off_world_zaxis, (3,))), ("walker/ref_displacement", (s.off_ref_displacement, (r, 3))),
            ("walker/ref_root_quat", (s.off_ref_root_quat, (r, 4)))])

    # ------------------------------------------------------------------------------------------ plumbing
    def _alloc_outputs(self, double_buffer: bool):
        torch, B, s = self._torch, self.batch_size, self.spec
        self._sets = []
        with torch.cuda.device(self.device):
            for _ in range(2 if double_buffer else 1):
                self._sets.append((torch.zeros(B, s.obs_dim, dtype=torch.float32, device=self.device),
                                   torch.zeros(B, dtype=torch.float32, device=self.device),
                                   torch.zeros(B, dtype=torch.float32, device=self.device),
                                   torch.zeros(B, dtype=torch.int32, device=self.device)))
        self._cur = 0
        self._obs, self._reward, self._discount, self._step_type = self._sets[0]

    def _next_outputs(self):
        """Selects the buffer set the next launch writes (the other one keeps the previous timestep when double-buffered)."""
        self._cur = (self._cur + 1) % len(self._sets)
        self._obs, self._reward, self._discount, self._step_type = self._sets[self._cur]

    def _timestep(self):
        obs = collections.OrderedDict()
        for key, (off, shape) in self._layout.items():
            n = int(np.prod(shape))
            obs[key] = self._obs[:, off:off + n].view(self.batch_size, *shape)
        return TimeStep(self._step_type, self._reward, self._discount, obs)

    # ------------------------------------------------------------------------------------------ dm_env surface
    def reset(self) -> TimeStep:
        self._next_outputs()
        self._check(self._L.ffe_reset(self._h, self._obs.data_ptr(), self._reward.data_ptr(), self._discount.data_ptr(),
                                      self._step_type.data_ptr(), self._stream()))
        return self._timestep()

    def reset_envs(self, mask) -> TimeStep:
        """Starts a new episode in the envs where `mask` (bool / uint8 [B], on the env's device) is set - the per-instance
        `Environment.reset()` of the reference's one-env-per-actor layout - and returns the timestep with those rows
        replaced by their FIRST observation; the other envs are not touched."""
        t = self._torch
        m = t.as_tensor(mask, device=self.device).to(t.uint8).contiguous()
        if tuple(m.shape) != (self.batch_size,):
            raise ValueError(f"mask must have shape ({self.batch_size},)")
        if len(self._sets) > 1:  # the untouched rows must carry over into the buffer set this call writes
            prev = self._sets[self._cur]
            self._next_outputs()
            for dst, src in zip(self._sets[self._cur], prev):
                dst.copy_(src)
        self._check(self._L.ffe_reset_envs(self._h, m.data_ptr(), self._obs.data_ptr(), self._reward.data_ptr(), self._discount.data_ptr(),
                                           self._step_type.data_ptr(), self._stream()))
        return self._timestep()

    def step(self, action) -> TimeStep:
        """`action`: float32 [B, action_dim] tensor on the env's device, in the raw action spec."""
        t = self._torch
        if not (isinstance(action, t.Tensor) and action.is_cuda and action.device == self.device and action.dtype == t.float32
                and action.is_contiguous() and tuple(action.shape) == (self.batch_size, self.spec.action_dim)):
            raise ValueError(f"action must be a contiguous float32 tensor of shape ({self.batch_size}, {self.spec.action_dim}) on {self.device}")
        self._next_outputs()
        self._check(self._L.ffe_step(self._h, action.data_ptr(), self._obs.data_ptr(), self._reward.data_ptr(),
                                     self._discount.data_ptr(), self._step_type.data_ptr(), self._stream()))
        return self._timestep()

    def action_spec(self):
        if self.canonical_actions:  # acme CanonicalSpecWrapper: every action dimension spans [-1, 1]
            return BoundedArray((self.spec.action_dim,), np.float32, -1.0, 1.0, name="\t".join(self._meta["action_names"]))
        return BoundedArray((self.spec.action_dim,), np.float32, self._action_min, self._action_max,
                            name="\t".join(self._meta["action_names"]))

    def observation_spec(self):
        return collections.OrderedDict((k, Array(shape, np.float32, name=k)) for k, (_, shape) in self._layout.items())

    def reward_spec(self):
        return Array((), np.float32, name="reward")

    def discount_spec(self):
        return BoundedArray((), np.float32, 0.0, 1.0, name="discount")

    def control_timestep(self) -> float:
        return self.spec.control_timestep

    @property
    def flat_observation(self):
        """The [B, obs_dim] buffer the observation dict views into."""
        return self._obs

    # ------------------------------------------------------------------------------------------ test / tooling hooks
    def set_next_trajectory_index(self, idx, phase):
        """`FlightImitationWBPG.set_next_trajectory_index` (`flight_imitation.py:87-91`) per env, plus the wing phase."""
        idx = np.ascontiguousarray(np.broadcast_to(idx, (self.batch_size,)), dtype=np.int32)
        phase = np.ascontiguousarray(np.broadcast_to(phase, (self.batch_size,)), dtype=np.float64)
        self._check(self._L.ffe_force_next_episode(self._h, idx.ctypes.data_as(C.POINTER(C.c_int32)), phase.ctypes.data_as(C.POINTER(C.c_double)),
                                                   self._stream()))

    def validity(self) -> Validity:
        """Whether the physics behind the current timestep was truncated (`ffe_get_validity`): `step_bits` of the launch that produced
        it (flight: bit 0 more contacts than `contact_capacity`, bit 1 the solver's iteration cap; walk_on_ball: the overflow bits of
        task-state int 7, this launch alone), and per episode the flagged control steps, the OR of their bits and the control steps so
        far.  The three episode fields are 0 on a FIRST row; read after a LAST row they are that episode's totals.

        The tensors are views of one int32 [B, 4] buffer the env owns (`validity_buffer`), overwritten by the next call.  One launch on
        the current stream, no synchronisation: usable under HIP-graph capture."""
        t = self._torch
        if getattr(self, "_validity", None) is None:
            with t.cuda.device(self.device):
                self._validity = t.zeros(self.batch_size, 4, dtype=t.int32, device=self.device)
        self._check(self._L.ffe_get_validity(self._h, self._validity.data_ptr(), self._stream()))
        return Validity(*self._validity.unbind(1))

    @property
    def validity_buffer(self):
        """The int32 [B, 4] buffer `validity()` fills (None before its first call)."""
        return getattr(self, "_validity", None)

    def time_kernel(self, action, iters: int) -> float:
        """Mean milliseconds of the step kernel alone over `iters` launches (HIP events immediately around it)."""
        ms = C.c_float()
        self._check(self._L.ffe_time_kernel(self._h, action.data_ptr(), self._obs.data_ptr(), self._reward.data_ptr(),
                                            self._discount.data_ptr(), self._step_type.data_ptr(), int(iters), self._stream(), C.byref(ms)))
        return float(ms.value)

    def time_steps(self, action, iters: int) -> float:
        """Mean milliseconds per step launch over `iters` launches, by HIP events on the current stream."""
        ms = C.c_float()
        self._check(self._L.ffe_time_steps(self._h, action.data_ptr(), self._obs.data_ptr(), self._reward.data_ptr(),
                                           self._discount.data_ptr(), self._step_type.data_ptr(), int(iters), self._stream(), C.byref(ms)))
        return float(ms.value)


class BatchedBallEnv(BatchedFlyEnv):
    """B independent `walk_on_ball` environments (`fly_envs.py:125-157`) on one MI355X: a tethered fly on a floating
    ball, 10 physics substeps (contacts, elliptic friction cones, noslip, adhesion, filtered actuators) per control step.
    Same dm_env surface and hooks as `BatchedFlyEnv`; `get_state` returns qpos[B, 106] = ball quaternion + 102 hinges and
    qvel[B, 105] = ball angular velocity + hinges."""

    task_kind = "walk_on_ball"

    def __init__(self, *, batch_size: int, device: int = 0, time_limit: float = 2.0, control_timestep: float = 2e-3,
                 pad_first_obs: bool = False, physics_flags: int = 0, canonical_actions: bool = False, clip_actions: bool = False,
                 double_buffer: bool = False, blob_path: str = BALL_BLOB):
        import json

        self._open(batch_size, device)
        with open(blob_path, "rb") as f:
            blob = f.read()
        with open(os.path.splitext(blob_path)[0] + ".json") as f:
            self._meta = json.load(f)
        from .model.blob import read_blob

        h_phys = float(read_blob(blob_path)["opt"][0])
        nsub = int(round(control_timestep / h_phys))
        task = _capi.BallTask(control_timestep=float(control_timestep), time_limit_steps=time_limit_control_steps(time_limit, h_phys, nsub),
                              pad_first_obs=int(pad_first_obs), physics_flags=int(physics_flags),
                              canonical_actions=int(canonical_actions), clip_actions=int(clip_actions))
        self.time_limit_steps = int(task.time_limit_steps)
        h = C.c_void_p()
        rc = self._L.ffe_create_walk_on_ball(blob, len(blob), C.byref(task), self.batch_size, device, C.byref(h))
        self._adopt("ffe_create_walk_on_ball", rc, h)
        self.canonical_actions = bool(canonical_actions)
        s = self.spec
        self._alloc_outputs(double_buffer)
        self._layout = collections.OrderedDict()
        off = 0
        for name, shape in (("accelerometer", (3,)), ("actuator_activation", (s.nu,)), ("appendages_pos", (21,)), ("ball_qvel", (3,)),
                            ("force", (18,)), ("gyro", (3,)), ("joints_pos", (s.n_obs_joints,)), ("joints_vel", (s.n_obs_joints,)),
                            ("touch", (6,)), ("velocimeter", (3,)), ("world_zaxis", (3,))):
            self._layout["walker/" + name] = (off, shape)
            off += int(np.prod(shape))
        assert off == s.obs_dim

    def set_next_trajectory_index(self, idx, phase):
        raise NotImplementedError("walk_on_ball has no reference trajectories")


class BatchedWalkEnv(BatchedFlyEnv):
    """B independent `walk_imitation` environments (`fly_envs.py:75-122`) on one MI355X: the free-root walking fly (10 physics
    substeps with joint limits and filtered actuators per control step), the thorax IMU, the DeepMimic reward against a reference
    clip, termination and auto-reset, all on the device.  Same dm_env surface and hooks as `BatchedBallEnv`; one `step()` is five
    launches.

    `floor_contacts=False` (the default): **the floor is off**.  The fly falls freely (or floats with FFE_NO_GRAVITY in
    `physics_flags`); force and touch read exact zeros.  The float64 oracle does the same with contacts switched off, so every row can
    be compared with it.

    `floor_contacts=True` adds FFE_WALK_FLOOR: the floor plane against the fly's 48 sphere / capsule geoms, as in
    `BatchedWalkPhysics(floor_contacts=True)` (elliptic cones, the model's noslip sweeps, the adhesion actuators; `physics_flags` may
    then also carry FFE_NO_NOSLIP / FFE_NO_ADHESION), with the 18 force and 6 touch columns live: the force sensors read the
    interaction force on each tarsus (inertial without a contact, so not zero), touch the normal forces on each claw.  The fly's own
    contacts, and the plane against ellipsoids and cylinders, stay off.  `get_task_state()` int 5 is then the floor contacts kept in the
    last substep, reals 0 / 1 the sum of their normal forces and the smallest distance; `validity()`'s step_bits carry the floor's
    overflow bits 1 / 2 / 4 next to the limit bit, sticky per episode in episode_bits.

    `self_contacts=True` (keyword-only; it needs `floor_contacts=True`) adds FFE_WALK_SELF | FFE_WALK_SELF_EPISODES: the fly's own
    contacts as in `BatchedWalkPhysics(floor_contacts=True, self_contacts=True)` - its 48 sphere / capsule geoms against each other and
    every candidate pair with an ellipsoid or a cylinder on one side, frictionless normal rows between the floor's cone blocks and the
    joint limits - with their forces in the force and touch columns (a fly-fly contact pushes both of its links).  The env can then be
    compared with the float64 oracle on the shipped model.  int 5 counts both kinds of contact, reals[:, 2] the fly-fly ones among them
    (int 3 is needs_reset on an env), real 1 is taken over both kinds, and step_bits bit value 8 says that a convex candidate pair was
    left out because a pair list of the substep was full.  The plane against ellipsoids and cylinders stays off.

    `floor_convex=True` (keyword-only; it needs `floor_contacts=True` and `self_contacts=True`) adds
    FFE_WALK_FLOOR_CONVEX: the floor plane against the fly's 16 ellipsoids and 6 cylinders as in
    `BatchedWalkPhysics(floor_contacts=True, self_contacts=True, floor_convex=True)`, floor cone blocks like the others, so that a
    fallen fly rests on its thorax, head, wings, coxae and abdomen.  This is the reference's whole contact set.  int 5 then counts
    all three kinds of contact, reals[:, 3] the plane-ellipsoid / plane-cylinder ones among them (zero on every other env), and
    bit 1 of step_bits says that more than 16 contacts were found and the deepest floor contacts were kept.

    `refs`: a `tasks.walking.WalkRefSet`; `view`: the `WalkModelView` that names the tracked joints and sites (None: the default
    one).  `get_state` / `set_state` / `get_act` / `set_act` / `physics_step` are `BatchedWalkPhysics`'s."""

    task_kind = "walk_imitation"

    def __init__(self, refs, view=None, *, batch_size: int, device: int = 0, seed: int = 0, env_id_base: int = 0, future_steps: int = 64,
                 time_limit: float = 10.0, terminal_com_dist: float = 0.3, control_timestep: float = 2e-3, pad_first_obs: bool = False,
                 physics_flags: int = 0, canonical_actions: bool = False, clip_actions: bool = False, double_buffer: bool = False,
                 inference_mode: bool = False, blob_path: str = WALK_BLOB, floor_contacts: bool = False, self_contacts: bool = False,
                 floor_convex: bool = False):
        import json

        if self_contacts and not floor_contacts:
            raise ValueError("BatchedWalkEnv: self_contacts=True needs floor_contacts=True (the fly's own contacts are built on the floor env)")
        if floor_convex and not (floor_contacts and self_contacts):
            raise ValueError("BatchedWalkEnv: floor_convex=True needs floor_contacts=True and self_contacts=True (the floor against "
                             "ellipsoids and cylinders is built on the env with the fly's own contacts)")

        from .model.blob import read_blob
        from .tasks.walk_tracker import make_task
        from .tasks.walking import WalkModelView

        self._open(batch_size, device)
        with open(blob_path, "rb") as f:
            blob = f.read()
        with open(os.path.splitext(blob_path)[0] + ".json") as f:
            self._meta = json.load(f)
        self.view = view = view or WalkModelView()
        self.refs = refs
        h_phys = float(read_blob(blob_path)["opt"][0])
        nsub = int(round(control_timestep / h_phys))
        wtask, self._keep = make_task(view, refs, future_steps=future_steps, terminal_com_dist=terminal_com_dist, time_limit=time_limit,
                                      control_timestep=control_timestep, inference_mode=inference_mode)
        force_switches = int(physics_flags) & (1 | 4 | 8 | 16 | 32)  # FFE_NO_FLUID / _DAMPER / _SPRING / _GRAVITY / _ACTUATION
        self.floor_contacts = bool(floor_contacts)
        if self.floor_contacts:
            force_switches |= int(physics_flags) & (128 | 256)  # FFE_NO_NOSLIP / FFE_NO_ADHESION
            if int(physics_flags) & ~(force_switches | FFE_NO_CONTACT | FFE_WALK_JOINT_LIMITS | FFE_WALK_EPISODES | FFE_WALK_FLOOR
                                      | (FFE_WALK_SELF | FFE_WALK_SELF_EPISODES if self_contacts else 0)
                                      | (FFE_WALK_FLOOR_CONVEX if floor_convex else 0)):
                raise ValueError("BatchedWalkEnv(floor_contacts=True): physics_flags takes the force switches, FFE_NO_NOSLIP and FFE_NO_ADHESION only")
        elif int(physics_flags) & ~(force_switches | FFE_NO_CONTACT | FFE_WALK_JOINT_LIMITS | FFE_WALK_EPISODES):
            raise ValueError("BatchedWalkEnv: physics_flags takes the force switches only (floor contacts are not built; joint limits are on)")
        self.self_contacts = bool(self_contacts)
        self.floor_convex = bool(floor_convex)
        self.physics_flags = (force_switches | FFE_NO_CONTACT | FFE_WALK_JOINT_LIMITS | FFE_WALK_EPISODES | (FFE_WALK_FLOOR if self.floor_contacts else 0)
                              | (FFE_WALK_SELF | FFE_WALK_SELF_EPISODES if self.self_contacts else 0)
                              | (FFE_WALK_FLOOR_CONVEX if self.floor_convex else 0))
        task = _capi.WalkPhysicsTask(physics_flags=self.physics_flags, task=C.pointer(wtask), seed=int(seed), env_id_base=int(env_id_base),
                                     time_limit_steps=time_limit_control_steps(time_limit, h_phys, nsub), pad_first_obs=int(pad_first_obs),
                                     canonical_actions=int(canonical_actions), clip_actions=int(clip_actions))
        self.time_limit_steps = int(task.time_limit_steps)
        h = C.c_void_p()
        rc = self._L.ffe_create_walk_physics(blob, len(blob), C.byref(task), self.batch_size, device, C.byref(h))
        self._adopt("ffe_create_walk_physics", rc, h)
        self.canonical_actions = bool(canonical_actions)
        s = self.spec
        self._alloc_outputs(double_buffer)
        F1 = s.n_ref
        self._layout = collections.OrderedDict()
        off = 0
        for name, shape in (("accelerometer", (3,)), ("actuator_activation", (s.nu,)), ("appendages_pos", (s.off_gyro - 18 - 3 - s.nu,)),
                            ("force", (18,)), ("gyro", (3,)), ("joints_pos", (s.n_obs_joints,)), ("joints_vel", (s.n_obs_joints,)),
                            ("ref_displacement", (F1, 3)), ("ref_root_quat", (F1, 4)), ("touch", (6,)), ("velocimeter", (3,)),
                            ("world_zaxis", (3,))):
            self._layout["walker/" + name] = (off, shape)
            off += int(np.prod(shape))
        assert off == s.obs_dim and self._layout["walker/gyro"][0] == s.off_gyro and self._layout["walker/velocimeter"][0] == s.off_velocimeter
        assert self._layout["walker/ref_root_quat"][0] == s.off_ref_root_quat and self._layout["walker/world_zaxis"][0] == s.off_world_zaxis

    def set_next_trajectory_index(self, idx, phase=0.0):
        """`WalkImitation.set_next_trajectory_index` (`walk_imitation.py:84-87`) per env: the clip of each env's next reset (negative: the
        counter-based draw).  walk_imitation draws no phase; the argument is accepted for the base class's signature and ignored."""
        super().set_next_trajectory_index(idx, 0.0)


class BatchedWalkPhysics(EnvHandle):
    """B walking flies (`assets/fly_walk.ffmb`: free thorax, 6 + 102 dofs, 59 filtered actuators) advanced on one MI355X by
    `ffe_physics_step`: the smooth dynamics of `walk_imitation` with constraints off or, with
    `joint_limits=True`, with the joint limits of the 102 hinges on (step 3a).  Not an environment: there is no reset, step, observation
    or reward (`BatchedWalkEnv` is the environment around the same physics; floor contacts are not built yet).  The handle starts at
    the model's `qpos0` at rest.

    `physics_flags` must contain FFE_NO_CONTACT and exactly one of FFE_NO_LIMIT (the default) or FFE_WALK_JOINT_LIMITS;
    `joint_limits=True` sets FFE_NO_CONTACT | FFE_WALK_JOINT_LIMITS plus whatever force switches (FFE_NO_FLUID, ...) `physics_flags`
    carries.  A limits handle carries up to 48 limit rows per env and substep; beyond that the rows that did not fit are dropped for the
    substep and `validity()`'s step_bits (and int 7 of `get_task_state()`) carry bit value 2.  `get_task_state()` ints 4 and 6 are the
    limit rows and the solver iterations of the last substep.

    `floor_contacts=True` (step 3b; it implies `joint_limits`) adds FFE_WALK_FLOOR: the floor plane against the fly's 48 sphere / capsule
    geoms, as elliptic-cone contacts with the model's noslip sweeps and the adhesion actuators (FFE_NO_NOSLIP / FFE_NO_ADHESION in
    `physics_flags` switch those off); the fly's own contacts stay off.  Up to 16 contacts and 48 rows per env and substep, 24 rows
    per block of the inertia; beyond that the deepest contacts are kept, rows without a column are switched off for the substep and
    step_bits carry 1 / 2 / 4.  `get_task_state()` then also gives int 5 = floor contacts of the last substep, real 0 = the sum of
    their normal forces, real 1 = the smallest contact distance.

    `self_contacts=True` (step 3c; it needs `floor_contacts=True`) adds FFE_WALK_SELF: the fly's own contacts, its 48 sphere / capsule
    geoms against each other and every candidate pair with an ellipsoid or a cylinder on one side, as frictionless normal rows between
    the floor's cone blocks and the joint limits.  The 16 contact slots hold the floor's contacts first and the fly-fly ones behind
    them.  `get_task_state()` int 5 then counts both kinds, int 3 the fly-fly ones among them, real 1 is taken over both kinds, and
    step_bits bit value 8 says that a convex candidate pair was left out because a pair list of the substep was full.

    `floor_convex=True` (keyword-only; step 3d; it needs both `floor_contacts=True` and `self_contacts=True`) adds FFE_WALK_FLOOR_CONVEX:
    the floor plane also against the fly's 16 ellipsoids (thorax, head, mouth parts, wings, coxae) and 6 cylinders (abdomen), so that a
    fly on its back or on its abdomen rests on the floor.  Their contacts are floor contacts like the others (slots behind the
    primitive floor contacts, the 16 deepest of both kinds kept); `get_task_state()` real 2 counts them among int 5.

    Tensor conventions are `BatchedBallEnv`'s: `get_state` returns float64 cuda tensors qpos[B, 109] = root position (float64 on the
    device too), root quaternion, 102 hinges and qvel[B, 108] = root linear velocity (world frame), root angular velocity (body
    frame), hinges; `set_state` takes the same and normalises the quaternion; `physics_step` takes float32 ctrl[B, 59]."""

    task_kind = "walk_physics"

    def __init__(self, *, batch_size: int, device: int = 0, physics_flags: int = FFE_NO_CONTACT | FFE_NO_LIMIT, blob_path: str = WALK_BLOB,
                 joint_limits: bool = False, floor_contacts: bool = False, self_contacts: bool = False, floor_convex: bool = False):
        if self_contacts and not floor_contacts:
            raise ValueError("BatchedWalkPhysics: self_contacts=True needs floor_contacts=True (the fly's own contacts are built on the floor handle)")
        if floor_convex and not (floor_contacts and self_contacts):
            raise ValueError("BatchedWalkPhysics: floor_convex=True needs floor_contacts=True and self_contacts=True (the floor against "
                             "ellipsoids and cylinders is built on the handle that carries both)")
        if joint_limits or floor_contacts:
            physics_flags = (int(physics_flags) & ~(FFE_NO_CONTACT | FFE_NO_LIMIT)) | FFE_NO_CONTACT | FFE_WALK_JOINT_LIMITS
        if floor_contacts:
            physics_flags |= FFE_WALK_FLOOR
        if self_contacts:
            physics_flags |= FFE_WALK_SELF
        if floor_convex:
            physics_flags |= FFE_WALK_FLOOR_CONVEX
        self._open(batch_size, device)
        with open(blob_path, "rb") as f:
            blob = f.read()
        task = _capi.WalkPhysicsTask(physics_flags=int(physics_flags))
        h = C.c_void_p()
        rc = self._L.ffe_create_walk_physics(blob, len(blob), C.byref(task), self.batch_size, device, C.byref(h))
        self._adopt("ffe_create_walk_physics", rc, h)
        self.physics_flags = int(physics_flags)
