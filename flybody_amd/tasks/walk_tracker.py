"""Device task layer of `fly_envs.walk_imitation` (include/flybody_env.h `ffe_walktask_*`, csrc/walk_task.hip): the walker
features of `tasks/rewards.py:36-61`, the four DeepMimic reward factors, the task's termination bits and the kinematic columns of
the observation row, as a pure function of (qpos, qvel, clip, step) on batches of states that live on the device.  No physics: the
environment (`batched_env.BatchedWalkEnv`) holds a handle of this layer of its own; this class scores
recorded states against clips (reward relabelling, dataset QC) and turns raw pose rows into reference tables (`walking.featurize`).
"""

from __future__ import annotations

import ctypes as C
import os
from collections import namedtuple

import numpy as np

from .. import _capi
from .rewards import DEFAULT_STD, FEATURES
from .walking import WalkModelView

WalkFeatures = namedtuple("WalkFeatures", "com qvel root2site joint_quat")
WalkEvaluation = namedtuple("WalkEvaluation", "factors reward term_bits obs")
WalkPose = namedtuple("WalkPose", "qpos qvel")

#: bits of `WalkEvaluation.term_bits`
TERM_COM_DIST, TERM_END_OF_CLIP, TERM_STEP_OUT_OF_RANGE = 1, 2, 4
#: the kinematic column groups `evaluate` writes, in row order
OBS_GROUPS = ("appendages_pos", "joints_pos", "joints_vel", "ref_displacement", "ref_root_quat", "world_zaxis")

_ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))  # noqa: E731
_dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731


def make_task(view: WalkModelView, refs=None, joints=None, sites=None, *, future_steps=64, terminal_com_dist=0.3, time_limit=10.0,
              control_timestep=2e-3, weights=(20, 1, 1, 1), std=None, inference_mode=False, overrides=None):
    """-> (`_capi.WalkTask`, the arrays it points to).  Host only: checks the shapes of the ragged reference tables against the
    tracked sets (`refs` is a `WalkRefSet`-like object or None for a handle that only featurises) and packs them contiguously."""
    keep = lambda a, dt: np.ascontiguousarray(a, dtype=dt)  # noqa: E731
    joints = keep(view.mocap_jnt if joints is None else joints, np.int32).reshape(-1)
    sites = keep(view.mocap_site if sites is None else sites, np.int32).reshape(-1)
    J, S = len(joints), len(sites)
    std = DEFAULT_STD if std is None else std
    std = [float(std[k]) for k in FEATURES] if isinstance(std, dict) else [float(x) for x in std]
    weights = [float(x) for x in weights]
    if len(std) != 4 or len(weights) != 4:
        raise ValueError("std and weights take four values: com, qvel, root2site, joint_quat")
    oq, ov = (view.retract_qadr, view.retract_val) if overrides is None else overrides
    oq, ov = keep(oq, np.int32).reshape(-1), keep(ov, np.float64).reshape(-1)
    if len(oq) != len(ov):
        raise ValueError(f"overrides: {len(oq)} addresses for {len(ov)} values")
    t = _capi.WalkTask()
    arrays = [joints, sites, oq, ov]
    t.n_joints, t.joints, t.n_sites, t.sites = J, _ip(joints), S, _ip(sites)
    if refs is not None:
        off = keep(refs.off, np.int32).reshape(-1)
        rows = int(off[-1])
        rq, rv = keep(refs.qpos, np.float64), keep(refs.qvel, np.float64)
        rs, rj = keep(refs.root2site, np.float64), keep(refs.joint_quat, np.float64)
        for name, a, shape in (("qpos", rq, (rows, 7 + J)), ("qvel", rv, (rows, 6 + J)), ("root2site", rs, (rows, S, 3)),
                               ("joint_quat", rj, (rows, J, 4))):
            if a.shape != shape:
                raise ValueError(f"refs.{name} has shape {a.shape}; {rows} rows of {J} tracked joints and {S} tracked sites need {shape}")
        arrays += [off, rq, rv, rs, rj]
        t.ntraj, t.traj_off = len(off) - 1, _ip(off)
        t.ref_qpos, t.ref_qvel, t.ref_root2site, t.ref_joint_quat = _dp(rq), _dp(rv), _dp(rs), _dp(rj)
    t.future_steps, t.control_timestep, t.time_limit = int(future_steps), float(control_timestep), float(time_limit)
    t.terminal_com_dist = float(terminal_com_dist)
    t.std, t.weights = (C.c_double * 4)(*std), (C.c_double * 4)(*weights)
    t.n_overrides, t.override_qadr, t.override_val = len(oq), _ip(oq), _dp(ov)
    t.inference_mode = int(bool(inference_mode))
    return t, arrays


def obs_layout(dims) -> dict:
    """{group: (offset, width)} of the kinematic observation columns from the 16 ints of `ffe_walktask_info`."""
    F1 = dims[5] + 1
    return {"appendages_pos": (dims[7], 3 * dims[13]), "joints_pos": (dims[8], dims[14]), "joints_vel": (dims[9], dims[14]),
            "ref_displacement": (dims[10], 3 * F1), "ref_root_quat": (dims[11], 4 * F1), "world_zaxis": (dims[12], 3)}


class WalkTracker(_capi.LibHandle):
    """Scores batches of device-resident states against reference clips.  `refs`: a `WalkRefSet` (None: `features` only);
    `dtype` "float32" (the product path) or "float64" (featurisation); tensors go in and come out on `cuda:device`."""

    _destroy, _last_error = "ffe_walktask_destroy", "ffe_walktask_last_error"

    def __init__(self, refs, view: WalkModelView | None = None, *, joints=None, sites=None, future_steps=64, terminal_com_dist=0.3,
                 time_limit=10.0, control_timestep=2e-3, weights=(20, 1, 1, 1), std=None, inference_mode=False, dtype="float32", device=0,
                 overrides=None, blob_path: str | None = None):
        import torch

        if dtype not in ("float32", "float64"):
            raise ValueError(f"dtype {dtype!r}: float32 or float64")
        if not torch.cuda.is_available():
            raise RuntimeError("WalkTracker needs a HIP device (MI355X); there is no CPU fallback")
        self._torch, self._L = torch, _capi.lib()
        self.view = view = view or WalkModelView()
        self.device = torch.device("cuda", device)
        self.dtype = torch.float64 if dtype == "float64" else torch.float32
        task, self._keep = make_task(view, refs, joints, sites, future_steps=future_steps, terminal_com_dist=terminal_com_dist, time_limit=time_limit,
                                     control_timestep=control_timestep, weights=weights, std=std, inference_mode=inference_mode, overrides=overrides)
        blob_path = blob_path or os.path.join(os.path.dirname(__file__), "..", "assets", "fly_walk.ffmb")
        with open(blob_path, "rb") as f:
            blob = f.read()
        h = C.c_void_p()
        self._check(self._L.ffe_walktask_create(blob, len(blob), C.byref(task), int(dtype == "float64"), device, C.byref(h)), None)
        self._h = h
        dims = (C.c_int32 * 16)()
        ep = (C.c_int32 * max(1, task.ntraj))()
        self._check(self._L.ffe_walktask_info(h, dims, ep))
        self.dims = list(dims)
        self.nq, self.nv, self.J, self.S, self.ntraj, self.future_steps, self.obs_dim = self.dims[:7]
        self.episode_steps = np.array(list(ep)[: self.ntraj], dtype=np.int32)
        self.obs_layout = obs_layout(self.dims)

    # ---------------------------------------------------------------------------------------------- plumbing
    def _stream(self):
        return C.c_void_p(self._torch.cuda.current_stream(self.device).cuda_stream)

    def _in(self, x, dtype, shape, name):
        t = self._torch
        x = t.as_tensor(x)
        if x.device != self.device or x.dtype != dtype or not x.is_contiguous():
            x = x.to(device=self.device, dtype=dtype).contiguous()
        if tuple(x.shape) != shape:
            raise ValueError(f"{name} has shape {tuple(x.shape)}, expected {shape}")
        return x

    def _states(self, qpos, qvel):
        t = self._torch
        qpos = t.as_tensor(qpos)
        n = qpos.shape[0] if qpos.dim() == 2 else -1
        return self._in(qpos, t.float64, (n, self.nq), "qpos"), self._in(qvel, t.float64, (n, self.nv), "qvel"), n

    # ---------------------------------------------------------------------------------------------- calls
    def features(self, qpos, qvel) -> WalkFeatures:
        """`get_walker_features` of qpos [N, nq], qvel [N, nv] (float64): com float64 [N, 3], qvel [N, 6 + J], root2site [N, S, 3],
        joint_quat [N, 1 + J, 4] in the handle's dtype."""
        t = self._torch
        qpos, qvel, n = self._states(qpos, qvel)
        kw = dict(device=self.device, dtype=self.dtype)
        out = WalkFeatures(t.empty((n, 3), device=self.device, dtype=t.float64), t.empty((n, 6 + self.J), **kw),
                           t.empty((n, self.S, 3), **kw), t.empty((n, 1 + self.J, 4), **kw))
        self._check(self._L.ffe_walktask_features(self._h, qpos.data_ptr(), qvel.data_ptr(), n, out.com.data_ptr(), out.qvel.data_ptr(),
                                                  out.root2site.data_ptr(), out.joint_quat.data_ptr(), self._stream()))
        return out

    def evaluate(self, qpos, qvel, clip, step, obs=None) -> WalkEvaluation:
        """Reward factors [N, 4], reward [N], term_bits int32 [N] and the kinematic observation columns of every state against
        row `step` of clip `clip` (int32 [N] each).  `obs`: a [N, >= obs_dim] buffer of the handle's dtype whose other columns are
        left as they are (the row stride is its first stride); None allocates a zeroed [N, obs_dim] one."""
        t = self._torch
        qpos, qvel, n = self._states(qpos, qvel)
        clip, step = self._in(clip, t.int32, (n,), "clip"), self._in(step, t.int32, (n,), "step")
        if obs is None:
            obs = t.zeros((n, self.obs_dim), device=self.device, dtype=self.dtype)
        if obs.device != self.device or obs.dtype != self.dtype or obs.dim() != 2 or obs.shape[0] != n or obs.stride(1) != 1:
            raise ValueError(f"obs must be a [{n}, >= {self.obs_dim}] {self.dtype} tensor on {self.device} with unit column stride")
        kw = dict(device=self.device, dtype=self.dtype)
        out = WalkEvaluation(t.empty((n, 4), **kw), t.empty((n,), **kw), t.empty((n,), device=self.device, dtype=t.int32), obs)
        stride = obs.stride(0) if n > 1 else max(obs.stride(0), obs.shape[1])
        self._check(self._L.ffe_walktask_evaluate(self._h, qpos.data_ptr(), qvel.data_ptr(), clip.data_ptr(), step.data_ptr(), n, out.factors.data_ptr(),
                                                  out.reward.data_ptr(), out.term_bits.data_ptr(), obs.data_ptr(), int(stride), self._stream()))
        return out

    def reference_pose(self, clip, step) -> WalkPose:
        """The state a reset onto row `step` of clip `clip` builds: qpos float64 [N, nq] (exact copies), qvel zeros [N, nv]."""
        t = self._torch
        clip = t.as_tensor(clip)
        n = clip.shape[0] if clip.dim() == 1 else -1
        clip, step = self._in(clip, t.int32, (n,), "clip"), self._in(step, t.int32, (n,), "step")
        out = WalkPose(t.empty((n, self.nq), device=self.device, dtype=t.float64), t.empty((n, self.nv), device=self.device, dtype=t.float64))
        self._check(self._L.ffe_walktask_reference_pose(self._h, clip.data_ptr(), step.data_ptr(), n, out.qpos.data_ptr(), out.qvel.data_ptr(),
                                                        self._stream()))
        return out

    def close(self):
        if self._h:
            self._torch.cuda.synchronize(self.device)
        super().close()
