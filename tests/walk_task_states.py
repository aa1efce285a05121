"""State sets and expected values shared by tests/test_walk_task_cpu.py (host build of csrc/walk_task.hpp) and
tests/test_gpu_walk_task.py (the kernels through `WalkTracker`): seeded, built once per session, identical on both sides.

 * S1: oracle rollouts - per clip a reset and 12 steps of RandomState(clip).uniform(-0.5, 0.5) actions on `OracleWalkEnv` with
   terminal_com_dist = inf; 39 states with the oracle's features, reward factors, reward and 741-float observation.  (The reset
   row's reward is the product of its factors: the env itself returns 0 on a FIRST step.)
 * S2: 64 states around rows of the clips, expected values from `walking.walker_features` + `rewards.reward_factors_deep_mimic`.
 * S3: 64 full-range poses, features only.

`quat_z2vec` is discontinuous where a joint axis in the root frame points along -z; that belongs to the reference.  States with a
tracked axis within 0.01 rad of -z would be left out; `left_out` counts them and the tests assert it is 0.
"""
import ctypes as C
import functools
import os
import subprocess
from types import SimpleNamespace

import numpy as np

from flybody_amd.model import quat as Q
from flybody_amd.tasks import rewards as R
from flybody_amd.tasks import walk_tracker as WT
from flybody_amd.tasks import walking as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLOB = os.path.join(ROOT, "flybody_amd", "assets", "fly_walk.ffmb")
WEIGHTS = (20, 1, 1, 1)
NEAR_MINUS_Z = 0.01


def min_angle_to_minus_z(joint_quat):
    """joint_quat [..., 1 + J, 4] -> the smallest angle (rad) between a tracked joint axis in the root frame and -z.  The axis is
    the image of z under the joint's orientation quaternion (z2vec takes z onto the axis, the hinge turn leaves it there)."""
    q = np.asarray(joint_quat)[..., 1:, :]
    if q.shape[-2] == 0:
        return np.inf
    w, x, y, z = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    az = (w * w - x * x - y * y + z * z) / (w * w + x * x + y * y + z * z)
    return float(np.arccos(np.clip(-az, -1, 1)).min())


def stack_features(fs):
    return {k: np.array([f[k] for f in fs]) for k in ("com", "qvel", "root2site", "joint_quat")}


def all_hinges_view(view):
    """The same model with every hinge joint and every site tracked."""
    import copy

    v = copy.copy(view)
    v.mocap_jnt = np.array([j for j in range(view.m.njnt) if view.m.jnt_type[j] == 3], dtype=np.int32)
    v.mocap_site = np.arange(len(view.m.sites_bodyid), dtype=np.int32)
    v.mocap_qadr, v.mocap_dadr = view.m.jnt_qposadr[v.mocap_jnt], view.m.jnt_dofadr[v.mocap_jnt]
    return v


def full_range_states(view, n, seed):
    rng = np.random.RandomState(seed)
    lo, hi = view.m.jnt_range[view.mocap_jnt].T
    qpos = np.tile(view.m.qpos0.astype(np.float64), (n, 1))
    qpos[:, view.mocap_qadr] = rng.uniform(lo, hi, (n, len(lo)))
    rq = rng.randn(n, 4)
    qpos[:, 3:7] = rq / np.linalg.norm(rq, axis=1, keepdims=True)
    qpos[:, :3] += rng.randn(n, 3)
    return qpos, rng.randn(n, view.nv)


@functools.lru_cache(maxsize=1)
def sets():
    from oracle import oracle as O

    view = W.WalkModelView()
    refs = W.WalkRefSet(W.synthetic_snippets(view, n=3, length=100))
    left_out = 0
    # ---- S1
    model = O.OracleModel(BLOB)
    rec = {k: [] for k in ("qpos", "qvel", "clip", "step", "feat", "factors", "reward", "obs")}
    layout = None
    for c in range(refs.ntraj):
        e = O.OracleWalkEnv(model, refs, view.mocap_jnt, view.mocap_site, (view.retract_qadr, view.retract_val), terminal_com_dist=float("inf"))
        layout = e.LAYOUT
        e.force_next(c)
        rng = np.random.RandomState(c)
        for k in range(13):
            st, r, d, obs = e.reset() if k == 0 else e.step(rng.uniform(-0.5, 0.5, e.naction))
            f4 = e.reward_factors(k)
            rec["qpos"].append(e.data.qpos.copy()); rec["qvel"].append(e.data.qvel.copy())
            rec["clip"].append(c); rec["step"].append(k)
            rec["feat"].append(e.features()); rec["factors"].append(f4)
            rec["reward"].append(float(np.prod(f4)) if k == 0 else r)
            rec["obs"].append(obs.copy())
    s1 = SimpleNamespace(qpos=np.array(rec["qpos"]), qvel=np.array(rec["qvel"]), clip=np.array(rec["clip"], dtype=np.int32),
                         step=np.array(rec["step"], dtype=np.int32), feat=stack_features(rec["feat"]), factors=np.array(rec["factors"]),
                         reward=np.array(rec["reward"]), obs=np.array(rec["obs"]))
    # ---- S2
    rng = np.random.RandomState(1234)
    ep = np.array([min(refs.off[c + 1] - refs.off[c] - 64 - 1, round(10.0 / 2e-3) + 1) for c in range(refs.ntraj)])
    qp, qv, cl, stp, fs, fac = [], [], [], [], [], []
    for i in range(64):
        c = int(rng.randint(refs.ntraj)); k = int(rng.randint(ep[c] + 1))
        sn = refs.snippet(c)
        q = view.full_qpos(sn["qpos"][k])
        q[view.mocap_qadr] += rng.normal(0, 0.05, len(view.mocap_qadr))
        q[:3] += rng.normal(0, 0.02, 3)
        ax = rng.randn(3)
        q[3:7] = Q.mul(q[3:7], Q.axis_angle(ax / np.linalg.norm(ax), 0.1))
        v = np.zeros(view.nv)
        v[:6] = sn["qvel"][k, :6] + rng.normal(0, 5, 6)
        v[view.mocap_dadr] = sn["qvel"][k, 6:] + rng.normal(0, 5, len(view.mocap_dadr))
        f = W.walker_features(view, q, v)
        if min_angle_to_minus_z(f["joint_quat"]) < NEAR_MINUS_Z:
            left_out += 1
            continue
        qp.append(q); qv.append(v); cl.append(c); stp.append(k); fs.append(f)
        fac.append(R.reward_factors_deep_mimic(f, R.get_reference_features(sn, k), weights=WEIGHTS))
    s2 = SimpleNamespace(qpos=np.array(qp), qvel=np.array(qv), clip=np.array(cl, dtype=np.int32), step=np.array(stp, dtype=np.int32),
                         feat=stack_features(fs), factors=np.array(fac), reward=np.prod(np.array(fac), axis=1))
    # ---- S3
    q3, v3 = full_range_states(view, 64, 4321)
    qp, qv, fs = [], [], []
    for q, v in zip(q3, v3):
        f = W.walker_features(view, q, v)
        if min_angle_to_minus_z(f["joint_quat"]) < NEAR_MINUS_Z:
            left_out += 1
            continue
        qp.append(q); qv.append(v); fs.append(f)
    s3 = SimpleNamespace(qpos=np.array(qp), qvel=np.array(qv), feat=stack_features(fs))
    min_axis_angle = min(min_angle_to_minus_z(s.feat["joint_quat"]) for s in (s1, s2, s3))
    return SimpleNamespace(view=view, refs=refs, s1=s1, s2=s2, s3=s3, left_out=left_out, min_axis_angle=min_axis_angle, episode_steps=ep,
                           layout=layout)


def oracle_obs_groups(layout):
    """{group: (offset, width)} of the kinematic columns in the oracle's observation row (OracleWalkEnv.LAYOUT)."""
    out, o = {}, 0
    for name, n in layout:
        if name in WT.OBS_GROUPS:
            out[name] = (o, n)
        o += n
    return out


# ---------------------------------------------------------------------------------------------------- error measures
def feature_errors(got, want):
    """max abs error per feature group (quaternions as they are: the kernel and the reference agree in sign)"""
    return {k: float(np.abs(np.asarray(got[k], dtype=np.float64) - want[k]).max()) if want[k].size else 0.0 for k in want}


def factor_error(got, want):
    """max over states and factors of |got - want| / max(1, want)"""
    got = np.asarray(got, dtype=np.float64)
    return float((np.abs(got - want) / np.maximum(1.0, np.abs(want))).max())


def obs_errors(got, want, groups_got, groups_want):
    """per kinematic group: max |got - want| / the group's magnitude (its largest |want|, at least 1)"""
    out = {}
    for name, (o, n) in groups_want.items():
        og, ng = groups_got[name]
        assert ng == n, name
        w = want[:, o : o + n]
        out[name] = float(np.abs(np.asarray(got[:, og : og + n], dtype=np.float64) - w).max() / max(1.0, np.abs(w).max()))
    return out


# ---------------------------------------------------------------------------------------------------- host build
class HostTask:
    """csrc/walk_task.hpp compiled for the host (tests/walk_task_host.cpp), one handle = one (task, scalar type)."""

    _lib = None

    @classmethod
    def lib(cls, build_dir):
        if cls._lib is None:
            out = os.path.join(str(build_dir), "libwalk_task_host.so")
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", out, os.path.join(ROOT, "tests", "walk_task_host.cpp")])
            L = C.CDLL(out)
            L.wth_create.restype = C.c_void_p
            L.wth_create.argtypes = [C.c_char_p, C.c_size_t, C.c_void_p, C.c_int, C.c_char_p, C.c_int]
            L.wth_destroy.argtypes = [C.c_void_p]
            vp = C.c_void_p
            L.wth_features.argtypes = [vp] * 2 + [vp, C.c_int] + [vp] * 4
            L.wth_evaluate.argtypes = [vp] * 5 + [C.c_int] + [vp] * 4 + [C.c_int]
            L.wth_reference_pose.argtypes = [vp, vp, vp, C.c_int, vp, vp]
            L.wth_info.argtypes = [vp, vp, vp]
            L.wth_table.argtypes = [vp, C.c_int, vp, C.c_int]
            L.wth_row_record.argtypes = [vp]
            L.wth_joint_orientation_quat.argtypes = [vp, C.c_double, C.c_int, vp]
            L.wth_short_arc_sq.argtypes = [vp, vp, C.c_int]
            L.wth_short_arc_sq.restype = C.c_double
            cls._lib = L
        return cls._lib

    def __init__(self, build_dir, view, refs, dtype="float64", raw_task=None, **kw):
        self.L = self.lib(build_dir)
        self.np_dtype = np.float64 if dtype == "float64" else np.float32
        if raw_task is None:
            task, self._keep = WT.make_task(view, refs, **kw)
            raw_task = C.addressof(task)
            self._task = task
        blob = open(BLOB, "rb").read()
        err = C.create_string_buffer(512)
        self.h = self.L.wth_create(blob, len(blob), raw_task, int(dtype == "float64"), err, 512)
        if not self.h:
            raise RuntimeError(err.value.decode())
        dims, ep = (C.c_int32 * 16)(), (C.c_int32 * max(1, refs.ntraj if refs is not None else 1))()
        self.L.wth_info(self.h, dims, ep)
        self.dims = list(dims)
        self.nq, self.nv, self.J, self.S, self.ntraj, self.future_steps, self.obs_dim = self.dims[:7]
        self.episode_steps = np.array(list(ep)[: self.ntraj], dtype=np.int32)
        self.obs_layout = WT.obs_layout(self.dims)

    @staticmethod
    def _p(a):
        return None if a is None else a.ctypes.data

    def features(self, qpos, qvel):
        qpos, qvel = np.ascontiguousarray(qpos, dtype=np.float64), np.ascontiguousarray(qvel, dtype=np.float64)
        n = len(qpos)
        out = {"com": np.zeros((n, 3)), "qvel": np.zeros((n, 6 + self.J), self.np_dtype), "root2site": np.zeros((n, self.S, 3), self.np_dtype),
               "joint_quat": np.zeros((n, 1 + self.J, 4), self.np_dtype)}
        self.L.wth_features(self.h, self._p(qpos), self._p(qvel), n, self._p(out["com"]), self._p(out["qvel"]), self._p(out["root2site"]),
                            self._p(out["joint_quat"]))
        return out

    def evaluate(self, qpos, qvel, clip, step, stride=None, fill=0.0):
        qpos, qvel = np.ascontiguousarray(qpos, dtype=np.float64), np.ascontiguousarray(qvel, dtype=np.float64)
        clip, step = np.ascontiguousarray(clip, dtype=np.int32), np.ascontiguousarray(step, dtype=np.int32)
        n = len(qpos)
        stride = stride or self.obs_dim
        out = SimpleNamespace(factors=np.zeros((n, 4), self.np_dtype), reward=np.zeros(n, self.np_dtype), term_bits=np.zeros(n, np.int32),
                              obs=np.full((n, stride), fill, self.np_dtype))
        rc = self.L.wth_evaluate(self.h, self._p(qpos), self._p(qvel), self._p(clip), self._p(step), n, self._p(out.factors), self._p(out.reward),
                                 self._p(out.term_bits), self._p(out.obs), stride)
        assert rc == 0
        return out

    def reference_pose(self, clip, step):
        clip, step = np.ascontiguousarray(clip, dtype=np.int32), np.ascontiguousarray(step, dtype=np.int32)
        qpos, qvel = np.full((len(clip), self.nq), np.nan), np.full((len(clip), self.nv), np.nan)
        self.L.wth_reference_pose(self.h, self._p(clip), self._p(step), len(clip), self._p(qpos), self._p(qvel))
        return qpos, qvel

    def table(self, which, dtype, cap=1 << 20):
        buf = np.zeros(cap, dtype)
        n = self.L.wth_table(self.h, which, self._p(buf), cap)
        assert n >= 0
        return buf[:n]

    def row_record(self):
        out = (C.c_longlong * 4)()
        self.L.wth_row_record(out)
        return list(out)

    def close(self):
        if self.h:
            self.L.wth_destroy(self.h)
            self.h = None
