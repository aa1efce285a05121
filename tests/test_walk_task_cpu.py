"""The walk_imitation task layer (flybody_amd/csrc/walk_task.hpp) compiled for the host in both scalar types by
tests/walk_task_host.cpp, against the float64 oracle (S1) and the numpy restatement (S2, S3) of tests/walk_task_states.py.  The same
header is what the HIP kernels run; tests/test_gpu_walk_task.py repeats these comparisons on the device with the same constants.

float32 bounds: 3 x the worst error measured in this host build over S1 / S2 / S3 (the project's convention, test_convex_f32_cpu.py).
Measured worst values, host build:
    features   qvel 9.4e-7   root2site 7.9e-8   joint_quat 3.8e-7 (S1, S2), 1.9e-5 (S3: full-range poses come within 0.06 rad of the
               -z discontinuity of quat_z2vec, which amplifies the float32 axis error by 1 / angle)
               all 102 hinges + 15 sites on 6 full-range poses: qvel 1.1e-7, root2site 5.2e-8, joint_quat 7.1e-6
    factors    3.5e-7 of max(1, value)      reward 8.0e-7 of max(1, value)
    obs        appendages_pos 6.3e-8   joints_pos 7.0e-9   joints_vel 3.1e-8   ref_displacement 5.1e-8   ref_root_quat 1.2e-7
               world_zaxis 3.1e-7   (each relative to the group's magnitude)
Two ceilings of the project hold whatever is measured: reward and factors 1e-5 of max(1, value), observation columns 1.4e-4.
"""
import ctypes as C

import numpy as np
import pytest

import walk_task_states as ST
from flybody_amd.tasks import walk_tracker as WT
from flybody_amd.tasks import walking as W

# ---- float64: the issue's figures
F64_FEATURES, F64_FACTORS, F64_OBS = 1e-10, 1e-9, 1e-10
# ---- float32: 3 x measured (see the module docstring), capped by the project's ceilings
CEIL_FACTORS, CEIL_OBS = 1e-5, 1.4e-4
F32_FEATURES = {"com": 0.0, "qvel": 2.9e-6, "root2site": 2.4e-7, "joint_quat": 1.2e-6}
F32_FEATURES_FULL_RANGE = {"com": 0.0, "qvel": 2.9e-6, "root2site": 2.4e-7, "joint_quat": 5.8e-5}
F32_FEATURES_ALL_TRACKED = {"com": 0.0, "qvel": 3.4e-7, "root2site": 1.6e-7, "joint_quat": 2.2e-5}
F32_FACTORS, F32_REWARD = 1.1e-6, 2.4e-6
F32_OBS = {"appendages_pos": 1.9e-7, "joints_pos": 2.1e-8, "joints_vel": 9.4e-8, "ref_displacement": 1.6e-7, "ref_root_quat": 3.5e-7,
           "world_zaxis": 9.3e-7}
assert F32_FACTORS <= CEIL_FACTORS and F32_REWARD <= CEIL_FACTORS and max(F32_OBS.values()) <= CEIL_OBS


@pytest.fixture(scope="module")
def s():
    return ST.sets()


@pytest.fixture(scope="module")
def build_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("walk_task_host")


@pytest.fixture(scope="module", params=["float64", "float32"])
def host(request, s, build_dir):
    h = ST.HostTask(build_dir, s.view, s.refs, dtype=request.param)
    h.dtype_name = request.param
    yield h
    h.close()


def check_features(got, want, bounds, what):
    err = ST.feature_errors(got, want)
    print(what, "feature errors", err)
    for k, e in err.items():
        assert e <= (bounds if isinstance(bounds, float) else bounds[k]), (what, k, e)


def test_no_state_sits_on_the_z2vec_discontinuity(s):
    assert s.left_out == 0 and s.min_axis_angle > ST.NEAR_MINUS_Z
    assert (len(s.s1.qpos), len(s.s2.qpos), len(s.s3.qpos)) == (39, 64, 64)


def test_features(host, s):
    f64 = host.dtype_name == "float64"
    check_features(host.features(s.s1.qpos, s.s1.qvel), s.s1.feat, F64_FEATURES if f64 else F32_FEATURES, "S1")
    check_features(host.features(s.s2.qpos, s.s2.qvel), s.s2.feat, F64_FEATURES if f64 else F32_FEATURES, "S2")
    check_features(host.features(s.s3.qpos, s.s3.qvel), s.s3.feat, F64_FEATURES if f64 else F32_FEATURES_FULL_RANGE, "S3")


def test_factors_and_reward(host, s):
    f64 = host.dtype_name == "float64"
    for name, S in (("S1", s.s1), ("S2", s.s2)):
        ev = host.evaluate(S.qpos, S.qvel, S.clip, S.step)
        if f64:  # relative to the value itself
            e = float((np.abs(ev.factors - S.factors) / np.abs(S.factors)).max())
            er = float((np.abs(ev.reward - S.reward) / np.abs(S.reward)).max())
            print(name, "factor / reward error, relative", e, er)
            assert e <= F64_FACTORS and er <= F64_FACTORS
        else:
            e, er = ST.factor_error(ev.factors, S.factors), ST.factor_error(ev.reward, S.reward)
            print(name, "factor / reward error, of max(1, value)", e, er)
            assert e <= F32_FACTORS and er <= F32_REWARD
        # inside the clip and within terminal_com_dist = 0.3 of the reference root: only the end-of-clip bit can be set
        assert np.array_equal(ev.term_bits, np.where(S.step == s.episode_steps[S.clip], 2, 0))


def test_kinematic_observation_columns(host, s):
    ev = host.evaluate(s.s1.qpos, s.s1.qvel, s.s1.clip, s.s1.step, fill=12345.0)
    groups = ST.oracle_obs_groups(s.layout)
    err = ST.obs_errors(ev.obs, s.s1.obs, host.obs_layout, groups)
    print("obs errors", err)
    for k, e in err.items():
        assert e <= (F64_OBS if host.dtype_name == "float64" else F32_OBS[k]), (k, e)
    written = np.zeros(host.obs_dim, bool)
    for o, n in host.obs_layout.values():
        written[o : o + n] = True
    assert written.sum() == 649
    assert (ev.obs[:, ~written] == 12345.0).all() and (ev.obs[:, written] != 12345.0).all()


def test_obs_layout_and_episode_steps_follow_the_oracle(host, s, build_dir):
    assert host.obs_layout == ST.oracle_obs_groups(s.layout) and host.obs_dim == 741
    assert list(host.episode_steps) == list(s.episode_steps)  # walk_imitation.py:99-100
    short = ST.HostTask(build_dir, s.view, s.refs, dtype=host.dtype_name, time_limit=0.05)  # round(0.05 / 2e-3) + 1 = 26 < every clip
    assert list(short.episode_steps) == [26, 26, 26]
    short.close()


def test_reference_pose_is_the_oracle_reset_state(host, s):
    first = np.flatnonzero(s.s1.step == 0)
    qpos, qvel = host.reference_pose(s.s1.clip[first], np.zeros(len(first), np.int32))
    assert np.array_equal(qpos, s.s1.qpos[first]) and not qvel.any()
    # any row: the pose full_qpos builds, the root quaternion normalised as the position stage leaves it
    qpos, _ = host.reference_pose([2, 0], [17, 40])
    for q, (c, k) in zip(qpos, ((2, 17), (0, 40))):
        want = s.view.full_qpos(s.refs.snippet(c)["qpos"][k])
        assert np.array_equal(np.delete(q, [3, 4, 5, 6]), np.delete(want, [3, 4, 5, 6])) and np.allclose(q[3:7], want[3:7], atol=3e-16, rtol=0)
    # on the pose, at step 0: position, end-effector and orientation factors are 20, 1, 1
    qpos, qvel = host.reference_pose([0, 1, 2], [0, 0, 0])
    f = host.evaluate(qpos, qvel, [0, 1, 2], [0, 0, 0]).factors.astype(np.float64)
    tol = F64_FACTORS if host.dtype_name == "float64" else F32_FACTORS
    assert np.abs(f[:, 0] - 20).max() <= 20 * tol and np.abs(f[:, 2:] - 1).max() <= tol


def test_termination_bits_follow_the_oracle_rule(s, build_dir):
    """walk_imitation.py:161-177 as the oracle states it: bit 0 |ref_root[step] - root| > terminal_com_dist, bit 1
    step == episode_steps, bit 2 step outside [0, episode_steps]."""
    for dt in ("float64", "float32"):
        h = ST.HostTask(build_dir, s.view, s.refs, dtype=dt, terminal_com_dist=0.035)
        S = s.s2
        ref_root = np.array([s.refs.snippet(c)["qpos"][k, :3] for c, k in zip(S.clip, S.step)])
        dist = np.linalg.norm(ref_root - S.qpos[:, :3], axis=1)
        want = (dist > 0.035).astype(np.int32) | np.where(S.step == s.episode_steps[S.clip], 2, 0)
        assert 8 < (dist > 0.035).sum() < 56  # both sides are exercised
        assert np.array_equal(h.evaluate(S.qpos, S.qvel, S.clip, S.step).term_bits, want)
        q, v = h.reference_pose([0] * 4 + [2] * 4, [35, 34, 36, -1, 69, 68, 70, -5])
        steps = np.array([35, 34, 36, -1, 69, 68, 70, -5], np.int32)
        got = h.evaluate(q, v, [0] * 4 + [2] * 4, steps).term_bits
        # (the pose of a clamped row sits on that row; for steps inside the clip it sits on the row itself: bit 0 stays clear)
        assert list(got & 6) == [2, 0, 4, 4, 2, 0, 4, 4] and not (got[[0, 1, 4, 5]] & 1).any()
        h.close()


def test_out_of_range_steps_never_leave_the_clip(host, s):
    host.row_record()
    for c in range(s.refs.ntraj):
        length = int(s.refs.off[c + 1] - s.refs.off[c])
        steps = np.concatenate([np.arange(s.episode_steps[c] + 1, length + 71), [-1, -70, 2**31 - 1, -(2**31)]]).astype(np.int32)
        clip = np.full(len(steps), c, np.int32)
        qpos, qvel = np.tile(s.s1.qpos[13 * c], (len(steps), 1)), np.tile(s.s1.qvel[13 * c], (len(steps), 1))
        ev = host.evaluate(qpos, qvel, clip, steps)
        assert ((ev.term_bits & 4) == 4).all() and np.isfinite(ev.obs).all() and np.isfinite(ev.reward).all()
        host.reference_pose(clip, steps)
        formed, outside, min_rel, max_rel_end = host.row_record()
        assert formed >= 67 * len(steps) and outside == 0 and min_rel == 0 and max_rel_end == -1, (c, formed, outside, min_rel, max_rel_end)
        # far past the end every preview row is the clip's last row
        o, n = host.obs_layout["ref_root_quat"]
        last = ev.obs[length + 70 - (s.episode_steps[c] + 1), o : o + n].reshape(65, 4)
        assert (last == last[0]).all()
    # a clip index outside the set is clamped too and flagged
    ev = host.evaluate(s.s1.qpos[:2], s.s1.qvel[:2], [-1, 3], [0, 0])
    assert ((ev.term_bits & 4) == 4).all() and host.row_record()[1] == 0


def test_every_hinge_and_every_site_can_be_tracked(s, build_dir):
    view = ST.all_hinges_view(s.view)
    assert len(view.mocap_jnt) == 102 and len(view.mocap_site) == 15
    qpos, qvel = ST.full_range_states(view, 6, 7)
    want = ST.stack_features([W.walker_features(view, q, v) for q, v in zip(qpos, qvel)])
    assert ST.min_angle_to_minus_z(want["joint_quat"]) > ST.NEAR_MINUS_Z  # 0 states left out
    for dt, bound in (("float64", F64_FEATURES), ("float32", F32_FEATURES_ALL_TRACKED)):
        h = ST.HostTask(build_dir, view, None, dtype=dt)
        assert (h.J, h.S, h.ntraj) == (102, 15, 0)
        check_features(h.features(qpos, qvel), want, bound, "all hinges " + dt)
        h.close()


def test_empty_tracked_set_in_inference_mode(s, build_dir):
    """`InferenceWalkingTrajectoryLoader`: root-only clips, the reward is the constant 1, the preview is still served."""
    snips = [W.inference_snippet(s.refs.snippet(c)["qpos"][:, :7], s.refs.snippet(c)["qvel"][:, :6]) for c in range(s.refs.ntraj)]
    none = np.zeros(0, np.int32)
    groups = ST.oracle_obs_groups(s.layout)
    for dt in ("float64", "float32"):
        h = ST.HostTask(build_dir, s.view, W.WalkRefSet(snips), dtype=dt, joints=none, sites=none, inference_mode=True)
        ev = h.evaluate(s.s1.qpos, s.s1.qvel, s.s1.clip, s.s1.step)
        assert (ev.reward == 1).all() and (ev.factors == 1).all()
        err = ST.obs_errors(ev.obs, s.s1.obs, h.obs_layout, groups)
        for k, e in err.items():
            assert e <= (F64_OBS if dt == "float64" else F32_OBS[k]), (k, e)
        f = h.features(s.s1.qpos[:3], s.s1.qvel[:3])
        assert f["qvel"].shape == (3, 6) and f["joint_quat"].shape == (3, 1, 4) and np.array_equal(f["joint_quat"][:, 0], s.s1.qpos[:3, 3:7].astype(h.np_dtype))
        h.close()


def test_quaternion_helpers_and_their_edge_branches(build_dir):
    """joint_orientation_quat on the reference's goldens and on axes exactly along +-z (the exact-zero branch of quat_z2vec);
    the squared short-arc distance next to 0, where acos of a float32 next to 1 would lose everything, and its min(1, .) clamp."""
    import os

    from flybody_amd.tasks import rewards as R

    L = ST.HostTask.lib(build_dir)
    g = np.load(os.path.join(ST.ROOT, "tests", "golden", "walker_features.npz"))

    def joq(axis, ang, f64):
        a, out = np.ascontiguousarray(axis, dtype=np.float64), np.zeros(4)
        L.wth_joint_orientation_quat(a.ctypes.data, float(ang), int(f64), out.ctypes.data)
        return out

    for axis, ang, want in zip(g["xaxis"], g["ang"], g["joint_orientation"]):
        assert np.abs(joq(axis, ang, True) - want).max() <= 1e-13 and np.abs(joq(axis, ang, False) - want).max() <= 1e-6
    for axis in ([0.0, 0.0, 1.0], [0.0, 0.0, -1.0], [0.0, 0.0, -2.5], [0.0, 0.0, 0.3]):
        for ang in (0.0, 0.7, -2.0):
            want = W.joint_orientation_quat(np.array(axis), ang)
            assert np.abs(joq(axis, ang, True) - want).max() <= 1e-15 and np.abs(joq(axis, ang, False) - want).max() <= 2e-7
    rng = np.random.RandomState(5)
    for ang in (0.0, 1e-7, 1e-4, 1e-2, 0.5, 2.0, 3.1):
        a = rng.randn(4)
        a /= np.linalg.norm(a)
        ax = rng.randn(3)
        b = ST.Q.mul(a, ST.Q.axis_angle(ax / np.linalg.norm(ax), ang)) * rng.choice([-1.0, 1.0]) * 1.7  # either sign, any norm
        arc = min(ang, 2 * np.pi - ang)
        pa, pb = a.ctypes.data, np.ascontiguousarray(b).ctypes.data
        assert abs(L.wth_short_arc_sq(pa, pb, 1) - arc**2) <= 1e-12 * max(arc**2, 1e-12) + 1e-22
        # float32: rounding the eight inputs moves |a - b| by up to 4 x 2^-24, the angle (2 |a - b| when small) by 5e-7 at the most;
        # past that the error is relative - where acos(1 - 2^-24) alone would be off by 3.5e-4 rad
        assert abs(L.wth_short_arc_sq(pa, pb, 0) - arc**2) <= 2 * arc * 5e-7 + 2.5e-13 + 2e-6 * arc**2
        if ang >= 1e-2:  # where the reference's own acos is still well-conditioned
            assert abs(R.quat_dist_short_arc(a, b) ** 2 - L.wth_short_arc_sq(pa, pb, 1)) <= 1e-12
    a = np.array([1.0, 0, 0, 0])
    assert L.wth_short_arc_sq(a.ctypes.data, a.ctypes.data, 0) == 0.0 and L.wth_short_arc_sq(a.ctypes.data, (-a).ctypes.data, 1) == 0.0


def test_table_packing(s, build_dir):
    h = ST.HostTask(build_dir, s.view, s.refs, dtype="float32")
    m = s.view.m
    depth = np.zeros(m.nbody, int)
    for b in range(1, m.nbody):
        depth[b] = depth[m.body_parentid[b]] + 1
    assert np.array_equal(h.table(0, np.int32), depth) and depth.max() == 9
    src, cst = h.table(1, np.int32), h.table(2, np.float64)
    want_src = np.full(s.view.nq, -1)
    want_src[:7] = np.arange(7)
    want_src[s.view.mocap_qadr] = 7 + np.arange(len(s.view.mocap_qadr))
    want_src[s.view.retract_qadr] = -1
    want_cst = m.qpos0.astype(np.float64).copy()
    want_cst[s.view.retract_qadr] = s.view.retract_val
    assert np.array_equal(src, want_src) and np.array_equal(cst[src < 0], want_cst[src < 0])
    assert np.array_equal(h.table(3, np.float64).reshape(-1, 7), s.refs.qpos[:, :7])  # the compact preview table, float64
    h.close()


def test_refusals_carry_a_text(s, build_dir):
    view, refs = s.view, s.refs
    mk = lambda **kw: ST.HostTask(build_dir, view, kw.pop("refs", refs), **kw)  # noqa: E731
    with pytest.raises(RuntimeError, match="tracked joint 0 is not a hinge"):
        mk(joints=np.array([0], np.int32), refs=None)
    with pytest.raises(RuntimeError, match=r"tracked joint index 103 is out of range \[0, 103\)"):
        mk(joints=np.array([5, 103], np.int32), refs=None)
    with pytest.raises(RuntimeError, match=r"tracked site index -1 is out of range \[0, 15\)"):
        mk(sites=np.array([-1], np.int32), refs=None)
    with pytest.raises(RuntimeError, match=r"clip 0 has 100 rows, fewer than future_steps \+ 2 = 101"):
        mk(future_steps=99)
    mk(future_steps=98).close()
    with pytest.raises(RuntimeError, match=r"override address 109 is out of range"):
        mk(overrides=(np.array([109]), np.array([0.0])))
    with pytest.raises(RuntimeError, match="std.0. must be positive"):
        mk(std=(0.0, 1.0, 1.0, 1.0))
    task, keep = WT.make_task(view, refs)
    task.ref_qvel = None
    with pytest.raises(RuntimeError, match="a null required pointer"):
        ST.HostTask(build_dir, view, refs, raw_task=C.addressof(task))
    with pytest.raises(RuntimeError, match="a null required pointer"):
        ST.HostTask(build_dir, view, refs, raw_task=0)
    # the Python packer refuses tables that do not match the tracked sets before anything reaches the library
    with pytest.raises(ValueError, match=r"refs.qpos has shape .351, 73.; 351 rows of 10 tracked joints"):
        WT.make_task(view, refs, joints=view.mocap_jnt[:10])
    with pytest.raises(ValueError, match="four values"):
        WT.make_task(view, refs, weights=(1, 1, 1))
    # an observation row narrower than the layout is refused by the evaluate call (the C ABI adds the text, checked on the device)
    h = mk(dtype="float32")
    with pytest.raises(AssertionError):
        h.evaluate(s.s1.qpos[:1], s.s1.qvel[:1], [0], [0], stride=740)
    h.close()


def test_float32_kernels_use_no_scratch():
    from flybody_amd import build

    usage = build.kernel_resource_usage("walk_task.hip", "walk_")
    f32 = {k: v for k, v in usage.items() if "IfE" in k}
    assert len(usage) == 6 and len(f32) == 3, sorted(usage)
    for k, v in usage.items():
        print(k, v)
    for k, v in f32.items():
        assert v["ScratchSize"] == 0, (k, v)
