"""The walk_imitation task layer on the device (flybody_amd/csrc/walk_task.hip through `WalkTracker` and the C ABI): the float64 and
the float32 handle on the state sets of tests/walk_task_states.py with the constants of tests/test_walk_task_cpu.py, then what only
the device can show - rows independent of their batch, columns it must not touch, NULL outputs, graph capture."""
import ctypes as C

import numpy as np
import pytest

import walk_task_states as ST
from test_walk_task_cpu import (F32_FACTORS, F32_FEATURES, F32_FEATURES_ALL_TRACKED, F32_FEATURES_FULL_RANGE, F32_OBS, F32_REWARD, F64_FACTORS,
                                F64_FEATURES, F64_OBS)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch

    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def s():
    return ST.sets()


@pytest.fixture(scope="module", params=["float64", "float32"])
def tracker(request, s, torch):
    from flybody_amd.tasks.walk_tracker import WalkTracker

    tr = WalkTracker(s.refs, s.view, dtype=request.param)
    tr.dtype_name = request.param
    yield tr
    tr.close()


@pytest.fixture(scope="module")
def tracker32(s, torch):
    from flybody_amd.tasks.walk_tracker import WalkTracker

    tr = WalkTracker(s.refs, s.view, dtype="float32")
    yield tr
    tr.close()


def feats(tr, qpos, qvel):
    f = tr.features(qpos, qvel)
    return {k: getattr(f, k).cpu().numpy() for k in f._fields}


def check_features(got, want, bounds, what):
    err = ST.feature_errors(got, want)
    print(what, "feature errors", err)
    for k, e in err.items():
        assert e <= (bounds if isinstance(bounds, float) else bounds[k]), (what, k, e)


def test_handle_dimensions_follow_the_oracle(tracker, s):
    assert (tracker.nq, tracker.nv, tracker.J, tracker.S, tracker.ntraj, tracker.obs_dim) == (109, 108, 66, 6, 3, 741)
    assert tracker.obs_layout == ST.oracle_obs_groups(s.layout) and list(tracker.episode_steps) == list(s.episode_steps)


def test_features(tracker, s):
    f64 = tracker.dtype_name == "float64"
    assert s.left_out == 0
    check_features(feats(tracker, s.s1.qpos, s.s1.qvel), s.s1.feat, F64_FEATURES if f64 else F32_FEATURES, "S1")
    check_features(feats(tracker, s.s2.qpos, s.s2.qvel), s.s2.feat, F64_FEATURES if f64 else F32_FEATURES, "S2")
    check_features(feats(tracker, s.s3.qpos, s.s3.qvel), s.s3.feat, F64_FEATURES if f64 else F32_FEATURES_FULL_RANGE, "S3")


def test_factors_reward_and_termination(tracker, s):
    f64 = tracker.dtype_name == "float64"
    for name, S in (("S1", s.s1), ("S2", s.s2)):
        ev = tracker.evaluate(S.qpos, S.qvel, S.clip, S.step)
        fac, rew = ev.factors.cpu().numpy().astype(np.float64), ev.reward.cpu().numpy().astype(np.float64)
        if f64:
            e, er = float((np.abs(fac - S.factors) / np.abs(S.factors)).max()), float((np.abs(rew - S.reward) / np.abs(S.reward)).max())
            print(name, "factor / reward error, relative", e, er)
            assert e <= F64_FACTORS and er <= F64_FACTORS
        else:
            e, er = ST.factor_error(fac, S.factors), ST.factor_error(rew, S.reward)
            print(name, "factor / reward error, of max(1, value)", e, er)
            assert e <= F32_FACTORS and er <= F32_REWARD
        assert np.array_equal(ev.term_bits.cpu().numpy(), np.where(S.step == s.episode_steps[S.clip], 2, 0))


def test_kinematic_observation_columns_and_sentinel(tracker, s, torch):
    """Row stride 768 over a buffer pre-filled with 12345: the 649 kinematic columns are written, the 92 physics columns and the 27
    padding floats keep the fill."""
    n = len(s.s1.qpos)
    buf = torch.full((n, 768), 12345.0, device=tracker.device, dtype=tracker.dtype)
    ev = tracker.evaluate(s.s1.qpos, s.s1.qvel, s.s1.clip, s.s1.step, obs=buf[:, :741])
    assert ev.obs.data_ptr() == buf.data_ptr()
    got = buf.cpu().numpy()
    err = ST.obs_errors(got, s.s1.obs, tracker.obs_layout, ST.oracle_obs_groups(s.layout))
    print("obs errors", err)
    for k, e in err.items():
        assert e <= (F64_OBS if tracker.dtype_name == "float64" else F32_OBS[k]), (k, e)
    written = np.zeros(768, bool)
    for o, w in tracker.obs_layout.values():
        written[o : o + w] = True
    assert written.sum() == 649 and (~written[:741]).sum() == 92
    assert (got[:, ~written] == 12345.0).all() and (got[:, written] != 12345.0).all()


def test_reference_pose_then_features_and_evaluate_at_step_zero(tracker, s, torch):
    first = np.flatnonzero(s.s1.step == 0)
    pose = tracker.reference_pose(s.s1.clip[first], np.zeros(len(first), np.int32))
    assert np.array_equal(pose.qpos.cpu().numpy(), s.s1.qpos[first]) and not pose.qvel.cpu().numpy().any()  # the oracle's reset state, exactly
    clip = torch.arange(3, dtype=torch.int32, device=tracker.device)
    ev = tracker.evaluate(pose.qpos, pose.qvel, clip, torch.zeros_like(clip))
    f = ev.factors.cpu().numpy().astype(np.float64)
    tol = F64_FACTORS if tracker.dtype_name == "float64" else F32_FACTORS
    assert np.abs(f[:, 0] - 20).max() <= 20 * tol and np.abs(f[:, 2:] - 1).max() <= tol
    ft = feats(tracker, pose.qpos, pose.qvel)
    want = np.array([s.refs.snippet(c)["root2site"][0] for c in range(3)])
    assert np.abs(ft["root2site"] - want).max() <= (F64_FEATURES if tracker.dtype_name == "float64" else F32_FEATURES["root2site"])
    o, w = tracker.obs_layout["ref_displacement"]
    assert np.abs(ev.obs[:, o : o + 3].cpu().numpy()).max() <= 1e-12


@pytest.mark.parametrize("n", [1, 63, 64, 65, 200])
def test_rows_do_not_depend_on_their_batch(tracker32, s, torch, n):
    """States cycled, clips and steps permuted: every output row is bit-identical to that state evaluated alone."""
    tr = tracker32
    pool_q, pool_v = np.concatenate([s.s1.qpos, s.s2.qpos]), np.concatenate([s.s1.qvel, s.s2.qvel])
    rng = np.random.RandomState(n)
    idx = np.arange(n) % len(pool_q)
    clip = rng.permutation(np.arange(n) % 3).astype(np.int32)
    step = rng.permutation(np.arange(n) % 36).astype(np.int32)
    dev = lambda a: torch.as_tensor(a, device=tr.device)  # noqa: E731
    q, v, c, k = dev(pool_q[idx]), dev(pool_v[idx]), dev(clip), dev(step)
    ev, ft = tr.evaluate(q, v, c, k), tr.features(q, v)
    together = [x.cpu().numpy() for x in (*ev, *ft)]
    alone = [[] for _ in together]
    for i in range(n):
        e1, f1 = tr.evaluate(q[i : i + 1], v[i : i + 1], c[i : i + 1], k[i : i + 1]), tr.features(q[i : i + 1], v[i : i + 1])
        for dst, x in zip(alone, (*e1, *f1)):
            dst.append(x)
    for name, a, b in zip(ev._fields + ft._fields, together, alone):
        b = torch.cat(b).cpu().numpy()
        assert a.tobytes() == b.tobytes(), name


def test_null_outputs_are_skipped(tracker32, s, torch):
    from flybody_amd import _capi

    tr, L = tracker32, _capi.lib()
    dev = lambda a, dt: torch.as_tensor(a, device=tr.device, dtype=dt)  # noqa: E731
    n = 9
    q, v = dev(s.s1.qpos[:n], torch.float64), dev(s.s1.qvel[:n], torch.float64)
    c, k = dev(s.s1.clip[:n], torch.int32), dev(s.s1.step[:n], torch.int32)
    stream = tr._stream()

    def run_eval(skip):
        out = [torch.full((n, 4), -7.0, device=tr.device), torch.full((n,), -7.0, device=tr.device),
               torch.full((n,), -7, device=tr.device, dtype=torch.int32), torch.full((n, 741), -7.0, device=tr.device)]
        p = [None if i == skip else x.data_ptr() for i, x in enumerate(out)]
        assert L.ffe_walktask_evaluate(tr._h, q.data_ptr(), v.data_ptr(), c.data_ptr(), k.data_ptr(), n, p[0], p[1], p[2], p[3], 741, stream) == 0
        return [x.cpu().numpy() for x in out]

    def run_feat(skip):
        out = [torch.full((n, 3), -7.0, device=tr.device, dtype=torch.float64), torch.full((n, 6 + tr.J), -7.0, device=tr.device),
               torch.full((n, tr.S, 3), -7.0, device=tr.device), torch.full((n, 1 + tr.J, 4), -7.0, device=tr.device)]
        p = [None if i == skip else x.data_ptr() for i, x in enumerate(out)]
        assert L.ffe_walktask_features(tr._h, q.data_ptr(), v.data_ptr(), n, p[0], p[1], p[2], p[3], stream) == 0
        return [x.cpu().numpy() for x in out]

    for run in (run_eval, run_feat):
        full = run(-1)
        for skip in range(4):
            got = run(skip)
            for i in range(4):
                if i == skip:
                    assert (got[i] == -7).all()
                else:
                    assert got[i].tobytes() == full[i].tobytes(), (run.__name__, skip, i)
    # reference_pose: either output alone
    a = torch.full((n, tr.nq), -7.0, device=tr.device, dtype=torch.float64)
    assert L.ffe_walktask_reference_pose(tr._h, c.data_ptr(), k.data_ptr(), n, a.data_ptr(), None, stream) == 0
    assert np.array_equal(a.cpu().numpy(), tr.reference_pose(c, k).qpos.cpu().numpy())


def test_refusals_carry_a_text(tracker32, s, torch):
    from flybody_amd import _capi
    from flybody_amd.tasks.walk_tracker import WalkTracker

    tr, L = tracker32, _capi.lib()
    q = torch.as_tensor(s.s1.qpos[:1], device=tr.device)
    v = torch.as_tensor(s.s1.qvel[:1], device=tr.device)
    z = torch.zeros(1, dtype=torch.int32, device=tr.device)
    obs = torch.zeros((1, 740), device=tr.device)
    assert L.ffe_walktask_evaluate(tr._h, q.data_ptr(), v.data_ptr(), z.data_ptr(), z.data_ptr(), 1, None, None, None, obs.data_ptr(), 740, tr._stream()) != 0
    assert b"obs_stride 740 is below the observation row of 741" in L.ffe_walktask_last_error(tr._h)
    assert L.ffe_walktask_evaluate(tr._h, q.data_ptr(), None, z.data_ptr(), z.data_ptr(), 1, None, None, None, None, 741, tr._stream()) != 0
    assert b"a null required pointer" in L.ffe_walktask_last_error(tr._h)
    with pytest.raises(RuntimeError, match="tracked joint 0 is not a hinge"):
        WalkTracker(None, s.view, joints=np.array([0], np.int32))
    with pytest.raises(RuntimeError, match=r"clip 0 has 100 rows, fewer than future_steps \+ 2 = 101"):
        WalkTracker(s.refs, s.view, future_steps=99)
    with pytest.raises(RuntimeError, match="created without reference clips"):
        t0 = WalkTracker(None, s.view)
        try:
            t0.evaluate(q, v, z, z)
        finally:
            t0.close()


def test_termination_bits_with_a_margin_float32_cannot_flip(tracker32, s, torch):
    tr = tracker32  # terminal_com_dist = 0.3
    ep = int(s.episode_steps[0])
    rng = np.random.RandomState(3)
    steps = np.array([5, 5, ep, ep - 1, ep + 1], np.int32)
    clip = np.zeros(5, np.int32)
    pose = tr.reference_pose(clip, steps)
    q = pose.qpos.cpu().numpy()
    for i, d in enumerate((0.29, 0.31)):
        u = rng.randn(3)
        q[i, :3] += d * u / np.linalg.norm(u)
    bits = tr.evaluate(q, pose.qvel, clip, steps).term_bits.cpu().numpy()
    assert list(bits) == [0, 1, 2, 0, 4]  # (step ep + 1 reads the row ep + 1, which the clip still has: bit 0 stays clear)


def test_every_hinge_and_every_site_can_be_tracked(s, torch):
    from flybody_amd.tasks import walking as W
    from flybody_amd.tasks.walk_tracker import WalkTracker

    view = ST.all_hinges_view(s.view)
    qpos, qvel = ST.full_range_states(view, 6, 7)
    want = ST.stack_features([W.walker_features(view, q, v) for q, v in zip(qpos, qvel)])
    assert ST.min_angle_to_minus_z(want["joint_quat"]) > ST.NEAR_MINUS_Z
    for dt, bound in (("float64", F64_FEATURES), ("float32", F32_FEATURES_ALL_TRACKED)):
        tr = WalkTracker(None, view, joints=view.mocap_jnt, sites=view.mocap_site, dtype=dt)
        assert (tr.J, tr.S) == (102, 15)
        check_features(feats(tr, qpos, qvel), want, bound, "all hinges " + dt)
        tr.close()


def test_featurize_reproduces_the_reference_tables(s, torch):
    from flybody_amd.tasks import walking as W

    sn = s.refs.snippet(1)
    got = W.featurize(s.view, sn["qpos"], sn["qvel"], [0, 60, len(sn["qpos"])])
    assert got.ntraj == 2 and list(got.off) == [0, 60, len(sn["qpos"])]
    assert np.abs(got.root2site - sn["root2site"]).max() <= 1e-10 and np.abs(got.joint_quat - sn["joint_quat"]).max() <= 1e-10
    assert np.array_equal(got.qpos, sn["qpos"]) and np.array_equal(got.qvel, sn["qvel"])


def test_evaluate_replays_from_a_captured_graph(tracker32, s, torch):
    tr = tracker32
    dev = lambda a, dt: torch.as_tensor(a, device=tr.device, dtype=dt).clone()  # noqa: E731
    n = 16
    q, v = dev(s.s2.qpos[:n], torch.float64), dev(s.s2.qvel[:n], torch.float64)
    c, k = dev(s.s2.clip[:n], torch.int32), dev(s.s2.step[:n], torch.int32)
    obs = torch.zeros((n, 741), device=tr.device)
    side = torch.cuda.Stream(device=tr.device)
    side.wait_stream(torch.cuda.current_stream(tr.device))
    with torch.cuda.stream(side):
        tr.evaluate(q, v, c, k, obs=obs)
    torch.cuda.current_stream(tr.device).wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ev = tr.evaluate(q, v, c, k, obs=obs)
    for lo in (16, 32):  # two replays, the inputs rewritten in place
        q.copy_(dev(s.s2.qpos[lo : lo + n], torch.float64)); v.copy_(dev(s.s2.qvel[lo : lo + n], torch.float64))
        c.copy_(dev(s.s2.clip[lo : lo + n], torch.int32)); k.copy_(dev(s.s2.step[lo : lo + n], torch.int32))
        g.replay()
        torch.cuda.synchronize(tr.device)
        replayed = [x.cpu().numpy().copy() for x in ev]
        eager = tr.evaluate(q, v, c, k)
        for name, a, b in zip(ev._fields, replayed, eager):
            assert a.tobytes() == b.cpu().numpy().tobytes(), name
