"""GPU parity tests of the walk_imitation environment with the floor off (csrc/walk_env.hip `imitation_step_kernel` and the episode
kernels around it, through `BatchedWalkEnv` and the C ABI) against the float64 oracle on identical
inputs.  Run with `-m gpu` on an MI355X.  No batch exceeds 24.  The oracle runs with FO_NO_CONTACT plus the case's force switches;
the opt-in bits are never passed to it.  Snippets: `synthetic_snippets(view, n=3, length=100)`, lengths 100 / 117 / 134, so the clips'
episodes end on control steps 35 / 52 / 69.  No case is excluded from any comparison.

Errors are per group, relative to max(1, max |reference| of the group) over the rows compared.  Bounds:
  state groups                     CAP10 of tests/test_gpu_walk_limits.py
  observation groups and reward    TOL of tests/test_gpu_ball.py (the same quantities on the tethered fly)
  ref_displacement, ref_root_quat  (not in TOL: the ball has no reference) from the state caps.  ref_root_quat = conj(q) r with |r| = 1
                                   is linear in the root quaternion: at most 2 x CAP10["root_quat"] = 4e-5.  ref_displacement =
                                   R(q)' (r - p): CAP10["root_pos"] for p plus the rotation's error 4 x CAP10["root_quat"] on a vector
                                   the normalisation already divides by, 2e-5 + 8e-5 = 1e-4
  accelerometer, gyro, velocimeter (exact zeros on the tethered fly, live here) 3 x the worst value measured on the MI355X, never above
                                   CAP10["root_lin"] (velocimeter), CAP10["root_ang"] (gyro) and 1e-2 (accelerometer)
Measured on the MI355X (teacher-forced step, reset row; both gravity settings, worst of all rows):
  accelerometer 7.088e-6 (floating; 1.063e-6 falling, 5.6e-7 on a reset row)   gyro 1.044e-6   velocimeter 1.456e-7
  reward 1.811e-7 (teacher-forced), 3.414e-7 (open loop over 69 steps, test 4); episode returns of test 8: 1.2e-7
and the other groups, all inside their caps: actuator_activation 3.5e-8, appendages_pos 5.6e-8, joints_pos 2.5e-8, joints_vel 2.4e-7,
ref_displacement 2.2e-7, ref_root_quat 1.5e-7, world_zaxis 2.6e-7; force and touch are exactly 0.  The reward is asserted at 3 x its
measured value as well, never above TOL["reward"]."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import ROOT
from test_gpu_ball import TOL
from test_gpu_walk_limits import CAP10

pytestmark = pytest.mark.gpu

BLOB = os.path.join(ROOT, "flybody_amd", "assets", "fly_walk.ffmb")
NO_GRAVITY, NO_CONTACT, NO_LIMIT, WALK_JOINT_LIMITS, WALK_EPISODES = 16, 64, 2, 512, 1024
IMU_MEASURED = {"accelerometer": 7.1e-6, "gyro": 1.05e-6, "velocimeter": 1.5e-7}
IMU_CAP = {"accelerometer": 1e-2, "gyro": CAP10["root_ang"], "velocimeter": CAP10["root_lin"]}
REWARD_MEASURED, REWARD_OPEN_MEASURED = 1.9e-7, 3.5e-7
OBS_TOL = dict({k: v for k, v in TOL.items() if k not in ("reward", "ball_qvel")},
               ref_root_quat=2 * CAP10["root_quat"], ref_displacement=CAP10["root_pos"] + 4 * CAP10["root_quat"])
EP_STEPS = (35, 52, 69)
SENTINEL = -12345.0


def bound(group):
    if group in IMU_MEASURED:
        assert 3 * IMU_MEASURED[group] <= IMU_CAP[group]
        return 3 * IMU_MEASURED[group]
    return OBS_TOL[group]


@pytest.fixture(scope="module")
def torch_mod():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


@pytest.fixture(scope="module")
def world():
    """(view, refs): the walk model's tracked sets and the three synthetic clips every test shares."""
    from flybody_amd.tasks import walking as W

    view = W.WalkModelView()
    return view, W.WalkRefSet(W.synthetic_snippets(view, n=3, length=100))


def make_env(world, B, flags=0, **kw):
    from flybody_amd.batched_env import BatchedWalkEnv

    return BatchedWalkEnv(world[1], world[0], batch_size=B, physics_flags=flags, **kw)


def make_oracle(world, flags=0, **kw):
    from oracle import oracle as O

    view, refs = world
    m = O.OracleModel(BLOB)
    m.set_flags(NO_CONTACT | flags)
    return O.OracleWalkEnv(m, refs, view.mocap_jnt, view.mocap_site, (view.retract_qadr, view.retract_val), **kw)


def split(layout, row):
    out, o = {}, 0
    for name, n in layout:
        out[name] = np.asarray(row[..., o:o + n], dtype=np.float64)
        o += n
    assert o == row.shape[-1]
    return out


def group_errors(layout, got, ref):
    """{group: max |got - ref| / max(1, max |ref|)} over all rows of [N, 741] arrays."""
    g, r = split(layout, np.asarray(got)), split(layout, np.asarray(ref))
    return {k: float(np.abs(g[k] - r[k]).max() / max(1.0, np.abs(r[k]).max())) for k in r}


def check_groups(layout, got, ref, what):
    err = group_errors(layout, got, ref)
    print(what, " ".join(f"{k} {v:.3e}" for k, v in err.items()))
    g = split(layout, np.asarray(got))
    assert not g["force"].any() and not g["touch"].any()  # exact zeros: no contacts
    for k, v in err.items():
        assert v <= bound(k), (what, k, v, bound(k))
    return err


def rel(got, ref):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.abs(got - ref).max() / max(1.0, np.abs(ref).max()))


def host(ts):
    return (ts.step_type.cpu().numpy().copy(), ts.reward.cpu().numpy().copy(), ts.discount.cpu().numpy().copy())


def actions(seed, n, amplitude, sign_only=False):
    rs = np.random.RandomState(seed)
    if sign_only:
        return [(amplitude * rs.choice([-1.0, 1.0], 59)).astype(np.float32) for _ in range(n)]
    return [(amplitude * rs.uniform(-1.0, 1.0, 59)).astype(np.float32) for _ in range(n)]


# ------------------------------------------------------------------------------------------------ 1. reset row
@pytest.mark.parametrize("pad", [False, True])
def test_reset_row(torch_mod, world, pad):
    torch = torch_mod
    env = make_env(world, 3, pad_first_obs=pad)
    for s in env._sets:
        s[0].fill_(SENTINEL)
    env.set_next_trajectory_index(np.arange(3))
    ts = env.reset()
    st, rew, disc = host(ts)
    obs = env.flat_observation.cpu().numpy()
    assert st.tolist() == [0, 0, 0] and rew.tolist() == [0.0, 0.0, 0.0] and disc.tolist() == [1.0, 1.0, 1.0]
    assert obs.shape == (3, 741) and not (obs == SENTINEL).any() and np.isfinite(obs).all()
    q, v = (x.cpu().numpy() for x in env.get_state())
    a = env.get_act().cpu().numpy()
    ints = env.get_task_state()[0].cpu().numpy()
    ref_obs = []
    for clip in range(3):
        o = make_oracle(world)
        o.set_pad_first_obs(pad)
        o.force_next(clip)
        rst, rr, rd, ro = o.reset()
        assert (rst, rr, rd) == (0, 0.0, 1.0)
        ref_obs.append(ro)
        layout = o.LAYOUT
        assert np.abs(q[clip, :3] - o.data.qpos[:3]).max() <= CAP10["root_pos"] and np.abs(q[clip, 7:] - o.data.qpos[7:]).max() <= CAP10["hinge_qpos"]
        assert np.abs(q[clip, 3:7] - o.data.qpos[3:7]).max() <= CAP10["root_quat"]
        assert not v[clip].any() and not a[clip].any() and not o.data.qvel.any() and not o.data.act.any()
    assert ints[:, 0].tolist() == [0, 1, 2] and not ints[:, 1].any() and not ints[:, 3].any()
    check_groups(layout, obs, np.stack(ref_obs), f"reset pad={pad}")
    env.close()


# ------------------------------------------------------------------------------------------------ 2. one control step, teacher-forced
SAMPLE_STEPS = (0, 2, 4, 7, 10, 14, 19, 27)  # under gravity the step from 27 is the one on which |velocimeter| passes 50 (49.0 -> 50.6 in the oracle)


def oracle_samples(world, flags):
    """Per clip, states along a +-0.5 rollout at SAMPLE_STEPS with the action and the outcome of the step that follows: 24 in all."""
    out = []
    for clip in range(3):
        o = make_oracle(world, flags, terminal_com_dist=np.inf)
        o.force_next(clip)
        o.reset()
        acts = actions(100 + clip, SAMPLE_STEPS[-1] + 1, 0.5)
        for k in range(SAMPLE_STEPS[-1] + 1):
            state = (o.data.qpos.copy(), o.data.qvel.copy(), o.data.act.copy())
            res = o.step(acts[k])
            if k in SAMPLE_STEPS:
                out.append(dict(clip=clip, step=k, state=state, action=acts[k], st=res[0], reward=res[1], discount=res[2], obs=res[3].copy()))
            assert res[0] == 1 or k == SAMPLE_STEPS[-1]
        layout = o.LAYOUT
    return out, layout


@pytest.mark.parametrize("flags,name", [(0, "gravity"), (NO_GRAVITY, "no_gravity")])
def test_one_control_step_teacher_forced(torch_mod, world, flags, name):
    torch = torch_mod
    samples, layout = oracle_samples(world, flags)
    B = len(samples)
    assert B == 24
    env = make_env(world, B, flags, terminal_com_dist=np.inf)
    env.reset()
    env.set_next_trajectory_index(np.array([s["clip"] for s in samples]))
    steps = np.array([s["step"] for s in samples])
    zero = torch.zeros(B, 59, device="cuda")
    T = int(steps.max())
    for t in range(T + 1):  # env i restarts T - steps[i] calls in, so that its counter stands at steps[i] when the loop ends
        mask = steps == T - t
        if mask.any():
            env.reset_envs(torch.tensor(mask, device="cuda"))
        if t < T:
            env.step(zero)
    ints = env.get_task_state()[0].cpu().numpy()
    assert ints[:, 0].tolist() == [s["clip"] for s in samples] and ints[:, 1].tolist() == steps.tolist() and not ints[:, 3].any()
    env.set_state(torch.tensor(np.stack([s["state"][0] for s in samples])), torch.tensor(np.stack([s["state"][1] for s in samples])))
    env.set_act(torch.tensor(np.stack([s["state"][2] for s in samples])))
    ts = env.step(torch.tensor(np.stack([s["action"] for s in samples]), device="cuda"))
    st, rew, disc = host(ts)
    obs = env.flat_observation.cpu().numpy()
    assert st.tolist() == [s["st"] for s in samples] and disc.tolist() == [s["discount"] for s in samples]
    if flags == 0:  # the free fall passes 50 cm/s on step 28 of every clip: LAST with discount 0 through the velocimeter rule
        assert [s["st"] for s in samples if s["step"] == 27] == [2, 2, 2] and [s["discount"] for s in samples if s["step"] == 27] == [0.0] * 3
    rerr = rel(rew, [s["reward"] for s in samples])
    print(f"{name}: reward {rerr:.3e} (measured {REWARD_MEASURED:.1e})")
    check_groups(layout, obs, np.stack([s["obs"] for s in samples]), name)
    assert 3 * REWARD_MEASURED <= TOL["reward"] and rerr <= 3 * REWARD_MEASURED
    env.close()


# ------------------------------------------------------------------------------------------------ 3. distance termination, auto-reset
def test_distance_termination_and_clip_draws(torch_mod, world):
    """Free fall leaves the reference root behind: 0.280 cm on control step 12, 0.327 on step 13 against terminal_com_dist = 0.3."""
    torch = torch_mod
    amps = (0.0, 0.3, 1.0)
    B, seed, base, nsteps = 9, 5, 40, 3 * 14 + 4
    env = make_env(world, B, seed=seed, env_id_base=base)
    oracles = [make_oracle(world, seed=seed, env_id=base + i) for i in range(B)]
    acts = [actions(200 + i, nsteps, amps[i % 3]) for i in range(B)]
    ts = env.reset()
    refs = [o.reset() for o in oracles]
    clips, lasts = [[] for _ in range(B)], [[] for _ in range(B)]
    for k in range(nsteps + 1):
        st, rew, disc = host(ts)
        ints = env.get_task_state()[0].cpu().numpy()
        for i in range(B):
            assert (st[i], disc[i]) == (refs[i][0], refs[i][2]), (k, i)
            assert ints[i, 0] == oracles[i].traj_idx, (k, i)
            if st[i] == 0:
                assert rew[i] == 0.0 and disc[i] == 1.0 and ints[i, 1] == 0
                clips[i].append(int(ints[i, 0]))
            if st[i] == 2:
                assert disc[i] == 0.0 and ints[i, 1] == 13, (k, i, ints[i])
                lasts[i].append(k)
        if k == nsteps:
            break
        ts = env.step(torch.tensor(np.stack([acts[i][k] for i in range(B)]), device="cuda"))
        refs = [oracles[i].step(acts[i][k]) for i in range(B)]
    from oracle import oracle as O

    for i in range(B):
        assert lasts[i] == [13, 27, 41], (i, lasts[i])  # LAST on control step 13 of each episode, FIRST on the call after it
        assert len(clips[i]) == 4 and clips[i] == [O.rng_u64(seed, base + i, ep, 0) % 3 for ep in range(4)], (i, clips[i])
    assert len({tuple(c) for c in clips}) > 1  # the envs do not share one sequence
    env.close()


# ------------------------------------------------------------------------------------------------ 4. end of snippet
def test_end_of_snippet(torch_mod, world):
    """Floating (FFE_NO_GRAVITY) with the distance rule off, +-1.0 actions: |velocimeter| < 0.13 and |gyro| < 4.7 over the run, so the
    only rule that fires is the end of the clip, with discount 1."""
    torch = torch_mod
    env = make_env(world, 3, NO_GRAVITY, terminal_com_dist=np.inf)
    oracles = [make_oracle(world, NO_GRAVITY, terminal_com_dist=np.inf) for _ in range(3)]
    env.set_next_trajectory_index(np.arange(3))
    for i, o in enumerate(oracles):
        o.force_next(i)
        o.reset()
    env.reset()
    acts = [actions(300 + i, 70, 1.0, sign_only=True) for i in range(3)]
    done, worst = [None] * 3, 0.0
    for k in range(1, 71):
        ts = env.step(torch.tensor(np.stack([acts[i][k - 1] for i in range(3)]), device="cuda"))
        st, rew, disc = host(ts)
        for i in range(3):
            if done[i] is not None:
                continue
            rst, rr, rd, _ = oracles[i].step(acts[i][k - 1])
            assert (st[i], disc[i]) == (rst, rd), (k, i)
            worst = max(worst, abs(float(rew[i]) - rr) / max(1.0, abs(rr)))
            if st[i] == 2:
                assert disc[i] == 1.0
                done[i] = k
    print(f"open-loop reward error {worst:.3e} (measured {REWARD_OPEN_MEASURED:.1e})")
    assert tuple(done) == EP_STEPS
    # open loop the states drift apart by rounding alone (no contacts, nothing discontinuous): the one-step cap holds along the way
    assert 3 * REWARD_OPEN_MEASURED <= TOL["reward"] and worst <= 3 * REWARD_OPEN_MEASURED
    env.close()


# ------------------------------------------------------------------------------------------------ 5. reset_envs(mask)
def _rows(env, ts):
    q, v = env.get_state()
    return [x.cpu().numpy().tobytes() for x in (env.flat_observation, ts.reward, ts.discount, ts.step_type, q, v, env.get_act())]


def test_reset_envs_restarts_only_the_masked(torch_mod, world):
    torch = torch_mod
    B = 8
    acts = [torch.tensor(np.stack(a), device="cuda") for a in zip(*[actions(400 + i, 10, 0.5) for i in range(B)])]
    mask = np.array([0, 1, 0, 0, 1, 1, 0, 0], dtype=bool)

    def run(masked):
        env = make_env(world, B, seed=3)
        env.reset()
        out = []
        for k in range(10):
            if k == 5 and masked:
                ts = env.reset_envs(torch.tensor(mask, device="cuda"))
                st = ts.step_type.cpu().numpy()
                ints = env.get_task_state()[0].cpu().numpy()
                assert (st[mask] == 0).all() and (st[~mask] == 1).all() and not ints[mask, 1].any() and (ints[~mask, 1] == 5).all()
                assert not ts.reward.cpu().numpy()[mask].any() and (ts.discount.cpu().numpy()[mask] == 1).all()
            ts = env.step(acts[k])
            obs = env.flat_observation.cpu().numpy()
            q, v = (x.cpu().numpy() for x in env.get_state())
            out.append([obs, ts.reward.cpu().numpy().copy(), ts.discount.cpu().numpy().copy(), ts.step_type.cpu().numpy().copy(), q, v,
                        env.get_act().cpu().numpy(), env.get_task_state()[0].cpu().numpy()])
        env.close()
        return out

    a, b = run(False), run(True)
    for k in range(10):
        for x, y in zip(a[k], b[k]):
            assert x[~mask].tobytes() == y[~mask].tobytes(), k  # the others go on bit for bit
        if k >= 5:
            assert (b[k][7][mask, 1] == k - 4).all() and (a[k][7][mask, 1] == k + 1).all()  # the masked envs count from their restart
            assert not np.array_equal(a[k][0][mask], b[k][0][mask])


# ------------------------------------------------------------------------------------------------ 6. batch independence
def test_rows_do_not_depend_on_the_batch(torch_mod, world):
    torch = torch_mod
    n, slot = 20, 7  # 20 steps under gravity: across the auto-reset on step 14, so the clip draw is part of the row
    mine = actions(500, n, 0.5)
    others = [actions(501 + i, n, 1.0) for i in range(16)]

    def run(B, base, at):
        env = make_env(world, B, seed=9, env_id_base=base)
        env.reset()
        out = []
        for k in range(n):
            a = np.stack([mine[k] if i == at else others[i][k] for i in range(B)])
            ts = env.step(torch.tensor(a, device="cuda"))
            q, v = env.get_state()
            out.append(b"".join(x[at].cpu().numpy().tobytes() for x in (env.flat_observation, ts.reward, ts.discount, ts.step_type, q, v,
                                                                         env.get_task_state()[0])))
        steps = [int(np.frombuffer(o[741 * 4 + 8:741 * 4 + 12], dtype=np.int32)[0]) for o in out]
        env.close()
        return out, steps

    alone, st1 = run(1, slot, 0)
    among, st16 = run(16, 0, slot)
    assert st1 == st16 and 2 in st1 and 0 in st1
    assert alone == among


# ------------------------------------------------------------------------------------------------ 7. graph capture
def test_step_replays_from_a_captured_graph(torch_mod, world):
    torch = torch_mod
    B = 8
    eager, graphed = make_env(world, B, seed=2), make_env(world, B, seed=2)
    acts = [torch.tensor(np.stack(a), device="cuda") for a in zip(*[actions(600 + i, 18, 0.5) for i in range(B)])]
    buf = acts[0].clone()
    eager.reset(); graphed.reset()
    side = torch.cuda.Stream(device=graphed.device)
    side.wait_stream(torch.cuda.current_stream(graphed.device))
    with torch.cuda.stream(side):
        graphed.step(buf)
    torch.cuda.current_stream(graphed.device).wait_stream(side)
    eager.step(acts[0])
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ts = graphed.step(buf)
    seen = set()
    for k in range(1, 18):  # 17 replays: across the auto-reset on step 14
        buf.copy_(acts[k])
        g.replay()
        torch.cuda.synchronize(graphed.device)
        want = eager.step(acts[k])
        for name, x, y in (("obs", graphed.flat_observation, eager.flat_observation), ("reward", ts.reward, want.reward),
                           ("discount", ts.discount, want.discount), ("step_type", ts.step_type, want.step_type)):
            assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes(), (k, name)
        seen |= set(ts.step_type.cpu().numpy().tolist())
    assert seen == {0, 1, 2}
    eager.close(); graphed.close()


# ------------------------------------------------------------------------------------------------ 8. downstream
def test_actor_loop_writer_and_episode_log(torch_mod, world):
    torch = torch_mod
    from flybody_amd import fly_envs
    from flybody_amd.actor_loop import BatchedActorLoop, EpisodeLog, NStepTransitionWriter
    from flybody_amd.batched_env import BatchedWalkEnv

    B, seed = 4, 11
    env = BatchedWalkEnv(world[1], world[0], batch_size=B, seed=seed)
    made = fly_envs.walk_imitation(floor_contacts=False, batch_size=2)  # the factory's env is this class, on the build's own snippets
    assert type(made) is BatchedWalkEnv and made.refs.ntraj == 4 and made.reset().step_type.tolist() == [0, 0]
    made.close()
    writer = NStepTransitionWriter(B, env.spec.obs_dim, env.spec.action_dim, n_step=5, capacity=1024)
    log = EpisodeLog(B, capacity=64)
    policy = lambda obs: torch.zeros(obs.shape[0], 59, device=obs.device)  # noqa: E731
    res = BatchedActorLoop(env, policy, writer).log_episodes(log).run(40)
    rec = log.records()
    # the oracle under the same zero policy: reset + 40 steps per env
    want = []
    for i in range(B):
        o = make_oracle(world, seed=seed, env_id=i)
        o.reset()
        ret = 0.0
        for _ in range(40):
            st, r, d, _ = o.step(np.zeros(59))
            if st == 0:
                ret = 0.0
                continue
            ret += r
            if st == 2:
                want.append((i, ret))
    assert res["episodes"] == len(rec) == len(want) == 2 * B  # LAST on calls 13 and 27; the third episode is still running
    assert (rec["length"] == 13).all() and res["episode_length"] == 13.0
    got = sorted((int(r["env"]), int(r["call"]), float(r["ret"])) for r in rec)
    want_ret = [w[1] for w in sorted(want, key=lambda w: w[0])]  # (stable: each env's episodes stay in order)
    rerr = rel([g[2] for g in got], want_ret)
    print(f"episode returns: error {rerr:.3e}")
    assert rerr <= 13 * TOL["reward"]  # a return is the sum of 13 rewards
    assert abs(res["episode_return"] - np.mean(want_ret)) <= 13 * TOL["reward"] * max(1.0, np.abs(want_ret).max())
    o, a, r, d, o2 = writer.transitions()
    assert len(o) > 0 and all(bool(torch.isfinite(x).all()) for x in (o, a, r, d, o2))
    env.close()


# ------------------------------------------------------------------------------------------------ 9. protocol
def test_create_refusals_and_old_handles(torch_mod, world):
    torch = torch_mod
    from flybody_amd import _capi
    from flybody_amd.batched_env import BatchedWalkPhysics
    from flybody_amd.tasks.walk_tracker import make_task

    L = _capi.lib()
    blob = open(BLOB, "rb").read()
    wtask, keep = make_task(world[0], world[1])

    def create(flags, with_task=True):
        t = _capi.WalkPhysicsTask(physics_flags=flags, time_limit_steps=5001)
        if with_task:
            t.task = C.pointer(wtask)
        h = C.c_void_p()
        rc = L.ffe_create_walk_physics(blob, len(blob), C.byref(t), 2, 0, C.byref(h))
        text = L.ffe_last_error(None).decode()
        if rc == 0:
            L.ffe_destroy(h)
        return rc, bool(h.value), text

    for flags in (WALK_EPISODES | NO_CONTACT, WALK_EPISODES | NO_CONTACT | NO_LIMIT, WALK_EPISODES | WALK_JOINT_LIMITS, WALK_EPISODES,
                  WALK_EPISODES | NO_CONTACT | WALK_JOINT_LIMITS | NO_LIMIT, WALK_EPISODES | NO_CONTACT | WALK_JOINT_LIMITS | 128):
        rc, made, text = create(flags)
        assert rc == -1 and not made and "FFE_WALK_EPISODES" in text, (flags, text)
    rc, made, text = create(WALK_EPISODES | NO_CONTACT | WALK_JOINT_LIMITS, with_task=False)
    assert rc == -1 and not made and "FFE_WALK_EPISODES" in text and "null" in text
    assert create(WALK_EPISODES | NO_CONTACT | WALK_JOINT_LIMITS | NO_GRAVITY)[:2] == (0, True)
    # without the bit: the texts of before, and ffe_step stays refused on both kinds of bare-physics handle
    assert create(NO_CONTACT)[2] == ("ffe_create_walk_physics: floor contacts and joint limits are not built yet: physics_flags must contain "
                                     "FFE_NO_CONTACT | FFE_NO_LIMIT")
    assert "FFE_WALK_JOINT_LIMITS needs" in create(WALK_JOINT_LIMITS)[2]
    for kw in ({}, {"joint_limits": True}):
        env = BatchedWalkPhysics(batch_size=2, **kw)
        obs = torch.zeros(2, 741, device="cuda")
        r, d, act = torch.zeros(2, device="cuda"), torch.zeros(2, device="cuda"), torch.zeros(2, 59, device="cuda")
        st = torch.zeros(2, dtype=torch.int32, device="cuda")
        assert L.ffe_step(env._h, act.data_ptr(), obs.data_ptr(), r.data_ptr(), d.data_ptr(), st.data_ptr(), env._stream()) == -1
        assert L.ffe_last_error(env._h).decode() == ("ffe_reset / ffe_reset_envs / ffe_step: not available on a walk physics handle (bare physics only: "
                                                     "limits, floor contacts, sensors and the episode protocol are not built yet)")
        assert env.spec.obs_dim == 0
        env.close()
    env = make_env(world, 2)
    s = env.spec
    assert (s.obs_dim, s.nq, s.nv, s.nu, s.action_dim, s.nsub, s.n_ref, s.n_obs_joints) == (741, 109, 108, 59, 59, 10, 65, 85)
    assert list(env.observation_spec()) == ["walker/" + k for k in ("accelerometer", "actuator_activation", "appendages_pos", "force", "gyro", "joints_pos",
                                                                     "joints_vel", "ref_displacement", "ref_root_quat", "touch", "velocimeter", "world_zaxis")]
    v = env.validity()
    env.reset()
    act = torch.zeros(2, 59, device="cuda")
    for _ in range(3):
        env.step(act)
    v = env.validity()
    assert v.episode_steps.tolist() == [3, 3] and v.step_bits.tolist() == [0, 0] and v.episode_bits.tolist() == [0, 0]
    assert env.time_steps(act, 2) > 0 and env.time_kernel(act, 2) > 0
    env.close()
