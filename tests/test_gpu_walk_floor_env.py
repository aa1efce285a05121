"""GPU parity tests of the walk_imitation environment on the floor (csrc/walk_floor_env.hip `imitation_floor_step` and the episode
kernels around it, through `BatchedWalkEnv(floor_contacts=True)` and the C ABI) against the float64 oracle
on identical inputs.  Run with `-m gpu` on an MI355X.  No batch exceeds 24 plus a few fillers.

The oracle collides the fly's own pairs on the committed blob and the kernel does not, so both sides of every comparison run on
`walk_floor_sets.floor_only_blob()` (the 48 floor pairs alone); `BatchedWalkEnv` reads a .json next to its blob, so `floor_blob()` copies
fly_walk.json beside the temporary blob.  Snippets: `synthetic_snippets(view, n=3, length=100)` as in tests/test_gpu_walk_episode.py.

Errors are per group, relative to max(1, max |reference| of the group) over the rows compared; each bound is min(3 x the worst value
measured on the MI355X, cap):
  force 1.7e-4, touch 1.1e-4, reward 6e-5    TOL of tests/test_gpu_ball.py
  accelerometer 1e-2; gyro, velocimeter, joints_vel   CAP10["root_ang"], CAP10["root_lin"], CAP10["hinge_vel"] of tests/test_gpu_walk_limits.py
  the rest                                   OBS_TOL of tests/test_gpu_walk_episode.py
MEASURED below holds the worst value over cases a, b and c (reset rows, no contact in reach, the teacher-forced step under three flag
sets)."""
import ctypes as C
import functools
import os
import shutil

import numpy as np
import pytest

import walk_floor_sets as S
from test_gpu_ball import TOL
from test_gpu_walk_episode import EP_STEPS, OBS_TOL, SAMPLE_STEPS, SENTINEL, actions, group_errors, host, rel, split, torch_mod, world  # noqa: F401
from test_gpu_walk_limits import CAP10
from walk_floor_sets import NO_ADHESION, NO_CONTACT, NO_FLUID, NO_GRAVITY, NO_LIMIT, NO_NOSLIP, WALK_EPISODES, WALK_FLOOR, WALK_JOINT_LIMITS

pytestmark = pytest.mark.gpu

CAP = dict(OBS_TOL, force=TOL["force"], touch=TOL["touch"], accelerometer=1e-2, gyro=CAP10["root_ang"], velocimeter=CAP10["root_lin"],
           joints_vel=CAP10["hinge_vel"])
REWARD_CAP = TOL["reward"]
# Worst values measured on the MI355X against the oracle over cases a, b, c (rounded up in the last digit kept):
#   accelerometer 9.538e-6 (c, no_fluid_no_adhesion)   actuator_activation 3.472e-8   appendages_pos 1.013e-7   force 3.063e-5 (a, padded
#   reset row: one sample of 0.091; 8.620e-6 on a step)   gyro 2.251e-5 (c, all)   joints_pos 2.170e-7   joints_vel 2.882e-5 (c, all)
#   ref_displacement 7.308e-8   ref_root_quat 2.755e-7   touch 1.128e-5 (a, padded reset row; 6.975e-6 on a step)   velocimeter 1.359e-5
#   world_zaxis 3.476e-7   reward 1.159e-6
# Case b (no contact: the inertial force alone, max |force| 1.6e-3): force 3.6e-10, touch exactly 0.  Case c leaves out 4 / 5 / 5 of 24
# states (all / no_noslip / no_fluid_no_adhesion).  Case e, open loop over whole episodes on the floor (110 calls, contacts opening and
# closing on the way): per-step reward 8.114e-4.  Case g: episode return 1.7e-7 of 91.15 at zero actions.
MEASURED = {"accelerometer": 9.6e-6, "actuator_activation": 3.5e-8, "appendages_pos": 1.1e-7, "force": 3.1e-5, "gyro": 2.3e-5, "joints_pos": 2.2e-7,
            "joints_vel": 2.9e-5, "ref_displacement": 7.4e-8, "ref_root_quat": 2.8e-7, "touch": 1.2e-5, "velocimeter": 1.4e-5, "world_zaxis": 3.5e-7}
REWARD_MEASURED = 1.2e-6
REWARD_OPEN_MEASURED = 8.2e-4  # case e: per-step reward over whole episodes, open loop
WEIGHT = 0.9677  # the fly's weight, dyn: the oracle's own floor pin (tests/test_oracle_walk.py)
FLAG_SETS = [(0, "all"), (NO_NOSLIP, "no_noslip"), (NO_FLUID | NO_ADHESION, "no_fluid_no_adhesion")]


def bound(group):
    assert MEASURED is not None, "the measured errors have not been recorded"
    return min(3 * MEASURED[group], CAP[group])


@functools.lru_cache(maxsize=1)
def floor_blob():
    path = S.floor_only_blob()
    meta = os.path.splitext(path)[0] + ".json"
    if not os.path.exists(meta):
        shutil.copy(os.path.splitext(S.WALK_BLOB)[0] + ".json", meta)
    return path


def make_env(world, B, flags=0, refs=None, blob=None, **kw):
    from flybody_amd.batched_env import BatchedWalkEnv

    return BatchedWalkEnv(refs or world[1], world[0], batch_size=B, physics_flags=flags, floor_contacts=True, blob_path=blob or floor_blob(), **kw)


def make_oracle(world, flags=0, refs=None, **kw):
    """An oracle env on a model of its own (the flags live in the model)."""
    from oracle import oracle as O

    view = world[0]
    m = O.OracleModel(S.floor_only_blob())
    assert m.npair == 48
    m.set_flags(flags)
    return O.OracleWalkEnv(m, refs or world[1], view.mocap_jnt, view.mocap_site, (view.retract_qadr, view.retract_val), **kw)


def check_groups(layout, got, ref, what):
    err = group_errors(layout, got, ref)
    print(what, " ".join(f"{k} {v:.3e}" for k, v in err.items()))
    for k, v in err.items():
        assert v <= bound(k), (what, k, v, bound(k))
    return err


def raised(world, dz=1.0):
    """The three clips with the reference root `dz` cm higher: no geom reaches the floor."""
    from flybody_amd.tasks import walking as W

    sn = []
    for i in range(3):
        s = {k: np.array(v, copy=True) for k, v in world[1].snippet(i).items()}
        s["qpos"][:, 2] += dz
        sn.append(s)
    return W.WalkRefSet(sn)


# ------------------------------------------------------------------------------------------------ a. reset row
@pytest.mark.parametrize("pad", [False, True])
def test_reset_row(torch_mod, world, pad):
    env = make_env(world, 3, pad_first_obs=pad)
    for s in env._sets:
        s[0].fill_(SENTINEL)
    env.set_next_trajectory_index(np.arange(3))
    ts = env.reset()
    st, rew, disc = host(ts)
    obs = env.flat_observation.cpu().numpy()
    ints, reals = (x.cpu().numpy() for x in env.get_task_state())
    assert st.tolist() == [0, 0, 0] and rew.tolist() == [0.0, 0.0, 0.0] and disc.tolist() == [1.0, 1.0, 1.0]
    assert obs.shape == (3, 741) and not (obs == SENTINEL).any() and np.isfinite(obs).all()
    ref_obs = []
    for clip in range(3):
        o = make_oracle(world)
        o.set_pad_first_obs(pad)
        o.force_next(clip)
        rst, rr, rd, ro = o.reset()
        assert (rst, rr, rd) == (0, 0.0, 1.0) and o.data.ncon == 6
        ref_obs.append(ro)
        layout = o.LAYOUT
    ref = split(layout, np.stack(ref_obs))
    scale = 1.0 if pad else 0.1  # (one sample: the mean over ten substeps without padding)
    assert (ref["touch"] > 0.04 * scale).all() and np.abs(ref["force"]).max() > 0.05 * scale  # compared as non-zero numbers
    assert ints[:, 0].tolist() == [0, 1, 2] and not ints[:, 1].any() and not ints[:, 3].any() and ints[:, 5].tolist() == [6, 6, 6]
    assert (reals[:, 0] > 0).all() and not env.validity().step_bits.any()
    check_groups(layout, obs, np.stack(ref_obs), f"reset pad={pad}")
    env.close()


# ------------------------------------------------------------------------------------------------ b. no contact in reach
def test_no_contact_in_reach(torch_mod, world):
    """Floating 1 cm higher: the oracle has no contact, touch is exactly zero and force is the inertial term alone - the free-root force
    sensor without the contact solve."""
    torch = torch_mod
    refs = raised(world)
    env = make_env(world, 3, NO_GRAVITY, refs=refs, terminal_com_dist=np.inf)
    env.set_next_trajectory_index(np.arange(3))
    env.reset()
    obs0 = env.flat_observation.cpu().numpy().copy()
    acts = [actions(100 + clip, 1, 0.5)[0] for clip in range(3)]
    ts = env.step(torch.tensor(np.stack(acts), device="cuda"))
    st, rew, disc = host(ts)
    obs1 = env.flat_observation.cpu().numpy()
    ints = env.get_task_state()[0].cpu().numpy()
    r0, r1, rr = [], [], []
    for clip in range(3):
        o = make_oracle(world, NO_GRAVITY, refs=refs, terminal_com_dist=np.inf)
        o.force_next(clip)
        r0.append(o.reset()[3])
        assert o.data.ncon == 0
        res = o.step(acts[clip])
        assert o.data.ncon == 0 and (res[0], res[2]) == (st[clip], disc[clip])
        r1.append(res[3])
        rr.append(res[1])
        layout = o.LAYOUT
    for got in (obs0, obs1):
        assert not split(layout, got)["touch"].any()
    ref = split(layout, np.stack(r1))
    print(f"no contact in reach: max |force| {np.abs(ref['force']).max():.3e} (oracle), reward error {rel(rew, rr):.3e}")
    assert np.abs(ref["force"]).max() > 1e-5 and not ints[:, 5].any()  # the inertial term is there
    check_groups(layout, obs0, np.stack(r0), "no contact, reset")
    check_groups(layout, obs1, np.stack(r1), "no contact, step")
    assert rel(rew, rr) <= min(3 * REWARD_MEASURED, REWARD_CAP)
    env.close()


# ------------------------------------------------------------------------------------------------ c. one control step, teacher-forced
def oracle_samples(world, flags):
    """tests/test_gpu_walk_episode.py::oracle_samples on the floor: per clip, states along a +-0.5 rollout at SAMPLE_STEPS with the action
    and the outcome of the step that follows, how close a candidate pair came to a switching distance during that step, and the
    contacts of its last substep."""
    m2 = S.model()
    out = []
    for clip in range(3):
        o = make_oracle(world, flags, terminal_com_dist=np.inf)
        o.force_next(clip)
        o.reset()
        acts = actions(100 + clip, SAMPLE_STEPS[-1] + 1, 0.5)
        for k in range(SAMPLE_STEPS[-1] + 1):
            state = (o.data.qpos.copy(), o.data.qvel.copy(), o.data.act.copy())
            o.data.contact_hist(reset=True)
            res = o.step(acts[k])
            gap = o.data.contact_hist(reset=True)[1]
            if k in SAMPLE_STEPS:
                tr = []
                S.oracle_advance(m2, state, o.data.ctrl.copy(), 10, flags, trace=tr)
                out.append(dict(clip=clip, step=k, state=state, action=acts[k], st=res[0], reward=res[1], discount=res[2], obs=res[3].copy(), gap=gap,
                                ncon=tr[-1][0]))
            assert res[0] == 1
        layout = o.LAYOUT
    return out, layout


@pytest.mark.parametrize("flags,name", FLAG_SETS)
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
    ints = env.get_task_state()[0].cpu().numpy()
    keep = [i for i, s in enumerate(samples) if s["gap"] >= S.BAND]
    print(f"{name}: {B - len(keep)} of {B} states within {S.BAND:g} cm of a switching distance are left out; contacts {ints[:, 5].tolist()}")
    assert B - len(keep) <= 6
    assert st[keep].tolist() == [samples[i]["st"] for i in keep] and disc[keep].tolist() == [samples[i]["discount"] for i in keep]
    assert ints[keep, 5].tolist() == [samples[i]["ncon"] for i in keep]
    assert not env.validity().step_bits.cpu().numpy().any()
    rerr = rel(rew[keep], [samples[i]["reward"] for i in keep])
    print(f"{name}: reward {rerr:.3e}")
    ref = np.stack([samples[i]["obs"] for i in keep])
    assert (split(layout, ref)["touch"] > 0).any()
    check_groups(layout, obs[keep], ref, name)
    assert rerr <= min(3 * REWARD_MEASURED, REWARD_CAP)
    env.close()


# ------------------------------------------------------------------------------------------------ d. the standing fly
def test_the_standing_fly(torch_mod, world):
    torch = torch_mod
    env = make_env(world, 2)
    env.set_next_trajectory_index(np.array([2, 2]))
    env.reset()
    zero = torch.zeros(2, 59, device="cuda")
    flagged = 0
    for _ in range(60):
        ts = env.step(zero)
        flagged += int(env.validity().step_bits.cpu().numpy().any())
    obs = env.flat_observation.cpu().numpy()
    touch = obs[:, env._layout["walker/touch"][0]:][:, :6]
    ints, reals = (x.cpu().numpy() for x in env.get_task_state())
    print(f"standing fly: touch {touch[0].tolist()} sum {touch[0].sum():.4f} (weight {WEIGHT}) contacts {ints[0, 5]} normal force {reals[0, 0]:.4f}")
    assert np.isfinite(obs).all() and np.array_equal(obs[0], obs[1]) and flagged == 0
    assert (host(ts)[0] == 1).all()
    assert abs(touch[0].sum() - WEIGHT) <= 0.05 * WEIGHT
    env.close()


# ------------------------------------------------------------------------------------------------ e. episodes open loop
def test_episodes_open_loop(torch_mod, world):
    """On the floor the fly keeps up with the reference: with the default terminal_com_dist every episode runs to the end of its clip
    (35 / 52 / 69 steps, LAST with discount 1), at zero and at +-0.5 actions.  110 calls: env 0 (clip 0 first) sees two auto-resets."""
    torch = torch_mod
    from oracle import oracle as O

    B, seed, base, nsteps = 3, 5, 40, 110
    amps = (0.0, 0.5, 0.5)
    env = make_env(world, B, seed=seed, env_id_base=base)
    oracles = [make_oracle(world, seed=seed, env_id=base + i) for i in range(B)]
    env.set_next_trajectory_index(np.arange(3))
    for i, o in enumerate(oracles):
        o.force_next(i)
    acts = [actions(700 + i, nsteps, amps[i]) for i in range(B)]
    ts = env.reset()
    refs = [o.reset() for o in oracles]
    clips, lengths, worst = [[] for _ in range(B)], [[] for _ in range(B)], 0.0
    for k in range(nsteps + 1):
        st, rew, disc = host(ts)
        ints = env.get_task_state()[0].cpu().numpy()
        for i in range(B):
            assert (st[i], disc[i]) == (refs[i][0], refs[i][2]), (k, i)
            assert ints[i, 0] == oracles[i].traj_idx, (k, i)
            worst = max(worst, abs(float(rew[i]) - refs[i][1]) / max(1.0, abs(refs[i][1])))
            if st[i] == 0:
                clips[i].append(int(ints[i, 0]))
            if st[i] == 2:
                assert disc[i] == 1.0, (k, i)
                lengths[i].append(int(ints[i, 1]))
        if k == nsteps:
            break
        ts = env.step(torch.tensor(np.stack([acts[i][k] for i in range(B)]), device="cuda"))
        refs = [oracles[i].step(acts[i][k]) for i in range(B)]
    print(f"open loop: clips {clips} episode lengths {lengths} per-step reward error {worst:.3e}")
    for i in range(B):
        assert clips[i][0] == i and clips[i][1:] == [O.rng_u64(seed, base + i, ep, 0) % 3 for ep in range(1, len(clips[i]))], (i, clips[i])
        assert lengths[i] == [EP_STEPS[c] for c in clips[i][:len(lengths[i])]] and len(lengths[i]) >= 1, (i, lengths[i])
    assert len(clips[0]) >= 3  # FIRST, and two auto-resets
    assert REWARD_OPEN_MEASURED is not None, "the measured open-loop error has not been recorded"
    assert worst <= 3 * REWARD_OPEN_MEASURED
    env.close()


# ------------------------------------------------------------------------------------------------ f. masked reset, batch independence, replay
def test_reset_envs_restarts_only_the_masked(torch_mod, world):
    torch = torch_mod
    B = 6
    acts = [torch.tensor(np.stack(a), device="cuda") for a in zip(*[actions(400 + i, 8, 0.5) for i in range(B)])]
    mask = np.array([0, 1, 0, 0, 1, 0], dtype=bool)

    def run(masked):
        env = make_env(world, B, seed=3)
        env.reset()
        out = []
        for k in range(8):
            if k == 4 and masked:
                ts = env.reset_envs(torch.tensor(mask, device="cuda"))
                st = ts.step_type.cpu().numpy()
                ints = env.get_task_state()[0].cpu().numpy()
                assert (st[mask] == 0).all() and (st[~mask] == 1).all() and not ints[mask, 1].any() and (ints[~mask, 1] == 4).all()
            ts = env.step(acts[k])
            q, v = (x.cpu().numpy() for x in env.get_state())
            out.append([env.flat_observation.cpu().numpy(), ts.reward.cpu().numpy().copy(), ts.discount.cpu().numpy().copy(),
                        ts.step_type.cpu().numpy().copy(), q, v, env.get_act().cpu().numpy(), env.get_task_state()[0].cpu().numpy()])
        env.close()
        return out

    a, b = run(False), run(True)
    for k in range(8):
        for x, y in zip(a[k], b[k]):
            assert x[~mask].tobytes() == y[~mask].tobytes(), k  # the others go on bit for bit
        if k >= 4:
            assert (b[k][7][mask, 1] == k - 3).all() and (a[k][7][mask, 1] == k + 1).all()
            assert not np.array_equal(a[k][0][mask], b[k][0][mask])


def test_rows_do_not_depend_on_the_batch(torch_mod, world):
    torch = torch_mod
    n, slot = 8, 7
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
            ints, reals = env.get_task_state()
            out.append(b"".join(x[at].cpu().numpy().tobytes() for x in (env.flat_observation, ts.reward, ts.discount, ts.step_type, q, v, ints, reals)))
        env.close()
        return out

    assert run(1, slot, 0) == run(16, 0, slot)


def test_step_replays_from_a_captured_graph(torch_mod, world):
    torch = torch_mod
    B, n = 4, 8
    eager, graphed = make_env(world, B, seed=2), make_env(world, B, seed=2)
    acts = [torch.tensor(np.stack(a), device="cuda") for a in zip(*[actions(600 + i, n, 0.5) for i in range(B)])]
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
    for k in range(1, n):
        buf.copy_(acts[k])
        g.replay()
        torch.cuda.synchronize(graphed.device)
        want = eager.step(acts[k])
        for name, x, y in (("obs", graphed.flat_observation, eager.flat_observation), ("reward", ts.reward, want.reward),
                           ("discount", ts.discount, want.discount), ("step_type", ts.step_type, want.step_type)):
            assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes(), (k, name)
    off = eager._layout["walker/touch"][0]
    assert eager.flat_observation.cpu().numpy()[:, off:off + 6].any()  # the fly stands on something
    eager.close(); graphed.close()


# ------------------------------------------------------------------------------------------------ g. downstream
def test_actor_loop_writer_and_episode_log(torch_mod, world):
    torch = torch_mod
    from flybody_amd import fly_envs
    from flybody_amd.actor_loop import BatchedActorLoop, EpisodeLog, NStepTransitionWriter
    from flybody_amd.batched_env import BatchedWalkEnv

    B, seed, calls = 3, 11, 40
    made = fly_envs.walk_imitation(floor_contacts="primitives", batch_size=2)  # the factory's env is this class, on the committed blob
    assert type(made) is BatchedWalkEnv and made.floor_contacts and made.physics_flags & WALK_FLOOR and made.reset().step_type.tolist() == [0, 0]
    off = made._layout["walker/touch"][0]
    assert (made.flat_observation.cpu().numpy()[:, off:off + 6] > 0).all()
    made.close()
    env = make_env(world, B, seed=seed)
    env.set_next_trajectory_index(np.zeros(B, dtype=np.int64))  # clip 0: its 35 steps end inside the run
    writer = NStepTransitionWriter(B, env.spec.obs_dim, env.spec.action_dim, n_step=5, capacity=1024)
    log = EpisodeLog(B, capacity=64)
    policy = lambda obs: torch.zeros(obs.shape[0], 59, device=obs.device)  # noqa: E731
    res = BatchedActorLoop(env, policy, writer).log_episodes(log).run(calls)
    rec = log.records()
    o = make_oracle(world, seed=seed, env_id=0)
    o.force_next(0)
    o.reset()
    ret = 0.0
    for _ in range(EP_STEPS[0]):
        st, r, d, _ = o.step(np.zeros(59))
        ret += r
    assert st == 2 and d == 1.0
    assert res["episodes"] == len(rec) == B and (rec["length"] == EP_STEPS[0]).all()
    rerr = rel(rec["ret"], [ret] * B)
    print(f"episode returns: error {rerr:.3e} of {ret:.4f}")
    assert rerr <= EP_STEPS[0] * 3 * REWARD_OPEN_MEASURED  # a return is the sum of 35 rewards
    ob, a, r, d, o2 = writer.transitions()
    assert len(ob) > 0 and all(bool(torch.isfinite(x).all()) for x in (ob, a, r, d, o2))
    env.close()


# ------------------------------------------------------------------------------------------------ h. protocol
def test_protocol(torch_mod, world):
    torch = torch_mod
    from flybody_amd import _capi
    from flybody_amd.batched_env import BatchedWalkEnv, BatchedWalkPhysics
    from flybody_amd.model.blob import read_blob
    from flybody_amd.tasks.walk_tracker import make_task

    L = _capi.lib()
    blob = open(S.WALK_BLOB, "rb").read()
    wtask, keep = make_task(world[0], world[1])
    ENV = NO_CONTACT | WALK_JOINT_LIMITS | WALK_EPISODES | WALK_FLOOR

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

    for flags in (ENV, ENV | NO_NOSLIP | NO_ADHESION | NO_FLUID | NO_GRAVITY):
        assert create(flags)[:2] == (0, True), flags
    for flags in (ENV | NO_LIMIT, ENV & ~NO_CONTACT, ENV & ~WALK_JOINT_LIMITS, ENV | 4096):
        rc, made, text = create(flags)
        assert rc == -1 and not made and "FFE_WALK_EPISODES" in text and "FFE_WALK_FLOOR" in text, (flags, text)
    rc, made, text = create(ENV, with_task=False)
    assert rc == -1 and not made and "FFE_WALK_EPISODES" in text and "FFE_WALK_FLOOR" in text and "null" in text
    with pytest.raises(RuntimeError, match="FFE_WALK_FLOOR"):
        BatchedWalkPhysics(batch_size=1, physics_flags=ENV)
    rc, made, text = create(NO_CONTACT | WALK_JOINT_LIMITS | WALK_EPISODES | NO_NOSLIP)  # the floor's switches need the floor
    assert rc == -1 and "FFE_WALK_EPISODES" in text
    with pytest.raises(ValueError):
        BatchedWalkEnv(world[1], world[0], batch_size=1, physics_flags=NO_NOSLIP)
    with pytest.raises(ValueError):
        make_env(world, 1, flags=NO_LIMIT)
    # the new flag set creates through the class; both blobs give the same bits
    act = torch.tensor(np.stack([actions(800 + i, 1, 0.5)[0] for i in range(2)]), device="cuda")
    rows = []
    for path in (floor_blob(), S.WALK_BLOB):
        env = make_env(world, 2, NO_NOSLIP, blob=path, seed=4)
        assert env.physics_flags == ENV | NO_NOSLIP
        env.reset()
        for _ in range(3):
            ts = env.step(act)
        rows.append(b"".join(x.cpu().numpy().tobytes() for x in (env.flat_observation, ts.reward, ts.discount, ts.step_type, *env.get_state(),
                                                                 *env.get_task_state())))
        v = env.validity()
        assert v.episode_steps.tolist() == [3, 3] and v.step_bits.tolist() == [0, 0] and v.episode_bits.tolist() == [0, 0]
        s = env.spec
        assert (s.obs_dim, s.nq, s.nv, s.nu, s.action_dim, s.nsub, s.n_ref, s.n_obs_joints) == (741, 109, 108, 59, 59, 10, 65, 85)
        assert env.time_steps(act, 2) > 0 and env.time_kernel(act, 2) > 0
        env.close()
    assert rows[0] == rows[1]
    # the floor-off handle is unchanged: the default keyword gives the flags of before, and its force / touch columns stay exact zeros
    old = BatchedWalkEnv(world[1], world[0], batch_size=2, seed=4)
    assert old.physics_flags == NO_CONTACT | WALK_JOINT_LIMITS | WALK_EPISODES and not old.floor_contacts
    old.reset()
    old.step(act)
    o = old.flat_observation.cpu().numpy()
    lay = old._layout
    assert not o[:, lay["walker/force"][0]:lay["walker/force"][0] + 18].any() and not o[:, lay["walker/touch"][0]:lay["walker/touch"][0] + 6].any()
    assert not old.get_task_state()[0].cpu().numpy()[:, 5].any() and not old.get_task_state()[1].cpu().numpy().any()
    old.close()
    # overflow: qpos0 with the root at z = 0.05 cm has far more than 16 geoms inside the margin
    env = make_env(world, 2, terminal_com_dist=np.inf)
    env.reset()
    q0 = np.asarray(read_blob(S.WALK_BLOB)["qpos0"], dtype=np.float64).ravel().copy()
    q0[2] = 0.05
    q, v = env.get_state()
    q[0] = torch.tensor(q0, device=q.device)
    v[0] = 0
    env.set_state(q, v)
    env.step(torch.zeros(2, 59, device="cuda"))
    val = env.validity()
    assert val.step_bits[0] & 1 and val.episode_bits[0] & 1 and not val.step_bits[1] and not val.episode_bits[1]
    assert np.isfinite(env.flat_observation.cpu().numpy()).all() and all(np.isfinite(x.cpu().numpy()).all() for x in env.get_state())
    env.close()
