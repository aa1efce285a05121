"""GPU parity tests of the walk_imitation environment on the floor with the fly's own contacts (csrc/walk_imit_self_env.hip
`imitation_self_step` and the episode kernels around it, through `BatchedWalkEnv(floor_contacts=True, self_contacts=True)` and the C
ABI) against the float64 oracle on identical inputs.  Run with `-m gpu` on an MI355X.  No batch exceeds 24
plus a few fillers.

Both sides of every comparison run on the SHIPPED blob (fly_walk.ffmb): the oracle collides the 48 floor pairs and the 2 288 fly-fly
pairs, and so does the env.  Snippets: `synthetic_snippets(view, n=3, length=100)` as in tests/test_gpu_walk_episode.py.

Errors are per group, relative to max(1, max |reference| of the group) over the rows compared (`group_errors`); each bound is min(3 x
the worst value measured on the MI355X against the oracle, cap), the caps being CAP and REWARD_CAP of tests/test_gpu_walk_floor_env.py.
The factor 3 covers run-to-run differences of float32 solves whose iteration counts change with rounding.  MEASURED holds the worst value
over cases a, b and c (reset rows, the teacher-forced step on R10 under three flag sets, the crafted contacts XS)."""
import ctypes as C

import numpy as np
import pytest

import walk_self_env_samples as E
import walk_self_sets as S
from test_gpu_walk_episode import EP_STEPS, SENTINEL, actions, group_errors, host, rel, split, torch_mod, world  # noqa: F401
from test_gpu_walk_floor_env import CAP, REWARD_CAP, WEIGHT
from walk_floor_sets import NO_ADHESION, NO_CONTACT, NO_FLUID, NO_GRAVITY, NO_LIMIT, NO_NOSLIP, WALK_EPISODES, WALK_FLOOR, WALK_JOINT_LIMITS
from walk_self_sets import WALK_SELF

pytestmark = pytest.mark.gpu

# Worst values measured on the MI355X against the oracle over cases a, b, c (rounded up in the last digit kept):
#   accelerometer 7.582e-6 (a, reset rows)   actuator_activation 7.813e-8   appendages_pos 6.314e-8   force 1.402e-5 (a, padded reset row:
#   one sample; 3.803e-6 on a step)   gyro 5.422e-6 (b, no_noslip)   joints_pos 1.411e-7   joints_vel 2.256e-6 (b, no_fluid_no_adhesion)
#   ref_displacement 5.860e-8   ref_root_quat 1.271e-7   touch 1.128e-5 (a, padded reset row; 3.124e-6 on a step)   velocimeter 3.362e-6
#   world_zaxis 2.536e-7   reward 4.647e-7
# Case b leaves out 4 / 2 / 5 of 24 states (all / no_noslip / no_fluid_no_adhesion), case c 2 of 12.  Case f, open loop over whole
# episodes (110 calls): per-step reward 1.645e-6, below the floor env's own 8.2e-4 (there the floor-only fly and the oracle part ways
# when a contact switches; here they did not).  Episode return at zero actions: 3.6e-7 of 91.97.
MEASURED = {"accelerometer": 7.6e-6, "actuator_activation": 7.9e-8, "appendages_pos": 6.4e-8, "force": 1.5e-5, "gyro": 5.5e-6, "joints_pos": 1.5e-7,
            "joints_vel": 2.3e-6, "ref_displacement": 5.9e-8, "ref_root_quat": 1.3e-7, "touch": 1.2e-5, "velocimeter": 3.4e-6, "world_zaxis": 2.6e-7}
REWARD_MEASURED = 4.7e-7
REWARD_OPEN_MEASURED = 1.7e-6  # case f: per-step reward over whole episodes, open loop
WALK_SELF_EPISODES = 8192  # FFE_WALK_SELF_EPISODES: the bit that asks for FFE_WALK_SELF under the environment
ENV = NO_CONTACT | WALK_JOINT_LIMITS | WALK_EPISODES | WALK_FLOOR | WALK_SELF | WALK_SELF_EPISODES


def bound(group):
    assert MEASURED is not None, "the measured errors have not been recorded"
    return min(3 * MEASURED[group], CAP[group])


def reward_bound():
    assert REWARD_MEASURED is not None, "the measured reward error has not been recorded"
    return min(3 * REWARD_MEASURED, REWARD_CAP)


def make_env(world, B, flags=0, self_contacts=True, **kw):
    from flybody_amd.batched_env import BatchedWalkEnv

    return BatchedWalkEnv(world[1], world[0], batch_size=B, physics_flags=flags, floor_contacts=True, self_contacts=self_contacts, **kw)


def make_oracle(world, flags=0, **kw):
    return E.make_oracle(flags, refs=world[1], **kw)


def check_groups(layout, got, ref, what):
    err = group_errors(layout, got, ref)
    print(what, " ".join(f"{k} {v:.3e}" for k, v in err.items()))
    for k, v in err.items():
        assert v <= bound(k), (what, k, v, bound(k))
    return err


def self_count(o):
    """(ncon_matter, the fly-fly contacts among them) of the oracle env's current contact list"""
    return o.data.ncon_matter, S._matter_self(o.model, o.data)


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
    ref_obs, counts = [], []
    for clip in range(3):
        o = make_oracle(world)
        o.set_pad_first_obs(pad)
        o.force_next(clip)
        rst, rr, rd, ro = o.reset()
        assert (rst, rr, rd) == (0, 0.0, 1.0)
        counts.append(self_count(o))
        ref_obs.append(ro)
        layout = o.LAYOUT
    assert [c[0] for c in counts] == [6, 6, 6]
    ref = split(layout, np.stack(ref_obs))
    scale = 1.0 if pad else 0.1  # (one sample: the mean over ten substeps without padding)
    assert (ref["touch"] > 0.04 * scale).all() and np.abs(ref["force"]).max() > 0.05 * scale  # compared as non-zero numbers
    assert ints[:, 0].tolist() == [0, 1, 2] and not ints[:, 1].any() and not ints[:, 3].any()
    assert ints[:, 5].tolist() == [c[0] for c in counts] and reals[:, 2].tolist() == [float(c[1]) for c in counts]
    assert (reals[:, 0] > 0).all() and not env.validity().step_bits.any()
    check_groups(layout, obs, np.stack(ref_obs), f"reset pad={pad}")
    env.close()


# ------------------------------------------------------------------------------------------------ b / c. one control step, teacher-forced
def forced_step(torch, world, samples, flags, self_contacts=True):
    """The device env brought to every sample's (clip, step), given its state and stepped with its action: (st, rew, disc, obs, ints, reals,
    step_bits)."""
    B = len(samples)
    env = make_env(world, B, flags, self_contacts=self_contacts, terminal_com_dist=np.inf)
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
    ints, reals = (x.cpu().numpy() for x in env.get_task_state())
    bits = env.validity().step_bits.cpu().numpy()
    env.close()
    return st, rew, disc, obs, ints, reals, bits


def check_forced(torch, world, which, flags, name):
    samples, layout = E.forced_samples(which, flags)
    B = len(samples)
    st, rew, disc, obs, ints, reals, bits = forced_step(torch, world, samples, flags)
    keep = E.kept(samples)
    print(f"{name}: {B - len(keep)} of {B} states within {S.BAND:g} cm of a switching distance are left out; contacts {ints[:, 5].tolist()} "
          f"fly-fly {reals[:, 2].tolist()}")
    assert B - len(keep) <= E.LEFT_OUT_CAP[which]
    assert st[keep].tolist() == [samples[i]["st"] for i in keep] and disc[keep].tolist() == [samples[i]["discount"] for i in keep]
    assert ints[keep, 5].tolist() == [samples[i]["ncon"] for i in keep]
    assert reals[keep, 2].tolist() == [float(samples[i]["nself"]) for i in keep]
    assert not bits.any()
    assert any(samples[i]["self_rows"] > 0 for i in keep)
    rerr = rel(rew[keep], [samples[i]["reward"] for i in keep])
    print(f"{name}: reward {rerr:.3e}")
    ref = np.stack([samples[i]["obs"] for i in keep])
    assert (split(layout, ref)["touch"] > 0).any()
    check_groups(layout, obs[keep], ref, name)
    assert rerr <= reward_bound()


@pytest.mark.parametrize("flags,name", E.FLAG_SETS)
def test_one_control_step_teacher_forced(torch_mod, world, flags, name):
    check_forced(torch_mod, world, "R10", flags, name)


def test_the_crafted_contacts(torch_mod, world):
    """XS: floor and fly-fly rows mixed, 5 - 13 contacts at the start of the step."""
    check_forced(torch_mod, world, "XS", 0, "crafted")


# ------------------------------------------------------------------------------------------------ d. without the keyword
def test_without_the_keyword_the_contacts_are_missed(torch_mod, world):
    """The kept states of case b on `BatchedWalkEnv(floor_contacts=True)` on the shipped blob: the older handle collides the floor alone,
    counts fewer contacts and leaves the oracle by more than the bound."""
    samples, layout = E.forced_samples("R10", 0)
    st, rew, disc, obs, ints, reals, bits = forced_step(torch_mod, world, samples, 0, self_contacts=False)
    keep = E.kept(samples)
    assert not reals[:, 2].any()
    want = np.array([samples[i]["ncon"] for i in keep])
    print(f"without self_contacts: contacts {ints[keep, 5].tolist()} against the oracle's {want.tolist()}")
    assert ints[keep, 5].sum() < want.sum() and (ints[keep, 5] < want).sum() > len(keep) // 2
    apart = 0
    for i in keep:
        err = group_errors(layout, obs[i:i + 1], samples[i]["obs"][None])
        apart += err["joints_vel"] > bound("joints_vel") or err["force"] > bound("force")
    print(f"without self_contacts: {apart} of {len(keep)} kept states leave the oracle by more than the bound in joints_vel or force")
    assert apart >= 1


# ------------------------------------------------------------------------------------------------ e. the standing fly
def test_the_standing_fly(torch_mod, world):
    torch = torch_mod
    env = make_env(world, 2)
    env.set_next_trajectory_index(np.array([2, 2]))
    env.reset()
    o = make_oracle(world)
    o.force_next(2)
    o.reset()
    zero = torch.zeros(2, 59, device="cuda")
    flagged = 0
    for _ in range(60):
        ts = env.step(zero)
        flagged += int(env.validity().step_bits.cpu().numpy().any())
        assert o.step(np.zeros(59))[0] == 1
    obs = env.flat_observation.cpu().numpy()
    touch = obs[:, env._layout["walker/touch"][0]:][:, :6]
    ints, reals = (x.cpu().numpy() for x in env.get_task_state())
    od = self_count(o)  # (9 contacts, 3 of them fly-fly: the fly is at rest, so the list after the last integration is the last substep's)
    print(f"standing fly: touch {touch[0].tolist()} sum {touch[0].sum():.4f} (weight {WEIGHT}) contacts {ints[0, 5]} fly-fly {reals[0, 2]} "
          f"(oracle {od}) normal force {reals[0, 0]:.4f}")
    assert np.isfinite(obs).all() and np.array_equal(obs[0], obs[1]) and flagged == 0
    assert (host(ts)[0] == 1).all()
    assert abs(touch[0].sum() - WEIGHT) <= 0.05 * WEIGHT
    assert (int(ints[0, 5]), float(reals[0, 2])) == (od[0], float(od[1]))
    env.close()


# ------------------------------------------------------------------------------------------------ f. episodes open loop
def test_episodes_open_loop(torch_mod, world):
    """tests/test_gpu_walk_floor_env.py::test_episodes_open_loop on the shipped blob: every episode runs to the end of its clip (35 / 52 /
    69 steps, LAST with discount 1), at zero and at +-0.5 actions."""
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
    clips, lengths, worst, at = [[] for _ in range(B)], [[] for _ in range(B)], 0.0, None
    for k in range(nsteps + 1):
        st, rew, disc = host(ts)
        ints = env.get_task_state()[0].cpu().numpy()
        for i in range(B):
            assert (st[i], disc[i]) == (refs[i][0], refs[i][2]), (k, i)
            assert ints[i, 0] == oracles[i].traj_idx, (k, i)
            e = abs(float(rew[i]) - refs[i][1]) / max(1.0, abs(refs[i][1]))
            if e > worst:
                worst, at = e, (k, i)
            if st[i] == 0:
                clips[i].append(int(ints[i, 0]))
            if st[i] == 2:
                assert disc[i] == 1.0, (k, i)
                lengths[i].append(int(ints[i, 1]))
        if k == nsteps:
            break
        ts = env.step(torch.tensor(np.stack([acts[i][k] for i in range(B)]), device="cuda"))
        refs = [oracles[i].step(acts[i][k]) for i in range(B)]
    print(f"open loop: clips {clips} episode lengths {lengths} per-step reward error {worst:.3e} at (call, env) {at}")
    for i in range(B):
        assert clips[i][0] == i and clips[i][1:] == [O.rng_u64(seed, base + i, ep, 0) % 3 for ep in range(1, len(clips[i]))], (i, clips[i])
        assert lengths[i] == [EP_STEPS[c] for c in clips[i][:len(lengths[i])]] and len(lengths[i]) >= 1, (i, lengths[i])
    assert len(clips[0]) >= 3  # FIRST, and two auto-resets
    assert REWARD_OPEN_MEASURED is not None, "the measured open-loop error has not been recorded"
    assert worst <= 3 * REWARD_OPEN_MEASURED
    env.close()


# ------------------------------------------------------------------------------------------------ g. masked reset, batch independence, replay
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
    """(with the default queue count: nothing here sets one)"""
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
    assert eager.get_task_state()[1].cpu().numpy()[:, 2].any()  # ... and touches itself
    eager.close(); graphed.close()


def test_no_history(torch_mod, world):
    """The same (state, act, action) after different preludes gives the same bytes: no separating direction or warm start is kept."""
    torch = torch_mod
    samples, _ = E.forced_samples("XS", 0)
    B = len(samples)
    q = torch.tensor(np.stack([s["state"][0] for s in samples]))
    v = torch.tensor(np.stack([s["state"][1] for s in samples]))
    a = torch.tensor(np.stack([s["state"][2] for s in samples]))
    act = torch.tensor(np.stack([s["action"] for s in samples]), device="cuda")
    rows = []
    for prelude, amp in ((3, 0.0), (3, 1.0)):
        env = make_env(world, B, seed=1, terminal_com_dist=np.inf)
        env.set_next_trajectory_index(np.zeros(B, dtype=np.int64))
        env.reset()
        for k in range(prelude):
            env.step(torch.tensor(np.stack(actions(900 + k, B, amp)), device="cuda"))
        env.set_state(q, v)
        env.set_act(a)
        ts = env.step(act)
        rows.append(b"".join(x.cpu().numpy().tobytes() for x in (env.flat_observation, ts.reward, ts.discount, ts.step_type, *env.get_state(),
                                                                 env.get_act(), *env.get_task_state())))
        env.close()
    assert rows[0] == rows[1]


# ------------------------------------------------------------------------------------------------ g. downstream
def test_actor_loop_writer_and_episode_log(torch_mod, world):
    torch = torch_mod
    from flybody_amd import fly_envs
    from flybody_amd.actor_loop import BatchedActorLoop, EpisodeLog, NStepTransitionWriter
    from flybody_amd.batched_env import BatchedWalkEnv

    B, seed, calls = 3, 11, 40
    made = fly_envs.walk_imitation(floor_contacts="primitives", self_contacts=True, batch_size=2)
    assert type(made) is BatchedWalkEnv and made.floor_contacts and made.self_contacts and made.physics_flags == ENV
    assert made.reset().step_type.tolist() == [0, 0]
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
    assert REWARD_OPEN_MEASURED is not None, "the measured open-loop error has not been recorded"
    assert rerr <= EP_STEPS[0] * 3 * REWARD_OPEN_MEASURED  # a return is the sum of 35 rewards
    ob, a, r, d, o2 = writer.transitions()
    assert len(ob) > 0 and all(bool(torch.isfinite(x).all()) for x in (ob, a, r, d, o2))
    env.close()


# ------------------------------------------------------------------------------------------------ g. protocol
def test_protocol(torch_mod, world):
    torch = torch_mod
    from flybody_amd import _capi
    from flybody_amd.batched_env import BatchedWalkEnv, BatchedWalkPhysics
    from flybody_amd.model.blob import read_blob
    from flybody_amd.tasks.walk_tracker import make_task

    L = _capi.lib()
    blob = open(S.WALK_BLOB, "rb").read()
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

    BARE = ENV & ~WALK_EPISODES & ~WALK_SELF_EPISODES
    for flags in (ENV, ENV | NO_NOSLIP | NO_ADHESION | NO_FLUID | NO_GRAVITY):
        assert create(flags)[:2] == (0, True), flags
    # with the task: without the floor, with FFE_NO_LIMIT, without FFE_NO_CONTACT or the limits
    for flags in (ENV & ~WALK_FLOOR, ENV | NO_LIMIT, ENV & ~NO_CONTACT, ENV & ~WALK_JOINT_LIMITS, ENV | 16384, ENV & ~WALK_SELF,
                  ENV & ~WALK_EPISODES):
        rc, made, text = create(flags)
        assert rc == -1 and not made and "FFE_WALK_SELF" in text, (flags, text)
    # the three bits without FFE_WALK_SELF_EPISODES are the refusal tests/test_gpu_walk_floor_env.py pins, task or not
    rc, made, text = create(ENV & ~WALK_SELF_EPISODES)
    assert rc == -1 and not made and all(w in text for w in ("FFE_WALK_EPISODES", "FFE_WALK_FLOOR", "FFE_WALK_SELF_EPISODES")), text
    # without the task, which is what BatchedWalkPhysics(physics_flags=...) passes
    rc, made, text = create(ENV, with_task=False)
    assert rc == -1 and not made and "FFE_WALK_SELF" in text and "does not carry" in text and "null" in text
    rc, made, text = create(ENV & ~WALK_FLOOR, with_task=False)
    assert rc == -1 and not made and "FFE_WALK_SELF" in text
    with pytest.raises(RuntimeError, match="FFE_WALK_SELF.*does not carry"):
        BatchedWalkPhysics(batch_size=1, physics_flags=ENV)
    for bad in (BARE & ~WALK_FLOOR, BARE | NO_LIMIT, ENV & ~WALK_SELF_EPISODES):
        with pytest.raises(RuntimeError, match="FFE_WALK_SELF"):
            BatchedWalkPhysics(batch_size=1, physics_flags=bad)
    with pytest.raises(ValueError, match="floor_contacts"):
        BatchedWalkEnv(world[1], world[0], batch_size=1, self_contacts=True)
    with pytest.raises(ValueError):
        make_env(world, 1, flags=NO_LIMIT)
    with pytest.raises(ValueError):
        make_env(world, 1, flags=WALK_SELF, self_contacts=False)  # the bit comes from the keyword alone
    act = torch.tensor(np.stack([actions(800 + i, 1, 0.5)[0] for i in range(2)]), device="cuda")
    env = make_env(world, 2, NO_NOSLIP, seed=4)
    assert env.physics_flags == ENV | NO_NOSLIP and env.self_contacts
    env.reset()
    for _ in range(3):
        env.step(act)
    v = env.validity()
    assert v.episode_steps.tolist() == [3, 3] and v.step_bits.tolist() == [0, 0] and v.episode_bits.tolist() == [0, 0]
    s = env.spec
    assert (s.obs_dim, s.nq, s.nv, s.nu, s.action_dim, s.nsub, s.n_ref, s.n_obs_joints) == (741, 109, 108, 59, 59, 10, 65, 85)
    assert env.time_steps(act, 2) > 0 and env.time_kernel(act, 2) > 0
    ints, reals = (x.cpu().numpy() for x in env.get_task_state())
    assert (reals[:, 2] >= 1).all() and (ints[:, 5] > reals[:, 2]).all() and (reals[:, 3:] == 0).all()
    env.close()
    # the older floor env is unchanged: no bit, no fly-fly count
    old = make_env(world, 2, self_contacts=False, seed=4)
    assert old.physics_flags == ENV & ~WALK_SELF & ~WALK_SELF_EPISODES and not old.self_contacts
    old.reset()
    old.step(act)
    assert not old.get_task_state()[1].cpu().numpy()[:, 2:].any()
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
