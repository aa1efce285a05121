"""Validity reporting on the device: `env.validity()` (ffe_get_validity) of both task families, the n-step writer's taint column and
the actor loop's flagged totals.  Every comparison is between integers and exact.  Run with `-m gpu` on an MI355X."""
import numpy as np
import pytest

from test_gpu_contact_capacity import _crowded_states
from test_gpu_parity import torch_mod  # noqa: F401
from test_nstep import _reference
from test_validity_cpu import taint_restatement

pytestmark = pytest.mark.gpu


def _val(env):
    """validity() as four host arrays (step_bits, episode_flagged_steps, episode_bits, episode_steps)"""
    return [x.cpu().numpy().copy() for x in env.validity()]


# ---------------------------------------------------------------------------------------------------------------- 1
def test_forced_overflow(torch_mod, wb_tables):
    """States with 7 .. 12 self-contacts by the oracle: one control step of a capacity-6 env flags every one and counts it once; a
    capacity-12 env reports nothing; bare physics sets step_bits and leaves the episode's count alone; reset_envs zeroes its rows only."""
    from flybody_amd.batched_env import BatchedFlyEnv

    torch = torch_mod
    om, ref, states, poses, counts = _crowded_states(24, 6000)
    assert len(states) == 24, (len(states), poses)
    B = len(states)
    qpos, qvel = torch.tensor(np.stack([s[0] for s in states])), torch.tensor(np.stack([s[1] for s in states]))
    ctrl = torch.tensor(np.stack([s[2] for s in states]).astype(np.float32), device="cuda")

    def run(cap, physics):
        env = BatchedFlyEnv(wb_tables, *ref, batch_size=B, seed=3, contact_capacity=cap)
        env.reset()
        assert all((x == 0).all() for x in _val(env)[1:])
        env.set_state(qpos, qvel)
        if physics:
            env.physics_step(ctrl, 1)
        else:
            env.step(torch.zeros(B, env.spec.action_dim, device="cuda"))
        return env, _val(env)

    env6, v6 = run(6, False)
    print("capacity 6, one step: step_bits", v6[0].tolist(), "episode_flagged_steps", v6[1].tolist(), "episode_bits", v6[2].tolist())
    assert ((v6[0] & 1) == 1).all() and (v6[1] == 1).all() and ((v6[2] & 1) == 1).all() and (v6[3] == 1).all()
    # reset_envs on half the envs: those rows read 0, the others keep their values
    mask = torch.arange(B, device="cuda") % 2 == 0
    env6.reset_envs(mask)
    w = _val(env6)
    m = mask.cpu().numpy()
    for k in range(4):
        assert (w[k][m] == 0).all(), k
        assert (w[k][~m] == v6[k][~m]).all(), k
    env6.close()

    env12, v12 = run(12, False)
    print("capacity 12, one step: step_bits", v12[0].tolist(), "episode_flagged_steps", v12[1].tolist())
    assert (v12[0] == 0).all() and (v12[1] == 0).all() and (v12[2] == 0).all() and (v12[3] == 1).all()
    env12.close()

    envp, vp = run(6, True)
    print("capacity 6, one physics step: step_bits", vp[0].tolist())
    assert ((vp[0] & 1) == 1).all() and (vp[1] == 0).all() and (vp[2] == 0).all() and (vp[3] == 0).all()
    envp.close()


# ---------------------------------------------------------------------------------------------------------------- 2
def test_rollout_bookkeeping_against_an_independent_count(torch_mod, wb_tables, ref_traj):
    """The workload of test_gpu_contact_capacity._full_range_run (B = 256, 300 control steps of full-range canonical actions, capacity
    6): after every step validity() equals what is accumulated here from the older interface alone - task-state int 7 bits 8-15 and
    step_type.  A step counts when its int 7 flag or step_bits & 2 (the solver's iteration cap, which no older interface reports) is
    set; how often the second term mattered is printed.

    Measured on an MI355X with the 300 steps as they are: 801 flagged env-steps, 508 finished episodes, 245 of them with flagged steps
    (at most 11) and 263 without - both kinds finish within the run, it was not lengthened; no launch left the solver on its iteration
    cap, so the second term never mattered and `episode_bits & 2` stayed 0 throughout."""
    from flybody_amd.batched_env import BatchedFlyEnv

    torch = torch_mod
    B, steps = 256, 300
    env = BatchedFlyEnv(wb_tables, *ref_traj, batch_size=B, seed=2, canonical_actions=True, clip_actions=True)
    env.set_next_trajectory_index(np.arange(B) % 8, np.linspace(0.02, 0.98, B))
    ts = env.reset()
    v = _val(env)
    assert (ts.step_type.cpu().numpy() == 0).all() and all((x == 0).all() for x in v[1:])
    g = torch.Generator(device="cuda").manual_seed(3)
    cnt, nsteps, ebits = np.zeros(B, np.int64), np.zeros(B, np.int64), np.zeros(B, np.int64)
    finished, cap_exits, cap_only, flagged_rows, first_rows = [], 0, 0, 0, 0
    for k in range(steps):
        a = (torch.rand(B, 12, device="cuda", generator=g) * 2 - 1).contiguous()
        ts = env.step(a)
        st = ts.step_type.cpu().numpy()
        flag = ((env.get_task_state()[0][:, 7].cpu().numpy() >> 8) & 255) != 0
        sb, ef, eb, es = _val(env)
        assert ((sb & 1) == flag).all(), k                      # on every row, FIRST included
        assert ((sb & ~3) == 0).all(), k
        first = st == 0
        counted = (flag | ((sb & 2) != 0)) & ~first
        cap_exits += int(((sb & 2) != 0).sum())
        cap_only += int((((sb & 2) != 0) & ~flag & ~first).sum())
        flagged_rows += int(counted.sum())
        first_rows += int(first.sum())
        cnt = np.where(first, 0, cnt + counted)
        nsteps = np.where(first, 0, nsteps + 1)
        ebits = np.where(first, 0, ebits | np.where(counted, sb, 0))
        assert (ef == cnt).all() and (es == nsteps).all() and (eb == ebits).all(), k
        assert ((eb != 0) == (ef > 0)).all(), k
        finished += cnt[st == 2].tolist()                       # LAST rows show the episode's total
    env.close()
    with_flags, without = sum(c > 0 for c in finished), sum(c == 0 for c in finished)
    print(f"{B} envs x {steps} steps: {flagged_rows} flagged env-steps, {first_rows} FIRST rows, {len(finished)} finished episodes: {with_flags} with flagged "
          f"steps (most {max(finished, default=0)}), {without} without; launches that left the solver on its iteration cap: {cap_exits} "
          f"(of them counted for that reason alone: {cap_only})")
    assert with_flags >= 1 and without >= 1, (with_flags, without)


# ---------------------------------------------------------------------------------------------------------------- 3
@pytest.mark.parametrize("kind", ["flight_6", "flight_12", "walk_on_ball"])
def test_reading_validity_changes_nothing(torch_mod, wb_tables, ref_traj, kind):
    """Two envs, same seed and actions, validity() read after every step on one and never on the other: observation, reward,
    discount, step_type and the task state (int 7 included) stay equal bit for bit over 200 steps."""
    from flybody_amd.batched_env import BatchedBallEnv, BatchedFlyEnv

    torch = torch_mod
    B = 128 if kind != "walk_on_ball" else 32

    def make():
        if kind == "walk_on_ball":
            return BatchedBallEnv(batch_size=B, canonical_actions=True, clip_actions=True)
        return BatchedFlyEnv(wb_tables, *ref_traj, batch_size=B, seed=2, canonical_actions=True, clip_actions=True,
                             contact_capacity=int(kind.split("_")[1]))

    envs = [make(), make()]
    for e in envs:
        e.reset()
    g = torch.Generator(device="cuda").manual_seed(5)
    A = envs[0].spec.action_dim
    seen = 0
    for k in range(200):
        a = torch.rand(B, A, device="cuda", generator=g) * 2 - 1
        if kind == "walk_on_ball":
            a = torch.sign(a)
        a = a.contiguous()
        outs = []
        for i, e in enumerate(envs):
            ts = e.step(a)
            if i == 0:
                seen += int((e.validity().step_bits != 0).sum())
            outs.append((e.flat_observation.clone(), ts.reward.clone(), ts.discount.clone(), ts.step_type.clone(), *e.get_task_state()))
        for x, y in zip(*outs):
            assert torch.equal(x, y), k
    print(f"{kind}: env-steps with step_bits != 0 while comparing: {seen}")
    for e in envs:
        e.close()


# ---------------------------------------------------------------------------------------------------------------- 4
def test_walk_on_ball_bookkeeping(torch_mod):
    """64 envs, 120 control steps at +-1.0 (saturating) canonical actions.  The sticky overflow word (int 7) gives no per-step value
    to count from, so the checks are relations: episode_bits is int 7, step_bits a subset of it, the count grows exactly on flagged
    steps, episode_steps is the step counter, FIRST rows read zero.  The number of flagged env-steps is printed (measured on an MI355X:
    21 of 7 680 - 15 without the masked reset below -, so the non-zero branch of every relation runs; no episode ends by itself within
    120 steps, which is why every other env is reset after step 60)."""
    from flybody_amd.batched_env import BatchedBallEnv

    torch = torch_mod
    B = 64
    env = BatchedBallEnv(batch_size=B, canonical_actions=True, clip_actions=True)
    ts = env.reset()
    sb, ef, eb, es = _val(env)
    assert (ts.step_type.cpu().numpy() == 0).all() and (ef == 0).all() and (eb == 0).all() and (es == 0).all()
    g = torch.Generator(device="cuda").manual_seed(7)
    prev = ef.astype(np.int64)
    flagged, firsts = 0, 0
    for k in range(120):
        a = torch.sign(torch.rand(B, env.spec.action_dim, device="cuda", generator=g) - 0.5).contiguous()
        ts = env.step(a)
        st = ts.step_type.cpu().numpy()
        ints = env.get_task_state()[0].cpu().numpy()
        sb, ef, eb, es = _val(env)
        first = st == 0
        firsts += int(first.sum())
        assert (ef[first] == 0).all() and (eb[first] == 0).all() and (es[first] == 0).all(), k
        nf = ~first
        assert (eb[nf] == ints[nf, 7]).all(), k
        assert ((sb[nf] & ~eb[nf]) == 0).all(), k
        assert ((ef[nf] > 0) == (eb[nf] != 0)).all(), k
        assert (ef[nf] == np.where(first, 0, prev)[nf] + (sb[nf] != 0)).all(), k
        assert (es == ints[:, 2]).all(), k
        flagged += int((sb[nf] != 0).sum())
        prev = ef.astype(np.int64)
        if k == 59:   # no episode ends by itself within 120 steps: FIRST rows in mid-run come from a masked reset of every other env
            mask = torch.arange(B, device="cuda") % 2 == 0
            ts = env.reset_envs(mask)
            m = mask.cpu().numpy()
            sb2, ef2, eb2, es2 = _val(env)
            assert (ts.step_type.cpu().numpy()[m] == 0).all()
            assert (ef2[m] == 0).all() and (eb2[m] == 0).all() and (es2[m] == 0).all()
            assert (sb2[~m] == sb[~m]).all() and (ef2[~m] == ef[~m]).all() and (eb2[~m] == eb[~m]).all() and (es2[~m] == es[~m]).all()
            prev = ef2.astype(np.int64)
    env.close()
    print(f"walk_on_ball, {B} envs x 120 saturated steps: {flagged} env-steps with step_bits != 0, {firsts} FIRST rows after the reset")


# ---------------------------------------------------------------------------------------------------------------- 5
@pytest.mark.parametrize("n_step", [1, 5, 50])
def test_writer_taint_column(torch_mod, n_step):
    """The scripted sequences of tests/test_nstep.py plus random step_bits (about one step in ten flagged, FIRST rows included): the
    five ring arrays equal those of an untracked writer fed the same data bit for bit, the taint column equals the restatement."""
    from flybody_amd.actor_loop import NStepTransitionWriter
    from flybody_amd.dm_types import TimeStep

    torch = torch_mod
    B, O, A, T, gamma = 7, 11, 3, 160, 0.95
    rng = np.random.RandomState(n_step)
    obs = rng.randn(T, B, O).astype(np.float32)
    act = rng.randn(T, B, A).astype(np.float32)
    rew = rng.rand(T, B).astype(np.float32)
    disc = (rng.rand(T, B) > 0.1).astype(np.float32)
    st = np.ones((T, B), np.int32)
    st[0] = 0
    for b in range(B):
        t = 0
        while True:
            t += rng.randint(2, 70)
            if t + 1 >= T:
                break
            st[t, b], st[t + 1, b] = 2, 0
            t += 1
    bits = np.where(rng.rand(T, B) < 0.1, rng.randint(1, 4, (T, B)), 0).astype(np.int32)
    firsts = np.argwhere(st == 0)
    for t, b in firsts[::2]:          # flags on some FIRST rows for certain
        bits[t, b] = 1
    assert (bits[st == 0] != 0).any() and (bits[st == 0] == 0).any()
    w = NStepTransitionWriter(B, O, A, n_step=n_step, discount=gamma, capacity=4096, track_validity=True)
    plain = NStepTransitionWriter(B, O, A, n_step=n_step, discount=gamma, capacity=4096)
    dev = lambda x: torch.tensor(x, device="cuda")
    buf = torch.full((B, 4), -1, dtype=torch.int32, device="cuda")   # the other three columns must not be read
    for t in range(T):
        ts = TimeStep(dev(st[t]), dev(rew[t]), dev(disc[t]), None)
        a, o = dev(act[t]), dev(obs[t])
        buf[:, 0] = dev(bits[t])
        # the three accepted forms: the [B, 4] buffer, its first column as a view, a contiguous [B] tensor
        w.observe(a, ts, o, step_bits=(buf, buf[:, 0], dev(bits[t]))[t % 3])
        plain.observe(a, ts, o)
    got6 = [x.cpu().numpy() for x in w.transitions(with_taint=True)]
    got5 = [x.cpu().numpy() for x in plain.transitions()]
    assert len(w.transitions()) == 5 and got6[5].dtype == np.uint8
    ref = [tr for b in range(B) for tr in _reference(obs[:, b], act[:, b], rew[:, b], disc[:, b], st[:, b], n_step, gamma)]
    taint = [x for b in range(B) for x in taint_restatement(st[:, b], bits[:, b], n_step)]
    assert len(ref) == len(taint) == w.num_written() == plain.num_written() == len(got6[5]) > 0
    key = lambda oo, nn: (oo.tobytes(), nn.tobytes())
    tracked = {key(got6[0][i], got6[4][i]): (got6[1][i], got6[2][i], got6[3][i], int(got6[5][i])) for i in range(len(got6[2]))}
    untracked = {key(got5[0][i], got5[4][i]): (got5[1][i], got5[2][i], got5[3][i]) for i in range(len(got5[2]))}
    assert len(tracked) == len(untracked) == len(ref)
    for (oo, aa, rr, dd, nn), tt in zip(ref, taint):
        ga, gr, gd, gt = tracked[key(oo, nn)]
        ua, ur, ud = untracked[key(oo, nn)]
        assert np.array_equal(ga, ua) and gr.tobytes() == ur.tobytes() and gd.tobytes() == ud.tobytes()
        assert np.array_equal(ga, aa) and gr == rr and gd == dd
        assert gt == tt
    print(f"n_step {n_step}: {len(ref)} transitions, {sum(taint)} tainted, {int((bits != 0).sum())} flagged calls of {T * B}")
    assert 0 < sum(taint) < len(taint)
    # the refusals
    with pytest.raises(ValueError, match="step_bits"):
        w.observe(dev(act[0]), TimeStep(dev(st[0]), dev(rew[0]), dev(disc[0]), None), dev(obs[0]))
    with pytest.raises(ValueError, match="track_validity"):
        plain.observe(dev(act[0]), TimeStep(dev(st[0]), dev(rew[0]), dev(disc[0]), None), dev(obs[0]), step_bits=buf)
    with pytest.raises(ValueError, match="track_validity"):
        plain.transitions(with_taint=True)
    import ctypes as C

    p = C.c_void_p()
    assert plain._L.ffe_nstep_taint_buffer(plain._h, C.byref(p)) != 0
    assert b"without validity tracking" in plain._L.ffe_nstep_last_error(plain._h)
    w.close(); plain.close()


# ---------------------------------------------------------------------------------------------------------------- 6
def _flight_loop(torch, B, track, capacity, seed=0):
    from flybody_amd import fly_envs
    from flybody_amd.actor_loop import BatchedActorLoop, NStepTransitionWriter

    env = fly_envs.flight_imitation(batch_size=B, random_state=0)
    w = NStepTransitionWriter(B, env.spec.obs_dim, env.spec.action_dim, n_step=50, discount=0.99, capacity=capacity, track_validity=track)
    lo, hi = (torch.tensor(x, device="cuda") for x in env.raw_action_bounds())
    torch.manual_seed(seed)  # (the default generator: the one a HIP-graph capture can advance)
    loop = BatchedActorLoop(env, lambda obs: (lo + (hi - lo) * torch.rand(B, 12, device="cuda")), adder=w, track_validity=track)
    return env, w, loop


def test_actor_loop_reports_and_taints(torch_mod):
    """64 flight envs, 300 steps, random policy over the raw action spec, tracking on: the loop's totals equal what a wrapper around
    env.validity() collected, the ring holds as many tainted rows as the restatement gives for the recorded per-env streams, a graph
    run reports consistent totals, and with tracking off the result has exactly the keys it had before."""
    torch = torch_mod
    B, steps = 64, 300
    env, w, loop = _flight_loop(torch, B, True, B * 700)
    rec, last_st = [], {}
    inner_validity, inner_step, inner_reset = env.validity, env.step, env.reset

    def step(a):
        ts = inner_step(a)
        last_st["st"] = ts.step_type
        return ts

    def reset():
        ts = inner_reset()
        last_st["st"] = ts.step_type
        return ts

    def validity():
        v = inner_validity()
        rec.append((last_st["st"].cpu().numpy().copy(), env.validity_buffer.cpu().numpy().copy()))
        return v

    env.step, env.reset, env.validity = step, reset, validity
    stats = loop.run(steps)
    assert len(rec) == steps + 1                                  # the reset's observe_first and every iteration
    st = np.stack([r[0] for r in rec])
    info = np.stack([r[1] for r in rec])
    bits = info[:, :, 0]
    want_steps = int(((bits != 0) & (st != 0)).sum())
    last = st == 2
    want_eps = int((last & (info[:, :, 1] > 0)).sum())
    want_sum = int(info[:, :, 1][last].sum())
    print("eager:", {k: v for k, v in stats.items() if k != "steps_per_second"}, "recorded:", want_steps, want_eps, want_sum)
    assert stats["flagged_env_steps"] == want_steps > 0
    assert stats["flagged_episodes"] == want_eps and stats["episodes"] == int(last.sum())
    if want_eps:
        assert stats["flagged_steps_per_flagged_episode"] == want_sum / want_eps
    n = w.num_written()
    assert 0 < n <= w.capacity                                    # the ring did not wrap
    taint = w.transitions(with_taint=True)[5]
    want_taint = sum(sum(taint_restatement(st[:, b], bits[:, b], 50)) for b in range(B))
    want_rows = sum(len(taint_restatement(st[:, b], bits[:, b], 50)) for b in range(B))
    print(f"ring: {n} transitions, {int(taint.sum())} tainted (restatement {want_taint} of {want_rows})")
    assert n == want_rows and int(taint.sum()) == want_taint > 0
    w.close(); env.close()

    env, w, loop = _flight_loop(torch, B, True, B * 700)
    gs = loop.run(steps, graph=True)
    print("graph:", {k: v for k, v in gs.items() if k != "steps_per_second"})
    assert gs["flagged_episodes"] <= gs["episodes"] and gs["flagged_env_steps"] >= gs["flagged_episodes"]
    assert gs["flagged_env_steps"] > 0 and (gs["flagged_episodes"] > 0 or want_eps == 0)
    if gs["flagged_episodes"]:
        assert gs["flagged_steps_per_flagged_episode"] >= 1.0
    assert int(w.transitions(with_taint=True)[5].sum()) > 0
    w.close(); env.close()

    env, w, loop = _flight_loop(torch, B, False, B * 700)
    off = loop.run(50)
    assert set(off) == {"episodes", "episode_return", "episode_length", "steps_per_second", "capacity_flagged_envs"}
    w.close(); env.close()


def test_grouped_actor_loop_sums_its_groups(torch_mod):
    """Two asynchronous groups of 32 flight envs with tracking on, eager and as HIP graphs: the grouped result carries the three
    totals, consistent with each other and with the per-group device totals; off, the keys are those it always had."""
    from flybody_amd import fly_envs
    from flybody_amd.actor_loop import GroupedActorLoop, NStepTransitionWriter
    from flybody_amd.groups import EnvGroups

    torch = torch_mod
    B, G = 64, 2
    for track in (True, False):
        grp = EnvGroups(fly_envs.flight_imitation, B, groups=G, random_state=0)
        lo, hi = (torch.tensor(x, device="cuda") for x in grp.envs[0].raw_action_bounds())
        torch.manual_seed(0)
        policy = lambda obs: lo + (hi - lo) * torch.rand(obs.shape[0], 12, device="cuda")
        adders = [NStepTransitionWriter(B // G, e.spec.obs_dim, e.spec.action_dim, n_step=50, capacity=B * 700, track_validity=track) for e in grp.envs]
        loop = GroupedActorLoop(grp, policy, adders, track_validity=track)
        for graph in (False, True):
            r = loop.run(300, graph=graph)
            if not track:
                assert set(r) == {"episodes", "episode_return", "episode_length", "steps_per_second", "capacity_flagged_envs"}
                continue
            print("groups, graph" if graph else "groups, eager", {k: v for k, v in r.items() if k != "steps_per_second"})
            assert r["flagged_env_steps"] == sum(int(lp._vtot[0].item()) for lp in loop.loops) > 0
            assert 0 < r["flagged_episodes"] <= r["episodes"] and r["flagged_env_steps"] >= r["flagged_episodes"]
            assert r["flagged_steps_per_flagged_episode"] >= 1.0
            assert sum(int(a.transitions(with_taint=True)[5].sum()) for a in adders) > 0
        for a in adders:
            a.close()
        grp.close()
