"""The actor loop's statistics kernels (`episode_stats_kernel`, `validity_stats_kernel`, flybody_amd/csrc/nstep.hip: wave
reductions, one atomic per wave) against a host count: called directly on scripted streams at batches with a ragged last wave and
several workgroups, then through `BatchedActorLoop` on flight at a ragged batch, eager and as a HIP graph.  Integers and the
per-env float32 returns are compared exactly; the float64 return total, whose atomic order is free, to N * 2^-53 * sum|x| over its
N addends.  Run with `-m gpu -s` on an MI355X."""
import ctypes as C
import math

import numpy as np
import pytest

from test_gpu_parity import torch_mod  # noqa: F401

pytestmark = pytest.mark.gpu
FIRST, MID, LAST = 0, 1, 2
CALLS = 200
NO_LAST, ALL_LAST, TAIL_LAST = range(10, 15), (50, 120), (80, 160)      # calls with a forced shape


def _streams(B, seed):
    """step_type, reward [CALLS, B], validity records [CALLS, B, 4].  LAST is followed by FIRST; some episodes are abandoned (FIRST
    after MID); FIRST rows carry rewards and bits like any other row; forced calls: no env LAST, every env LAST, only the envs of
    the last (ragged) wave LAST."""
    rng = np.random.RandomState(seed)
    st = np.zeros((CALLS, B), np.int32)
    tail = np.arange(B) >= ((B - 1) // 64) * 64
    for t in range(1, CALLS):
        u = rng.rand(B)
        nxt = np.where(u < 0.08, LAST, np.where(u < 0.11, FIRST, MID))
        if t in NO_LAST or t + 1 in ALL_LAST or t + 1 in TAIL_LAST:
            nxt = np.where(nxt == LAST, MID, nxt)
        nxt = np.where(st[t - 1] == LAST, FIRST, nxt)
        if t in ALL_LAST:
            nxt = np.full(B, LAST)
        if t in TAIL_LAST:
            nxt = np.where(tail, LAST, np.where(nxt == LAST, MID, nxt))
        st[t] = nxt
    rew = (rng.rand(CALLS, B) - 0.3).astype(np.float32)
    info = np.full((CALLS, B, 4), -1, np.int32)
    info[:, :, 0] = np.where(rng.rand(CALLS, B) < 0.2, rng.randint(1, 4, (CALLS, B)), 0)
    info[:, :, 1] = np.where(rng.rand(CALLS, B) < 0.5, rng.randint(1, 12, (CALLS, B)), 0)
    info[:, :, 2:] = rng.randint(-5, 5, (CALLS, B, 2))               # episode_bits / episode_steps: not read by the totals
    return st, rew, info, tail


def _bound(addends):
    return len(addends) * 2.0 ** -53 * math.fsum(abs(x) for x in addends)


@pytest.mark.parametrize("B", [1, 63, 64, 65, 255, 257, 1000, 8192])
def test_statistics_kernels_against_a_host_count(torch_mod, B):
    from flybody_amd import _capi

    torch = torch_mod
    L = _capi.lib()
    st, rew, info, tail = _streams(B, seed=B)
    # the forced shapes are there
    assert all((st[t] != LAST).all() for t in NO_LAST) and all((st[t] == LAST).all() for t in ALL_LAST)
    assert all((st[t][tail] == LAST).all() and (st[t][~tail] != LAST).all() for t in TAIL_LAST)
    first = st == FIRST
    assert (rew[first] != 0).any() and (info[:, :, 0][first] != 0).any() and (info[:, :, 1][first] != 0).any()
    dev = lambda x: torch.tensor(x, device="cuda")
    st_d, rew_d, info_d = dev(st), dev(rew), dev(info)
    ep_ret = torch.zeros(B, device="cuda")
    ep_len = torch.zeros(B, dtype=torch.int64, device="cuda")
    tot = torch.zeros(2, dtype=torch.int64, device="cuda")
    sum_ret = torch.zeros(1, dtype=torch.float64, device="cuda")
    vtot = torch.zeros(3, dtype=torch.int64, device="cuda")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    h_ret, h_len = np.zeros(B, np.float32), np.zeros(B, np.int64)
    addends, h_tot, h_v = [], [0, 0], [0, 0, 0]
    worst = 0.0
    for t in range(CALLS):
        assert L.ffe_episode_stats(st_d[t].data_ptr(), rew_d[t].data_ptr(), ep_ret.data_ptr(), ep_len.data_ptr(), tot.data_ptr(), sum_ret.data_ptr(), B, stream) == 0
        assert info_d[t].data_ptr() % 16 == 0
        assert L.ffe_validity_stats(st_d[t].data_ptr(), info_d[t].data_ptr(), vtot.data_ptr(), B, stream) == 0
        nf, done = st[t] != FIRST, st[t] == LAST
        h_ret = np.where(nf, h_ret + rew[t], h_ret).astype(np.float32)      # float32, one add per step: bitwise
        h_len = h_len + nf
        addends += [float(x) for x in h_ret[done]]
        h_tot[0] += int(done.sum()); h_tot[1] += int(h_len[done].sum())
        h_ret[done], h_len[done] = 0.0, 0
        h_v[0] += int((nf & (info[t, :, 0] != 0)).sum())
        flagged = done & (info[t, :, 1] > 0)
        h_v[1] += int(flagged.sum()); h_v[2] += int(info[t, :, 1][flagged].sum())
        assert np.array_equal(ep_ret.cpu().numpy().view(np.uint32), h_ret.view(np.uint32)), t
        assert np.array_equal(ep_len.cpu().numpy(), h_len), t
        assert tot.tolist() == h_tot and vtot.tolist() == h_v, (t, tot.tolist(), h_tot, vtot.tolist(), h_v)
        err = abs(float(sum_ret.item()) - math.fsum(addends))
        assert err <= _bound(addends), (t, err, _bound(addends))
        worst = max(worst, err / _bound(addends) if addends else 0.0)
    assert h_tot[0] >= 2 * B and h_v[1] > 0 and h_v[0] > 0
    # a record buffer that is not 16-byte aligned is refused before anything is launched
    odd = torch.zeros(B * 4 + 4, dtype=torch.int32, device="cuda")
    before = vtot.tolist()
    assert L.ffe_validity_stats(st_d[0].data_ptr(), odd.data_ptr() + 4, vtot.data_ptr(), B, stream) == -1
    assert L.ffe_validity_stats(st_d[0].data_ptr(), odd.data_ptr() + 8, vtot.data_ptr(), B, stream) == -1
    torch.cuda.synchronize()
    assert vtot.tolist() == before
    print(f"\nB {B}: {CALLS} calls, {h_tot[0]} finished episodes of {h_tot[1]} steps, flagged steps / episodes / their sum {h_v}; float64 return total "
          f"{float(sum_ret.item()):.12f} (host {math.fsum(addends):.12f}), largest error / bound {worst:.3f} (bound at the end {_bound(addends):.2e})")


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_actor_loop_totals_at_a_ragged_batch(torch_mod, graph):
    """BatchedActorLoop on 1000 flight envs (15 full waves and one of 40), 300 steps, validity tracking on: episodes, episode_length,
    episode_return and the flagged totals against a host accumulation of every TimeStep and validity record the loop saw.  The
    wrappers record on the device (a counter tensor indexes the history), so a HIP graph's replays are recorded as well; a graph run
    executes its three warm-up iterations and the 300 replays (the capture itself executes nothing) and its totals cover all 303."""
    from flybody_amd import fly_envs
    from flybody_amd.actor_loop import BatchedActorLoop

    torch = torch_mod
    B, steps = 1000, 300
    env = fly_envs.flight_imitation(batch_size=B, random_state=0)
    lo, hi = (torch.tensor(x, device="cuda") for x in env.raw_action_bounds())
    torch.manual_seed(1)
    loop = BatchedActorLoop(env, lambda obs: (lo + (hi - lo) * torch.rand(B, 12, device="cuda")), track_validity=True)
    room = steps + 8
    h_st = torch.full((room, B), -1, dtype=torch.int32, device="cuda")
    h_rew = torch.zeros(room, B, device="cuda")
    h_info = torch.zeros(room, B, 4, dtype=torch.int32, device="cuda")
    n_step, n_val = torch.zeros(1, dtype=torch.int64, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda")
    inner_step, inner_validity, inner_reset = env.step, env.validity, env.reset

    def step(a):
        ts = inner_step(a)
        h_st.index_copy_(0, n_step, ts.step_type[None]); h_rew.index_copy_(0, n_step, ts.reward[None]); n_step.add_(1)
        return ts

    def validity():
        v = inner_validity()
        h_info.index_copy_(0, n_val, env.validity_buffer[None]); n_val.add_(1)
        return v

    def reset():
        ts = inner_reset()
        n_step.zero_(); n_val.zero_()
        return ts

    env.step, env.validity, env.reset = step, validity, reset
    stats = loop.run(steps, graph=graph)
    torch.cuda.synchronize()
    ran = int(n_step.item())
    assert ran == int(n_val.item()) == steps + (3 if graph else 0), ran
    st, rew, info = h_st[:ran].cpu().numpy(), h_rew[:ran].cpu().numpy(), h_info[:ran].cpu().numpy()
    assert (st >= 0).all()
    h_ret, h_len = np.zeros(B, np.float32), np.zeros(B, np.int64)
    addends, eps, length, v = [], 0, 0, [0, 0, 0]
    tail_last = 0
    for t in range(ran):
        nf, done = st[t] != FIRST, st[t] == LAST
        h_ret = np.where(nf, h_ret + rew[t], h_ret).astype(np.float32)
        h_len = h_len + nf
        addends += [float(x) for x in h_ret[done]]
        eps += int(done.sum()); length += int(h_len[done].sum())
        tail_last += int(done[960:].sum())
        h_ret[done], h_len[done] = 0.0, 0
        v[0] += int((nf & (info[t, :, 0] != 0)).sum())
        flagged = done & (info[t, :, 1] > 0)
        v[1] += int(flagged.sum()); v[2] += int(info[t, :, 1][flagged].sum())
    print(f"\n{'graph' if graph else 'eager'}: {ran} iterations recorded; host: {eps} episodes, {length} steps, return sum {math.fsum(addends):.9f}, flagged {v}, "
          f"{tail_last} episodes ended in the ragged last wave; loop:", {k: x for k, x in stats.items() if k != "steps_per_second"})
    assert eps > B // 2 and tail_last > 0 and v[1] > 0
    assert stats["episodes"] == eps == int(loop._tot[0].item()) and int(loop._tot[1].item()) == length
    assert stats["episode_length"] == length / eps
    assert np.array_equal(loop._ret.cpu().numpy().view(np.uint32), h_ret.view(np.uint32)) and np.array_equal(loop._len.cpu().numpy(), h_len)
    total = float(loop._sum_ret.item())
    assert abs(total - math.fsum(addends)) <= _bound(addends), (total, math.fsum(addends), _bound(addends))
    assert stats["episode_return"] == total / eps
    assert stats["flagged_env_steps"] == v[0] and stats["flagged_episodes"] == v[1] and stats["flagged_steps_per_flagged_episode"] == v[2] / v[1]
    env.close()
