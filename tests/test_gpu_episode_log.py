"""The per-episode log on the device (`ffe_eplog_*`, flybody_amd/csrc/episode_log.hip; `flybody_amd.actor_loop.EpisodeLog`,
`BatchedEvaluator`) against its numpy restatement (tests/episode_log_restatement.py, pinned without a device by
tests/test_episode_log_cpu.py).

The kernel is driven through the C ABI on scripted streams (no env), then through `BatchedActorLoop` on flight and walk_on_ball and
through `BatchedEvaluator`.  Records are compared bit for bit after the canonical (call, env) sort; the one tolerance here is on the
loop's float64 return total, whose atomic order is free.  Run with `-m gpu -s` on an MI355X."""
import ctypes as C
import math

import numpy as np
import pytest

import episode_log_restatement as R
from episode_log_restatement import FIRST, LAST, MID
from test_gpu_parity import torch_mod  # noqa: F401

pytestmark = pytest.mark.gpu


def _script(B, calls, seed, all_last_at):
    """step_type [calls, B]: episodes drawn with 1 .. 29 steps (half of them 1 .. 3 steps, a sixth exactly one: FIRST then LAST; 30 when
    stretched by one step to end in the all-LAST call), each followed by FIRST; three MID rows in a hundred are replaced by FIRST (the episode is abandoned); at call `all_last_at` every env is LAST
    (the call before it has none).  FIRST rows carry rewards, discounts, info and tags like any other row."""
    rng = np.random.RandomState(seed)

    def lengths(n):
        u = rng.rand(n)
        return np.where(u < 1 / 6, 1, np.where(u < 0.5, rng.randint(1, 4, n), rng.randint(1, 30, n)))

    st = np.zeros((calls, B), np.int32)
    rem = lengths(B)                                                 # steps the running episode still has to make
    for t in range(1, calls):
        prev, fresh, abandon = st[t - 1], lengths(B), rng.rand(B) < 0.03
        if t == all_last_at:
            st[t], rem = LAST, np.zeros(B, np.int64)
            continue
        restart = (prev == LAST) | (abandon & (prev == MID))
        rem = np.where(restart, fresh, rem - 1)
        nxt = np.where(restart, FIRST, np.where(rem == 0, LAST, MID))
        if t + 1 == all_last_at:                                     # no LAST here: those episodes get one more step
            rem = np.where(nxt == LAST, 1, rem)
            nxt = np.where(nxt == LAST, MID, nxt)
        st[t] = nxt
    return st


def _inputs(B, calls, seed, all_last_at):
    rng = np.random.RandomState(seed + 1000)
    st = _script(B, calls, seed, all_last_at)
    rew = (rng.rand(calls, B) - 0.3).astype(np.float32)
    disc = (rng.rand(calls, B) < 0.5).astype(np.float32)             # LAST rows with discount 0 (terminated) and 1 (time limit)
    info = rng.randint(0, 1 << 20, (calls, B, 4)).astype(np.int32)
    info[:, :, 1] = np.where(rng.rand(calls, B) < 0.5, rng.randint(1, 3000, (calls, B)), 0)
    wide = rng.randint(-(1 << 31), 1 << 31, (calls, B, 8)).astype(np.int32)  # tags as column 3 of a [B, 8] buffer: any int32
    return st, rew, disc, info, wide


class Handle:
    """an ffe_eplog handle through the raw C ABI"""

    def __init__(self, torch, B, capacity, flags=0):
        from flybody_amd import _capi
        from flybody_amd.actor_loop import _device_view

        self.torch, self.L, self.B, self.capacity = torch, _capi.lib(), B, capacity
        self.h = C.c_void_p()
        rc = self.L.ffe_eplog_create(B, capacity, flags, 0, C.byref(self.h))
        assert rc == 0, self.L.ffe_eplog_last_error(None).decode()
        rec, info = C.c_void_p(), C.c_void_p()
        assert self.L.ffe_eplog_buffers(self.h, C.byref(rec), C.byref(info)) == 0
        assert rec.value % 32 == 0
        dev = torch.device("cuda", 0)
        self._rec = _device_view(torch, dev, rec.value, (capacity * 32,), "|u1")
        self._info = _device_view(torch, dev, info.value, (4,), "<i8")

    def stream(self):
        return C.c_void_p(self.torch.cuda.current_stream().cuda_stream)

    def observe(self, st, rew, disc, info=None, tag=None, stride=1):
        rc = self.L.ffe_eplog_observe(self.h, st.data_ptr(), rew.data_ptr(), disc.data_ptr(), info.data_ptr() if info is not None else None,
                                      tag.data_ptr() if tag is not None else None, stride, self.stream())
        assert rc == 0, self.L.ffe_eplog_last_error(self.h).decode()

    def arm(self, mask=None):
        return self.L.ffe_eplog_arm(self.h, mask.data_ptr() if mask is not None else None, self.stream())

    def info(self):
        self.torch.cuda.synchronize()
        return self._info.tolist()

    def slots(self):
        """the ring as it lies, slot order (synchronises)"""
        self.torch.cuda.synchronize()
        return self._rec.cpu().numpy().view(R.DTYPE)

    def close(self):
        assert self.L.ffe_eplog_destroy(self.h) == 0


def _check_ring(h, ref):
    """info block and ring of handle `h` against restatement `ref`; `call` non-decreasing in count order"""
    info = h.info()
    assert info[0] == ref.count and info[1] == ref.calls and info[3] == 0, (info, ref.count, ref.calls)
    slots = h.slots()
    n = min(ref.count, h.capacity)
    ref.check_ring(slots[:n])
    if n:
        start = ref.count % h.capacity if ref.count > h.capacity else 0
        in_count_order = np.concatenate([slots[start:n], slots[:start]])
        assert (np.diff(in_count_order["call"]) >= 0).all(), "records of a later call lie before those of an earlier one"
    if n < h.capacity:
        assert not slots[n:].view(np.uint8).any(), "a slot beyond the count was written"


# variant: (ring wraps, info given, tags: None / 1 = contiguous [B] / 8 = column 3 of [B, 8])
VARIANTS = {"wrap-info-col3": (True, True, 8), "nowrap-noinfo-notag": (False, False, None), "wrap-noinfo-stride1": (True, False, 1),
            "nowrap-info-stride1": (False, True, 1)}


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("B", [1, 63, 64, 65, 257, 8192])
def test_kernel_against_the_restatement(torch_mod, B, variant):
    torch = torch_mod
    wrap, with_info, tag_mode = VARIANTS[variant]
    calls = 200 if B < 8192 else 100
    all_last_at = calls // 2
    st, rew, disc, info, wide = _inputs(B, calls, seed=B, all_last_at=all_last_at)
    # the script has what it promises
    assert (st[all_last_at] == LAST).all() and (st[all_last_at - 1] != LAST).all()
    assert ((st[1:] == LAST) & (st[:-1] == FIRST)).any() or B == 1          # one-step episodes
    assert ((st[1:] == FIRST) & (st[:-1] == MID)).any() or B == 1           # abandoned episodes
    total = int((st == LAST).sum())
    capacity = B if wrap else total + 3
    assert total >= 6 * B
    dev = lambda x: torch.tensor(x, device="cuda")
    st_d, rew_d, disc_d, info_d, wide_d = dev(st), dev(rew), dev(disc), dev(info), dev(wide)
    flat_d = dev(np.ascontiguousarray(wide[:, :, 3]))
    h = Handle(torch, B, capacity)
    ref = R.EpisodeLogRestatement(B, capacity)
    seen_last_disc = set()
    for t in range(calls):
        tag_d, tag_h, stride = None, None, 1
        if tag_mode == 8:
            tag_d, tag_h, stride = wide_d[t][:, 3], wide[t, :, 3], 8
            assert tag_d.data_ptr() == wide_d[t].data_ptr() + 12
        elif tag_mode == 1:
            tag_d, tag_h = flat_d[t], wide[t, :, 3]
        h.observe(st_d[t], rew_d[t], disc_d[t], info_d[t] if with_info else None, tag_d, stride)
        ref.observe(st[t], rew[t], disc[t], info[t] if with_info else None, tag_h)
        seen_last_disc |= set(disc[t][st[t] == LAST].tolist())
        if t in (all_last_at - 1, all_last_at, calls - 1):
            _check_ring(h, ref)
    assert seen_last_disc == {0.0, 1.0} or B == 1
    assert ref.count == total and (ref.count >= 6 * capacity if wrap else ref.count < capacity)
    print(f"\nB {B} {variant}: {calls} calls, {ref.count} records, capacity {capacity} ({ref.count / capacity:.1f} x the ring)")
    h.close()


def test_one_shot_arming(torch_mod):
    """B = 130 (two full wavefronts and one of two lanes): nothing armed, a mask, all envs mid-run, a mask again; armed_left after every
    call, the ring at the end; arm on a plain log fails with a text"""
    torch = torch_mod
    B, calls = 130, 120
    st, rew, disc, info, wide = _inputs(B, calls, seed=7, all_last_at=70)
    dev = lambda x: torch.tensor(x, device="cuda")
    st_d, rew_d, disc_d, info_d, wide_d = dev(st), dev(rew), dev(disc), dev(info), dev(wide)
    h = Handle(torch, B, 4 * B, flags=1)
    ref = R.EpisodeLogRestatement(B, 4 * B, one_shot=True)
    rng = np.random.RandomState(3)
    arms = {10: (rng.rand(B) < 0.4).astype(np.uint8), 50: None, 75: (np.arange(B) >= 126).astype(np.uint8)}
    zero_at = []
    for t in range(calls):
        if t in arms:
            m = arms[t]
            assert h.arm(dev(m) if m is not None else None) == 0
            ref.arm(m)
            assert h.info()[2] == ref.armed_left == (B if m is None else int(m.sum()))
        h.observe(st_d[t], rew_d[t], disc_d[t], info_d[t], wide_d[t][:, 3], 8)
        before = ref.armed_left
        rec = ref.observe(st[t], rew[t], disc[t], info[t], wide[t, :, 3])
        got = h.info()
        assert got[2] == ref.armed_left and got[0] == ref.count, (t, got, ref.armed_left, ref.count)
        if t < 10:
            assert len(rec) == 0 and got[0] == 0                         # nothing armed yet: LAST rows emit nothing
        if before > 0 and ref.armed_left == 0:
            zero_at.append(t)
    assert len(zero_at) == 3 and zero_at[0] < 50 < zero_at[1] <= 70 < 75 < zero_at[2], zero_at  # each arming runs out; the second at the all-LAST call at the latest
    _check_ring(h, ref)
    got = R.canonical(h.slots()[:ref.count])
    armed_envs = np.nonzero(arms[10])[0]
    first_round = got[got["call"] < 50]
    assert sorted(first_round["env"].tolist()) == sorted(armed_envs.tolist())  # every armed env once, no other env at all
    assert sorted(got[got["call"] > 75]["env"].tolist()) == [126, 127, 128, 129]
    h.close()
    plain = Handle(torch, 8, 8)
    assert plain.arm() < 0 and "not created one-shot" in plain.L.ffe_eplog_last_error(plain.h).decode()
    assert plain.info() == [0, 0, 0, 0]
    plain.close()


def test_refusals_have_a_text(torch_mod):
    from flybody_amd import _capi
    from flybody_amd.actor_loop import EpisodeLog
    from flybody_amd.dm_types import TimeStep

    torch = torch_mod
    L = _capi.lib()
    out = C.c_void_p()
    for args, text in (((8, 7, 0, 0), "capacity 7 is below batch = 8"), ((0, 4, 0, 0), "batch 0"), ((4, 4, 2, 0), "unknown flags"), ((4, 4, 0, 99), "no such HIP device")):
        assert L.ffe_eplog_create(*args, C.byref(out)) < 0 and not out.value
        assert text in L.ffe_eplog_last_error(None).decode(), (args, L.ffe_eplog_last_error(None).decode())
    assert L.ffe_eplog_create(4, 4, 0, 0, None) < 0 and "null out" in L.ffe_eplog_last_error(None).decode()
    h = Handle(torch, 4, 4)
    st, x = torch.zeros(4, dtype=torch.int32, device="cuda"), torch.zeros(4, device="cuda")
    tag = torch.zeros(4, dtype=torch.int32, device="cuda")
    s = h.stream()
    for args, text in (((None, x.data_ptr(), x.data_ptr(), None, None, 1), "a null input"), ((st.data_ptr(), None, x.data_ptr(), None, None, 1), "a null input"),
                       ((st.data_ptr(), x.data_ptr(), None, None, None, 1), "a null input"), ((st.data_ptr(), x.data_ptr(), x.data_ptr(), None, tag.data_ptr(), 0), "tag_stride_ints 0"),
                       ((st.data_ptr(), x.data_ptr(), x.data_ptr(), None, tag.data_ptr(), -8), "tag_stride_ints -8")):
        assert L.ffe_eplog_observe(h.h, *args, s) < 0 and text in L.ffe_eplog_last_error(h.h).decode(), args
    assert L.ffe_eplog_observe(h.h, st.data_ptr(), x.data_ptr(), x.data_ptr(), None, None, 0, s) == 0   # the stride is not read without tags
    assert L.ffe_eplog_buffers(h.h, None, None) < 0 and "null output" in L.ffe_eplog_last_error(h.h).decode()
    assert h.info() == [0, 1, 0, 0]                                  # the refused calls launched nothing
    h.close()
    rec = C.c_void_p()
    for call, text in ((lambda: L.ffe_eplog_observe(None, st.data_ptr(), x.data_ptr(), x.data_ptr(), None, None, 1, s), "ffe_eplog_observe: null handle"),
                       (lambda: L.ffe_eplog_arm(None, None, s), "ffe_eplog_arm: null handle"), (lambda: L.ffe_eplog_buffers(None, C.byref(rec), C.byref(rec)), "ffe_eplog_buffers: null handle"),
                       (lambda: L.ffe_eplog_destroy(None), "ffe_eplog_destroy: null handle")):
        assert call() < 0 and L.ffe_eplog_last_error(None).decode() == text
    # the Python class checks what the raw pointers cannot
    log = EpisodeLog(4, capacity=4)
    good = TimeStep(st, x, x, None)
    log.observe(good)
    for ts in (TimeStep(st.long(), x, x, None), TimeStep(st, x.double(), x, None), TimeStep(st.cpu(), x, x, None), TimeStep(st, x, torch.zeros(8, device="cuda")[::2], None),
               TimeStep(st, torch.zeros(5, device="cuda"), x, None)):
        with pytest.raises(ValueError, match="step_type int32"):
            log.observe(ts)
    with pytest.raises(ValueError, match="validity"):
        log.observe(good, validity=torch.zeros(4, 3, dtype=torch.int32, device="cuda"))
    with pytest.raises(TypeError, match="tags must be an int32"):
        log.observe(good, tags=torch.zeros(4, dtype=torch.int64, device="cuda"))
    with pytest.raises(ValueError, match="tags must have shape"):
        log.observe(good, tags=torch.zeros(4, 2, dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError, match="tags must live"):
        log.observe(good, tags=torch.zeros(4, dtype=torch.int32))
    with pytest.raises(ValueError, match="one_shot=True"):
        log.arm()
    assert log.info() == {"written": 0, "calls": 1, "armed_left": 0} and len(log.records()) == 0
    log.close()
    with pytest.raises(RuntimeError, match="closed"):
        log.observe(good)


def test_observe_captured_into_a_graph_equals_the_eager_run(torch_mod):
    """one observe (info given, tags as column 3 at stride 8) captured once, after three eager calls on a side stream as
    BatchedActorLoop.run(graph=True) does, and replayed 50 times over input tensors that are rewritten between the replays: records
    and info block equal those of a second handle fed the same 53 calls eagerly, and the restatement"""
    torch = torch_mod
    B, calls = 200, 53
    st, rew, disc, info, wide = _inputs(B, calls, seed=11, all_last_at=30)
    dev = lambda x: torch.tensor(x, device="cuda")
    st_d, rew_d, disc_d, info_d, wide_d = dev(st), dev(rew), dev(disc), dev(info), dev(wide)
    capacity = int((st == LAST).sum()) + 1
    eager, graphed, ref = Handle(torch, B, capacity), Handle(torch, B, capacity), R.EpisodeLogRestatement(B, capacity)
    for t in range(calls):
        eager.observe(st_d[t], rew_d[t], disc_d[t], info_d[t], wide_d[t][:, 3], 8)
        ref.observe(st[t], rew[t], disc[t], info[t], wide[t, :, 3])
    s_st, s_rew, s_disc, s_info, s_wide = (torch.zeros_like(x[0]) for x in (st_d, rew_d, disc_d, info_d, wide_d))

    def load(t):
        for dst, src in ((s_st, st_d), (s_rew, rew_d), (s_disc, disc_d), (s_info, info_d), (s_wide, wide_d)):
            dst.copy_(src[t])

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for t in range(3):
            load(t)
            graphed.observe(s_st, s_rew, s_disc, s_info, s_wide[:, 3], 8)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        graphed.observe(s_st, s_rew, s_disc, s_info, s_wide[:, 3], 8)   # captured, not run
    torch.cuda.synchronize()
    assert graphed.info()[1] == 3
    for t in range(3, calls):
        load(t)
        g.replay()
    assert graphed.info() == eager.info() == [ref.count, calls, 0, 0]
    a, b = R.canonical(eager.slots()[:ref.count]), R.canonical(graphed.slots()[:ref.count])
    assert a.tobytes() == b.tobytes() == ref.all_records().tobytes() and ref.count > B
    eager.close(); graphed.close()


# ------------------------------------------------------------------------------------------------ through the loop
def _recorded_loop(torch, env, policy, steps, graph):
    """BatchedActorLoop with a log and validity tracking over `env`, every TimeStep, validity record and task-state traj_idx the loop
    saw recorded on the device (the method of tests/test_gpu_loop_stats.py: a counter tensor indexes the history, so a graph's
    replays are recorded too).  Returns (stats, loop, log, history as numpy)."""
    from flybody_amd.actor_loop import BatchedActorLoop, EpisodeLog

    B = env.batch_size
    log = EpisodeLog(B)
    loop = BatchedActorLoop(env, policy, track_validity=True).log_episodes(log)
    room = steps + 8
    h_st = torch.full((room, B), -1, dtype=torch.int32, device="cuda")
    h_rew, h_disc = torch.zeros(room, B, device="cuda"), torch.zeros(room, B, device="cuda")
    h_traj = torch.zeros(room, B, dtype=torch.int32, device="cuda")
    h_info = torch.zeros(room, B, 4, dtype=torch.int32, device="cuda")
    n_step, n_val = torch.zeros(1, dtype=torch.int64, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda")
    inner_step, inner_validity, inner_reset = env.step, env.validity, env.reset
    is_flight = env.task_kind == "flight_imitation"

    def step(a):
        ts = inner_step(a)
        h_st.index_copy_(0, n_step, ts.step_type[None]); h_rew.index_copy_(0, n_step, ts.reward[None]); h_disc.index_copy_(0, n_step, ts.discount[None])
        if is_flight:
            h_traj.index_copy_(0, n_step, env.get_task_state()[0][:, 3][None])
        n_step.add_(1)
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
    assert ran == int(n_val.item()) == steps + (3 if graph else 0)
    hist = [x[:ran].cpu().numpy() for x in (h_st, h_rew, h_disc, h_info, h_traj)]
    assert (hist[0] >= 0).all()
    return stats, loop, log, hist


def _check_loop(stats, loop, log, hist, B, tagged):
    st, rew, disc, info, traj = hist
    ref = R.EpisodeLogRestatement(B, log.capacity)
    ref.observe(np.full(B, FIRST), np.zeros(B), np.ones(B))          # call 0: the timestep of the loop's reset
    for t in range(len(st)):
        ref.observe(st[t], rew[t], disc[t], info[t], traj[t] if tagged else None)
    want = ref.all_records()
    got = log.records()
    assert stats["episode_log"] is log and log.info() == {"written": ref.count, "calls": len(st) + 1, "armed_left": 0}
    assert ref.count <= log.capacity and got.dtype == R.DTYPE and got.tobytes() == want.tobytes()
    assert set(got["env"].tolist()) == set(range(B)), "an env finished no episode"
    # the loop's own totals (ffe_episode_stats): counts exactly, the float64 return total up to its free atomic order
    n = len(got)
    assert stats["episodes"] == n == int(loop._tot[0].item()) and int(loop._tot[1].item()) == int(got["length"].sum())
    rets = [float(x) for x in got["ret"]]
    total = float(loop._sum_ret.item())
    bound = n * 2.0 ** -52 * math.fsum(abs(x) for x in rets)
    assert abs(total - math.fsum(rets)) <= bound, (total, math.fsum(rets), bound)
    s = log.summary()
    assert s["episodes"] == n and s["flagged_episodes"] == stats["flagged_episodes"] and abs(s["avg_episode_length"] - stats["episode_length"]) <= 1e-9 * stats["episode_length"]
    return got


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_flight_loop_records_equal_a_host_accumulation(torch_mod, wb_tables, ref_traj, graph):
    """128 flight envs, 8 synthetic clips, random full-range actions, a 0.05 s time limit: time limit + 2 steps, by which every env
    has finished an episode whatever it did (most terminate long before)"""
    from flybody_amd.batched_env import BatchedFlyEnv

    torch = torch_mod
    B = 128
    env = BatchedFlyEnv(wb_tables, *ref_traj, batch_size=B, seed=3, time_limit=0.05)
    lo, hi = (torch.tensor(x, device="cuda") for x in env.raw_action_bounds())
    torch.manual_seed(2)
    steps = env.time_limit_steps + 2
    stats, loop, log, hist = _recorded_loop(torch, env, lambda obs: lo + (hi - lo) * torch.rand(B, 12, device="cuda"), steps, graph)
    got = _check_loop(stats, loop, log, hist, B, tagged=True)
    assert len(set(got["tag"].tolist())) > 1 and 0 <= got["tag"].min() and got["tag"].max() < 8
    term = (got["bits"] & 256) != 0
    per_clip = log.summary(by_tag=True, num_tags=8)
    assert per_clip["episodes"].sum() == len(got)
    print(f"\nflight {'graph' if graph else 'eager'}: {len(hist[0])} steps, {len(got)} episodes, {int(term.sum())} terminated, lengths {got['length'].min()} .. {got['length'].max()}, "
          f"flagged episodes {int((got['flagged_steps'] > 0).sum())}, episodes per clip {per_clip['episodes'].tolist()}")
    assert got["length"].max() <= env.time_limit_steps
    log.close(); env.close()


def test_ball_loop_records_equal_a_host_accumulation(torch_mod):
    """64 walk_on_ball envs with a 0.2 s time limit, time limit + 2 steps; no clips: every tag is 0"""
    from flybody_amd.batched_env import BatchedBallEnv

    torch = torch_mod
    B = 64
    env = BatchedBallEnv(batch_size=B, time_limit=0.2)
    lo, hi = (torch.tensor(x, device="cuda") for x in env.raw_action_bounds())
    torch.manual_seed(4)
    A = env.spec.action_dim
    steps = env.time_limit_steps + 2
    stats, loop, log, hist = _recorded_loop(torch, env, lambda obs: lo + (hi - lo) * torch.rand(B, A, device="cuda"), steps, False)
    got = _check_loop(stats, loop, log, hist, B, tagged=False)
    assert not got["tag"].any()
    print(f"\nwalk_on_ball: {len(hist[0])} steps, {len(got)} episodes, lengths {got['length'].min()} .. {got['length'].max()}, bits {sorted(set(got['bits'].tolist()))}")
    log.close(); env.close()


def test_grouped_loop_logs_equal_one_handle(torch_mod):
    """64 flight envs as two asynchronous groups of 32, one log per group, against the same envs as one handle with one log: envs do
    not depend on the grouping and the policy here is a function of the observation, so the groups' records - env index shifted by
    the group's first env - are the single handle's, byte for byte, and `summarize` of their concatenation is its summary"""
    from flybody_amd import fly_envs
    from flybody_amd.actor_loop import BatchedActorLoop, EpisodeLog, GroupedActorLoop, summarize
    from flybody_amd.groups import EnvGroups

    torch = torch_mod
    B, G, steps = 64, 2, 300
    one = fly_envs.flight_imitation(batch_size=B, random_state=0)
    lo, hi = (torch.tensor(x, device="cuda") for x in one.raw_action_bounds())
    policy = lambda obs: lo + (hi - lo) * (0.5 + 0.5 * torch.sin(37.0 * obs[:, :12]))
    log = EpisodeLog(B)
    stats = BatchedActorLoop(one, policy).log_episodes(log).run(steps)
    want = log.records()
    assert stats["episodes"] == len(want) > 0
    groups = EnvGroups(fly_envs.flight_imitation, B, groups=G, random_state=0)
    logs = [EpisodeLog(B // G) for _ in range(G)]
    gstats = GroupedActorLoop(groups, policy, episode_logs=logs).run(steps)
    assert gstats["episode_logs"] == logs and gstats["episodes"] == len(want)
    parts = []
    for g, lg in enumerate(logs):
        rec = lg.records()
        rec["env"] += g * (B // G)
        parts.append(rec)
    both = np.concatenate(parts)
    assert R.canonical(both).tobytes() == want.tobytes()
    assert summarize(both) == log.summary() and len(set(want["tag"].tolist())) > 1
    print(f"\ngrouped: {len(want)} episodes in {steps} steps, {[len(p) for p in parts]} per group")
    for lg in logs + [log]:
        lg.close()
    groups.close(); one.close()


# ------------------------------------------------------------------------------------------------ evaluator
def _evaluate(torch, wb_tables, ref_traj, B, seed):
    from flybody_amd.actor_loop import BatchedEvaluator
    from flybody_amd.batched_env import BatchedFlyEnv

    env = BatchedFlyEnv(wb_tables, *ref_traj, batch_size=B, seed=9, time_limit=0.03)
    snaps = []

    def policy(obs):
        snaps.append(env.get_task_state()[0][:, 3].clone())
        return torch.zeros(B, env.spec.action_dim, device="cuda")

    ev = BatchedEvaluator(env, policy, episodes_per_clip=3, seed=seed, poll_every=16)
    out = ev.run()
    snaps = torch.stack(snaps).cpu().numpy()
    env.close()
    return ev, out, snaps


@pytest.mark.parametrize("B", [16, 5])
def test_evaluator_gives_every_env_its_first_episode_of_every_round(torch_mod, wb_tables, ref_traj, B):
    torch = torch_mod
    ntraj = 8
    ev, out, snaps = _evaluate(torch, wb_tables, ref_traj, B, seed=5)
    rounds = -(-3 * ntraj // B)
    rec = out["records"]
    assert ev.rounds == rounds == len(out["rounds"]) and ev.ntraj == ntraj
    assert len(rec) == rounds * B == out["episodes"]
    offset = 0                                                       # policy calls before the round
    for r, (first, end) in enumerate(out["rounds"]):
        mine = rec[(rec["call"] >= first) & (rec["call"] < end)]
        assert sorted(mine["env"].tolist()) == list(range(B)), r     # every env exactly once per round
        assert (mine["call"] > first).all()
        # the tag is the clip the env was flying when the episode closed: the snapshot taken by the policy call before that step
        assert np.array_equal(mine["tag"], snaps[offset + (mine["call"] - first - 1), mine["env"]]), r
        assert np.array_equal(mine["tag"], (r * B + mine["env"]) % ntraj), r
        offset += end - first - 1
    assert offset == len(snaps)
    per_clip = out["per_clip"]
    assert per_clip["episodes"].shape == (ntraj,) and (per_clip["episodes"] >= 3).all() and per_clip["episodes"].sum() == rounds * B
    assert out["max_episode_length"] <= ev.max_steps - 2 and out["min_episode_length"] >= 1
    # the same seed on a fresh handle: the same bytes; another seed draws other wing phases
    _, again, _ = _evaluate(torch, wb_tables, ref_traj, B, seed=5)
    assert again["records"].tobytes() == rec.tobytes()
    print(f"\nevaluator B {B}: {rounds} rounds {out['rounds']}, {len(rec)} episodes, lengths {out['min_episode_length']:.0f} .. {out['max_episode_length']:.0f}, "
          f"terminated {out['terminated_fraction']:.2f}, per clip {per_clip['episodes'].tolist()}, {out['wall_seconds']:.2f} s")
