"""The per-episode log without a device: the numpy restatement (tests/episode_log_restatement.py) on hand-worked scripts, the host
aggregate `flybody_amd.actor_loop.summarize` against direct numpy, and the argument refusals of `EpisodeLog` that need no GPU."""
import numpy as np
import pytest

import episode_log_restatement as R
from episode_log_restatement import FIRST, LAST, MID


def _rec(rows):
    return np.array(rows, dtype=R.DTYPE)


def _run(log, script, rewards=None, discounts=None, info=None, tags=None):
    """script: [calls][B] step types"""
    out = []
    for t, st in enumerate(script):
        B = len(st)
        out.append(log.observe(st, np.ones(B, np.float32) if rewards is None else rewards[t], np.ones(B, np.float32) if discounts is None else discounts[t],
                               None if info is None else info[t], None if tags is None else tags[t]))
    return out


# ------------------------------------------------------------------------------------------------ the restatement, by hand
def test_first_then_last_is_a_one_step_episode():
    log = R.EpisodeLogRestatement(1, 4)
    _run(log, [[FIRST], [LAST]], rewards=[[5.0], [0.25]], discounts=[[1.0], [0.0]], info=[[[9, 9, 9, 9]], [[1, 3, 0x302, 1]]], tags=[[7], [4]])
    # the FIRST row's reward, info and tag are not read; bits = (0x302 & 255) | 256 for the zero discount
    assert log.all_records().tolist() == [(0, 4, 1, 0.25, 1, 3, 0x102)]
    assert (log.count, log.calls) == (1, 2)


def test_abandoned_episode_leaves_no_record():
    log = R.EpisodeLogRestatement(2, 2)
    script = [[FIRST, FIRST], [MID, MID], [FIRST, MID], [MID, LAST], [LAST, FIRST]]
    rew = [[0, 0], [1, 10], [100, 20], [2, 30], [4, 1000]]
    _run(log, script, rewards=np.array(rew, np.float32))
    # env 0: the episode of call 1 is abandoned at call 2 (its reward 1 and the FIRST row's 100 are gone), then 2 + 4 over 2 steps;
    # env 1: 10 + 20 + 30 over 3 steps, closed at call 3; discount 1 everywhere: cut by the time limit, bit 8 clear
    assert log.all_records().tolist() == [(1, 0, 3, 60.0, 3, 0, 0), (0, 0, 2, 6.0, 4, 0, 0)]


def test_float32_running_sum_in_step_order():
    log = R.EpisodeLogRestatement(1, 1)
    rew = np.array([[0], [1e8], [1], [-1e8]], np.float32)
    _run(log, [[FIRST], [MID], [MID], [LAST]], rewards=rew)
    assert log.all_records()["ret"].tolist() == [0.0]            # (1e8 + 1) - 1e8 in float32; float64 would give 1


def test_every_env_last_in_one_call():
    B = 5
    log = R.EpisodeLogRestatement(B, B)
    rew = np.arange(3 * B, dtype=np.float32).reshape(3, B)
    _run(log, [[FIRST] * B, [MID] * B, [LAST] * B], rewards=rew, tags=np.arange(3 * B).reshape(3, B))
    rec = log.all_records()
    assert rec["env"].tolist() == list(range(B)) and (rec["call"] == 2).all() and (rec["length"] == 2).all()
    assert rec["ret"].tolist() == [float(B + i + 2 * B + i) for i in range(B)] and rec["tag"].tolist() == [2 * B + i for i in range(B)]
    full, partial, n_partial = log.ring()
    assert full.tobytes() == rec.tobytes() and n_partial == 0 and len(partial) == 0


def test_ring_of_capacity_batch_wrapping_three_times():
    """B = 3 = capacity; every env finishes a one-step episode on every odd call, env 0 alone on calls 8 and 10: 3 + 3 + 3 + 1 + 1 = 11
    records.  The ring keeps the last three: calls 10 and 8 whole (one record each) and ONE of the three records of call 5."""
    B = 3
    log = R.EpisodeLogRestatement(B, B)
    script = [[FIRST] * B, [LAST] * B, [FIRST] * B, [LAST] * B, [FIRST] * B, [LAST] * B, [FIRST] * B, [FIRST, MID, MID], [LAST, MID, MID], [FIRST, MID, MID],
              [LAST, MID, MID]]
    rew = np.arange(len(script) * B, dtype=np.float32).reshape(len(script), B)
    _run(log, script, rewards=rew)
    assert log.count == 11 and log.count // B == 3
    full, partial, n_partial = log.ring()
    assert full.tolist() == [(0, 0, 1, 24.0, 8, 0, 0), (0, 0, 1, 30.0, 10, 0, 0)]
    assert n_partial == 1 and partial.tolist() == [(i, 0, 1, 15.0 + i, 5, 0, 0) for i in range(B)]
    for survivor in range(B):                                      # whichever record of call 5 the kernel kept is accepted ...
        log.check_ring(np.concatenate([partial[survivor:survivor + 1], full]))
    with pytest.raises(AssertionError):                            # ... a record of call 3 is not
        log.check_ring(np.concatenate([_rec([(0, 0, 1, 9.0, 3, 0, 0)]), full]))
    with pytest.raises(AssertionError):
        log.check_ring(full)
    wrong = full.copy(); wrong["length"][0] = 2
    with pytest.raises(AssertionError):
        log.check_ring(np.concatenate([partial[:1], wrong]))


def test_one_shot_mask_and_rearming():
    B = 4
    log = R.EpisodeLogRestatement(B, 8, one_shot=True)
    one = lambda st: log.observe(st, np.ones(B, np.float32), np.zeros(B, np.float32))
    assert len(one([FIRST] * B)) == 0 and len(one([LAST] * B)) == 0 and log.count == 0       # nothing armed: nothing emitted
    log.arm([1, 0, 1, 0])
    assert log.armed_left == 2
    one([FIRST] * B)
    assert one([LAST, LAST, MID, MID])["env"].tolist() == [0] and log.armed_left == 1        # env 1 is not armed
    one([FIRST, FIRST, MID, MID])
    assert len(one([LAST, LAST, MID, MID])) == 0 and log.armed_left == 1                     # env 0 disarmed on its LAST
    rec = one([FIRST, FIRST, LAST, LAST])
    assert rec.tolist() == [(2, 0, 4, 4.0, 6, 0, 256)] and log.armed_left == 0
    log.arm()                                                                                 # re-arming, all envs, mid-episode for none
    assert log.armed_left == B
    one([FIRST] * B)
    assert one([LAST] * B)["env"].tolist() == [0, 1, 2, 3] and log.armed_left == 0 and log.count == 6


# ------------------------------------------------------------------------------------------------ summarize
def _random_records(rng, n, tags=4, call0=0):
    rec = np.zeros(n, R.DTYPE)
    rec["env"] = rng.permutation(n)                                 # (call, env) unique: the canonical order has no ties
    rec["tag"] = rng.randint(0, tags, n)
    rec["length"] = rng.randint(1, 3001, n)
    rec["ret"] = rng.uniform(-5, 900, n).astype(np.float32)
    rec["call"] = call0 + np.sort(rng.randint(0, 40, n))
    rec["flagged_steps"] = np.where(rng.rand(n) < 0.3, rng.randint(1, 20, n), 0)
    rec["bits"] = np.where(rng.rand(n) < 0.6, 256, 0) | rng.randint(0, 4, n)
    return rec


def _direct(rec):
    ret, ln = rec["ret"].astype(np.float64), rec["length"].astype(np.float64)
    return {"avg_episode_return": np.mean(ret), "var_episode_return": np.var(ret), "max_episode_return": np.max(ret), "min_episode_return": np.min(ret),
            "avg_episode_length": np.mean(ln), "var_episode_length": np.var(ln), "max_episode_length": np.max(ln), "min_episode_length": np.min(ln),
            "episodes": len(rec), "terminated_fraction": np.mean((rec["bits"] & 256) != 0), "flagged_episodes": int((rec["flagged_steps"] > 0).sum()),
            "flagged_steps": int(rec["flagged_steps"].sum())}


def _same(got, want, where=""):
    """counts, max and min exactly; means and variances to 1e-12 relative: summarize adds in canonical order, the direct call in the
    order given, and a float64 sum of n <= 300 terms moves by at most n * 2^-53 relative to sum|x| under reordering"""
    assert set(got) == set(want), where
    for k in want:
        if k.startswith(("avg_", "var_")) or k == "terminated_fraction":
            assert abs(got[k] - want[k]) <= 1e-12 * max(1.0, abs(want[k])) * 300, (k, where, got[k], want[k])
        else:
            assert got[k] == want[k], (k, where)


def test_record_dtype_is_the_restatements():
    from flybody_amd.actor_loop import record_dtype

    assert record_dtype() == R.DTYPE and record_dtype().itemsize == 32


def test_summarize_against_direct_numpy():
    from flybody_amd.actor_loop import canonical_order, summarize

    rng = np.random.RandomState(0)
    rec = _random_records(rng, 300)
    shuffled = rec[rng.permutation(len(rec))]
    got = summarize(shuffled)
    want = _direct(rec)
    _same(got, want)                                                # the reference's _eval_agg_stat keys plus the four additions
    assert canonical_order(shuffled).tobytes() == R.canonical(rec).tobytes()
    # the last 37 of the canonical order, whatever order they arrive in; a window beyond the count takes everything
    want = _direct(R.canonical(rec)[-37:])
    got = summarize(shuffled, last=37)
    _same(got, want, "last 37")
    assert summarize(shuffled, last=10 ** 6) == summarize(shuffled) and summarize(shuffled, last=len(rec)) == summarize(shuffled)
    empty = summarize(rec[:0])
    assert empty["episodes"] == 0 and empty["flagged_steps"] == 0 and np.isnan(empty["avg_episode_return"]) and np.isnan(empty["terminated_fraction"])
    assert summarize(shuffled, last=0)["episodes"] == 0


def test_summarize_by_tag_with_an_empty_tag():
    from flybody_amd.actor_loop import summarize

    rng = np.random.RandomState(1)
    rec = _random_records(rng, 200, tags=6)
    rec = rec[rec["tag"] != 2]                                      # clip 2 never finished an episode
    got = summarize(rec, by_tag=True, num_tags=8)                   # ... and clips 6 and 7 do not occur
    for k, v in got.items():
        assert isinstance(v, np.ndarray) and v.shape == (8,), k
    for tag in range(8):
        sub = rec[rec["tag"] == tag]
        if len(sub) == 0:
            assert tag in (2, 6, 7) and got["episodes"][tag] == 0 and got["flagged_episodes"][tag] == 0 and got["flagged_steps"][tag] == 0
            assert all(np.isnan(got[k][tag]) for k in got if k not in ("episodes", "flagged_episodes", "flagged_steps"))
        else:
            _same({k: v[tag] for k, v in got.items()}, _direct(sub), f"tag {tag}")
    assert got["episodes"].sum() == len(rec)
    assert summarize(rec, by_tag=True)["episodes"].shape == (6,)    # default: the largest tag present + 1
    with pytest.raises(ValueError, match="num_tags"):
        summarize(rec, by_tag=True, num_tags=3)


def test_summarize_takes_concatenated_logs():
    from flybody_amd.actor_loop import summarize

    rng = np.random.RandomState(2)
    a, b = _random_records(rng, 120), _random_records(rng, 80)
    both = np.concatenate([a, b])
    _same(summarize(both), _direct(both))
    sa, sb = summarize(a, by_tag=True, num_tags=4), summarize(b, by_tag=True, num_tags=4)
    sab = summarize(both, by_tag=True, num_tags=4)
    for k in ("episodes", "flagged_episodes", "flagged_steps"):
        assert np.array_equal(sab[k], sa[k] + sb[k])                # groups can be summed
    with pytest.raises(TypeError, match="structured array"):
        summarize(np.zeros(3))


# ------------------------------------------------------------------------------------------------ refusals without a device
def test_episode_log_refuses_bad_arguments_before_touching_a_device():
    from flybody_amd.actor_loop import BatchedEvaluator, EpisodeLog

    with pytest.raises(ValueError, match="capacity 7 is below batch_size = 8"):
        EpisodeLog(8, capacity=7)
    for kw in ({"batch_size": 0}, {"batch_size": -3}, {"batch_size": 2.5}, {"batch_size": True}, {"batch_size": 4, "capacity": 0},
               {"batch_size": 4, "capacity": 8.0}, {"batch_size": 4, "device": -1}, {"batch_size": 1 << 31, "capacity": 1 << 32}):
        with pytest.raises(ValueError):
            EpisodeLog(**kw)
    with pytest.raises(TypeError, match="one_shot"):
        EpisodeLog(4, one_shot=1)
    with pytest.raises(ValueError, match="episodes_per_clip"):
        BatchedEvaluator(None, None, episodes_per_clip=0)
    with pytest.raises(ValueError, match="poll_every"):
        BatchedEvaluator(None, None, poll_every=0)
    with pytest.raises(ValueError, match="seed"):
        BatchedEvaluator(None, None, seed=-1)


def test_loops_take_a_log_without_changing_their_constructor():
    import inspect

    from flybody_amd.actor_loop import BatchedActorLoop, GroupedActorLoop

    assert list(inspect.signature(BatchedActorLoop.log_episodes).parameters) == ["self", "episode_log"]
    assert inspect.signature(GroupedActorLoop.__init__).parameters["episode_logs"].default is None


def test_kernels_need_no_scratch():
    """compiled with the library's own flags for gfx950: no scratch, no spills, full occupancy - for both instantiations of the
    observe kernel and the arm kernel"""
    from flybody_amd import build

    usage = build.kernel_resource_usage("episode_log.hip", "episode_log")
    assert len(usage) == 3 and sum("episode_log_kernel" in k for k in usage) == 2, list(usage)
    for name, u in usage.items():
        assert u["ScratchSize"] == 0 and u["VGPRs Spill"] == 0 and u["SGPRs Spill"] == 0 and u["Occupancy"] == 8, (name, u)
