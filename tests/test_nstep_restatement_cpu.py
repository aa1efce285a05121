"""The numpy restatement of the n-step writer (tests/nstep_restatement.py) pinned by what flybody_amd/csrc/nstep.hip's header
states, the vectorised form pinned to the scalar one, and the scripts of tests/test_gpu_nstep_shapes.py checked for the paths they
must take.  No device."""
import ctypes as C

import numpy as np
import pytest

import nstep_restatement as R
from nstep_restatement import FIRST, LAST, MID, batched_restatement, taint_restatement, writer_restatement


def _episode(T, last=True):
    """FIRST, T - 1 MID, LAST (or T MID rows when the episode stays open)"""
    return [FIRST] + [MID] * (T - 1) + [LAST if last else MID]


def _run(st, n, gamma=0.99, rew=None, disc=None):
    T = len(st)
    obs = np.arange(T, dtype=np.float32)[:, None]
    act = np.arange(T, dtype=np.float32)[:, None] + 0.5
    rew = np.ones(T, np.float32) if rew is None else np.asarray(rew, np.float32)
    disc = np.ones(T, np.float32) if disc is None else np.asarray(disc, np.float32)
    return writer_restatement(obs, act, rew, disc, np.asarray(st), n, gamma, with_call=True)


@pytest.mark.parametrize("n", [1, 2, 5, 64, 65])
def test_rows_per_episode(n):
    """an episode of T < n steps leaves 2 T - 1 transitions, one of T >= n leaves T + n - 1 (nstep.hip's header)"""
    for T in (1, 2, 3, n - 1, n, n + 1, n + 7, 2 * n + 1):
        if T < 1:
            continue
        tr = _run(_episode(T), n)
        assert len(tr) == (2 * T - 1 if T < n else T + n - 1), (n, T)
        # every MID call writes one row, the LAST call the held entries; the call index is the one that wrote the row
        calls = [x[5] for x in tr]
        assert calls == list(range(1, T)) + [T] * min(T, n)
        # rows start at the oldest held entry and end in the call's observation
        for o, a, r, d, o2, t in tr[:T - 1]:
            assert o2[0] == t and o[0] == max(0, t - n) and a[0] == o[0] + 1.5


def test_abandoned_episode_leaves_only_the_rows_before_the_first():
    n = 5
    st = [FIRST, MID, MID, MID, FIRST, MID, LAST]
    tr = _run(st, n)
    assert [x[5] for x in tr] == [1, 2, 3, 5, 6, 6]
    # nothing spans the second FIRST: the rows after it start at its observation (4) or later
    assert [(int(x[0][0]), int(x[4][0])) for x in tr] == [(0, 1), (0, 2), (0, 3), (4, 5), (4, 6), (5, 6)]
    tt = taint_restatement(st, [0, 0, 1, 0, 0, 0, 0], n, with_call=True)
    assert tt == [(0, 1), (1, 2), (1, 3), (0, 5), (0, 6), (0, 6)]                 # the dropped entries take their marks with them


@pytest.mark.parametrize("gamma", [0.99, 0.5, 1.0])
def test_return_of_ones_is_the_float32_geometric_sum(gamma):
    n, T = 50, 60
    tr = _run(_episode(T), n, gamma)
    g = np.float32(gamma)
    for o, a, r, d, o2, t in tr:
        m = int(o2[0] - o[0])
        ret, td = np.float32(1), np.float32(1)
        for _ in range(1, m):
            td = np.float32(td * g)
            ret = np.float32(ret + td)
        assert r == ret and d == td, (m, r, ret)
    assert max(int(x[4][0] - x[0][0]) for x in tr) == n


def test_gamma_zero_and_zero_env_discount_cut_the_chain():
    n = 4
    rew = [0, 1, 2, 4, 8, 16]
    tr = _run(_episode(5), n, 0.0, rew=rew)
    for o, a, r, d, o2, t in tr:
        s = int(o[0]) + 1                                        # first entry
        assert r == rew[s] and d == (1.0 if o2[0] == s else 0.0)
    # env discount 0 at entry 3 (gamma 1): chains that pass it keep their reward up to and including entry 3 and end with discount 0
    disc = [1, 1, 1, 0, 1, 1]
    tr = _run(_episode(5), 8, 1.0, rew=rew, disc=disc)
    for o, a, r, d, o2, t in tr:
        s, e = int(o[0]) + 1, int(o2[0])
        want = sum(rew[i] for i in range(s, e + 1) if not (s <= 3 < i))
        assert r == want and d == (0.0 if s <= 3 <= e else 1.0), (s, e, r, want, d)


def test_existing_importers_see_the_same_functions():
    import test_nstep
    import test_validity_cpu

    assert test_validity_cpu.taint_restatement is taint_restatement
    rng = np.random.RandomState(0)
    T = 40
    st = np.array(_episode(9) + _episode(3) + [FIRST] + [MID] * 5 + _episode(20))[:T]
    obs, act = rng.randn(T, 3).astype(np.float32), rng.randn(T, 2).astype(np.float32)
    rew, disc = rng.rand(T).astype(np.float32), (rng.rand(T) > 0.2).astype(np.float32)
    a = test_nstep._reference(obs, act, rew, disc, st, 5, 0.9)
    b = writer_restatement(obs, act, rew, disc, st, 5, 0.9, with_call=True)
    assert len(a) == len(b) and all(len(x) == 5 and len(y) == 6 for x, y in zip(a, b))
    assert all(all(np.array_equal(p, q) for p, q in zip(x, y[:5])) for x, y in zip(a, b))


@pytest.mark.parametrize("name", [c.name for c in R.CONFIGS if c.batch <= 64])
def test_vectorised_restatement_is_the_scalar_one(name):
    """bitwise, row for row, call index and taint included, on the scripts the GPU test uses"""
    cfg = R.get_config(name)
    s = R.make_script(cfg)
    ids = R.row_ids(cfg)
    tr = batched_restatement(s.rew, s.disc, s.st, cfg.n_step, cfg.discount, s.bits)
    envs = range(cfg.batch) if cfg.batch <= 20 else range(0, cfg.batch, 7)
    for b in envs:
        ref = writer_restatement(ids[:, b, None], ids[:, b, None], s.rew[:, b], s.disc[:, b], s.st[:, b], cfg.n_step, cfg.discount, with_call=True)
        tnt = taint_restatement(s.st[:, b], s.bits[:, b], cfg.n_step, with_call=True)
        k = np.nonzero(tr.env == b)[0]
        assert len(k) == len(ref) == len(tnt) > 0
        assert [x[5] for x in ref] == tr.call[k].tolist() == [x[1] for x in tnt]
        assert np.array_equal(np.array([x[0][0] for x in ref]), ids[tr.t_start[k], b])
        assert np.array_equal(np.array([x[1][0] for x in ref]), ids[tr.t_start[k] + 1, b])      # the action is the start entry's
        assert np.array_equal(np.array([x[2] for x in ref], np.float32).view(np.uint32), tr.ret[k].view(np.uint32))
        assert np.array_equal(np.array([x[3] for x in ref], np.float32).view(np.uint32), tr.disc[k].view(np.uint32))
        assert [x[0] for x in tnt] == tr.taint[k].tolist()
        assert np.array_equal(tr.m[k], tr.call[k] - tr.t_start[k])
    assert np.array_equal(np.bincount(tr.call, minlength=cfg.calls), tr.per_call)


def test_scripts_take_every_path_and_cover_the_axes():
    counts = R.check_conditions()
    for c in R.CONFIGS:
        v = {k: x for k, x in counts[c.name].items() if k != "per_call"}
        extra = ""
        if c.capacity is not None:
            f = R.wrap_facts(c, counts[c.name]["per_call"])
            extra = f"  W / C = {f['W']} / {c.capacity} = {f['W'] / c.capacity:.2f}, calls across the ring's end {len(f['across_the_end'])}, straddling call keeps {f['straddler_kept']}"
        print(f"{c.name}: {v}{extra}")


def test_row_keys_are_unique_by_construction():
    for c in R.CONFIGS:
        ids = R.row_ids(c)
        assert len(np.unique(ids)) == ids.size and ids.min() >= 1
        assert np.array_equal(ids.astype(np.int64).astype(np.float32), ids)        # exact in float32
    for c in R.CONFIGS:
        if c.batch * c.calls * c.obs_dim > 4_000_000:
            continue
        obs, act = R.make_rows(c)
        assert np.array_equal(obs[:, :, 0], R.row_ids(c)) and obs.shape == (c.calls, c.batch, c.obs_dim) and act.shape[2] == c.act_dim
        # (obs row, next_obs row) of every transition: distinct pairs of counters
        s = R.make_script(c)
        tr = batched_restatement(s.rew, s.disc, s.st, c.n_step, c.discount, s.bits)
        pair = tr.t_start * c.batch * c.calls * 2 + tr.call * c.batch + tr.env
        assert len(np.unique(pair)) == len(pair)


def test_wrap_facts_on_a_hand_made_ring():
    cfg = R.Config("x", 2, 1, 1, 2, 0.99, 0, (), 0, False, 10, 0, "")
    f = R.wrap_facts(cfg, np.array([0, 4, 4, 4, 0, 4, 3]))      # W = 19: the claims 9 .. 18 survive
    assert f["W"] == 19 and f["keep_from"] == 9 and f["straddler"] == 3 and f["straddler_kept"] == 3
    assert f["whole_calls"] == [5, 6] and f["across_the_end"] == [3]            # call 3 claimed 8 .. 11


def test_capacity_below_one_calls_output_is_refused_on_both_layers():
    """One call can write batch x n_step rows (every env LAST on a full ring); in a smaller ring two transitions of that launch
    would share a slot and their arrays are stored by different waves.  Both layers refuse before they touch a device."""
    from flybody_amd import _capi
    from flybody_amd.actor_loop import NStepTransitionWriter

    with pytest.raises(ValueError, match=r"capacity.*batch_size \* n_step"):
        NStepTransitionWriter(7, 11, 3, n_step=50, capacity=349)
    with pytest.raises(ValueError, match=r"capacity.*batch_size \* n_step"):
        NStepTransitionWriter(7, 11, 3, n_step=50, capacity=349, track_validity=True)
    L = _capi.lib()
    for create in (L.ffe_nstep_create, L.ffe_nstep_create_tracked):
        h = C.c_void_p(123)
        assert create(7, 11, 3, 50, 0.99, 349, 0, C.byref(h)) != 0 and not h.value
        msg = L.ffe_nstep_last_error(None).decode()
        assert "capacity" in msg and "batch x n_step" in msg and "350" in msg, msg
