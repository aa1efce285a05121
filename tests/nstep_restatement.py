"""Plain numpy restatements of the device n-step writer (flybody_amd/csrc/nstep.hip) and of its taint rule, the scripted
`observe` streams the GPU tests feed it, and the counts that say which of the kernel's paths a script takes.  Nothing here needs
a device: tests/test_nstep_restatement_cpu.py pins this module, tests/test_gpu_nstep_shapes.py compares the kernel with it.

acme is not available, so these restate the semantics written down in nstep.hip's header; float32 and acme's left-to-right order
are kept so that equality with the kernel is bitwise."""
from collections import namedtuple

import numpy as np

FIRST, MID, LAST = 0, 1, 2


# ------------------------------------------------------------------------------------------------ one env, scalar
def writer_restatement(obs, act, rew, disc, st, n, gamma, with_call=False):
    """One env.  obs[t], rew[t], disc[t], st[t] = timestep t (t = 0 is FIRST); act[t] = action applied to reach timestep t.
    Returns the transitions (obs, action, return, discount, next_obs) in the order the adder writes them; with `with_call` every
    tuple carries a sixth item, the index t of the `observe` call that wrote it."""
    out, hist = [], []   # hist entries: (o_s, a_s, r_{s+1}, d_{s+1})
    last = None
    for t in range(len(st)):
        if st[t] == 0:
            hist, last = [], obs[t]
            continue
        hist.append((last, act[t], np.float32(rew[t]), np.float32(disc[t])))
        hist = hist[-n:]
        # acme's NStepTransitionAdder._write runs on every add() and does not wait for n entries: during an episode's first n - 1
        # steps it writes the short transitions (o_0 -> o_1), (o_0 -> o_2), ...; _write_last then flushes the tails
        starts = [0]
        if st[t] == 2:
            starts += list(range(1, len(hist)))
        for s in starts:
            ret, td = hist[s][2], hist[s][3]
            for i in range(s + 1, len(hist)):
                td = np.float32(td * np.float32(gamma))
                ret = np.float32(ret + np.float32(hist[i][2] * td))
                td = np.float32(td * hist[i][3])
            tr = (hist[s][0], hist[s][1], ret, td, obs[t])
            out.append(tr + (t,) if with_call else tr)
        last = obs[t]
    return out


def taint_restatement(step_type, bits, n_step, with_call=False):
    """One env.  step_type[t] / bits[t] = what call t passed (t = 0 is FIRST).  The entry appended at step t is marked when
    bits[t] | bits[t - 1] != 0 (a FIRST call appends nothing, but its bits count as the previous bits of the episode's first entry);
    a transition is tainted when any of the at most n_step entries it spans is marked.  Returns the taint of every transition in the
    order the adder writes them (`writer_restatement`: one from the oldest held entry per step, on LAST also the tails); with
    `with_call`, pairs (taint, index of the call that wrote it)."""
    out, marks, prev = [], [], 0
    for t in range(len(step_type)):
        b = int(bits[t])
        if step_type[t] == 0:
            marks, prev = [], b
            continue
        marks.append(int((b | prev) != 0))
        marks = marks[-n_step:]
        prev = b
        starts = [0] + (list(range(1, len(marks))) if step_type[t] == 2 else [])
        out += [(int(any(marks[s:])), t) if with_call else int(any(marks[s:])) for s in starts]
    return out


# ------------------------------------------------------------------------------------------------ a batch, vectorised over envs
# One row per transition, in (call, env, start) order.  `t_start` is the timestep whose observation the transition starts from
# (obs[t_start, env]); its action is act[t_start + 1, env]; it ends in obs[call, env] and spans m = call - t_start entries.
Transitions = namedtuple("Transitions", "call env t_start m ret disc taint per_call")


def batched_restatement(rew, disc, st, n, gamma, bits=None):
    """`writer_restatement` + `taint_restatement` for [T, B] streams at once.  Elementwise float32 numpy over the envs keeps each
    chain's operation order, so the returns and discounts are the scalar restatement's bit for bit (pinned by the CPU tests).
    Every env's first call must be FIRST.  `per_call[t]` = rows written by call t."""
    st = np.asarray(st)
    T, B = st.shape
    assert (st[0] == FIRST).all()
    rew, disc, g = np.asarray(rew, np.float32), np.asarray(disc, np.float32), np.float32(gamma)
    if bits is None:
        bits = np.zeros((T, B), np.int32)
    mark = np.zeros((T, B), np.int64)
    mark[1:] = ((bits[1:] | bits[:-1]) != 0) & (st[1:] != FIRST)       # entry t exists only on MID / LAST calls
    cmark = np.concatenate([np.zeros((1, B), np.int64), np.cumsum(mark, axis=0)])  # cmark[t + 1] - cmark[s] = marks of entries s .. t
    first = np.zeros(B, np.int64)                                       # index of the env's last FIRST call
    cols = {k: [] for k in ("call", "env", "t_start", "m", "ret", "disc", "taint")}
    per_call = np.zeros(T, np.int64)
    for t in range(T):
        isf = st[t] == FIRST
        first[isf] = t
        act_envs = np.nonzero(~isf)[0]
        if not len(act_envs):
            continue
        lo = np.maximum(first[act_envs] + 1, t - n + 1)                 # oldest held entry (entries are named by their call index)
        ln = t - lo + 1                                                 # entries held, 1 .. n
        is_last = st[t, act_envs] == LAST
        total = np.where(is_last, ln, 1)
        L = int(ln.max())
        # chains in lock step, as the kernel runs them: column j is the chain that starts at held entry j; step i feeds entry i
        K = int(total.max())
        ret = np.zeros((len(act_envs), K), np.float32)
        td = np.ones((len(act_envs), K), np.float32)
        j = np.arange(K)[None, :]
        for i in range(L):
            e = np.minimum(lo + i, t)
            r_, d_ = rew[e, act_envs][:, None], disc[e, act_envs][:, None]
            live = (i < ln)[:, None]
            init = live & (j == i)
            upd = live & (j < i)
            td1 = td * g
            ret1 = ret + r_ * td1
            td2 = td1 * d_
            ret = np.where(init, r_, np.where(upd, ret1, ret))
            td = np.where(init, d_, np.where(upd, td2, td))
        keep = j < total[:, None]                                       # row-major: env order, then start order
        rows, starts = np.nonzero(keep)
        envs = act_envs[rows]
        s_entry = lo[rows] + starts                                     # call index of the transition's first entry
        cols["call"].append(np.full(len(rows), t, np.int64))
        cols["env"].append(envs)
        cols["t_start"].append(s_entry - 1)
        cols["m"].append(t - s_entry + 1)
        cols["ret"].append(ret[rows, starts])
        cols["disc"].append(td[rows, starts])
        cols["taint"].append(((cmark[t + 1, envs] - cmark[s_entry, envs]) > 0).astype(np.uint8))
        per_call[t] = len(rows)
    dt = {"ret": np.float32, "disc": np.float32, "taint": np.uint8}
    out = {k: (np.concatenate(v) if v else np.zeros(0, dt.get(k, np.int64))) for k, v in cols.items()}
    return Transitions(per_call=per_call, **out)


# ------------------------------------------------------------------------------------------------ scripts
# A configuration names one writer shape and the script it is fed.  `episodes`: the menu the per-env episode lengths are drawn
# from (in steps: an episode of L steps is FIRST, L - 1 MID calls, LAST); "n-1" / "n" / "n+1" / "n+70" are resolved against n_step.
# `abandon`: probability that an episode is cut by a FIRST after a MID row instead of ending in LAST (what reset_envs produces).
# `sync_last`: after the ragged part every env starts an episode in the same call and ends it together n_step + 3 steps later -
# one call in which every env is LAST with a full ring, batch x n_step rows at once.  `capacity` None: no wrap (room for all).
Config = namedtuple("Config", "name batch obs_dim act_dim n_step discount calls episodes abandon sync_last capacity seed why")

CONFIGS = [
    Config("single_env", 1, 1, 1, 1, 0.99, 160, (1, 2, 3, 7), 0.15, True, None, 1,
           "batch 1, rows of one float, n_step 1: every ring index is 0, the grid is one workgroup with 15 idle waves"),
    Config("one_full_workgroup", 16, 63, 12, 2, 1.0, 140, (1, "n-1", "n", "n+1", 9), 0.15, True, None, 2,
           "exactly 16 envs: no idle wave; obs row one short of a pass; discount 1.0"),
    Config("second_workgroup_of_one", 17, 64, 59, 50, 0.99, 260, (1, "n-1", "n", "n+1", 5, 120), 0.1, True, None, 3,
           "17 envs: a second workgroup with one live wave claims after / before the first; obs row exactly one pass; the deployed n"),
    Config("ragged_grid_gamma_zero", 250, 65, 70, 63, 0.0, 200, (1, "n-1", "n", "n+1", 4, 30, 140), 0.1, True, None, 4,
           "16 workgroups, the last with 10 live waves; obs and action rows one over a pass; gamma 0 cuts every chain after its start"),
    Config("ballot_shift_boundary", 33, 104, 12, 64, 0.99, 240, (1, "n-1", "n", "n+1", 6, 150), 0.1, True, None, 5,
           "n_step 64: the last value fed from lanes, every lane of the ballot in use; flight's row widths"),
    Config("lane_chains_fed_from_ring", 40, 289, 59, 65, 1.0, 260, (1, 3, "n-1", "n", "n+1", 20, 40, 150), 0.1, True, None, 6,
           "n_step 65: rewards from the ring, the taint loop, LAST with total <= 64 and > 64; walk_on_ball's row widths (5 passes)"),
    Config("sequential_chains", 24, 11, 3, 100, 0.99, 420, (1, 10, 50, 63, 64, 65, "n-1", "n", "n+1", "n+70"), 0.1, True, None, 7,
           "n_step 100: the sequential branch at every total from 65 to 100, MID calls with a full ring of 100 read back in chains"),
    Config("long_window_long_episodes", 19, 104, 12, 130, 0.99, 700, (1, 30, 70, "n-1", "n", "n+1", "n+70", 330), 0.08, True, None, 8,
           "n_step 130 (three passes of the taint loop), episodes longer than n + 64 so the ring index wraps several times"),
    Config("wrap_small_ring", 17, 65, 3, 50, 0.99, 420, (1, 2, "n-1", "n", "n+1", 8, 90), 0.1, True, 17 * 50 + 3, 9,
           "ring of 853 slots (odd; no multiple of 16, 50 or 17), three slots above the largest call: wraps a dozen times"),
    Config("wrap_sequential_ring", 35, 11, 3, 100, 1.0, 520, (1, 20, 64, 65, "n-1", "n", "n+1", "n+70"), 0.1, True, 35 * 100 + 3, 10,
           "wrap with n_step > 64: the sequential branch and the taint loop write across the ring's end"),
    Config("deployed_batch_wrap", 8192, 104, 12, 5, 0.99, 34, (1, 2, 3, "n-1", "n", "n+1", 9, 14), 0.1, True, 8192 * 5 + 9043, 11,
           "8192 envs, 512 workgroups claiming at once into a ring of 50 003 slots that wraps five times; flight's rows"),
]


def get_config(name):
    return next(c for c in CONFIGS if c.name == name)


def _resolve(L, n):
    if isinstance(L, str):
        return max(1, n + int(L[1:] or 0)) if L.startswith("n") else int(L)
    return int(L)


Script = namedtuple("Script", "st rew disc bits sync_call")


def make_script(cfg):
    """step_type / reward / discount / step_bits [calls, B] of a configuration (deterministic; no observation or action rows)."""
    rng = np.random.RandomState(1000 + cfg.seed)
    T, B, n = cfg.calls, cfg.batch, cfg.n_step
    menu = [_resolve(L, n) for L in cfg.episodes]
    tail = 6                                                      # ragged calls after the synchronised LAST
    sync_first = T - tail - (n + 3) - 1 if cfg.sync_last else T   # the call in which every env is FIRST
    assert sync_first > 2 * max(2, min(menu)), (cfg.name, sync_first)
    st = np.ones((T, B), np.int32)
    st[0] = FIRST

    def ragged(b, t, end, k):
        """episodes from the menu starting with a FIRST at call t, until `end`; what does not fit stays open (MID rows)"""
        misses = 0
        while misses < 2 * len(menu):
            L = menu[(k + b) % len(menu)] if k < len(menu) else menu[rng.randint(len(menu))]   # every env goes through the menu first
            k += 1
            cut = rng.rand() < cfg.abandon and L > 1
            if cut:
                L = rng.randint(1, L)                             # L MID rows, then the next FIRST
            if t + L + 1 >= end:                                  # does not fit any more: try another length
                misses += 1
                continue
            if not cut:
                st[t + L, b] = LAST
            st[t + L + 1, b] = FIRST
            t += L + 1

    for b in range(B):
        ragged(b, 0, sync_first, 0)
    sync_call = None
    if cfg.sync_last:
        st[sync_first] = FIRST
        sync_call = sync_first + n + 3
        st[sync_first + 1:sync_call] = MID
        st[sync_call] = LAST
        st[sync_call + 1] = FIRST
        for b in range(B):
            ragged(b, sync_call + 1, T, len(menu))
    rew = rng.rand(T, B).astype(np.float32)
    disc = (rng.rand(T, B) > 0.1).astype(np.float32)              # zero env discounts: terminations, also in mid-episode
    bits = np.where(rng.rand(T, B) < 0.1, rng.randint(1, 4, (T, B)), 0).astype(np.int32)
    firsts = np.argwhere(st == FIRST)
    bits[firsts[::2, 0], firsts[::2, 1]] = 1                      # flags on FIRST rows for certain
    return Script(st, rew, disc, bits, sync_call)


def row_ids(cfg):
    """float32 [calls, B]: the counter every observation row carries in column 0 (1 .. calls * B, exact in float32), which makes
    the key (obs row, next_obs row) unique by construction"""
    ids = np.arange(1, cfg.calls * cfg.batch + 1, dtype=np.int64).reshape(cfg.calls, cfg.batch)
    assert ids.max() < 1 << 24
    return ids.astype(np.float32)


def make_rows(cfg):
    """obs [calls, B, O] (column 0 = `row_ids`) and act [calls, B, A], float32"""
    rng = np.random.RandomState(2000 + cfg.seed)
    obs = rng.standard_normal((cfg.calls, cfg.batch, cfg.obs_dim)).astype(np.float32)
    obs[:, :, 0] = row_ids(cfg)
    act = rng.standard_normal((cfg.calls, cfg.batch, cfg.act_dim)).astype(np.float32)
    return obs, act


# ------------------------------------------------------------------------------------------------ which paths a script takes
def path_counts(cfg, script=None, tr=None):
    """Counted from the script and the restatement alone (per env and call):
      last_lanes       LAST calls with n_step <= 64 (chains in lanes, fed from lanes, taint by ballot)
      last_ring_lanes  LAST calls with n_step > 64 and total <= 64 (chains in lanes, fed from the ring, taint loop)
      last_sequential  LAST calls with n_step > 64 and total > 64 (one chain after the other)
      mid_full_ring    MID calls with n_step > 64 that span a full ring (n_step entries read back from memory)
      one_step         episodes of one step (FIRST then LAST)
      abandoned        FIRST calls that follow a MID row
      longest_episode  steps of the longest episode
      all_last_full    calls in which every env is LAST and writes n_step rows"""
    script = script or make_script(cfg)
    tr = tr or batched_restatement(script.rew, script.disc, script.st, cfg.n_step, cfg.discount, script.bits)
    st, n = script.st, cfg.n_step
    T, B = st.shape
    # rows a (call, env) wrote and the span of its first row
    total = np.zeros((T, B), np.int64)
    np.add.at(total, (tr.call, tr.env), 1)
    span = np.zeros((T, B), np.int64)
    np.maximum.at(span, (tr.call, tr.env), tr.m)
    last, mid = st == LAST, st == MID
    prev = np.concatenate([np.full((1, B), -1), st[:-1]])
    ep_len = np.zeros((T, B), np.int64)                           # steps of the episode so far
    for t in range(1, T):
        ep_len[t] = np.where(st[t] == FIRST, 0, ep_len[t - 1] + 1)
    return {
        "last_lanes": int(last.sum()) if n <= 64 else 0,
        "last_ring_lanes": int((last & (total <= 64)).sum()) if n > 64 else 0,
        "last_sequential": int((last & (total > 64)).sum()) if n > 64 else 0,
        "mid_full_ring": int((mid & (span == n)).sum()) if n > 64 else 0,
        "one_step": int((last & (prev == FIRST)).sum()),
        "abandoned": int(((st == FIRST) & (prev == MID)).sum()),
        "longest_episode": int(ep_len.max()),
        "all_last_full": int(sum(1 for t in range(T) if last[t].all() and (total[t] == n).all())),
        "rows": int(tr.per_call.sum()),
    }


def wrap_facts(cfg, per_call):
    """For a ring of `cfg.capacity` slots and W rows claimed in call order: W, the first claimed index still in the ring, the call
    that straddles it (or None), how many of its rows survive, and the calls whose first and last slot lie in different laps."""
    C = cfg.capacity
    end = np.cumsum(per_call)
    begin = end - per_call
    W = int(end[-1])
    keep_from = max(0, W - C)
    straddler = [t for t in range(len(per_call)) if begin[t] < keep_from < end[t]]
    assert len(straddler) <= 1
    t = straddler[0] if straddler else None
    laps = [int(u) for u in range(len(per_call)) if per_call[u] and begin[u] // C != (end[u] - 1) // C]
    return {"W": W, "keep_from": keep_from, "straddler": t, "straddler_kept": int(end[t] - keep_from) if t is not None else 0,
            "whole_calls": [int(u) for u in range(len(per_call)) if per_call[u] and begin[u] >= keep_from], "across_the_end": laps,
            "begin": begin, "end": end}


# what the configuration list must exercise (the issue's conditions): checked on the CPU, asserted again by the GPU tests
REQUIRED = {"last_lanes": 20, "last_ring_lanes": 20, "last_sequential": 20, "mid_full_ring": 20, "one_step": 5, "abandoned": 5}


def check_conditions(configs=None):
    """Asserts that the configuration list covers the axes and takes every path often enough; returns {name: path_counts}."""
    configs = configs or CONFIGS
    counts, scripts = {}, {}
    for c in configs:
        s = make_script(c)
        tr = batched_restatement(s.rew, s.disc, s.st, c.n_step, c.discount, s.bits)
        counts[c.name] = dict(path_counts(c, s, tr), per_call=tr.per_call)
        scripts[c.name] = s
    for k, need in REQUIRED.items():
        got = sum(v[k] for v in counts.values())
        assert got >= need, (k, got, need)
    B = {c.batch for c in configs}
    assert {1, 16, 17, 8192} <= B and any(b > 32 and b % 16 for b in B), B
    assert {1, 63, 64, 65, 104, 289} <= {c.obs_dim for c in configs}
    A = {c.act_dim for c in configs}
    assert {1, 12, 59} <= A and max(A) > 64
    N = {c.n_step for c in configs}
    assert {1, 2, 50, 63, 64, 65, 100} <= N and max(N) >= 130
    assert {0.99, 1.0, 0.0} <= {c.discount for c in configs}
    for c in configs:
        v, n, st = counts[c.name], c.n_step, scripts[c.name].st
        # episodes of 1, n - 1, n, n + 1 steps finish in every configuration; one call has every env LAST on a full ring
        T, Bc = st.shape
        ep = np.zeros(Bc, np.int64)
        ended = set()
        for t in range(1, T):
            ep = np.where(st[t] == FIRST, 0, ep + 1)
            ended |= set(ep[st[t] == LAST].tolist())
        want = {1, max(1, n - 1), n, n + 1}
        assert want <= ended, (c.name, sorted(want - ended))
        assert v["all_last_full"] >= 1 and v["one_step"] >= 1 and v["abandoned"] >= 1, (c.name, v)
        if c.capacity is not None:
            assert c.capacity >= c.batch * n and c.capacity % 16 and c.capacity % n and c.capacity % c.batch, c.name
            f = wrap_facts(c, v["per_call"])
            assert f["W"] >= 3 * c.capacity and f["across_the_end"] and f["straddler"] is not None, (c.name, f["W"], c.capacity)
            assert int(v["per_call"].max()) <= c.capacity
    assert any(v["longest_episode"] > c.n_step + 64 for c, v in ((c, counts[c.name]) for c in configs) if c.n_step > 64)
    wraps = [c for c in configs if c.capacity is not None]
    assert len(wraps) >= 2 and any(c.n_step > 64 for c in wraps)
    return counts
