"""The device n-step writer (`nstep_observe_kernel`, flybody_amd/csrc/nstep.hip) at the shapes it is deployed at, bit for bit
against the numpy restatement (tests/nstep_restatement.py, itself pinned without a device by tests/test_nstep_restatement_cpu.py):
several workgroups claiming slots at once, a replay ring that wraps, n_step on both sides of 64, rows wider than one pass of the
lanes, episodes of 1 / n - 1 / n / n + 1 / more than n + 64 steps, abandoned episodes, every env on LAST in one call.  A plain and a
tracked writer are fed the same calls; both are compared with the restatement and with each other.  Nothing here has a tolerance.
Run with `-m gpu -s` on an MI355X: every case prints its configuration, the rows compared, the rows per path and W / C."""
import ctypes as C

import numpy as np
import pytest

import nstep_restatement as R
from test_gpu_parity import torch_mod  # noqa: F401

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def path_counts():
    """the conditions on the scripts, asserted again here: a script that stops taking a path fails instead of passing empty"""
    return R.check_conditions()


def _bits32(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def _lookup(cfg, tr, o, o2):
    """ring rows -> index of the restatement's transition with the same (obs row, next_obs row) key.  Column 0 of every observation
    row is a counter (R.row_ids), so the key is the pair of counters; the whole rows are compared by the caller."""
    T, B = cfg.calls, cfg.batch
    io, inx = o[:, 0].astype(np.int64), o2[:, 0].astype(np.int64)
    assert np.array_equal(io.astype(np.float32), o[:, 0]) and np.array_equal(inx.astype(np.float32), o2[:, 0]), "a counter that is no integer"
    assert io.min() >= 1 and inx.min() >= 1 and io.max() <= T * B and inx.max() <= T * B, "a counter outside the script (an unwritten or torn slot)"
    ts, es = np.divmod(io - 1, B)
    te, ee = np.divmod(inx - 1, B)
    assert np.array_equal(es, ee), "obs and next_obs rows of different envs in one slot"
    key = (ts * T + te) * B + es
    ref_key = (tr.t_start * T + tr.call) * B + tr.env
    order = np.argsort(ref_key)
    assert len(np.unique(ref_key)) == len(ref_key)
    pos = np.searchsorted(ref_key[order], key)
    pos = np.minimum(pos, len(order) - 1)
    idx = order[pos]
    assert np.array_equal(ref_key[idx], key), f"{int((ref_key[idx] != key).sum())} ring rows are no transition of the restatement"
    assert len(np.unique(key)) == len(key), "a transition sits in two slots"
    return idx


def _check_ring(cfg, tr, obs, act, got, W, tag):
    """(a) every slot holds one whole transition of the restatement, none twice; (b) - (d) which calls' rows are present"""
    o, a, r, d, o2 = got[:5]
    C_ = cfg.capacity if cfg.capacity is not None else W
    N = min(W, C_)
    assert len(r) == N == len(o) == len(a) == len(d) == len(o2), (tag, len(r), N)
    idx = _lookup(cfg, tr, o, o2)
    env, ts, te = tr.env[idx], tr.t_start[idx], tr.call[idx]
    assert np.array_equal(_bits32(o), _bits32(obs[ts, env])), tag
    assert np.array_equal(_bits32(o2), _bits32(obs[te, env])), tag
    assert np.array_equal(_bits32(a), _bits32(act[ts + 1, env])), tag
    bad_r, bad_d = _bits32(r) != _bits32(tr.ret[idx]), _bits32(d) != _bits32(tr.disc[idx])
    assert not bad_r.any(), (tag, int(bad_r.sum()), r[bad_r][:4], tr.ret[idx][bad_r][:4], tr.m[idx][bad_r][:4])
    assert not bad_d.any(), (tag, int(bad_d.sum()), d[bad_d][:4], tr.disc[idx][bad_d][:4], tr.m[idx][bad_d][:4])
    if len(got) == 6:
        assert got[5].dtype == np.uint8
        bad_t = got[5] != tr.taint[idx]
        assert not bad_t.any(), (tag, int(bad_t.sum()), tr.m[idx][bad_t][:8], tr.call[idx][bad_t][:8])
    present = np.bincount(te, minlength=cfg.calls)
    if cfg.capacity is None:
        assert np.array_equal(present, tr.per_call), tag
        return idx, None
    f = R.wrap_facts(cfg, tr.per_call)
    whole = np.zeros(cfg.calls, bool)
    whole[f["whole_calls"]] = True
    assert np.array_equal(present[whole], tr.per_call[whole]), (tag, "a row of a call inside the last C claims is missing")
    assert present[f["straddler"]] == f["straddler_kept"], (tag, present[f["straddler"]], f["straddler_kept"])
    older = ~whole
    older[f["straddler"]] = False
    assert present[older].sum() == 0, (tag, "a row of an older call survived", np.nonzero(present * older)[0][:8])
    return idx, f


@pytest.mark.parametrize("name", [c.name for c in R.CONFIGS])
def test_writer_at_deployed_shapes(torch_mod, path_counts, name):
    from flybody_amd.actor_loop import NStepTransitionWriter
    from flybody_amd.dm_types import TimeStep

    torch = torch_mod
    cfg = R.get_config(name)
    pc = path_counts[name]
    n, B, T = cfg.n_step, cfg.batch, cfg.calls
    # the paths this configuration is there for are really taken (counted from the script and the restatement alone)
    if n <= 64:
        assert pc["last_lanes"] > 0
    else:
        assert pc["last_ring_lanes"] > 0 and pc["last_sequential"] > 0 and pc["mid_full_ring"] > 0
    assert pc["one_step"] > 0 and pc["abandoned"] > 0 and pc["all_last_full"] >= 1
    s = R.make_script(cfg)
    obs, act = R.make_rows(cfg)
    tr = R.batched_restatement(s.rew, s.disc, s.st, n, cfg.discount, s.bits)
    W = int(tr.per_call.sum())
    assert W == pc["rows"] and int(tr.per_call[s.sync_call]) == B * n          # the call in which every env flushes a full ring
    cap = cfg.capacity if cfg.capacity is not None else max(W, B * n) + 5
    if cfg.capacity is not None:
        f = R.wrap_facts(cfg, tr.per_call)
        assert W >= 3 * cap and f["across_the_end"] and cap % 16 and cap % n and cap % B
    tracked = NStepTransitionWriter(B, cfg.obs_dim, cfg.act_dim, n_step=n, discount=cfg.discount, capacity=cap, track_validity=True)
    plain = NStepTransitionWriter(B, cfg.obs_dim, cfg.act_dim, n_step=n, discount=cfg.discount, capacity=cap)
    dev = lambda x: torch.tensor(x, device="cuda")
    obs_d, act_d, st_d, rew_d, disc_d, bits_d = dev(obs), dev(act), dev(s.st), dev(s.rew), dev(s.disc), dev(s.bits)
    buf = torch.full((B, 4), -1, dtype=torch.int32, device="cuda")   # the other three columns must not be read
    for t in range(T):
        ts = TimeStep(st_d[t], rew_d[t], disc_d[t], None)
        buf[:, 0] = bits_d[t]
        tracked.observe(act_d[t], ts, obs_d[t], step_bits=(buf, buf[:, 0], bits_d[t])[t % 3])
        plain.observe(act_d[t], ts, obs_d[t])
    assert tracked.num_written() == plain.num_written() == W
    got6 = [x.cpu().numpy() for x in tracked.transitions(with_taint=True)]
    got5 = [x.cpu().numpy() for x in plain.transitions()]
    idx6, f = _check_ring(cfg, tr, obs, act, got6, W, name + " (tracked)")
    idx5, _ = _check_ring(cfg, tr, obs, act, got5, W, name + " (plain)")
    # the two writers with each other, on the transitions both hold (all of them unless the ring wrapped: which rows of the straddling
    # call survive depends on the order of its workgroups)
    common, i6, i5 = np.intersect1d(idx6, idx5, return_indices=True)
    assert len(common) >= min(W, cap) - (f["straddler_kept"] if f else 0)
    for k in range(5):
        assert np.array_equal(_bits32(got6[k][i6]), _bits32(got5[k][i5])), k
    tainted = int(got6[5].sum())
    assert 0 < tainted < len(got6[5])
    m = tr.m[idx6]
    print(f"\n{name}: B {B} O {cfg.obs_dim} A {cfg.act_dim} n_step {n} gamma {cfg.discount} calls {T} capacity {cap} - {cfg.why}\n"
          f"  rows written W {W}, rows compared bit for bit {len(idx6)} (tracked) + {len(idx5)} (plain), {tainted} tainted, spans 1 .. {int(m.max())}"
          f" ({int((m == n).sum())} of n_step entries), all-LAST call wrote {int(tr.per_call[s.sync_call])} rows\n"
          f"  per path: { {k: v for k, v in pc.items() if k not in ('per_call', 'rows')} }"
          + (f"\n  W / C = {W} / {cap} = {W / cap:.2f}; calls whose claim runs across the ring's end {len(f['across_the_end'])}; whole calls in the ring "
             f"{len(f['whole_calls'])}, straddling call {f['straddler']} keeps {f['straddler_kept']} of {int(tr.per_call[f['straddler']])} rows" if f else ""))
    tracked.close(); plain.close()


def test_ring_smaller_than_one_call_is_refused(torch_mod):
    """capacity < batch x n_step: refused by the constructors of both layers with a text that says so; exactly batch x n_step is
    accepted and takes the call that fills it."""
    from flybody_amd import _capi
    from flybody_amd.actor_loop import NStepTransitionWriter
    from flybody_amd.dm_types import TimeStep

    torch = torch_mod
    L = _capi.lib()
    for create in (L.ffe_nstep_create, L.ffe_nstep_create_tracked):
        h = C.c_void_p()
        assert create(250, 104, 12, 50, 0.99, 250 * 50 - 1, 0, C.byref(h)) != 0 and not h.value
        msg = L.ffe_nstep_last_error(None).decode()
        assert "capacity 12499" in msg and "batch x n_step = 12500" in msg, msg
        assert create(250, 104, 12, 50, 0.99, 250 * 50, 0, C.byref(h)) == 0 and h.value
        assert L.ffe_nstep_destroy(h) == 0
    for track in (False, True):
        with pytest.raises(ValueError, match=r"capacity 63 is below batch_size \* n_step = 64"):
            NStepTransitionWriter(16, 3, 2, n_step=4, capacity=63, track_validity=track)
    # the smallest ring allowed, filled by one call: 16 envs x 4 entries, every env LAST
    B, n = 16, 4
    w = NStepTransitionWriter(B, 3, 2, n_step=n, discount=0.5, capacity=B * n)
    ids = np.arange(1, 6 * B + 1, dtype=np.float32).reshape(6, B)
    obs = np.stack([ids, ids, ids], axis=2)
    act = np.stack([ids, -ids], axis=2)
    st = np.array([0, 1, 1, 1, 2, 0], np.int32)[:, None].repeat(B, 1)
    one = np.ones(B, np.float32)
    for t in range(5):
        w.observe(torch.tensor(act[t], device="cuda"), TimeStep(torch.tensor(st[t], device="cuda"), torch.tensor(one, device="cuda"),
                                                              torch.tensor(one, device="cuda"), None), torch.tensor(obs[t], device="cuda"))
    assert w.num_written() == 3 * B + B * n                       # 112 rows into 64 slots: the LAST call's 64 are what is left
    o, a, r, d, o2 = [x.cpu().numpy() for x in w.transitions()]
    assert len(r) == B * n and (o2[:, 0] > 4 * B).all()
    start = ((o[:, 0] - 1) // B).astype(int)
    assert sorted(zip(((o[:, 0] - 1) % B).astype(int).tolist(), start.tolist())) == [(b, s) for b in range(B) for s in range(4)]
    want = {0: 1.875, 1: 1.75, 2: 1.5, 3: 1.0}
    assert all(r[i] == want[start[i]] and d[i] == 0.5 ** (3 - start[i]) for i in range(len(r)))
    w.close()
