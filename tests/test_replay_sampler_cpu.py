"""The replay sampler's draw without a device: the restatement (tests/replay_sampler_restatement.py) the GPU tests compare the
kernel with is itself pinned here - range and edges, calls and seeds, uniformity (chi-square, deterministic), the eight-try
rejection - together with the argument validation of `ReplaySampler` that needs no device and the header's declarations."""
import os
import re

import numpy as np
import pytest

import replay_sampler_restatement as R
from conftest import ROOT


# ------------------------------------------------------------------------------------------------ the two forms agree
def test_numpy_form_equals_the_integer_definition():
    rng = np.random.RandomState(1)
    xs = [0, 1, R.M64, 0x9E3779B97F4A7C15] + [int(x) for x in rng.randint(0, 1 << 62, 50)]
    assert [int(v) for v in R.splitmix64(np.array(xs, dtype=np.uint64))] == [R.splitmix64_int(x) for x in xs]
    for b in (1, 2, 3, 0xFFFFFFFF, 1 << 32, (1 << 40) - 1, R.M64, 12345678901234567):
        a = np.array(xs, dtype=np.uint64)
        assert [int(v) for v in R.mulhi64(a, b)] == [(x * b) >> 64 for x in xs], b
    for seed, call, total in ((0, 0, 1), (7, 3, 1000), (R.M64, 1 << 40, (1 << 43) - 5), (5, 2, R.M64)):
        for t in (0, 7):
            got = R.draws(seed, call, 33, total, t)
            assert [int(v) for v in got] == [R.draw_int(seed, call, k, t, total) for k in range(33)]


# ------------------------------------------------------------------------------------------------ range and edges
@pytest.mark.parametrize("total", [1, 2, 3, 7, 64, 1000, (1 << 20) + 1, (1 << 40) - 1, 8 * ((1 << 40) - 1)])
def test_every_draw_is_below_total(total):
    for t in (0, 5):
        g = R.draws(11, 4, 4096, total, t)
        assert int(g.max()) < total
    if total == 1:
        assert not R.draws(11, 4, 4096, 1).any()                   # total = 1: every draw is row 0
    if total <= 64:
        # every row is reachable, the last one included (4096 draws miss a given one of 64 rows with probability e^-64)
        assert len(np.unique(R.draws(11, 4, 4096, total))) == total


def test_total_zero_is_not_ready_and_draws_nothing():
    out = R.sample(0, 0, 16, [0, 0], [8, 8])
    assert out == {"ready": False, "total": 0}
    out = R.sample(0, 0, 16, [3], [8], min_size=4)
    assert out == {"ready": False, "total": 3}
    assert R.sample(0, 0, 16, [4], [8], min_size=4)["ready"]
    assert R.sample(0, 0, 16, [100], [8], min_size=8)["total"] == 8  # a wrapped ring counts its capacity


def test_ring_lookup_at_the_prefix_boundaries():
    n, prefix, total = R.eligible([3, 0, 9, 100], [8, 8, 2, 5])
    assert n == [3, 0, 2, 5] and prefix == [0, 3, 3, 5, 10] and total == 10
    ring, slot = R.locate(np.arange(10), prefix)
    assert ring.tolist() == [0, 0, 0, 2, 2, 3, 3, 3, 3, 3]        # the empty ring 1 is never named
    assert slot.tolist() == [0, 1, 2, 0, 1, 0, 1, 2, 3, 4]
    # empty rings at either end, and a single ring
    assert R.locate(np.arange(4), R.eligible([0, 4, 0], [4, 4, 4])[1])[0].tolist() == [1, 1, 1, 1]
    assert R.locate(np.arange(4), R.eligible([4], [9])[1])[0].tolist() == [0, 0, 0, 0]
    out = R.sample(3, 1, 4096, [3, 0, 9, 100], [8, 8, 2, 5])
    assert set(out["ring"].tolist()) == {0, 2, 3}
    assert np.array_equal(out["index"], (out["ring"] << 40) | out["slot"])
    for r, cnt in enumerate(n):
        assert (out["slot"][out["ring"] == r] < max(cnt, 1)).all()


# ------------------------------------------------------------------------------------------------ calls and seeds
def test_calls_and_seeds():
    a = [R.draws(0, c, 256, 1 << 20) for c in (0, 1, 2)]
    assert not np.array_equal(a[0], a[1]) and not np.array_equal(a[1], a[2]) and not np.array_equal(a[0], a[2])
    assert not np.array_equal(R.draws(1, 0, 256, 1 << 20), a[0])
    assert np.array_equal(R.draws(0, 1, 256, 1 << 20), a[1])       # the same (seed, call) repeats
    assert len({R.call_key(s, c) for s in range(8) for c in range(8)}) == 64
    # tries of one row are distinct draws, rows do not share them: k << 3 leaves room for t = 0 .. 7
    u = np.stack([R.draws(9, 0, 64, R.M64, t) for t in range(8)])
    assert len(np.unique(u)) == u.size


# ------------------------------------------------------------------------------------------------ uniformity
@pytest.mark.parametrize("N,K", [(64, 65536), (7, 7000), (1000, 200000)])
def test_uniformity_chi_square(N, K):
    """seeds 0 .. 15, call 3: every seed's chi-square statistic against the uniform law on N rows stays below the 99.9 % quantile for
    N - 1 degrees of freedom.  The draw is deterministic, so this cannot flake (worst seed at 0.77 / 0.49 / 0.94 of the quantile)."""
    from scipy.stats import chi2

    q = chi2.ppf(0.999, N - 1)
    worst = 0.0
    for seed in range(16):
        cnt = np.bincount(R.draws(seed, 3, K, N).astype(np.int64), minlength=N)
        assert len(cnt) == N
        e = K / N
        stat = float(((cnt - e) ** 2).sum() / e)
        worst = max(worst, stat / q)
        assert stat < q, (seed, stat, q)
    print(f"N {N} K {K}: worst seed at {worst:.2f} of the 99.9 % quantile {q:.1f}")


# ------------------------------------------------------------------------------------------------ rejection
def test_rejection_clean_and_all_tainted():
    K = 500
    clean = R.sample(2, 5, K, [40, 24], [64, 24], taints=[np.zeros(64, np.uint8), np.zeros(24, np.uint8)])
    plain = R.sample(2, 5, K, [40, 24], [64, 24])
    assert not clean["tries"].any() and clean["kept_tainted"] == 0 and np.array_equal(clean["index"], plain["index"])
    bad = R.sample(2, 5, K, [40, 24], [64, 24], taints=[np.ones(64, np.uint8), np.ones(24, np.uint8)])
    assert (bad["tries"] == 7).all() and bad["kept_tainted"] == K
    ring, slot = R.locate(R.draws(2, 5, K, 64, 7), [0, 40, 64])
    assert np.array_equal(bad["ring"], ring) and np.array_equal(bad["slot"], slot)    # the eighth draw is the one kept


def test_rejection_mixed_pattern_by_hand():
    """three rows followed through their tries with the integer definition"""
    seed, call, total = 4, 1, 10
    g = [[R.draw_int(seed, call, k, t, total) for t in range(8)] for k in range(3)]
    # taint the first two distinct rows that output row 0 draws: it has to go on to a third try at least
    taint = np.zeros(total, np.uint8)
    taint[g[0][0]] = 1
    first_other = next(t for t in range(8) if g[0][t] != g[0][0])
    taint[g[0][first_other]] = 1
    want_try, want_row = [], []
    for k in range(3):
        t = next((t for t in range(8) if not taint[g[k][t]]), 7)
        want_try.append(t)
        want_row.append(g[k][t])
    assert want_try[0] >= 2                                         # row 0 really was redrawn at least twice
    out = R.sample(seed, call, 3, [total], [16], taints=[taint])
    assert out["tries"].tolist() == want_try and out["slot"].tolist() == want_row and out["kept_tainted"] == 0
    assert not taint[out["slot"]].any()
    # a row whose eight tries are all tainted keeps the eighth and is counted; the others are not
    taint2 = np.zeros(total, np.uint8)
    taint2[list(set(g[1]))] = 1
    out2 = R.sample(seed, call, 3, [total], [16], taints=[taint2])
    kept = [all(taint2[g[k][t]] for t in range(8)) for k in range(3)]
    assert kept[1] and out2["kept_tainted"] == sum(kept)
    assert out2["slot"][1] == g[1][7] and out2["tries"][1] == 7


# ------------------------------------------------------------------------------------------------ arguments, header
def _stub(obs_dim=5, act_dim=2, capacity=64, tracked=False, device="cuda:0", handle=1):
    from flybody_amd.actor_loop import NStepTransitionWriter

    w = object.__new__(NStepTransitionWriter)
    w.obs_dim, w.act_dim, w.capacity, w.track_validity, w.device, w._h = obs_dim, act_dim, capacity, tracked, device, handle
    return w


def _defuse(*stubs):
    for w in stubs:
        w._h = None      # (nothing to destroy: the stubs never had a handle)


def test_sampler_arguments_are_checked_before_any_device_work():
    from flybody_amd.actor_loop import ReplaySampler

    w = _stub()
    try:
        with pytest.raises(TypeError, match="writers must be"):
            ReplaySampler(None)
        with pytest.raises(TypeError, match="writers must be"):
            ReplaySampler("writer")
        with pytest.raises(ValueError, match="1 to 8 writers, got 0"):
            ReplaySampler([])
        nine = [_stub() for _ in range(9)]
        with pytest.raises(ValueError, match="1 to 8 writers, got 9"):
            ReplaySampler(nine)
        _defuse(*nine)
        with pytest.raises(TypeError, match=r"writers\[1\] is no NStepTransitionWriter"):
            ReplaySampler([w, object()])
        closed = _stub(handle=None)
        with pytest.raises(ValueError, match=r"writers\[1\] is closed"):
            ReplaySampler([w, closed])
        for bad in (0, -1, (1 << 20) + 1, 2.0, True, "256", None):
            with pytest.raises(ValueError, match="batch_size must be an integer"):
                ReplaySampler(w, bad)
        for bad in (0, -5, 1.5, False):
            with pytest.raises(ValueError, match="min_size must be an integer"):
                ReplaySampler(w, 4, min_size=bad)
        for bad in (-1, 1 << 64, 0.5):
            with pytest.raises(ValueError, match="seed must be an integer"):
                ReplaySampler(w, 4, seed=bad)
        with pytest.raises(TypeError, match="skip_tainted must be a bool"):
            ReplaySampler(w, 4, skip_tainted=1)
        other = _stub(obs_dim=6)
        with pytest.raises(ValueError, match=r"writers\[1\] has rows of \(obs_dim, act_dim\) = \(6, 2\)"):
            ReplaySampler([w, other])
        other2 = _stub(act_dim=3)
        with pytest.raises(ValueError, match=r"writers\[1\] has rows"):
            ReplaySampler((w, other2))
        far = _stub(device="cuda:1")
        with pytest.raises(ValueError, match="one sampler reads one device"):
            ReplaySampler([w, far])
        big = _stub(capacity=1 << 40)
        with pytest.raises(ValueError, match="capacity of 2\\^40 or more"):
            ReplaySampler([big])
        tr = _stub(tracked=True)
        with pytest.raises(ValueError, match="skip_tainted needs every writer"):
            ReplaySampler([tr, w], skip_tainted=True)
        _defuse(closed, other, other2, far, big, tr)
    finally:
        _defuse(w)


def test_header_declares_the_sampler():
    from flybody_amd import _capi

    hdr = open(os.path.join(ROOT, "include", "flybody_env.h")).read()
    declared = set(re.findall(r"\b(ffe_[a-z_]+)\s*\(", hdr))
    new = {"ffe_sampler_create", "ffe_sampler_sample", "ffe_sampler_info", "ffe_sampler_destroy", "ffe_sampler_last_error"}
    assert new <= declared and new <= set(_capi.SYMBOLS)
    assert "typedef struct ffe_sampler *ffe_sampler_handle;" in hdr and re.search(r"FFE_SAMPLE_SKIP_TAINTED\s*=\s*1\b", hdr)
    # the contract a caller has to know: lifetime, stream order, unpinned parity
    for phrase in ("must outlive", "stream-ordered", "parity unpinned"):
        assert phrase in hdr, phrase
