"""The device replay sampler (`ffe_sampler_*`, flybody_amd/csrc/replay.hip; `flybody_amd.actor_loop.ReplaySampler`) against the
restatement of its draw (tests/replay_sampler_restatement.py, pinned without a device by tests/test_replay_sampler_cpu.py).

Rings are filled through `NStepTransitionWriter.observe` with a scripted feed (n_step 3, capacity = B x n_step, so a few calls wrap
the ring); column 0 of every observation row is a counter >= 1 and unwritten slots are zero, so a read of one shows.  Expected rows
are the ring's own (`transitions(with_taint=True)` read just before sampling), expected indices the restatement's on the `written`
counts read back.  Every comparison is bit for bit; nothing here has a tolerance."""
import ctypes as C

import numpy as np
import pytest

import replay_sampler_restatement as R
from test_gpu_parity import torch_mod  # noqa: F401

pytestmark = pytest.mark.gpu

N_STEP = 3


def _bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.uint32) if x.dtype == np.float32 else x


class Feed:
    """One writer and its script: call 0 is FIRST for every env (no row); every later call steps envs 0 .. m - 1 (MID, one row each)
    and restarts the others (FIRST, no row), so the rows written are exactly the sum of the m."""

    def __init__(self, torch, B, O, A, tracked, ring_id=0, capacity=None):
        from flybody_amd.actor_loop import NStepTransitionWriter

        self.torch, self.B, self.O, self.A, self.tracked = torch, B, O, A, tracked
        self.capacity = capacity if capacity is not None else B * N_STEP
        self.w = NStepTransitionWriter(B, O, A, n_step=N_STEP, discount=0.9, capacity=self.capacity, track_validity=tracked)
        self.rng = np.random.RandomState(100 + ring_id)
        self.base, self.t, self.rows = ring_id * 100000, 0, 0
        self.call(0)

    def stage(self, m, bits=None):
        """the device tensors of the next call (host-to-device copies: they block the host), to be handed to `enqueue`"""
        from flybody_amd.dm_types import TimeStep

        torch, B = self.torch, self.B
        assert 0 <= m <= B and (self.t > 0 or m == 0)
        obs = self.rng.standard_normal((B, self.O)).astype(np.float32)
        obs[:, 0] = self.base + 1 + self.t * B + np.arange(B)
        act = self.rng.standard_normal((B, self.A)).astype(np.float32)
        st = np.where(np.arange(B) < m, 1, 0).astype(np.int32)
        rew = self.rng.standard_normal(B).astype(np.float32)
        disc = self.rng.uniform(0.5, 1.0, B).astype(np.float32)
        dev = lambda x: torch.tensor(x, device="cuda")
        kw = {}
        if self.tracked:
            kw["step_bits"] = dev(np.zeros(B, np.int32) if bits is None else np.asarray(bits, np.int32))
        self.t += 1
        return m, (dev(act), TimeStep(dev(st), dev(rew), dev(disc), None), dev(obs)), kw

    def enqueue(self, staged):
        """one observe on torch's current stream: a launch, nothing that blocks the host"""
        m, args, kw = staged
        self.w.observe(*args, **kw)
        self.rows += m

    def call(self, m, bits=None):
        self.enqueue(self.stage(m, bits))

    def fill(self, rows, bits_p=None):
        """steps until `rows` more rows are written; bits_p: probability of a set step bit per env and call (tracked writers)"""
        while rows > 0:
            m = min(rows, self.B)
            self.call(m, None if bits_p is None else (self.rng.uniform(size=self.B) < bits_p).astype(np.int32))
            rows -= m

    def ring(self):
        """the ring's columns as numpy (synchronises): obs, act, ret, disc, next_obs, taint (zeros for an untracked writer)"""
        got = [x.cpu().numpy() for x in self.w.transitions(with_taint=self.tracked)]
        assert len(got[0]) == min(self.rows, self.capacity) and self.w.num_written() == self.rows
        if not self.tracked:
            got.append(np.zeros(len(got[0]), np.uint8))
        return got

    def close(self):
        self.w.close()


def _check(sampler, feeds, call, *, drawn_before=0, tag=""):
    """one sample() against the restatement and the rings; returns (out as numpy, info, expectation)"""
    rings = [f.ring() for f in feeds]
    written, caps = [f.rows for f in feeds], [f.capacity for f in feeds]
    taints = [r[5] for r in rings] if sampler.skip_tainted else None
    K = sampler.batch_size
    exp = R.sample(sampler.seed, call, K, written, caps, sampler.min_size, taints)
    out = sampler.sample()
    info = sampler.info()
    assert exp["ready"], tag
    assert info == {"ready": True, "total": exp["total"], "call": call, "tainted_kept": exp["kept_tainted"], "samples_drawn": drawn_before + K}, (tag, info)
    got = [None if x is None else x.cpu().numpy() for x in out]
    assert np.array_equal(got[6], exp["index"]), (tag, got[6][:8], exp["index"][:8])
    assert (got[0][:, 0] >= 1).all() and (got[4][:, 0] >= 1).all(), (tag, "a sampled row was never written")
    for r, ring in enumerate(rings):
        m = exp["ring"] == r
        if not m.any():
            continue
        s = exp["slot"][m]
        assert s.max() < len(ring[0]), tag
        for col in range(5):
            assert np.array_equal(_bits(got[col][m]), _bits(ring[col][s])), (tag, r, col)
        if got[5] is not None:
            assert np.array_equal(got[5][m], ring[5][s]), (tag, r)
    assert (got[5] is not None) == all(f.tracked for f in feeds)
    return got, info, exp


# ------------------------------------------------------------------------------------------------ shapes x fill states
@pytest.mark.parametrize("tracked", [False, True])
@pytest.mark.parametrize("O,A", [(104, 12), (289, 59), (1, 1), (577, 131)])
def test_rows_and_indices_at_every_shape_and_fill(torch_mod, O, A, tracked):
    """row wider than one pass of the lanes / odd and 4-byte aligned only / narrower than a wave / wider than what the kernel moves
    at once (512 columns of obs, 128 of act: the chunked continuation); K below a workgroup, ragged last workgroup; ring with one
    row, partly filled, wrapped"""
    from flybody_amd.actor_loop import ReplaySampler

    B = 12
    for K in (1, 3, 257):
        f = Feed(torch_mod, B, O, A, tracked)
        s = ReplaySampler(f.w, K, seed=5 + K)
        drawn = 0
        for call, (more, what) in enumerate([(1, "W = 1"), (B + 4, "W < capacity"), (3 * B * N_STEP, "wrapped")]):
            f.fill(more, 0.2 if tracked else None)
            got, info, exp = _check(s, [f], call, drawn_before=drawn, tag=f"O {O} A {A} K {K} {what}")
            drawn += K
            assert info["total"] == min(f.rows, f.capacity) and int(exp["slot"].max()) < info["total"]
            if what == "W = 1":
                assert not got[6].any()
            if what == "wrapped":
                assert f.rows > f.capacity == info["total"]
                if K == 257:
                    assert len(np.unique(got[6])) == f.capacity      # every slot of the ring is reached, the last included
        s.close(); f.close()


# ------------------------------------------------------------------------------------------------ not ready
@pytest.mark.parametrize("short", [0, 6])
def test_not_ready_writes_nothing(torch_mod, short):
    """W = 0 and W = min_size - 1: sentinel-filled outputs come back unchanged, info says so, the call counter still advances; the
    next call, with W = min_size, is ready.  The sampler exists before the ring has any row."""
    from flybody_amd.actor_loop import ReplaySampler

    torch = torch_mod
    min_size = short + 1
    f = Feed(torch, 8, 7, 3, True)
    s = ReplaySampler(f.w, 5, seed=1, min_size=min_size)
    f.fill(short)
    out = s.sample()
    for x in out:
        x.view(torch.uint8).fill_(0xA5)
    for call in (1, 2):
        out = s.sample()
        assert s.info() == {"ready": False, "total": short, "call": call, "tainted_kept": 0, "samples_drawn": 0}
        for x in out:
            assert bool((x.view(torch.uint8) == 0xA5).all())
    f.fill(1)
    got, info, _ = _check(s, [f], 3, tag="ready once W = min_size")
    assert info["total"] == min_size
    s.close(); f.close()


# ------------------------------------------------------------------------------------------------ several rings
@pytest.mark.parametrize("fills", [(5, 0), (0, 20, 7), (30, 0, 4), (9, 9, 0)])
def test_several_rings(torch_mod, fills):
    """two and three rings of different sizes and fills, one of them empty: ring ids and slots equal the restatement, rows are the
    named ring's slot (the rings' counters differ by 100 000 per ring), the empty ring is never named"""
    from flybody_amd.actor_loop import ReplaySampler

    Bs = (4, 6, 5)
    feeds = [Feed(torch_mod, Bs[r], 10, 3, r != 1, ring_id=r) for r in range(len(fills))]
    for f, n in zip(feeds, fills):
        f.fill(n)
    s = ReplaySampler([f.w for f in feeds], 257, seed=3)
    got, info, exp = _check(s, feeds, 0, tag=str(fills))
    named = set((got[6] >> 40).tolist())
    assert named == {r for r, n in enumerate(fills) if n > 0}
    assert np.array_equal((got[0][:, 0].astype(np.int64) - 1) // 100000, got[6] >> 40)
    assert got[5] is None                                            # ring 1 is untracked: no taint output
    s.close()
    for f in feeds:
        f.close()


# ------------------------------------------------------------------------------------------------ skip_tainted
def test_skip_tainted_mixed_and_all_tainted(torch_mod):
    from flybody_amd.actor_loop import ReplaySampler

    K = 257
    f = Feed(torch_mod, 16, 9, 2, True)
    f.fill(16 * N_STEP + 10, 0.16)                                   # marks span up to four calls' bits: about half the rows tainted
    taint = f.ring()[5]
    assert 0.15 < taint.mean() < 0.85, taint.mean()
    s = ReplaySampler(f.w, K, seed=8, skip_tainted=True)
    plain = ReplaySampler(f.w, K, seed=8)
    got, info, exp = _check(s, [f], 0, tag="mixed")
    assert exp["tries"].max() >= 2 and int(got[5].sum()) == info["tainted_kept"] == exp["kept_tainted"]
    gotp, _, _ = _check(plain, [f], 0, tag="mixed, no rejection")
    assert 0 < gotp[5].sum() < K and np.array_equal(gotp[5], taint[gotp[6]])  # the taint output is the ring's column
    first = exp["tries"] == 0
    assert np.array_equal(got[6][first], gotp[6][first]) and not np.array_equal(got[6], gotp[6])
    s.close(); plain.close()
    # every row tainted: all eight tries fail, the eighth draw is kept and counted, and it is still a whole row of the ring
    g = Feed(torch_mod, 16, 9, 2, True)
    g.fill(16 * N_STEP, 1.0)
    assert g.ring()[5].all()
    s = ReplaySampler(g.w, K, seed=9, skip_tainted=True)
    got, info, exp = _check(s, [g], 0, tag="all tainted")
    assert info["tainted_kept"] == K and got[5].all() and (exp["tries"] == 7).all()
    s.close(); f.close(); g.close()


# ------------------------------------------------------------------------------------------------ stream order, after=
def test_sample_is_ordered_after_observe_on_its_stream(torch_mod):
    """observe immediately followed by sample, no host synchronisation in between: the sample sees the rows of that observe"""
    from flybody_amd.actor_loop import ReplaySampler

    f = Feed(torch_mod, 48, 104, 12, False)
    s = ReplaySampler(f.w, 64, seed=2)
    for _ in range(4):
        f.call(48)
        out = s.sample()
    total = s.info()["total"]
    assert total == min(f.w.num_written(), f.capacity) == 144
    ring = f.ring()
    idx = out.index.cpu().numpy()
    assert np.array_equal(_bits(out.obs.cpu().numpy()), _bits(ring[0][idx])) and np.array_equal(_bits(out.next_obs.cpu().numpy()), _bits(ring[4][idx]))
    s.close(); f.close()


def test_after_waits_for_the_writers_streams(torch_mod):
    """two writers fed on two streams, each behind a device-side delay, every tensor staged beforehand so that the host runs
    ahead: when sample() is enqueued none of the ten observes has started.  Without the waits of `after=` the prologue would count
    rings that are still empty."""
    from flybody_amd.actor_loop import ReplaySampler

    torch = torch_mod
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    feeds = [Feed(torch, 8, 20, 4, False, ring_id=r) for r in range(2)]
    staged = [[f.stage(8) for _ in range(5)] for f in feeds]
    s = ReplaySampler([f.w for f in feeds], 128, seed=4)
    torch.cuda.synchronize()
    for f, st, calls in zip(feeds, streams, staged):
        with torch.cuda.stream(st):
            torch.cuda._sleep(2_000_000)                             # a millisecond or more of device time, far longer than the enqueues below
            for c in calls:
                f.enqueue(c)
    out = s.sample(after=streams)
    info = s.info()
    assert info["total"] == 48 and info["ready"]
    rings = [f.ring() for f in feeds]
    exp = R.sample(4, 0, 128, [40, 40], [24, 24])
    idx = out.index.cpu().numpy()
    assert np.array_equal(idx, exp["index"])
    o = out.obs.cpu().numpy()
    for r in range(2):
        m = exp["ring"] == r
        assert m.any() and np.array_equal(_bits(o[m]), _bits(rings[r][0][exp["slot"][m]]))
    assert (out.next_obs.cpu().numpy()[:, 0] % 100000 > 3 * 8).all()  # only rows of the last three calls are left in a ring of 24
    s.close()
    for f in feeds:
        f.close()


# ------------------------------------------------------------------------------------------------ calls, graph replay
def test_call_counter_lives_on_the_device(torch_mod):
    """three successive calls use c, c + 1, c + 2; the same three captured once into one graph (after warm-up on a side stream, as
    BatchedActorLoop.run(graph=True) does; a straight line: the three calls share the handle's control block, one after the other)
    and replayed three times do as well - calls 6 .. 14, every one drawing its own batch.  Each captured call's outputs are copied
    to a log inside the graph, because the next call overwrites them."""
    from flybody_amd.actor_loop import ReplaySampler

    torch = torch_mod
    K = 67
    f = Feed(torch, 16, 104, 12, True)
    f.fill(40, 0.1)
    s = ReplaySampler(f.w, K, seed=6)
    seen = []
    for c in range(3):
        got, _, _ = _check(s, [f], c, drawn_before=K * c, tag=f"eager call {c}")
        seen.append(got[6])
    assert not np.array_equal(seen[0], seen[1]) and not np.array_equal(seen[1], seen[2])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            s.sample()                                               # calls 3, 4, 5
    torch.cuda.current_stream().wait_stream(side)
    out = s._out
    logs = [[torch.zeros_like(x) for x in out] + [torch.zeros_like(s._info)] for _ in range(3)]
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for j in range(3):                                           # captured, not run
            got = s.sample()
            for dst, src in zip(logs[j], list(got) + [s._info]):
                dst.copy_(src)
    torch.cuda.synchronize()
    ring = f.ring()
    c = 6
    for _ in range(3):
        g.replay()
        torch.cuda.synchronize()
        for j in range(3):
            exp = R.sample(6, c, K, [f.rows], [f.capacity])
            assert logs[j][7].tolist() == [1, 40, c, 0, K * (c + 1), 0, 0, 0], (c, logs[j][7].tolist())
            idx = logs[j][6].cpu().numpy()
            assert np.array_equal(idx, exp["index"]), c
            for col in range(6):
                assert np.array_equal(_bits(logs[j][col].cpu().numpy()), _bits(ring[col][idx])), (c, col)
            c += 1
    assert s.info()["call"] == 14
    s.close(); f.close()


# ------------------------------------------------------------------------------------------------ determinism, lifetime
def test_two_samplers_with_one_seed_agree(torch_mod):
    from flybody_amd.actor_loop import ReplaySampler

    feeds = [Feed(torch_mod, 6, 289, 59, True, ring_id=r) for r in range(2)]
    a = ReplaySampler([f.w for f in feeds], 100, seed=77, skip_tainted=True)   # created before the rings have any row
    for f in feeds:
        f.fill(15, 0.2)
    b = ReplaySampler([f.w for f in feeds], 100, seed=77, skip_tainted=True)
    c = ReplaySampler([f.w for f in feeds], 100, seed=78, skip_tainted=True)
    ga, gb, gc = ([None if x is None else x.cpu().numpy() for x in s.sample()] for s in (a, b, c))
    for x, y in zip(ga, gb):
        assert np.array_equal(_bits(x), _bits(y))
    assert not np.array_equal(ga[6], gc[6])
    assert a._writers[0] is feeds[0].w                               # the sampler holds its writers
    for s in (a, b, c):
        s.close()
    for f in feeds:
        f.close()


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_have_a_text_and_launch_nothing(torch_mod):
    from flybody_amd import _capi
    from flybody_amd.actor_loop import ReplaySampler

    torch = torch_mod
    L = _capi.lib()
    w = Feed(torch, 4, 10, 3, False)
    w2 = Feed(torch, 4, 11, 3, False)
    wt = Feed(torch, 4, 10, 3, True)

    def create(handles, batch=4, min_size=1, flags=0, n=None):
        arr = (C.c_void_p * len(handles))(*handles)
        h = C.c_void_p()
        rc = L.ffe_sampler_create(arr, len(handles) if n is None else n, batch, 0, min_size, flags, 0, C.byref(h))
        return rc, h, L.ffe_sampler_last_error(None).decode()

    hw, hw2, hwt = w.w._h.value, w2.w._h.value, wt.w._h.value
    for args, text in (((([hw, hw2]),), "obs_dim and act_dim must be equal"), ((([hw] * 9),), "outside 1 .. 8"), ((([hw]), 0), "batch 0"),
                       ((([hw]), (1 << 20) + 1), "batch"), ((([hw]), 4, 0), "min_size 0"), ((([hwt, hw]), 4, 1, 1), "FFE_SAMPLE_SKIP_TAINTED needs every writer"),
                       ((([hw, None]),), "writer 1 is null"), ((([hw]), 4, 1, 0, 0), "n_writers 0"), ((([hw]), 4, 1, 2), "unknown flags")):
        rc, h, msg = create(*args)
        assert rc < 0 and not h.value and text in msg, (args, rc, msg)
    # a taint output on an untracked writer: refused by the call, which launches nothing - the next call is still call 0
    rc, h, _ = create([hw])
    assert rc == 0 and h.value
    w.fill(3)
    bufs = [torch.zeros(4, 10, device="cuda"), torch.zeros(4, 3, device="cuda"), torch.zeros(4, device="cuda"), torch.zeros(4, device="cuda"),
            torch.zeros(4, 10, device="cuda")]
    taint, index = torch.zeros(4, dtype=torch.uint8, device="cuda"), torch.zeros(4, dtype=torch.int64, device="cuda")
    ptrs = [b.data_ptr() for b in bufs]
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert L.ffe_sampler_sample(h, *ptrs, taint.data_ptr(), index.data_ptr(), stream) < 0
    assert "taint_dev needs every writer" in L.ffe_sampler_last_error(h).decode()
    assert L.ffe_sampler_sample(h, None, *ptrs[1:], None, None, stream) < 0
    assert L.ffe_sampler_sample(h, *ptrs, None, None, stream) == 0   # taint_dev and index_dev may be NULL
    info_p = C.c_void_p()
    assert L.ffe_sampler_info(h, C.byref(info_p)) == 0
    torch.cuda.synchronize()
    info = w.w._view(info_p.value, (8,), torch.int64).tolist()
    assert info == [1, 3, 0, 0, 4, 0, 0, 0], info
    assert (bufs[0][:, 0] >= 1).all() and not index.any()
    assert L.ffe_sampler_info(h, None) < 0 and "null info_dev" in L.ffe_sampler_last_error(h).decode()
    assert L.ffe_sampler_destroy(h) == 0
    # a null handle: refused with a text where a text can be kept without one
    for call, text in ((lambda: L.ffe_sampler_sample(None, *ptrs, None, None, stream), "ffe_sampler_sample: null handle"),
                       (lambda: L.ffe_sampler_info(None, C.byref(info_p)), "ffe_sampler_info: null handle"),
                       (lambda: L.ffe_sampler_destroy(None), "ffe_sampler_destroy: null handle")):
        rc = call()
        assert rc < 0 and L.ffe_sampler_last_error(None).decode() == text, (rc, text)
    with pytest.raises(ValueError, match="skip_tainted needs every writer"):
        ReplaySampler([wt.w, w.w], skip_tainted=True)
    for f in (w, w2, wt):
        f.close()
