"""Batched actor loop: the on-device counterpart of the reference's per-process acme loop
(`agents/ray_distributed_dmpo.py:401-440` `EnvironmentLoop.run_episode`, `agents/actors.py:59-101`).

The reference steps one env per OS process and calls its policy with a batch of 1.  Here observations never leave the
GPU: the policy is any callable `flat_obs[B, O] -> action[B, A]` (e.g. a torch module), and per-env episode statistics
are accumulated with the same keys the reference logs (`episode_length`, `episode_return`, `steps_per_second`).
"""

from __future__ import annotations

import collections
import ctypes as C
import numbers
import time

from . import _capi


def _step_bits_arg(step_bits, batch_size: int, device):
    """(tensor, stride in ints) of the `step_bits` a tracked writer is fed: the int32 [B, 4] buffer of `env.validity()` (its column 0
    is read in place) or an int32 [B] tensor - that buffer's first column, or a contiguous one.  Checked here because the C ABI takes
    a raw device pointer."""
    import torch

    x = step_bits
    if hasattr(x, "step_bits") and not isinstance(x, torch.Tensor):  # the Validity tuple itself
        x = x.step_bits
    if not isinstance(x, torch.Tensor) or x.dtype != torch.int32:
        raise TypeError("step_bits must be an int32 tensor: env.validity().step_bits or the [B, 4] validity buffer")
    if not x.is_cuda or x.device != device:
        raise ValueError(f"step_bits must live on the writer's device {device}")
    if x.dim() == 2 and tuple(x.shape) == (batch_size, 4) and x.is_contiguous():
        return x, 4
    if x.dim() == 1 and x.shape[0] == batch_size and x.stride(0) >= 1:
        return x, int(x.stride(0))
    raise ValueError(f"step_bits must have shape ({batch_size},) or be the contiguous ({batch_size}, 4) validity buffer")


class NStepTransitionWriter:
    """Device-resident batched n-step transition adder (`ffe_nstep_*`, flybody_amd/csrc/nstep.hip): what the reference's
    actors do one env at a time through `acme.adders.reverb.NStepTransitionAdder(n_step=50, discount=...)`
    (`agents/ray_distributed_dmpo.py:514-521`, `agents/actors.py:91-101`), for B envs per call, into a replay ring in HBM.

    `observe(action, timestep)` takes the action that was applied and the `TimeStep` the env returned for it (FIRST rows start
    an episode; their action is ignored).  `transitions()` returns views (obs, action, n_step_return, discount, next_obs) of the
    slots written so far; the learner applies one more factor of `discount` to the bootstrap value, as with acme.

    `track_validity=True` adds a taint column to the ring: `observe(..., step_bits=env.validity().step_bits)` (or the `[B, 4]`
    validity buffer) is then required, and `transitions(with_taint=True)` returns a sixth tensor, uint8 [N], 1 where the transition
    spans an env-step whose physics was truncated - or the step after one, because a launch's last position stage drives the first
    substep of the next (include/flybody_env.h, ffe_nstep_observe_flagged).  Off (the default), everything is as without it."""

    def __init__(self, batch_size: int, obs_dim: int, act_dim: int, *, n_step: int = 50, discount: float = 0.99, capacity: int = 1 << 20,
                 device: int = 0, track_validity: bool = False):
        if not isinstance(track_validity, bool):
            raise TypeError(f"track_validity must be a bool, got {track_validity!r}")
        for name, v in (("batch_size", batch_size), ("obs_dim", obs_dim), ("act_dim", act_dim), ("n_step", n_step), ("capacity", capacity)):
            if isinstance(v, bool) or int(v) != v or v <= 0:
                raise ValueError(f"{name} must be a positive integer, got {v!r}")
        if capacity < batch_size * n_step:
            raise ValueError(f"capacity {capacity} is below batch_size * n_step = {batch_size * n_step}, the rows one observe() can write "
                             "(every env on LAST with a full ring): they would share slots of the replay ring")
        import torch

        self.track_validity = track_validity
        self._t, self._L = torch, _capi.lib()
        self.batch_size, self.obs_dim, self.act_dim, self.n_step, self.discount, self.capacity = batch_size, obs_dim, act_dim, n_step, discount, capacity
        self.device = torch.device("cuda", device)
        h = C.c_void_p()
        create = self._L.ffe_nstep_create_tracked if track_validity else self._L.ffe_nstep_create
        if create(batch_size, obs_dim, act_dim, n_step, float(discount), capacity, device, C.byref(h)) != 0:
            raise RuntimeError("ffe_nstep_create: " + self._L.ffe_nstep_last_error(None).decode())
        self._h = h
        ptr = [C.c_void_p() for _ in range(6)]
        assert self._L.ffe_nstep_buffers(self._h, *[C.byref(p) for p in ptr]) == 0
        self._ptr = [p.value for p in ptr]
        self._taint_ptr = None
        if track_validity:
            tp = C.c_void_p()
            if self._L.ffe_nstep_taint_buffer(self._h, C.byref(tp)) != 0:
                raise RuntimeError("ffe_nstep_taint_buffer: " + self._L.ffe_nstep_last_error(self._h).decode())
            self._taint_ptr = tp.value

    def observe(self, action, timestep, flat_observation, step_bits=None):
        t = self._t
        if self.track_validity and step_bits is None:
            raise ValueError("a writer with track_validity=True needs step_bits (env.validity()) with every observe()")
        if not self.track_validity and step_bits is not None:
            raise ValueError("step_bits given to a writer created without track_validity=True")
        bits = _step_bits_arg(step_bits, self.batch_size, self.device) if self.track_validity else None
        st = timestep.step_type
        # the C ABI takes raw device pointers: everything it will read is checked here (a float64 reward, a strided view or a host
        # tensor would otherwise be read as garbage, or fault)
        def ok(x, dtype, shape):
            return x.is_cuda and x.device == self.device and x.dtype == dtype and x.is_contiguous() and tuple(x.shape) == shape

        B = self.batch_size
        assert ok(action, t.float32, (B, self.act_dim)), "action: float32 [B, A] contiguous on the writer's device"
        assert ok(flat_observation, t.float32, (B, self.obs_dim)), "flat_observation: float32 [B, O] contiguous on the writer's device"
        assert ok(st, t.int32, (B,)) and ok(timestep.reward, t.float32, (B,)) and ok(timestep.discount, t.float32, (B,)), \
            "step_type int32 [B], reward / discount float32 [B], contiguous on the writer's device"
        stream = C.c_void_p(t.cuda.current_stream(self.device).cuda_stream)
        if bits is not None:
            rc = self._L.ffe_nstep_observe_flagged(self._h, action.data_ptr(), st.data_ptr(), timestep.reward.data_ptr(), timestep.discount.data_ptr(),
                                                   flat_observation.data_ptr(), bits[0].data_ptr(), bits[1], stream)
        else:
            rc = self._L.ffe_nstep_observe(self._h, action.data_ptr(), st.data_ptr(), timestep.reward.data_ptr(), timestep.discount.data_ptr(),
                                           flat_observation.data_ptr(), stream)
        if rc != 0:
            raise RuntimeError("ffe_nstep_observe: " + self._L.ffe_nstep_last_error(self._h).decode())

    def num_written(self) -> int:
        """Transitions written since creation (synchronises)."""
        import numpy as np

        t = self._t
        t.cuda.synchronize(self.device)
        out = np.zeros(1, dtype=np.uint64)
        # 8 bytes device -> host through a torch view of the counter
        cnt = self._view(self._ptr[5], (1,), t.int64)
        return int(cnt.cpu()[0])

    def _view(self, ptr, shape, dtype):
        """torch tensor over library-owned device memory (no copy), via the CUDA array interface."""
        t = self._t
        itemsize = {t.float32: 4, t.int64: 8, t.uint8: 1}[dtype]
        typestr = {t.float32: "<f4", t.int64: "<i8", t.uint8: "|u1"}[dtype]

        class _Mem:
            __cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr, "data": (int(ptr), False), "version": 2, "strides": None}

        del itemsize
        return t.as_tensor(_Mem(), device=self.device)

    def transitions(self, with_taint: bool = False):
        """(obs [N,O], action [N,A], n_step_return [N], discount [N], next_obs [N,O]) views of the N = min(written, capacity) filled slots.
        Slots are claimed before their rows are stored: a reader must be stream-ordered after the last `observe` (this method
        synchronises the device through `num_written`); after the ring has wrapped the slots are in no particular age order.
        `with_taint` (tracked writers only) appends the uint8 [N] taint column."""
        if with_taint and not self.track_validity:
            raise ValueError("transitions(with_taint=True) needs a writer created with track_validity=True")
        t, n = self._t, min(self.num_written(), self.capacity)
        o = self._view(self._ptr[0], (self.capacity, self.obs_dim), t.float32)[:n]
        a = self._view(self._ptr[1], (self.capacity, self.act_dim), t.float32)[:n]
        r = self._view(self._ptr[2], (self.capacity,), t.float32)[:n]
        d = self._view(self._ptr[3], (self.capacity,), t.float32)[:n]
        o2 = self._view(self._ptr[4], (self.capacity, self.obs_dim), t.float32)[:n]
        if with_taint:
            return o, a, r, d, o2, self._view(self._taint_ptr, (self.capacity,), t.uint8)[:n]
        return o, a, r, d, o2

    def close(self):
        if getattr(self, "_h", None):
            self._L.ffe_nstep_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


ReplaySample = collections.namedtuple("ReplaySample", ["obs", "action", "n_step_return", "discount", "next_obs", "taint", "index"])


class ReplaySampler:
    """Uniform minibatches from one or several writers' replay rings, drawn and gathered on the device (`ffe_sampler_*`,
    flybody_amd/csrc/replay.hip): the read side of the table the reference builds at `agents/ray_distributed_dmpo.py:85-113`,
    `reverb.Table(sampler=Uniform(), remover=Fifo(), max_size=..., rate_limiter=MinSize(min_replay_size) | SampleToInsertRatio(...))`,
    read by the learner in batches of 256.  The writers' rings are the `Fifo` remover and `max_size`; this is the `Uniform` sampler
    (with replacement), the `MinSize` gate (`min_size`) and the batching.  Reverb is not in the reference tree: its behaviour is
    restated, parity with it is unpinned.

    `writers`: one `NStepTransitionWriter` or a sequence of up to eight (one per env group), on one device, with equal `obs_dim`
    and `act_dim`.  The sampler keeps references to them (it reads their rings through raw pointers), so they cannot be collected
    first; closing a writer by hand before its sampler is an error of the caller.

    `sample()` is two launches on torch's current stream with no host synchronisation: it can be captured into a HIP graph (the
    call counter lives on the device, so every replay draws a fresh batch).  It must be stream-ordered after every `observe()` whose
    rows it may see - the same stream, or `sample(after=streams)` - or a row that is being overwritten can be read torn.  While fewer
    than `min_size` rows are in the rings the call writes nothing (see `info()["ready"]`).
    The `sample()` calls of one sampler must be stream-ordered among themselves too (its control block, counters and outputs are one
    per sampler): consumers on unordered streams each take a sampler of their own.

    `skip_tainted` (tracked writers only): a draw that hits a tainted row is redrawn, up to eight tries; the eighth is kept and
    counted in `info()["tainted_kept"]`."""

    def __init__(self, writers, batch_size: int = 256, *, seed: int = 0, min_size: int = 1, skip_tainted: bool = False):
        if isinstance(writers, NStepTransitionWriter):
            writers = [writers]
        if not isinstance(writers, (list, tuple)):
            raise TypeError(f"writers must be an NStepTransitionWriter or a list / tuple of them, got {type(writers).__name__}")
        if not 1 <= len(writers) <= 8:
            raise ValueError(f"a sampler reads 1 to 8 writers, got {len(writers)}")
        for i, w in enumerate(writers):
            if not isinstance(w, NStepTransitionWriter):
                raise TypeError(f"writers[{i}] is no NStepTransitionWriter: {type(w).__name__}")
            if not getattr(w, "_h", None):
                raise ValueError(f"writers[{i}] is closed")
        if not isinstance(skip_tainted, bool):
            raise TypeError(f"skip_tainted must be a bool, got {skip_tainted!r}")
        for name, v, lo, hi in (("batch_size", batch_size, 1, 1 << 20), ("min_size", min_size, 1, (1 << 63) - 1), ("seed", seed, 0, (1 << 64) - 1)):
            if isinstance(v, bool) or not isinstance(v, numbers.Integral) or not lo <= v <= hi:
                raise ValueError(f"{name} must be an integer in {lo} .. {hi}, got {v!r}")
        w0 = writers[0]
        for i, w in enumerate(writers):
            if (w.obs_dim, w.act_dim) != (w0.obs_dim, w0.act_dim):
                raise ValueError(f"writers[{i}] has rows of (obs_dim, act_dim) = ({w.obs_dim}, {w.act_dim}), writers[0] of ({w0.obs_dim}, {w0.act_dim}): "
                                 "they must be equal")
            if w.device != w0.device:
                raise ValueError(f"writers[{i}] is on {w.device}, writers[0] on {w0.device}: one sampler reads one device")
            if w.capacity >= 1 << 40:
                raise ValueError(f"writers[{i}] has a capacity of 2^40 or more: index packs the slot into 40 bits")
        self.tracked = all(w.track_validity for w in writers)
        if skip_tainted and not self.tracked:
            raise ValueError("skip_tainted needs every writer created with track_validity=True")
        import torch

        self._t, self._L = torch, _capi.lib()
        self._writers = tuple(writers)
        self.batch_size, self.seed, self.min_size, self.skip_tainted = int(batch_size), int(seed), int(min_size), skip_tainted
        self.obs_dim, self.act_dim, self.device = w0.obs_dim, w0.act_dim, w0.device
        handles = (C.c_void_p * len(writers))(*[w._h.value for w in writers])
        h = C.c_void_p()
        if self._L.ffe_sampler_create(handles, len(writers), self.batch_size, self.seed, self.min_size, 1 if skip_tainted else 0, self.device.index,
                                      C.byref(h)) != 0:
            raise RuntimeError(self._L.ffe_sampler_last_error(None).decode())
        self._h = h
        K, dev = self.batch_size, self.device
        self._out = ReplaySample(torch.zeros(K, self.obs_dim, device=dev), torch.zeros(K, self.act_dim, device=dev), torch.zeros(K, device=dev),
                                 torch.zeros(K, device=dev), torch.zeros(K, self.obs_dim, device=dev),
                                 torch.zeros(K, dtype=torch.uint8, device=dev) if self.tracked else None, torch.zeros(K, dtype=torch.int64, device=dev))
        p = C.c_void_p()
        assert self._L.ffe_sampler_info(self._h, C.byref(p)) == 0
        self._info = w0._view(p.value, (8,), torch.int64)

    def sample(self, after=()):
        """One minibatch as `ReplaySample(obs [K,O], action [K,A], n_step_return [K], discount [K], next_obs [K,O], taint [K] uint8 or
        None for untracked writers, index [K] int64 = (ring << 40) | slot)`.  The tensors are owned by the sampler, the same ones on
        every call, and are OVERWRITTEN by the next call (fixed addresses are what make graph capture possible): clone what must
        last.  `after`: streams the current stream is made to wait on first, e.g. `EnvGroups.streams` the writers are fed on."""
        t = self._t
        if not self._h:
            raise RuntimeError("the sampler is closed")
        cur = t.cuda.current_stream(self.device)
        for s in after:
            cur.wait_stream(s)
        o = self._out
        rc = self._L.ffe_sampler_sample(self._h, o.obs.data_ptr(), o.action.data_ptr(), o.n_step_return.data_ptr(), o.discount.data_ptr(), o.next_obs.data_ptr(),
                                        o.taint.data_ptr() if o.taint is not None else None, o.index.data_ptr(), C.c_void_p(cur.cuda_stream))
        if rc != 0:
            raise RuntimeError(self._L.ffe_sampler_last_error(self._h).decode())
        return o

    def info(self) -> dict:
        """What the last `sample()` found (synchronises the device): `ready`, `total` (rows eligible), `call` (the index the call used),
        `tainted_kept` (draws that stayed tainted after eight tries) and the cumulative `samples_drawn` - with the writers'
        `num_written()` the sample-to-insert ratio the reference's `SampleToInsertRatio` limiter enforces; the host can throttle on
        it, the device never blocks."""
        self._t.cuda.synchronize(self.device)
        v = self._info.tolist()
        return {"ready": bool(v[0]), "total": v[1], "call": v[2], "tainted_kept": v[3], "samples_drawn": v[4]}

    def close(self):
        if getattr(self, "_h", None):
            self._L.ffe_sampler_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class BatchedActorLoop:
    def __init__(self, env, policy, adder: NStepTransitionWriter | None = None, track_validity: bool = False):
        """`adder`: optional `NStepTransitionWriter`; fed as the reference's actor feeds its adder (`observe_first` on FIRST,
        `observe(action, next_timestep)` otherwise).

        `track_validity`: every iteration also reads `env.validity()`, hands its `step_bits` to the adder (which must then have
        been created with `track_validity=True` as well) and accumulates batch totals on the device; `run()` then also reports
        `flagged_env_steps` (MID / LAST env-steps whose physics was truncated), `flagged_episodes` (finished episodes with at least
        one) and `flagged_steps_per_flagged_episode`.  Off (the default): the launches and result keys are those without it."""
        import torch

        if not isinstance(track_validity, bool):
            raise TypeError(f"track_validity must be a bool, got {track_validity!r}")
        if adder is not None and bool(getattr(adder, "track_validity", False)) != track_validity:
            raise ValueError("the loop and its adder must agree on track_validity")
        if track_validity and not hasattr(env, "validity"):
            raise ValueError("track_validity needs an env with validity()")
        self.track_validity = track_validity
        self._t, self.env, self.policy, self.adder = torch, env, policy, adder
        B, dev = env.batch_size, env.device
        self._ret = torch.zeros(B, device=dev)
        self._len = torch.zeros(B, dtype=torch.int64, device=dev)
        # episode statistics accumulate on the device: nothing in the loop reads a value back, so launches stay queued ahead
        self._tot = torch.zeros(2, dtype=torch.int64, device=dev)  # finished episodes, sum of their lengths
        self._sum_ret = torch.zeros(1, dtype=torch.float64, device=dev)
        self._vtot = torch.zeros(3, dtype=torch.int64, device=dev) if track_validity else None  # ffe_validity_stats totals
        self._L = _capi.lib()

    @property
    def episodes(self) -> int:
        return int(self._tot[0].item())

    def _iteration(self):
        t = self._t
        with t.no_grad():
            action = self.policy(self.env.flat_observation)
        action = action.contiguous()
        ts = self.env.step(action)
        if self.track_validity:
            self._observe_validity(action, ts)
        elif self.adder is not None:
            self.adder.observe(action, ts, self.env.flat_observation)
        # per-env return / length and the totals of finished episodes: one fused launch (ffe_episode_stats)
        with t.cuda.device(self.env.device):  # (ffe_episode_stats launches on the current device: make it the env's)
            rc = self._L.ffe_episode_stats(ts.step_type.data_ptr(), ts.reward.data_ptr(), self._ret.data_ptr(), self._len.data_ptr(), self._tot.data_ptr(),
                                           self._sum_ret.data_ptr(), self.env.batch_size, C.c_void_p(t.cuda.current_stream(self.env.device).cuda_stream))
        if rc != 0:
            raise RuntimeError("ffe_episode_stats failed")

    def _observe_validity(self, action, ts):
        """validity of the timestep just produced -> the adder's taint column and the batch totals (two or three small launches)"""
        t = self._t
        v = self.env.validity()
        if self.adder is not None:
            self.adder.observe(action, ts, self.env.flat_observation, step_bits=v.step_bits)
        with t.cuda.device(self.env.device):
            rc = self._L.ffe_validity_stats(ts.step_type.data_ptr(), self.env.validity_buffer.data_ptr(), self._vtot.data_ptr(), self.env.batch_size,
                                            C.c_void_p(t.cuda.current_stream(self.env.device).cuda_stream))
        if rc != 0:
            raise RuntimeError("ffe_validity_stats failed")

    def _validity_result(self) -> dict:
        if not self.track_validity:
            return {}
        steps, eps, total = (int(x) for x in self._vtot.tolist())
        return {"flagged_env_steps": steps, "flagged_episodes": eps, "flagged_steps_per_flagged_episode": total / eps if eps else float("nan")}

    def run(self, num_steps: int, graph: bool = False) -> dict:
        """Steps every env `num_steps` times (episodes roll over through the env's auto-reset).  With `graph` one iteration
        (policy, env step, adder, statistics) is captured once into a HIP graph and replayed, which takes the host out of the
        loop (measured neutral with the reference-shaped policy at B = 8192, where the GPU is the bound: tools/bench_actor_loop.py;
        it matters for small batches).  Needs a policy whose work is all on the
        env's device and free of host synchronisation; the env must not be double-buffered."""
        t = self._t
        self._begin()
        if graph:
            side = t.cuda.Stream(self.env.device)
            side.wait_stream(t.cuda.current_stream(self.env.device))
            with t.cuda.stream(side):
                for _ in range(3):
                    self._iteration()
            t.cuda.current_stream(self.env.device).wait_stream(side)
            g = t.cuda.CUDAGraph()
            with t.cuda.graph(g):
                self._iteration()
            t.cuda.synchronize(self.env.device)
            start = time.perf_counter()
            for _ in range(num_steps):
                g.replay()
            t.cuda.synchronize(self.env.device)
            wall = time.perf_counter() - start
            n = int(self._tot[0].item())
            return {"episodes": n, "episode_return": float(self._sum_ret.item()) / n if n else float("nan"),
                    "episode_length": float(self._tot[1].item()) / n if n else float("nan"),
                    "steps_per_second": num_steps * self.env.batch_size / wall, "capacity_flagged_envs": self._flagged(), **self._validity_result()}
        start = time.perf_counter()
        for _ in range(num_steps):
            self._iteration()
        t.cuda.synchronize(self.env.device)
        wall = time.perf_counter() - start
        n = int(self._tot[0].item())
        return {"episodes": n, "episode_return": float(self._sum_ret.item()) / n if n else float("nan"),
                "episode_length": float(self._tot[1].item()) / n if n else float("nan"),
                "steps_per_second": num_steps * self.env.batch_size / wall, "capacity_flagged_envs": self._flagged(), **self._validity_result()}

    def _begin(self):
        """reset + `observe_first`, statistics zeroed (on torch's current stream)"""
        t = self._t
        ts = self.env.reset()
        self._ret.zero_(); self._len.zero_(); self._tot.zero_(); self._sum_ret.zero_()
        if self.track_validity:
            self._vtot.zero_()
        if self.adder is not None:
            kw = {"step_bits": self.env.validity().step_bits} if self.track_validity else {}
            self.adder.observe(t.zeros(self.env.batch_size, self.adder.act_dim, device=self.env.device), ts, self.env.flat_observation, **kw)

    def _flagged(self) -> int:
        """Envs whose step met more simultaneous contacts / constraint rows than the kernel carries (`ffe_get_task_state` int 7: the
        deepest contacts are kept, the env is flagged - walk_on_ball: sticky over the episode; flight: the last control step)."""
        if not hasattr(self.env, "get_task_state"):
            return 0
        w = self.env.get_task_state()[0][:, 7]
        is_flight = self.env.task_kind == "flight_imitation"
        return int((((w >> 8) & 255) != 0).sum()) if is_flight else int((w != 0).sum())



class GroupedActorLoop:
    """The actor loop over asynchronous env groups (`flybody_amd.groups.EnvGroups`): one `BatchedActorLoop` per group, everything a group
    does - policy, env step, adder, statistics - on that group's stream, the host enqueueing the groups round-robin.  No group waits for
    another, as the reference's actor processes do not (`train_dmpo_ray.py:432-452`); one group's launch drains while the next group's
    fills the device.  The policy is shared (its weights are read-only here)."""

    def __init__(self, groups, policy, adders=None, track_validity: bool = False):
        self.groups = groups
        self.loops = [BatchedActorLoop(e, policy, adders[g] if adders is not None else None, track_validity) for g, e in enumerate(groups.envs)]

    def run(self, num_steps: int, graph: bool = False) -> dict:
        """`graph`: every group's iteration is captured once into a HIP graph on the group's stream and replayed (two dozen launches per
        group and step otherwise: with several groups the host becomes the bound before the device does)."""
        import torch

        for g, lp in enumerate(self.loops):
            with self.groups.on(g):
                lp._begin()
        self.groups.synchronize()
        graphs = None
        if graph:
            graphs = []
            for g, lp in enumerate(self.loops):
                with self.groups.on(g):
                    for _ in range(3):
                        lp._iteration()
                self.groups.streams[g].synchronize()
                gr = torch.cuda.CUDAGraph()
                with torch.cuda.graph(gr, stream=self.groups.streams[g]):
                    lp._iteration()
                graphs.append(gr)
            self.groups.synchronize()
        start = time.perf_counter()
        for _ in range(num_steps):
            for g, lp in enumerate(self.loops):
                with self.groups.on(g):
                    if graphs is not None:
                        graphs[g].replay()
                    else:
                        lp._iteration()
        self.groups.synchronize()
        wall = time.perf_counter() - start
        n = sum(int(lp._tot[0].item()) for lp in self.loops)
        ret = sum(float(lp._sum_ret.item()) for lp in self.loops)
        length = sum(int(lp._tot[1].item()) for lp in self.loops)
        return {"episodes": n, "episode_return": ret / n if n else float("nan"), "episode_length": length / n if n else float("nan"),
                "steps_per_second": num_steps * self.groups.batch_size / wall, "capacity_flagged_envs": sum(lp._flagged() for lp in self.loops),
                **self._validity_result()}

    def _validity_result(self) -> dict:
        if not self.loops or not self.loops[0].track_validity:
            return {}
        steps, eps, total = (sum(int(lp._vtot[k].item()) for lp in self.loops) for k in range(3))
        return {"flagged_env_steps": steps, "flagged_episodes": eps, "flagged_steps_per_flagged_episode": total / eps if eps else float("nan")}
