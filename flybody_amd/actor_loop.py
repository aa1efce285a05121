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


_device_view = _capi.device_view


class NStepTransitionWriter(_capi.LibHandle):
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

    _destroy, _last_error = "ffe_nstep_destroy", "ffe_nstep_last_error"

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
        self._check(create(batch_size, obs_dim, act_dim, n_step, float(discount), capacity, device, C.byref(h)), None, "ffe_nstep_create: ")
        self._h = h
        ptr = [C.c_void_p() for _ in range(6)]
        assert self._L.ffe_nstep_buffers(self._h, *[C.byref(p) for p in ptr]) == 0
        self._ptr = [p.value for p in ptr]
        self._taint_ptr = None
        if track_validity:
            tp = C.c_void_p()
            self._check(self._L.ffe_nstep_taint_buffer(self._h, C.byref(tp)), prefix="ffe_nstep_taint_buffer: ")
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
        self._check(rc, prefix="ffe_nstep_observe: ")

    def num_written(self) -> int:
        """Transitions written since creation (synchronises)."""
        t = self._t
        t.cuda.synchronize(self.device)
        # 8 bytes device -> host through a torch view of the counter
        cnt = self._view(self._ptr[5], (1,), t.int64)
        return int(cnt.cpu()[0])

    def _view(self, ptr, shape, dtype):
        """`_capi.device_view` on the writer's device, by torch dtype"""
        t = self._t
        return _device_view(t, self.device, ptr, shape, {t.float32: "<f4", t.int64: "<i8", t.uint8: "|u1"}[dtype])

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


ReplaySample = collections.namedtuple("ReplaySample", ["obs", "action", "n_step_return", "discount", "next_obs", "taint", "index"])


class ReplaySampler(_capi.LibHandle):
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

    _destroy, _last_error = "ffe_sampler_destroy", "ffe_sampler_last_error"

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
        self._check(self._L.ffe_sampler_create(handles, len(writers), self.batch_size, self.seed, self.min_size, 1 if skip_tainted else 0, self.device.index,
                                               C.byref(h)), None)
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
        self._check(rc)
        return o

    def info(self) -> dict:
        """What the last `sample()` found (synchronises the device): `ready`, `total` (rows eligible), `call` (the index the call used),
        `tainted_kept` (draws that stayed tainted after eight tries) and the cumulative `samples_drawn` - with the writers'
        `num_written()` the sample-to-insert ratio the reference's `SampleToInsertRatio` limiter enforces; the host can throttle on
        it, the device never blocks."""
        self._t.cuda.synchronize(self.device)
        v = self._info.tolist()
        return {"ready": bool(v[0]), "total": v[1], "call": v[2], "tainted_kept": v[3], "samples_drawn": v[4]}


def record_dtype():
    """numpy dtype of one episode record (32 bytes; include/flybody_env.h, ffe_eplog_*)"""
    import numpy as np

    return np.dtype([("env", "<i4"), ("tag", "<i4"), ("length", "<i4"), ("ret", "<f4"), ("call", "<i8"), ("flagged_steps", "<i4"), ("bits", "<i4")])


TERMINATED_BIT = 256  # record["bits"] bit 8: the LAST row's discount was 0

_SUMMARY_STATS = ("avg", "var", "max", "min")


def canonical_order(records):
    """The records sorted by (call, env): the order `EpisodeLog.records()` returns and `summarize` counts `last` in (stable, so the
    concatenation of several logs keeps the logs' order among equal keys)."""
    import numpy as np

    records = np.asarray(records)
    if records.dtype != record_dtype():
        raise TypeError(f"records must be a structured array of dtype {record_dtype()}, got {records.dtype}")
    return records[np.lexsort((records["env"], records["call"]))]


def summarize(records, last=None, by_tag=False, num_tags=None):
    """The evaluator's aggregate of the reference, `_eval_agg_stat` (`agents/ray_distributed_dmpo.py:417-440`), over the last `last`
    records of the canonical (call, env) order (None = all; a `last` beyond the record count takes all; the reference's window is
    `eval_average_over`): `avg_` / `var_` / `max_` / `min_` of `episode_return` and `episode_length` - `np.var`, the population
    variance, as there - plus `episodes`, `terminated_fraction` (episodes whose LAST row had discount 0, as opposed to the time limit),
    `flagged_episodes` (with at least one control step of truncated physics) and `flagged_steps` (their sum).  float64 numpy on the
    host, on purpose: this is no hot path, a record is 32 bytes.  Without episodes the statistics are nan and the counts 0.

    `by_tag=True`: every value is an array indexed by tag (flight imitation: the reference clip), of `num_tags` entries (default: the
    largest tag present + 1); tags without episodes give nan and a count of 0.  `records` may be the concatenation of several logs'
    records (one log per env group): counts and statistics are then those of the groups together.

    The reference also logs a per-episode `steps_per_second` and its mean; it is not recorded here: in a batched loop an episode
    has no wall time of its own (`run()` reports the loop's)."""
    import numpy as np

    rec = canonical_order(records)
    if last is not None:
        if isinstance(last, bool) or not isinstance(last, numbers.Integral) or last < 0:
            raise ValueError(f"last must be a non-negative integer or None, got {last!r}")
        rec = rec[len(rec) - min(int(last), len(rec)):]

    def one(r):
        out = {}
        for key, field in (("episode_return", "ret"), ("episode_length", "length")):
            x = r[field].astype(np.float64)
            for stat, fn in zip(_SUMMARY_STATS, (np.mean, np.var, np.max, np.min)):
                out[f"{stat}_{key}"] = float(fn(x)) if len(x) else float("nan")
        out["episodes"] = int(len(r))
        out["terminated_fraction"] = float(np.mean((r["bits"] & TERMINATED_BIT) != 0)) if len(r) else float("nan")
        out["flagged_episodes"] = int((r["flagged_steps"] > 0).sum())
        out["flagged_steps"] = int(r["flagged_steps"].astype(np.int64).sum())
        return out

    if not by_tag:
        return one(rec)
    if len(rec) and int(rec["tag"].min()) < 0:
        raise ValueError("by_tag needs non-negative tags")
    n = (int(rec["tag"].max()) + 1 if len(rec) else 0) if num_tags is None else int(num_tags)
    if len(rec) and int(rec["tag"].max()) >= n:
        raise ValueError(f"a record has tag {int(rec['tag'].max())}, num_tags is {n}")
    rows = [one(rec[rec["tag"] == k]) for k in range(n)]
    keys = list(one(rec[:0]))
    ints = ("episodes", "flagged_episodes", "flagged_steps")
    return {k: np.array([row[k] for row in rows], dtype=np.int64 if k in ints else np.float64) for k in keys}


class EpisodeLog(_capi.LibHandle):
    """One record per finished episode, written on the device (`ffe_eplog_*`, flybody_amd/csrc/episode_log.hip): what the reference's
    `EnvironmentLoop` logs per episode and its evaluator keeps in `self._stats` (`agents/ray_distributed_dmpo.py:401-440`), for B envs
    per call.  `observe(timestep)` is one launch on torch's current stream with no host read (capturable into a HIP graph): per env a
    FIRST row restarts the running return and length, MID adds reward and a step, LAST does the same and emits
    (env, tag, length, ret, call, flagged_steps, bits) into a ring of `capacity >= batch_size` records (slot = count mod capacity).

    `one_shot=True`: only envs armed by `arm(mask)` emit, and an env disarms on its LAST - every armed env contributes exactly its next
    finished episode; `info()["armed_left"]` counts the ones still running (`BatchedEvaluator` polls it)."""

    _destroy, _last_error = "ffe_eplog_destroy", "ffe_eplog_last_error"

    def __init__(self, batch_size: int, *, capacity: int = 1 << 16, device: int = 0, one_shot: bool = False):
        if not isinstance(one_shot, bool):
            raise TypeError(f"one_shot must be a bool, got {one_shot!r}")
        for name, v in (("batch_size", batch_size), ("capacity", capacity)):
            if isinstance(v, bool) or not isinstance(v, numbers.Integral) or v <= 0:
                raise ValueError(f"{name} must be a positive integer, got {v!r}")
        if isinstance(device, bool) or not isinstance(device, numbers.Integral) or device < 0:
            raise ValueError(f"device must be a non-negative integer, got {device!r}")
        if batch_size >= 1 << 31:
            raise ValueError(f"batch_size {batch_size} does not fit the record's int32 env index")
        if capacity < batch_size:
            raise ValueError(f"capacity {capacity} is below batch_size = {batch_size}, the records one observe() can write (every env on LAST): "
                             "they would share slots of the ring")
        import torch

        self._t, self._L = torch, _capi.lib()
        self.batch_size, self.capacity, self.one_shot = int(batch_size), int(capacity), one_shot
        self.device = torch.device("cuda", int(device))
        h = C.c_void_p()
        self._check(self._L.ffe_eplog_create(self.batch_size, self.capacity, 1 if one_shot else 0, int(device), C.byref(h)), None)
        self._h = h
        rec, info = C.c_void_p(), C.c_void_p()
        assert self._L.ffe_eplog_buffers(self._h, C.byref(rec), C.byref(info)) == 0
        self._records = _device_view(torch, self.device, rec.value, (self.capacity * 32,), "|u1")
        self._info = _device_view(torch, self.device, info.value, (4,), "<i8")

    def _check_open(self):
        if not self._h:
            raise RuntimeError("the episode log is closed")

    def _stream(self):
        return C.c_void_p(self._t.cuda.current_stream(self.device).cuda_stream)

    def observe(self, timestep, *, validity=None, tags=None):
        """`timestep`: the `TimeStep` of `env.reset()` / `env.step()` (step_type int32 [B], reward / discount float32 [B]).
        `validity`: the env's int32 [B, 4] validity buffer for the same timestep (`env.validity_buffer` after `env.validity()`) or None
        (records then carry flagged_steps 0 and no episode bits).  `tags`: int32 [B] tensor, or a column of a contiguous int32 [B, k]
        tensor (its stride is passed through), read on LAST rows; None = tag 0."""
        t, B = self._t, self.batch_size
        self._check_open()

        # the C ABI takes raw device pointers: everything it will read is checked here
        def ok(x, dtype, shape):
            return isinstance(x, t.Tensor) and x.is_cuda and x.device == self.device and x.dtype == dtype and x.is_contiguous() and tuple(x.shape) == shape

        st, rew, disc = timestep.step_type, timestep.reward, timestep.discount
        if not (ok(st, t.int32, (B,)) and ok(rew, t.float32, (B,)) and ok(disc, t.float32, (B,))):
            raise ValueError(f"step_type int32 [{B}], reward / discount float32 [{B}], contiguous on the log's device {self.device}")
        if validity is not None and not ok(validity, t.int32, (B, 4)):
            raise ValueError(f"validity must be the contiguous int32 [{B}, 4] validity buffer on the log's device {self.device}")
        tag_ptr, stride = None, 1
        if tags is not None:
            if not isinstance(tags, t.Tensor) or tags.dtype != t.int32:
                raise TypeError("tags must be an int32 tensor")
            if not tags.is_cuda or tags.device != self.device:
                raise ValueError(f"tags must live on the log's device {self.device}")
            if tags.dim() != 1 or tags.shape[0] != B or (B > 1 and tags.stride(0) < 1):
                raise ValueError(f"tags must have shape ({B},): an int32 [{B}] tensor or a column of a contiguous int32 [{B}, k] tensor")
            tag_ptr, stride = tags.data_ptr(), max(1, int(tags.stride(0)))
        rc = self._L.ffe_eplog_observe(self._h, st.data_ptr(), rew.data_ptr(), disc.data_ptr(), validity.data_ptr() if validity is not None else None,
                                       tag_ptr, stride, self._stream())
        self._check(rc)

    def arm(self, mask=None):
        """One-shot logs: envs with `mask[i] != 0` (bool / uint8 [B] on the log's device; None = all) emit their next finished episode.
        One launch on the current stream, nothing read back."""
        t = self._t
        self._check_open()
        if not self.one_shot:
            raise ValueError("arm() needs a log created with one_shot=True: a plain log records every episode")
        m = None
        if mask is not None:
            if not isinstance(mask, t.Tensor) or mask.dtype not in (t.bool, t.uint8):
                raise TypeError("mask must be a bool or uint8 tensor")
            if not mask.is_cuda or mask.device != self.device or tuple(mask.shape) != (self.batch_size,) or not mask.is_contiguous():
                raise ValueError(f"mask must be contiguous, of shape ({self.batch_size},), on the log's device {self.device}")
            m = mask.view(t.uint8) if mask.dtype == t.bool else mask
        self._check(self._L.ffe_eplog_arm(self._h, m.data_ptr() if m is not None else None, self._stream()))

    def info(self) -> dict:
        """`written` (records since creation), `calls` (observe calls), `armed_left` (one-shot: armed envs still in their episode).
        Synchronises the device."""
        self._check_open()
        self._t.cuda.synchronize(self.device)
        v = self._info.tolist()
        return {"written": v[0], "calls": v[1], "armed_left": v[2]}

    def records(self):
        """The min(written, capacity) records in the ring as a numpy structured array (`record_dtype()`), sorted by (call, env) - the
        canonical order; slots inside one call are claimed in no particular order.  Synchronises and copies to the host."""
        n = min(self.info()["written"], self.capacity)
        raw = self._records[:n * 32].cpu().numpy()
        return canonical_order(raw.view(record_dtype()))

    def summary(self, last=None, by_tag=False, num_tags=None):
        """`summarize(self.records(), ...)`"""
        return summarize(self.records(), last=last, by_tag=by_tag, num_tags=num_tags)

    def close(self):
        super().close()
        self._records = self._info = None


class BatchedEvaluator:
    """The reference's evaluator loop for a batch: `EnvironmentLoop(actor_or_evaluator="evaluator")`
    (`agents/ray_distributed_dmpo.py:342-352, 401-440`), which runs the deterministic policy episode after episode and reports
    `_eval_agg_stat`.  `env` is a handle of the evaluator's own, not the one the actors step; `policy` is whatever callable gives the
    deterministic action for `flat_obs [B, O]` (the reference uses `StochasticMeanHead`).

    `run()` works in rounds, `ceil(episodes_per_clip * ntraj / B)` of them: env i of round r gets clip `(r * B + i) mod ntraj` and a wing
    phase from `np.random.RandomState(seed)`, both through `set_next_trajectory_index`; the assignment is the tag tensor.  Each round
    arms a one-shot `EpisodeLog`, resets, and steps until `armed_left` is 0 - one value read on the host every `poll_every` steps, so
    envs that finished go on stepping (auto-reset) unrecorded meanwhile.  Every env contributes exactly its first episode of every
    round: long and short episodes weigh equally, where a "first N finished" rule would favour the short ones.  Envs without clips
    (`walk_on_ball`) run as one clip with tag 0.  More than the env's time-limit control steps + 2 in one round raises."""

    def __init__(self, env, policy, *, episodes_per_clip: int = 1, seed: int = 0, poll_every: int = 64):
        for name, v in (("episodes_per_clip", episodes_per_clip), ("poll_every", poll_every)):
            if isinstance(v, bool) or not isinstance(v, numbers.Integral) or v <= 0:
                raise ValueError(f"{name} must be a positive integer, got {v!r}")
        if isinstance(seed, bool) or not isinstance(seed, numbers.Integral) or not 0 <= seed < 1 << 32:
            raise ValueError(f"seed must be an integer in 0 .. 2^32 - 1, got {seed!r}")
        self.env, self.policy = env, policy
        self.episodes_per_clip, self.seed, self.poll_every = int(episodes_per_clip), int(seed), int(poll_every)
        self.has_clips = getattr(env, "task_kind", None) == "flight_imitation"
        self.ntraj = int(env.refs.ntraj) if self.has_clips else 1
        B = env.batch_size
        self.rounds = -(-self.episodes_per_clip * self.ntraj // B)
        self.max_steps = int(env.time_limit_steps) + 2

    def run(self) -> dict:
        """`summarize` of the rounds' records, plus `"per_clip"` (its `by_tag` tables over the `ntraj` clips), `"records"` (the raw
        records, canonical order), `"rounds"` ((first, one past the last) observe-call index of every round) and `"wall_seconds"`."""
        import numpy as np
        import torch

        env, B = self.env, self.env.batch_size
        rng = np.random.RandomState(self.seed)
        log = EpisodeLog(B, capacity=max(B, self.rounds * B), device=env.device.index, one_shot=True)
        track = hasattr(env, "validity")
        spans, call = [], 0
        start = time.perf_counter()
        try:
            with torch.cuda.device(env.device):
                for r in range(self.rounds):
                    tags = None
                    if self.has_clips:
                        clips = ((r * B + np.arange(B)) % self.ntraj).astype(np.int32)
                        env.set_next_trajectory_index(clips, rng.uniform(size=B))
                        tags = torch.tensor(clips, device=env.device)
                    log.arm()
                    ts = env.reset()
                    log.observe(ts, tags=tags)
                    first, steps, left = call, 0, B
                    while left:
                        if steps >= self.max_steps:
                            raise RuntimeError(f"round {r}: {left} envs still in their first episode after {steps} steps, the time limit is {self.max_steps - 2}")
                        for _ in range(min(self.poll_every, self.max_steps - steps)):
                            with torch.no_grad():
                                action = self.policy(env.flat_observation)
                            ts = env.step(action.contiguous())
                            if track:
                                env.validity()
                            log.observe(ts, validity=env.validity_buffer if track else None, tags=tags)
                            steps += 1
                        left = log.info()["armed_left"]
                    call = first + 1 + steps  # one observe for the reset, one per step
                    spans.append((first, call))
                records = log.records()
        finally:
            log.close()
        wall = time.perf_counter() - start
        assert len(records) == self.rounds * B, (len(records), self.rounds, B)
        out = summarize(records)
        out.update({"per_clip": summarize(records, by_tag=True, num_tags=self.ntraj), "records": records, "rounds": spans, "wall_seconds": wall})
        return out


class BatchedActorLoop:
    def __init__(self, env, policy, adder: NStepTransitionWriter | None = None, track_validity: bool = False):
        """`adder`: optional `NStepTransitionWriter`; fed as the reference's actor feeds its adder (`observe_first` on FIRST,
        `observe(action, next_timestep)` otherwise).

        `track_validity`: every iteration also reads `env.validity()`, hands its `step_bits` to the adder (which must then have
        been created with `track_validity=True` as well) and accumulates batch totals on the device; `run()` then also reports
        `flagged_env_steps` (MID / LAST env-steps whose physics was truncated), `flagged_episodes` (finished episodes with at least
        one) and `flagged_steps_per_flagged_episode`.  Off (the default): the launches and result keys are those without it.

        `log_episodes(log)` attaches an `EpisodeLog`; the constructor keeps the parameter list its callers know."""
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
        self.episode_log = self._task_ints = self._task_reals = None

    def log_episodes(self, episode_log: EpisodeLog | None):
        """Attaches an `EpisodeLog` of the env's batch size (None detaches it) and returns the loop, so that
        `BatchedActorLoop(env, policy, ...).log_episodes(log).run(n)` reads in one line.  Every iteration then also calls the log's
        `observe` (one launch) - with the validity buffer when `track_validity` is on, and for `flight_imitation` with the episode's clip
        as the tag: column 3 (`traj_idx`) of a task-state buffer the loop owns and refills each step (`ffe_get_task_state`, one more
        launch, logged loops only) - and `run()` adds `"episode_log": log`.  Without a log the launches and result keys are those of a
        loop that never had one."""
        t, B, dev = self._t, self.env.batch_size, self.env.device
        if episode_log is not None:
            if not isinstance(episode_log, EpisodeLog):
                raise TypeError(f"episode_log must be an EpisodeLog, got {type(episode_log).__name__}")
            if episode_log.batch_size != B or episode_log.device != dev:
                raise ValueError(f"episode_log is for {episode_log.batch_size} envs on {episode_log.device}, the env has {B} on {dev}")
        self.episode_log = episode_log
        self._task_ints = self._task_reals = None
        if episode_log is not None and getattr(self.env, "task_kind", None) == "flight_imitation":
            self._task_ints = t.zeros(B, 8, dtype=t.int32, device=dev)
            self._task_reals = t.zeros(B, 8, dtype=t.float64, device=dev)
        return self

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
        if self.episode_log is not None:
            self._observe_log(ts, self.env.validity_buffer if self.track_validity else None)

    def _observe_log(self, ts, validity):
        """the timestep just produced -> the episode log (flight: the task state is refilled first, its traj_idx column is the tag)"""
        t, tags = self._t, None
        if self._task_ints is not None:
            if self._L.ffe_get_task_state(self.env._h, self._task_ints.data_ptr(), self._task_reals.data_ptr(),
                                          C.c_void_p(t.cuda.current_stream(self.env.device).cuda_stream)) != 0:
                raise RuntimeError("ffe_get_task_state failed")
            tags = self._task_ints[:, 3]
        self.episode_log.observe(ts, validity=validity, tags=tags)

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

    def _log_result(self) -> dict:
        return {} if self.episode_log is None else {"episode_log": self.episode_log}

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
                    "steps_per_second": num_steps * self.env.batch_size / wall, "capacity_flagged_envs": self._flagged(), **self._validity_result(),
                    **self._log_result()}
        start = time.perf_counter()
        for _ in range(num_steps):
            self._iteration()
        t.cuda.synchronize(self.env.device)
        wall = time.perf_counter() - start
        n = int(self._tot[0].item())
        return {"episodes": n, "episode_return": float(self._sum_ret.item()) / n if n else float("nan"),
                "episode_length": float(self._tot[1].item()) / n if n else float("nan"),
                "steps_per_second": num_steps * self.env.batch_size / wall, "capacity_flagged_envs": self._flagged(), **self._validity_result(),
                    **self._log_result()}

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
        if self.episode_log is not None:  # the FIRST rows: whatever episode the log was following is abandoned
            self._observe_log(ts, None)

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

    def __init__(self, groups, policy, adders=None, track_validity: bool = False, episode_logs=None):
        """`episode_logs`: optional sequence of one `EpisodeLog` per group (of the group's batch size); group g's loop feeds logs[g] on
        the group's stream, `run()` then adds `"episode_logs": logs`; `summarize` takes the concatenation of their `records()`."""
        self.groups = groups
        if episode_logs is not None and len(episode_logs) != len(groups.envs):
            raise ValueError(f"episode_logs has {len(episode_logs)} logs for {len(groups.envs)} groups")
        self.episode_logs = list(episode_logs) if episode_logs is not None else None
        self.loops = [BatchedActorLoop(e, policy, adders[g] if adders is not None else None, track_validity) for g, e in enumerate(groups.envs)]
        if self.episode_logs is not None:
            for lp, log in zip(self.loops, self.episode_logs):
                lp.log_episodes(log)

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
                **self._validity_result(), **({"episode_logs": self.episode_logs} if self.episode_logs is not None else {})}

    def _validity_result(self) -> dict:
        if not self.loops or not self.loops[0].track_validity:
            return {}
        steps, eps, total = (sum(int(lp._vtot[k].item()) for lp in self.loops) for k in range(3))
        return {"flagged_env_steps": steps, "flagged_episodes": eps, "flagged_steps_per_flagged_episode": total / eps if eps else float("nan")}
