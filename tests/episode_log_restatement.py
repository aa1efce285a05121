"""Numpy restatement of the per-episode log (include/flybody_env.h, ffe_eplog_*; flybody_amd/csrc/episode_log.hip): the per-env
rule, the ring and one-shot arming, one `observe` at a time.  Nothing here is shared with the kernel or imported from the package.

Per env: FIRST restarts the running return and length and adds nothing; MID adds its reward (float32, step order) and one step;
LAST does the same, then emits (env, tag, length, ret, call, flagged_steps, bits) and restarts.  One-shot: only armed envs emit, an
env disarms on its LAST.  Ring: slot = count mod capacity; a call's records take one contiguous range of count, in no particular
order inside it - so after a wrap the OLDEST call still in the ring may survive in part, and which of its records do is free.
`ring()` therefore answers in three parts."""
import numpy as np

FIRST, MID, LAST = 0, 1, 2
DTYPE = np.dtype([("env", "<i4"), ("tag", "<i4"), ("length", "<i4"), ("ret", "<f4"), ("call", "<i8"), ("flagged_steps", "<i4"), ("bits", "<i4")])
assert DTYPE.itemsize == 32


def canonical(rec):
    rec = np.asarray(rec, dtype=DTYPE)
    return rec[np.lexsort((rec["env"], rec["call"]))]


class EpisodeLogRestatement:
    def __init__(self, batch, capacity, one_shot=False):
        assert capacity >= batch >= 1
        self.B, self.capacity, self.one_shot = batch, capacity, one_shot
        self.ret = np.zeros(batch, np.float32)
        self.len = np.zeros(batch, np.int32)
        self.armed = np.zeros(batch, bool)
        self.calls = 0
        self.count = 0
        self.armed_left = 0
        self.per_call = []  # one DTYPE array per observe call (env order), the call's range of count starts at sum of the earlier lengths

    def arm(self, mask=None):
        assert self.one_shot
        self.armed = np.ones(self.B, bool) if mask is None else np.asarray(mask) != 0
        self.armed_left = int(self.armed.sum())

    def observe(self, step_type, reward, discount, info=None, tags=None):
        """tags: [B] values (already the strided column); info: [B, 4].  Returns this call's records."""
        st = np.asarray(step_type)
        assert st.shape == (self.B,) and np.isin(st, (FIRST, MID, LAST)).all()
        rew, disc = np.asarray(reward, np.float32), np.asarray(discount, np.float32)
        first, last = st == FIRST, st == LAST
        # FIRST restarts and adds nothing; MID and LAST add the reward (one float32 addition per step) and one step
        self.ret = np.where(first, np.float32(0), self.ret + rew).astype(np.float32)
        self.len = np.where(first, 0, self.len + 1).astype(np.int32)
        emit = last & self.armed if self.one_shot else last
        if self.one_shot:  # an armed env disarms on its LAST
            self.armed = self.armed & ~last
            self.armed_left -= int(emit.sum())
        rec = np.zeros(int(emit.sum()), DTYPE)
        rec["env"] = np.nonzero(emit)[0]
        rec["tag"] = np.asarray(tags)[emit] if tags is not None else 0
        rec["length"], rec["ret"], rec["call"] = self.len[emit], self.ret[emit], self.calls
        if info is not None:
            info = np.asarray(info)
            rec["flagged_steps"], rec["bits"] = info[emit, 1], info[emit, 2] & 255
        rec["bits"] |= np.where(disc[emit] == 0, 256, 0).astype(np.int32)
        # LAST restarts the counters, whether or not a record was emitted
        self.ret[last], self.len[last] = 0.0, 0
        self.per_call.append(rec)
        self.count += len(rec)
        self.calls += 1
        return rec

    def all_records(self):
        """every record ever emitted, canonical order"""
        return canonical(np.concatenate(self.per_call)) if self.per_call else np.zeros(0, DTYPE)

    def ring(self):
        """(full, partial, n_partial): `full` - the records of the calls that are wholly among the last `capacity` records, canonical
        order; `partial` - the records of the one older call the ring's oldest slots cut through (canonical order, empty when
        there is none), of which exactly `n_partial` are still in the ring, any of them."""
        keep = min(self.count, self.capacity)
        full, partial, n_partial = [], np.zeros(0, DTYPE), 0
        for rec in reversed(self.per_call):
            if keep == 0:
                break
            if len(rec) <= keep:
                full.append(rec)
                keep -= len(rec)
            else:
                partial, n_partial, keep = canonical(rec), keep, 0
        full = canonical(np.concatenate(full)) if full else np.zeros(0, DTYPE)
        return full, partial, n_partial

    def check_ring(self, got):
        """`got`: the ring's min(count, capacity) records in canonical order.  Asserts that they are what `ring()` allows, bit for bit."""
        full, partial, n_partial = self.ring()
        got = canonical(got)
        assert len(got) == min(self.count, self.capacity) == len(full) + n_partial, (len(got), self.count, self.capacity, len(full), n_partial)
        if n_partial:
            cut = int(partial["call"][0])
            head, tail = got[got["call"] == cut], got[got["call"] != cut]
            assert len(head) == n_partial, (len(head), n_partial)
            assert len(np.unique(head["env"])) == n_partial
            where = np.searchsorted(partial["env"], head["env"])
            assert (where < len(partial)).all() and head.tobytes() == partial[where].tobytes(), "a surviving record of the cut call differs"
        else:
            tail = got
        assert tail.tobytes() == full.tobytes(), "the ring's records differ from the restatement"
