"""Restatement of the replay sampler's draw (flybody_amd/csrc/replay.hip, include/flybody_env.h ffe_sampler_sample), once in plain
Python integers (the definition, `*_int`) and once vectorised in numpy uint64 (what the tests use at size; pinned to the integer
form by tests/test_replay_sampler_cpu.py):

    key    = splitmix64(splitmix64(seed ^ 0x5A3B1E) + call)      call = number of earlier sample calls on the handle
    u(k,t) = splitmix64(key + (k << 3) + t)                      k = output row, t = try 0..7
    g(k,t) = (u(k,t) * total) >> 64                              total = sum of N_r = min(written_r, capacity_r)

Row k is g(k,0); with skip_tainted the first try whose row has taint 0, the eighth when all eight are tainted (counted).  The ring of a
global row g is the one whose range [prefix[r], prefix[r + 1]) holds it, slot = g - prefix[r], index = (r << 40) | slot.
"""
import numpy as np

M64 = (1 << 64) - 1
TRIES = 8
SLOT_BITS = 40


def splitmix64_int(x: int) -> int:
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def call_key(seed: int, call: int) -> int:
    return splitmix64_int((splitmix64_int((seed ^ 0x5A3B1E) & M64) + call) & M64)


def draw_int(seed: int, call: int, k: int, t: int, total: int) -> int:
    """g(k, t) in Python integers: the definition"""
    u = splitmix64_int((call_key(seed, call) + (k << 3) + t) & M64)
    return (u * total) >> 64


def splitmix64(x):
    """numpy uint64, wrapping"""
    x = np.asarray(x, dtype=np.uint64)
    with np.errstate(over="ignore"):
        x = x + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return x ^ (x >> np.uint64(31))


def mulhi64(a, b: int):
    """high 64 bits of the 128-bit product of uint64 array `a` and the integer 0 <= b < 2^64, from 32-bit halves"""
    a = np.asarray(a, dtype=np.uint64)
    m32, s32 = np.uint64(0xFFFFFFFF), np.uint64(32)
    a0, a1 = a & m32, a >> s32
    b0, b1 = np.uint64(b & 0xFFFFFFFF), np.uint64(b >> 32)
    with np.errstate(over="ignore"):
        p00, p01, p10, p11 = a0 * b0, a0 * b1, a1 * b0, a1 * b1
        mid = (p00 >> s32) + (p01 & m32) + (p10 & m32)          # < 3 * 2^32
        return p11 + (p01 >> s32) + (p10 >> s32) + (mid >> s32)


def draws(seed: int, call: int, K: int, total: int, t: int = 0):
    """g(k, t) for k = 0 .. K - 1 as uint64; total >= 1"""
    assert total >= 1
    with np.errstate(over="ignore"):
        x = np.uint64(call_key(seed, call)) + (np.arange(K, dtype=np.uint64) << np.uint64(3)) + np.uint64(t)
    return mulhi64(splitmix64(x), total)


def eligible(written, capacity):
    """N_r = min(written_r, capacity_r), their exclusive prefix sums (length n + 1) and the total"""
    n = [min(int(w), int(c)) for w, c in zip(written, capacity)]
    prefix = [0]
    for v in n:
        prefix.append(prefix[-1] + v)
    return n, prefix, prefix[-1]


def locate(g, prefix):
    """global rows -> (ring, slot): ring = number of r in 1 .. n - 1 with prefix[r] <= g, so an empty ring is never named"""
    g = np.asarray(g, dtype=np.uint64)
    inner = np.asarray(prefix[1:-1], dtype=np.uint64)
    ring = (inner[None, :] <= g[:, None]).sum(axis=1).astype(np.int64) if len(inner) else np.zeros(len(g), np.int64)
    slot = (g - np.asarray(prefix, dtype=np.uint64)[ring]).astype(np.int64)
    return ring, slot


def sample(seed: int, call: int, K: int, written, capacity, min_size: int = 1, taints=None):
    """One sample call.  `taints`: None (no rejection) or one uint8 array per ring (its taint column, at least N_r long).
    Returns a dict: ready, total, and when ready ring [K], slot [K], index [K] (int64), tries [K] (the t that was kept), kept_tainted
    (draws whose eight tries were all tainted).  Not ready (total < min_size, total = 0 included): nothing is drawn."""
    _, prefix, total = eligible(written, capacity)
    if total < min_size or total == 0:
        return {"ready": False, "total": total}
    ring, slot = locate(draws(seed, call, K, total, 0), prefix)
    tries = np.zeros(K, np.int64)
    kept = 0
    if taints is not None:
        def tainted(r, s):
            out = np.zeros(len(r), bool)
            for i in range(len(taints)):
                m = r == i
                out[m] = np.asarray(taints[i])[s[m]] != 0
            return out

        bad = tainted(ring, slot)
        for t in range(1, TRIES):
            if not bad.any():
                break
            r2, s2 = locate(draws(seed, call, K, total, t), prefix)
            ring[bad], slot[bad], tries[bad] = r2[bad], s2[bad], t
            bad = bad & tainted(ring, slot)
        kept = int(bad.sum())
    return {"ready": True, "total": total, "ring": ring, "slot": slot, "index": (ring << SLOT_BITS) | slot, "tries": tries, "kept_tainted": kept}
