"""One fused `ReplaySampler.sample()` (two launches: prologue + gather, flybody_amd/csrc/replay.hip) against the only way to draw a
minibatch without it: a device `torch.randint` plus `index_select` on each of the five `NStepTransitionWriter.transitions()` views.
The views and the row count are taken once, outside the timed region, which flatters the baseline (each real draw would pay a
device synchronisation for the count).

Shapes: flight (O 104, A 12) and walk_on_ball (O 289, A 59), each on a filled ring of 2^20 rows; K in {256, 4096, 65536}.
Timing: device events around 200 calls after 20 warm-up calls; the two variants alternate in one process, three rounds, so the
spread (max - min over the rounds) is visible.  Bytes/s are on K x (2 O + A + 2) x 4 bytes read plus the same written.
Needs an MI355X; fails without one.    python tools/bench_replay_sampler.py [--out profiles/replay_sampler_bench.log]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
import torch

from flybody_amd.actor_loop import NStepTransitionWriter, ReplaySampler
from flybody_amd.dm_types import TimeStep

ROWS, WARMUP, CALLS, ROUNDS = 1 << 20, 20, 200, 3


def filled_writer(O, A, B=8192, n_step=5):
    """a ring of exactly ROWS rows: one FIRST call, then ROWS / B calls in which every env steps (one row per env and call)"""
    w = NStepTransitionWriter(B, O, A, n_step=n_step, discount=0.99, capacity=ROWS)
    st = torch.zeros(B, dtype=torch.int32, device="cuda")
    one = torch.ones(B, device="cuda")
    for t in range(ROWS // B + 1):
        w.observe(torch.randn(B, A, device="cuda"), TimeStep(st, torch.randn(B, device="cuda"), one, None), torch.randn(B, O, device="cuda"))
        st.fill_(1)
    assert w.num_written() == ROWS
    return w


def time_calls(fn):
    for _ in range(WARMUP):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(CALLS):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / CALLS  # us per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(__file__), "..", "profiles", "replay_sampler_bench.log"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_replay_sampler: no GPU - this measurement has no CPU fallback")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say(f"replay sampler: fused sample() vs torch.randint + 5 x index_select; ring {ROWS} rows, {WARMUP} warm-up + {CALLS} timed calls, {ROUNDS} alternating rounds")
    say(f"device: {torch.cuda.get_device_name(0)}; dword copy path only (no 16-byte path is built)")
    verdicts = []
    for name, O, A in (("flight", 104, 12), ("walk_on_ball", 289, 59)):
        w = filled_writer(O, A)
        views = w.transitions()
        n = len(views[2])
        for K in (256, 4096, 65536):
            s = ReplaySampler(w, K, seed=1)

            def baseline():
                idx = torch.randint(n, (K,), device="cuda")
                return [v.index_select(0, idx) for v in views]

            fused, base = [], []
            for _ in range(ROUNDS):
                fused.append(time_calls(s.sample))
                base.append(time_calls(baseline))
            assert s.info()["ready"] and s.info()["total"] == ROWS
            moved = 2 * K * (2 * O + A + 2) * 4
            med = lambda x: sorted(x)[len(x) // 2]
            spread = max(max(fused) - min(fused), max(base) - min(base))
            say(f"{name:13s} O {O:3d} A {A:2d} K {K:6d}: fused {med(fused):8.2f} us/call (rounds {', '.join(f'{x:.2f}' for x in fused)}) | "
                f"baseline {med(base):8.2f} us/call (rounds {', '.join(f'{x:.2f}' for x in base)}) | spread {spread:.2f} us | "
                f"ratio baseline/fused {med(base) / med(fused):.2f} | fused {moved / med(fused) * 1e-3:8.2f} GB/s, baseline {moved / med(base) * 1e-3:8.2f} GB/s "
                f"on {moved} bytes read + written per call")
            if K == 256:
                ok, what = med(base) - med(fused) > spread, "fused faster than the baseline by more than the spread"
            else:
                ok, what = med(fused) - med(base) <= spread, "fused not slower than the baseline by more than the spread"
            verdicts.append(f"{name} K {K}: {what}: {'met' if ok else 'MISSED'} (difference {med(base) - med(fused):+.2f} us, spread {spread:.2f} us)")
            s.close()
        del views
        w.close()
    say()
    for v in verdicts:
        say(v)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
