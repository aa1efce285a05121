"""Physics substeps/s of the free-root walking fly (`BatchedWalkPhysics`, csrc/walk_env.hip) at B = 4 096, beside the tethered fly's
`ffe_physics_step` (`BatchedBallEnv`) with the same flags in the same process.  The comparison is the point: the tethered kernel still
carries its (idle) collision and constraint code, the free-root kernel has them compiled out.  The ratio is reported, not asserted.

    python tools/bench_walk_physics.py [--batch 4096] [--windows 5] [--launches 40] [--nsteps 10] [--log profiles/bench_walk_physics.log]

Method: device events around `launches` calls of `physics_step(ctrl, nsteps)`; `windows` windows per handle, the two handles
alternating window by window so that clock and neighbours act on both alike; every window is printed, the summary is the median and
the best window.  Each window starts from the same state (the handle's initial pose at rest) under the same seeded controls (uniform
+-0.2); the first window of each handle is a warm-up and is not counted.  Without contacts both flies simply move their legs in free
space (the free-root one falls: 0.08 s of free fall per window at the defaults)."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))

FLAGS = 64 | 2  # FFE_NO_CONTACT | FFE_NO_LIMIT


def main():
    import torch

    from flybody_amd.batched_env import BatchedBallEnv, BatchedWalkPhysics

    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--launches", type=int, default=40)
    ap.add_argument("--nsteps", type=int, default=10)
    ap.add_argument("--amp", type=float, default=0.2)
    ap.add_argument("--log", default=None, help="append the printed lines to this file")
    args = ap.parse_args()
    lines = []

    def say(obj):
        line = json.dumps(obj)
        print(line, flush=True)
        lines.append(line)

    B = args.batch
    g = torch.Generator(device="cuda").manual_seed(0)
    ctrl = (torch.rand(B, 59, device="cuda", generator=g) * 2 * args.amp - args.amp).contiguous()
    walk = BatchedWalkPhysics(batch_size=B, physics_flags=FLAGS)
    ball = BatchedBallEnv(batch_size=B, physics_flags=FLAGS)
    ball.reset()
    handles = {"walk_physics": walk, "walk_on_ball_physics": ball}
    start = {k: tuple(x.clone() for x in h.get_state()) + (h.get_act().clone(),) for k, h in handles.items()}
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    rates = {k: [] for k in handles}
    for w in range(args.windows + 1):  # window 0 warms up
        for name, h in handles.items():
            q, v, a = start[name]
            h.set_state(q, v)
            h.set_act(a)
            torch.cuda.synchronize()
            ev0.record()
            for _ in range(args.launches):
                h.physics_step(ctrl, args.nsteps)
            ev1.record()
            torch.cuda.synchronize()
            ms = ev0.elapsed_time(ev1)
            rate = B * args.launches * args.nsteps / ms * 1e3
            finite = bool(torch.isfinite(h.get_state()[1]).all())
            say({"handle": name, "window": w, "warmup": w == 0, "ms": ms, "substeps_per_s": rate, "finite": finite})
            if w > 0:
                rates[name].append(rate)
    out = {"batch": B, "flags": FLAGS, "launches_per_window": args.launches, "substeps_per_launch": args.nsteps, "windows": args.windows}
    for name, r in rates.items():
        out[name] = {"median_substeps_per_s": statistics.median(r), "best_substeps_per_s": max(r), "worst_substeps_per_s": min(r)}
    out["ratio_walk_over_ball_median"] = out["walk_physics"]["median_substeps_per_s"] / out["walk_on_ball_physics"]["median_substeps_per_s"]
    say(out)
    for h in handles.values():
        h.close()
    if args.log:
        os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
        with open(args.log, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
