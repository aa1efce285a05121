"""What the joint-limit rows cost: the time of one `physics_step(ctrl, 10)` (one control step) of `BatchedWalkPhysics` at B = 4 096 for
  plain        a plain handle (FFE_NO_CONTACT | FFE_NO_LIMIT, `walk_step_kernel`) on set A tiled,
  limits_A     a limits handle (`joint_limits=True`, `walk_limits_kernel`) on the same states: 15 of 24 instantiate one or two rows,
  limits_C     a limits handle on set C tiled: 1 ... 32 hinges pushed out of range, every substep of the step solves.
The sets are those of tests/walk_limit_sets.py (built on the CPU with the oracle).  Reported, not asserted.

    python tools/walk_limits_cost.py [--batch 4096] [--windows 20] [--nsteps 10] [--log profiles/walk_limits_cost.log]

Method: device events around ONE call per window, every window from the same start state (set C's rows are gone after a few control
steps, so a longer window would time something else); the three cases alternate window by window so that clock and neighbours act on
all alike; two warm-up windows per case are not counted; every window is printed, the summary is the median with the best and the
worst window.  `ffe_time_kernel` stays refused on these handles."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

WARMUP = 2


def main():
    import numpy as np
    import torch

    import walk_limit_sets as S
    from flybody_amd.batched_env import BatchedWalkPhysics

    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--windows", type=int, default=20)
    ap.add_argument("--nsteps", type=int, default=10)
    ap.add_argument("--amp", type=float, default=0.5)
    ap.add_argument("--log", default=None, help="append the printed lines to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("walk_limits_cost: no GPU (a time measured elsewhere says nothing about the MI355X)")
    lines = []

    def say(obj):
        line = json.dumps(obj)
        print(line, flush=True)
        lines.append(line)

    B = args.batch
    _, A, C = S.sets()

    def tiled(states):
        pick = [states[k % len(states)] for k in range(B)]
        return tuple(torch.tensor(np.stack([s[j] for s in pick]), dtype=torch.float64, device="cuda") for j in range(3))

    g = torch.Generator(device="cuda").manual_seed(0)
    ctrl = (torch.rand(B, 59, device="cuda", generator=g) * 2 * args.amp - args.amp).contiguous()
    cases = {"plain": (BatchedWalkPhysics(batch_size=B), tiled(A)),
             "limits_A": (BatchedWalkPhysics(batch_size=B, joint_limits=True), tiled(A)),
             "limits_C": (BatchedWalkPhysics(batch_size=B, joint_limits=True), tiled(C))}
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = {k: [] for k in cases}
    for w in range(args.windows + WARMUP):
        for name, (h, (q, v, a)) in cases.items():
            h.set_state(q, v)
            h.set_act(a)
            torch.cuda.synchronize()
            ev0.record()
            h.physics_step(ctrl, args.nsteps)
            ev1.record()
            torch.cuda.synchronize()
            t = ev0.elapsed_time(ev1)
            ints, _ = h.get_task_state()
            torch.cuda.synchronize()
            ints = ints.cpu().numpy()
            say({"case": name, "window": w, "warmup": w < WARMUP, "ms": t, "finite": bool(torch.isfinite(h.get_state()[1]).all()),
                 "rows_last_substep_mean": float(ints[:, 4].mean()), "iters_last_substep_mean": float(ints[:, 6].mean()),
                 "flagged_envs": int((ints[:, 7] != 0).sum())})
            if w >= WARMUP:
                ms[name].append(t)
    out = {"batch": B, "substeps_per_call": args.nsteps, "windows": args.windows}
    for name, r in ms.items():
        med = statistics.median(r)
        out[name] = {"median_ms": med, "best_ms": min(r), "worst_ms": max(r), "substeps_per_s_median": B * args.nsteps / med * 1e3}
    out["limits_A_over_plain"] = out["limits_A"]["median_ms"] / out["plain"]["median_ms"]
    out["limits_C_over_plain"] = out["limits_C"]["median_ms"] / out["plain"]["median_ms"]
    say(out)
    for h, _ in cases.values():
        h.close()
    if args.log:
        os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
        with open(args.log, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
