"""What the fly's own contacts cost: the time of one `physics_step(ctrl, 10)` (one control step) of `BatchedWalkPhysics` at B = 4 096 for
  floor_R10   a floor handle (`floor_contacts=True`, `floor_step`) on set R10 tiled: the fly's own geoms pass through each other,
  self_R10    a handle with the fly's own contacts (`floor_contacts=True, self_contacts=True`, `floor_self_step`) on the same states.
The set is R10 of tests/walk_self_sets.py (built on the CPU with the oracle); both handles run the committed blob.  Reported, not
asserted.

    python tools/walk_self_cost.py [--batch 4096] [--windows 20] [--nsteps 10] [--log profiles/walk_self_cost.log]

Method (tools/walk_floor_cost.py's): device events around ONE call per window, every window from the same start state; the cases
alternate window by window so that clock and neighbours act on both alike; two warm-up windows per case are not counted; every window
is printed, the summary is the median with the best and the worst window."""
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

    import walk_self_sets as S
    from flybody_amd.batched_env import BatchedWalkPhysics

    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--windows", type=int, default=20)
    ap.add_argument("--nsteps", type=int, default=10)
    ap.add_argument("--amp", type=float, default=0.5)
    ap.add_argument("--log", default=None, help="append the printed lines to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("walk_self_cost: no GPU (a time measured elsewhere says nothing about the MI355X)")
    lines = []

    def say(obj):
        line = json.dumps(obj)
        print(line, flush=True)
        lines.append(line)

    B = args.batch
    R10 = S.r10()
    pick = [R10[k % len(R10)] for k in range(B)]
    q, v, a = (torch.tensor(np.stack([s[j] for s in pick]), dtype=torch.float64, device="cuda") for j in range(3))
    g = torch.Generator(device="cuda").manual_seed(0)
    ctrl = (torch.rand(B, 59, device="cuda", generator=g) * 2 * args.amp - args.amp).contiguous()
    cases = {"floor_R10": BatchedWalkPhysics(batch_size=B, floor_contacts=True),
             "self_R10": BatchedWalkPhysics(batch_size=B, floor_contacts=True, self_contacts=True)}
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = {k: [] for k in cases}
    for w in range(args.windows + WARMUP):
        for name, h in cases.items():
            h.set_state(q, v)
            h.set_act(a)
            torch.cuda.synchronize()
            ev0.record()
            h.physics_step(ctrl, args.nsteps)
            ev1.record()
            torch.cuda.synchronize()
            t = ev0.elapsed_time(ev1)
            ints, reals = h.get_task_state()
            torch.cuda.synchronize()
            ints = ints.cpu().numpy()
            say({"case": name, "window": w, "warmup": w < WARMUP, "ms": t, "finite": bool(torch.isfinite(h.get_state()[1]).all()),
                 "contacts_last_substep_mean": float(ints[:, 5].mean()), "fly_fly_last_substep_mean": float(ints[:, 3].mean()),
                 "limit_rows_last_substep_mean": float(ints[:, 4].mean()), "iters_last_substep_mean": float(ints[:, 6].mean()),
                 "flagged_envs": int((ints[:, 7] != 0).sum())})
            if w >= WARMUP:
                ms[name].append(t)
    out = {"batch": B, "substeps_per_call": args.nsteps, "windows": args.windows}
    for name, r in ms.items():
        med = statistics.median(r)
        out[name] = {"median_ms": med, "best_ms": min(r), "worst_ms": max(r), "substeps_per_s_median": B * args.nsteps / med * 1e3}
    out["self_R10_over_floor"] = out["self_R10"]["median_ms"] / out["floor_R10"]["median_ms"]
    say(out)
    for h in cases.values():
        h.close()
    if args.log:
        os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
        with open(args.log, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
