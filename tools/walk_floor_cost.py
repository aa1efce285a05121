"""What the floor contacts cost: the time of one `physics_step(ctrl, 10)` (one control step) of `BatchedWalkPhysics` at B = 4 096 for
  limits_F10     a limits handle (`joint_limits=True`, `walk_limits_kernel`) on set F10 tiled: the fly falls through the floor,
  floor_F10      a floor handle (`floor_contacts=True`, `floor_step`) on the same states: 2 ... 6 contacts, 7 ... 18 rows,
  limits_stand   a limits handle on the standing fly (the state a floor handle reaches 60 control steps after the reset pose, zero ctrl),
  floor_stand    a floor handle on the same state: six legs on the floor.
The sets are those of tests/walk_floor_sets.py (built on the CPU with the oracle); every handle runs the committed blob.  Reported, not
asserted.

    python tools/walk_floor_cost.py [--batch 4096] [--windows 20] [--nsteps 10] [--log profiles/walk_floor_cost.log]

Method (tools/walk_limits_cost.py's): device events around ONE call per window, every window from the same start state; the cases
alternate window by window so that clock and neighbours act on all alike; two warm-up windows per case are not counted; every window
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

    import walk_floor_sets as S
    from flybody_amd.batched_env import BatchedWalkPhysics

    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--windows", type=int, default=20)
    ap.add_argument("--nsteps", type=int, default=10)
    ap.add_argument("--amp", type=float, default=0.5)
    ap.add_argument("--log", default=None, help="append the printed lines to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("walk_floor_cost: no GPU (a time measured elsewhere says nothing about the MI355X)")
    lines = []

    def say(obj):
        line = json.dumps(obj)
        print(line, flush=True)
        lines.append(line)

    B = args.batch
    _, _, F10 = S.sets()

    def tiled(states):
        pick = [states[k % len(states)] for k in range(B)]
        return tuple(torch.tensor(np.stack([s[j] for s in pick]), dtype=torch.float64, device="cuda") for j in range(3))

    g = torch.Generator(device="cuda").manual_seed(0)
    ctrl = (torch.rand(B, 59, device="cuda", generator=g) * 2 * args.amp - args.amp).contiguous()
    zero = torch.zeros(B, 59, device="cuda")
    floor, limits = BatchedWalkPhysics(batch_size=B, floor_contacts=True), BatchedWalkPhysics(batch_size=B, joint_limits=True)
    # the standing fly: 60 control steps from the reset pose of clip 0 with zero ctrl
    q0 = torch.tensor(np.tile(S.reset_pose(), (B, 1)), dtype=torch.float64, device="cuda")
    floor.set_state(q0, torch.zeros(B, 108, dtype=torch.float64, device="cuda"))
    floor.set_act(torch.zeros(B, 59, dtype=torch.float64, device="cuda"))
    for _ in range(60):
        floor.physics_step(zero, 10)
    sq, sv = floor.get_state()
    stand = (sq.clone(), sv.clone(), floor.get_act().clone())
    cases = {"limits_F10": (limits, tiled(F10), ctrl), "floor_F10": (floor, tiled(F10), ctrl),
             "limits_stand": (limits, stand, zero), "floor_stand": (floor, stand, zero)}
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = {k: [] for k in cases}
    for w in range(args.windows + WARMUP):
        for name, (h, (q, v, a), c) in cases.items():
            h.set_state(q, v)
            h.set_act(a)
            torch.cuda.synchronize()
            ev0.record()
            h.physics_step(c, args.nsteps)
            ev1.record()
            torch.cuda.synchronize()
            t = ev0.elapsed_time(ev1)
            ints, reals = h.get_task_state()
            torch.cuda.synchronize()
            ints, reals = ints.cpu().numpy(), reals.cpu().numpy()
            say({"case": name, "window": w, "warmup": w < WARMUP, "ms": t, "finite": bool(torch.isfinite(h.get_state()[1]).all()),
                 "contacts_last_substep_mean": float(ints[:, 5].mean()), "rows_last_substep_mean": float((3 * ints[:, 5] + ints[:, 4]).mean()),
                 "iters_last_substep_mean": float(ints[:, 6].mean()), "normal_force_mean": float(reals[:, 0].mean()),
                 "flagged_envs": int((ints[:, 7] != 0).sum())})
            if w >= WARMUP:
                ms[name].append(t)
    out = {"batch": B, "substeps_per_call": args.nsteps, "windows": args.windows}
    for name, r in ms.items():
        med = statistics.median(r)
        out[name] = {"median_ms": med, "best_ms": min(r), "worst_ms": max(r), "substeps_per_s_median": B * args.nsteps / med * 1e3}
    out["floor_F10_over_limits"] = out["floor_F10"]["median_ms"] / out["limits_F10"]["median_ms"]
    out["floor_stand_over_limits"] = out["floor_stand"]["median_ms"] / out["limits_stand"]["median_ms"]
    say(out)
    floor.close()
    limits.close()
    if args.log:
        os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
        with open(args.log, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
