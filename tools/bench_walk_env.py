"""Control steps/s of the walk_imitation environment (`BatchedWalkEnv`) at B = 4 096, and the share of each launch in a step: with the
floor off (csrc/walk_env.hip `imitation_step_kernel` and the four launches around it) or, with `--floor`, on the floor plane
(csrc/walk_floor_env.hip `imitation_floor_step` in its place; `walk_imitation(floor_contacts="primitives")`).  Nothing is asserted and
there is no target.  `--self` compares the environment on the floor with the fly's own contacts (csrc/walk_imit_self_env.hip
`imitation_self_step`; `walk_imitation(floor_contacts="primitives", self_contacts=True)`) with the one without them in one session:
the two envs and the two action cases alternate window by window, and the summary holds the medians, their ratio and the flagged steps.
`--full` does the same for the environment with the plane against ellipsoids and cylinders too (csrc/walk_imit_full_env.hip
`imitation_full_step`; `floor_convex=True`) against the one with `self_contacts=True` alone.

    python tools/bench_walk_env.py [--floor | --self | --full] [--batch 4096] [--windows 5] [--iters 50] [--log profiles/bench_walk_env.log] [--no-trace]

Timing: `ffe_time_steps` (device events around `iters` step launches on the env's stream) per window; the cases - zero actions and
uniform +-0.5 actions - alternate window by window so that clock and neighbours act on both alike; window 0 of each case warms up and
is not counted; the summary is the median and the best window.  Every window starts from a reset (a fly without a floor falls, and an
episode ends on its 13th step when the root has left the reference by 0.3 cm, so auto-resets are part of the steady state measured;
on the floor the states are the reset poses standing on it and what 50 steps make of them: the episodes run to the end of their clips).

Shares: a run of its own under `rocprofv3 --kernel-trace --stats` (a fresh child process, `--trace-child`, 200 steps at +-0.5), whose
kernel statistics are folded by launch."""
import argparse
import csv
import glob
import json
import os
import statistics
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))

def launches(floor):
    return ("episode_begin_kernel", "walk_reference_pose_kernel", "imitation_floor_step" if floor else "imitation_step_kernel", "walk_evaluate_kernel",
            "episode_close_kernel")


def make_env(batch, floor=False, self_contacts=False, floor_convex=False):
    from flybody_amd import fly_envs

    return fly_envs.walk_imitation(floor_contacts="primitives" if floor else False, self_contacts=self_contacts, floor_convex=floor_convex,
                                   batch_size=batch)


def compare_self(args, say, new="floor_self", old="floor"):
    """`--self`: windows alternate between the env with the fly's own contacts and the floor env without them, case by case; `--full`:
    between the env with the plane against ellipsoids and cylinders too (`floor_full`) and the one with the fly's own contacts."""
    import numpy as np
    import torch

    B = args.batch
    kinds = {"floor": (True, False, False), "floor_self": (True, True, False), "floor_full": (True, True, True)}
    envs = {new: make_env(B, *kinds[new]), old: make_env(B, *kinds[old])}
    cases = action_cases(torch, B)
    ms = {(e, c): [] for e in envs for c in cases}
    flagged = {e: 0 for e in envs}
    for w in range(args.windows + 1):  # window 0 warms up
        for case, act in cases.items():
            for name, env in envs.items():
                env.reset()
                t = env.time_steps(act, args.iters)
                v = env.validity()
                nflag = int(v.episode_flagged_steps.sum())  # (flagged control steps of the episodes the window's steps belong to)
                say({"env": name, "case": case, "window": w, "warmup": w == 0, "ms_per_step": t, "env_steps_per_s": B / t * 1e3,
                     "finite": bool(torch.isfinite(env.flat_observation).all()), "episode_flagged_steps": nflag,
                     "episode_bits": int(np.bitwise_or.reduce(v.episode_bits.cpu().numpy(), initial=0))})
                if w > 0:
                    ms[(name, case)].append(t)
                    flagged[name] += nflag
    out = {"batch": B, "iters_per_window": args.iters, "windows": args.windows, "flagged_steps": flagged}
    for case in cases:
        a, b = statistics.median(ms[(new, case)]), statistics.median(ms[(old, case)])
        out[case] = {new + "_median_ms_per_step": a, old + "_median_ms_per_step": b, "ratio": a / b,
                     new + "_step_kernel_alone_ms": envs[new].time_kernel(cases[case], args.iters),
                     old + "_step_kernel_alone_ms": envs[old].time_kernel(cases[case], args.iters)}
    say(out)
    for env in envs.values():
        env.close()


def action_cases(torch, batch):
    g = torch.Generator(device="cuda").manual_seed(0)
    return {"zero": torch.zeros(batch, 59, device="cuda"), "uniform_0.5": (torch.rand(batch, 59, device="cuda", generator=g) - 0.5).contiguous()}


def trace_child(batch, steps, floor):
    import torch

    env = make_env(batch, floor)
    act = action_cases(torch, batch)["uniform_0.5"]
    env.reset()
    for _ in range(steps):
        env.step(act)
    torch.cuda.synchronize()
    env.close()


def launch_shares(batch, steps, floor):
    """{launch: {"calls", "mean_us", "share"}} from a rocprofv3 run of `trace_child`."""
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "-o", "walk_env", "--", sys.executable,
               os.path.abspath(__file__), "--trace-child", "--batch", str(batch), "--trace-steps", str(steps)] + (["--floor"] if floor else [])
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        if r.returncode != 0:
            raise RuntimeError("rocprofv3 failed: " + (r.stderr or r.stdout)[-2000:])
        files = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
        if not files:
            raise RuntimeError("rocprofv3 wrote no kernel statistics")
        rows = list(csv.DictReader(open(files[0])))
    LAUNCHES = launches(floor)
    out, total = {}, 0.0
    for name in LAUNCHES:
        mine = [r for r in rows if name in r["Name"]]
        ns = sum(float(r["TotalDurationNs"]) for r in mine)
        calls = sum(int(r["Calls"]) for r in mine)
        out[name] = {"calls": calls, "mean_us": ns / calls / 1e3 if calls else 0.0, "total_ns": ns}
        total += ns
    for name in LAUNCHES:
        out[name]["share"] = out[name].pop("total_ns") / total if total else 0.0
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--trace-steps", type=int, default=200)
    ap.add_argument("--floor", action="store_true", help="the environment on the floor plane instead of the one with the floor off")
    ap.add_argument("--self", dest="self_contacts", action="store_true",
                    help="compare the environment on the floor with the fly's own contacts with the one without them (no trace)")
    ap.add_argument("--full", dest="full", action="store_true",
                    help="compare the environment with the plane against ellipsoids and cylinders too with the one with the fly's own contacts (no trace)")
    ap.add_argument("--no-trace", action="store_true", help="skip the rocprofv3 run")
    ap.add_argument("--trace-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--log", default=None, help="append the printed lines to this file")
    args = ap.parse_args()
    if args.trace_child:
        trace_child(args.batch, args.trace_steps, args.floor)
        return
    lines = []

    def say(obj):
        line = json.dumps(obj)
        print(line, flush=True)
        lines.append(line)

    if args.self_contacts or args.full:
        if args.full:
            compare_self(args, say, new="floor_full", old="floor_self")
        else:
            compare_self(args, say)
        if args.log:
            os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
            with open(args.log, "a") as f:
                f.write("\n".join(lines) + "\n")
        return
    if not args.no_trace:  # first, while this process has not touched the device
        say({"batch": args.batch, "floor": args.floor, "trace_steps": args.trace_steps,
             "launch_shares": launch_shares(args.batch, args.trace_steps, args.floor)})
    import torch

    B = args.batch
    env = make_env(B, args.floor)
    cases = action_cases(torch, B)
    ms = {k: [] for k in cases}
    for w in range(args.windows + 1):  # window 0 warms up
        for name, act in cases.items():
            env.reset()
            t = env.time_steps(act, args.iters)
            finite = bool(torch.isfinite(env.flat_observation).all())
            say({"case": name, "floor": args.floor, "window": w, "warmup": w == 0, "ms_per_step": t, "env_steps_per_s": B / t * 1e3, "finite": finite})
            if w > 0:
                ms[name].append(t)
    kernel_ms = {name: env.time_kernel(act, args.iters) for name, act in cases.items()}
    out = {"batch": B, "floor": args.floor, "iters_per_window": args.iters, "windows": args.windows, "launches_per_step": len(launches(args.floor))}
    for name, t in ms.items():
        out[name] = {"median_ms_per_step": statistics.median(t), "best_ms_per_step": min(t), "median_env_steps_per_s": B / statistics.median(t) * 1e3,
                     "step_kernel_alone_ms": kernel_ms[name]}
    say(out)
    env.close()
    if args.log:
        os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
        with open(args.log, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
