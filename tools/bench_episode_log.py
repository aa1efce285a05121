"""What the per-episode log costs the actor loop, and what one evaluation sweep takes (flybody_amd/csrc/episode_log.hip;
`flybody_amd.actor_loop.EpisodeLog`, `BatchedEvaluator`).

Flight, B = 8192, the reference-shaped policy of tools/bench_actor_loop.py (LayerNormMLP 512-512-256 + a Gaussian head, random
weights, canonical clipped actions), no adder.  Configurations, each run REPEATS times of STEPS steps after a warm-up run, the
configurations alternating inside every repeat so that drift over the session shows in all of them alike:

  parent             the loop of the parent commit: --parent-actor-loop FILE names a copy of that commit's flybody_amd/actor_loop.py
                     (e.g. `git show HEAD~1:flybody_amd/actor_loop.py > FILE`), loaded beside the current one over the same
                     library; skipped when not given
  no_log             this loop without a log
  log                this loop with a log               (+ 2 launches per step: ffe_get_task_state for the clip, ffe_eplog_observe)
  log_validity       this loop with a log and track_validity
  validity           this loop with track_validity alone (+ 2 launches per step without an adder: ffe_get_validity, ffe_validity_stats)

Conditions (decided before anything was measured; reported as met / MISSED, never tuned):
  1. no_log lies inside the parent's run-to-run spread: |median(no_log) - median(parent)| <= max(parent) - min(parent)
  2. the drop no_log -> log is no larger than the drop no_log -> validity of the same session
Then one `BatchedEvaluator` sweep (episodes_per_clip = 1, the policy's mean) over the 64 synthetic clips at B = 256: wall time.
Needs an MI355X; fails without one.    python tools/bench_episode_log.py [--parent-actor-loop FILE] [--out profiles/episode_log_bench.log]"""
import argparse
import importlib.util
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
import torch

from flybody_amd import actor_loop, fly_envs

B, STEPS, WARMUP, REPEATS = 8192, 300, 30, 5


class Policy(torch.nn.Module):
    def __init__(self, obs, act):
        super().__init__()
        self.l0 = torch.nn.Linear(obs, 512); self.ln = torch.nn.LayerNorm(512)
        self.l1 = torch.nn.Linear(512, 512); self.l2 = torch.nn.Linear(512, 256)
        self.mean = torch.nn.Linear(256, act); self.std = torch.nn.Linear(256, act)

    def trunk(self, o):
        h = torch.tanh(self.ln(self.l0(o)))
        return torch.nn.functional.elu(self.l2(torch.nn.functional.elu(self.l1(h))))

    def forward(self, o):
        h = self.trunk(o)
        mu, sd = self.mean(h), torch.nn.functional.softplus(self.std(h)) + 1e-4
        return torch.clamp(mu + sd * torch.randn_like(mu), -1.0, 1.0)

    def mean_action(self, o):  # what the reference's evaluator runs (StochasticMeanHead)
        return torch.clamp(self.mean(self.trunk(o)), -1.0, 1.0)


def load_parent(path):
    spec = importlib.util.spec_from_file_location("flybody_amd._parent_actor_loop", path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    return mod


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-actor-loop", default=None)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(__file__), "..", "profiles", "episode_log_bench.log"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_episode_log: no GPU - this measurement has no CPU fallback")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say(f"episode log: actor-loop throughput, flight B {B}, {WARMUP} warm-up + {STEPS} timed steps, {REPEATS} alternating repeats; device {torch.cuda.get_device_name(0)}")
    torch.manual_seed(0)
    env = fly_envs.flight_imitation(batch_size=B, random_state=0, canonical_actions=True, clip_actions=True)
    pol = Policy(env.spec.obs_dim, env.spec.action_dim).cuda()
    log = actor_loop.EpisodeLog(B, capacity=1 << 20)
    log_v = actor_loop.EpisodeLog(B, capacity=1 << 20)
    loops = {}
    if args.parent_actor_loop:
        loops["parent"] = load_parent(args.parent_actor_loop).BatchedActorLoop(env, pol)
    loops["no_log"] = actor_loop.BatchedActorLoop(env, pol)
    loops["log"] = actor_loop.BatchedActorLoop(env, pol).log_episodes(log)
    loops["log_validity"] = actor_loop.BatchedActorLoop(env, pol, track_validity=True).log_episodes(log_v)
    loops["validity"] = actor_loop.BatchedActorLoop(env, pol, track_validity=True)
    for lp in loops.values():
        lp.run(WARMUP)
    rates = {k: [] for k in loops}
    for _ in range(REPEATS):
        for k, lp in loops.items():
            rates[k].append(lp.run(STEPS)["steps_per_second"])
    med = lambda x: sorted(x)[len(x) // 2]
    for k, v in rates.items():
        say(f"{k:13s} median {med(v) / 1e6:8.4f} M env-steps/s  spread {(max(v) - min(v)) / 1e6:7.4f}  runs " + ", ".join(f"{x / 1e6:.4f}" for x in v))
    info = log.info()
    say(f"log: {info['written']} records in {info['calls']} calls; last 200: " + str({k: round(v, 3) for k, v in log.summary(last=200).items()}))
    say()
    if "parent" in rates:
        d, spread = abs(med(rates["no_log"]) - med(rates["parent"])), max(rates["parent"]) - min(rates["parent"])
        say(f"1. no_log inside the parent's spread: {'met' if d <= spread else 'MISSED'} (|difference of medians| {d / 1e6:.4f} M, parent's spread {spread / 1e6:.4f} M)")
    else:
        say("1. no_log inside the parent's spread: not measured (no --parent-actor-loop)")
    drop_log, drop_val = med(rates["no_log"]) - med(rates["log"]), med(rates["no_log"]) - med(rates["validity"])
    say(f"2. drop no_log -> log no larger than no_log -> validity: {'met' if drop_log <= drop_val else 'MISSED'} (log {drop_log / 1e6:+.4f} M = {100 * drop_log / med(rates['no_log']):+.2f} %, "
        f"validity {drop_val / 1e6:+.4f} M = {100 * drop_val / med(rates['no_log']):+.2f} %; launches added per step: log 2, validity 2)")
    log.close(); log_v.close(); env.close()
    # one evaluation sweep
    Be = 256
    ev_env = fly_envs.flight_imitation(batch_size=Be, random_state=1, canonical_actions=True, clip_actions=True)
    ev = actor_loop.BatchedEvaluator(ev_env, pol.mean_action, episodes_per_clip=1, seed=0)
    out = ev.run()
    say()
    say(f"evaluator: one sweep of {ev.ntraj} synthetic clips at B {Be} ({ev.rounds} round, {out['episodes']} episodes, lengths {out['min_episode_length']:.0f} .. "
        f"{out['max_episode_length']:.0f}, mean {out['avg_episode_length']:.1f}): {out['wall_seconds']:.3f} s wall")
    ev_env.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
