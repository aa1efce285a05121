"""flight_imitation at the benchmark's workload (B = 8192, actions uniform over the raw action spec) with contact_capacity 6 and 12:
env-steps in which a position stage met more contacts than the solver carries (ffe_get_task_state int 7 bits 8-15), envs flagged at
the end of the run, the largest number of contacts a substep used, per finished episode (env.validity(), read on LAST rows) the share
with at least one flagged control step and the mean number of flagged steps in those, and env-steps/s of both capacities through ffe_time_steps, measured
alternately in one process (median of `rounds` blocks each).
    python tools/flight_overflow_stats.py [batch] [steps] [rounds] [timed launches per block]"""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
import torch

from flybody_amd import fly_envs

B = int(sys.argv[1]) if len(sys.argv) > 1 else 8192
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 300
rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 7
iters = int(sys.argv[4]) if len(sys.argv) > 4 else 100

envs = {cap: fly_envs.flight_imitation(batch_size=B, contact_capacity=cap) for cap in (6, 12)}
spec = envs[6].action_spec()
lo, hi = torch.tensor(spec.minimum, device="cuda"), torch.tensor(spec.maximum, device="cuda")
out = {"envs": B, "steps": steps}
for cap, env in envs.items():
    env.reset()
    g = torch.Generator(device="cuda").manual_seed(1234)
    flagged_steps, most = 0, 0
    episodes, flagged_eps, flagged_in_eps, cap_exits = 0, 0, 0, 0
    for k in range(steps):
        ts = env.step((lo + (hi - lo) * torch.rand(B, len(spec.minimum), device="cuda", generator=g)).contiguous())
        w = env.get_task_state()[0][:, 7]
        flagged_steps += int((((w >> 8) & 255) != 0).sum())
        most = max(most, int(torch.stack([(w >> (16 + 4 * q)) & 15 for q in range(4)]).max()))
        v = env.validity()
        last = ts.step_type == 2
        episodes += int(last.sum())
        flagged_eps += int((last & (v.episode_flagged_steps > 0)).sum())
        flagged_in_eps += int(v.episode_flagged_steps[last].sum())
        cap_exits += int(((v.step_bits & 2) != 0).sum())
    out[f"capacity_{cap}"] = {"env_steps_flagged": flagged_steps, "flagged_fraction": flagged_steps / (B * steps),
                              "envs_flagged_at_the_end": int((((w >> 8) & 255) != 0).sum()), "most_contacts_in_a_substep": most,
                              "finished_episodes": episodes, "episodes_with_a_flagged_step": flagged_eps,
                              "share_of_episodes_flagged": flagged_eps / episodes if episodes else float("nan"),
                              "mean_flagged_steps_in_flagged_episodes": flagged_in_eps / flagged_eps if flagged_eps else float("nan"),
                              "launches_that_left_the_solver_on_its_iteration_cap": cap_exits}
g = torch.Generator(device="cuda").manual_seed(99)
a = (lo + (hi - lo) * torch.rand(B, len(spec.minimum), device="cuda", generator=g)).contiguous()
rate = {6: [], 12: []}
for r in range(rounds):
    for cap, env in envs.items():
        rate[cap].append(B / (env.time_steps(a, iters) * 1e-3))
for cap in rate:
    out[f"capacity_{cap}"]["env_steps_per_s_median"] = statistics.median(rate[cap])
    out[f"capacity_{cap}"]["env_steps_per_s_min_max"] = [min(rate[cap]), max(rate[cap])]
out["ratio_12_over_6"] = out["capacity_12"]["env_steps_per_s_median"] / out["capacity_6"]["env_steps_per_s_median"]
print(json.dumps(out), flush=True)
for env in envs.values():
    env.close()
