"""Records what the walk_on_ball kernel returns on a fixed batch of 32 states, so that a change that must not move a single bit of its
results (one sphere / capsule pass and one convex pair pass for the ball and walk kernels, csrc/self_pairs.hpp) can be pinned against
the library that came before it.

    python tools/record_ball_digest.py --out tests/golden/ball_parent_digest.npz --commit <hash of the tree that is run>

Run it in a checkout of the commit whose results are to be kept (its own built library is what records), on an MI355X.
tests/test_gpu_ball_bytes_vs_parent.py replays `run()` below on the current library and compares every entry byte for byte.

The batch (one wavefront is one env) is built once with the float64 oracle on the machine that records; states, controls and actions
are stored in the file, so the replay needs neither the oracle nor the reference:
  rows  0-19  poses in which the fly's own geoms touch (tests/ball_fly_fly_states.py, seed FLY_FLY_SEED): five each of the kinds claw,
              mouth, convex and other, the first of each kind that stay within the tile's 16 contact slots and in which, by the
              oracle, the fly still touches itself at the end of every physics run below,
  rows 20-31  forced overflow: every hinge uniform over its range (tests/test_gpu_ball.py::test_forced_capacity_overflow_stays_finite),
              chosen by the oracle's own contact list at the state, of which the contacts that take a slot are counted (active, or a
              claw's): rows 20-25 have >= OVER ball contacts and sphere / capsule pairs, at most BALL_MOST of them the ball's so that the
              primitive pass finds free slots (`primitive`: its replacement loop), rows 26-31 at most FEW of those but >= OVER with
              the convex pairs (`convex`: the ranking of the convex pass).  OVER - NC = 4 contacts are the margin against a float32 /
              float64 disagreement on borderline pairs.
Controls: RandomState(CTRL_SEED).uniform(-0.5, 0.5, 59) per env; actions of the env run: RandomState(ACTION_SEED) likewise, three rows.

Physics runs on `BatchedBallEnv(batch_size=32)` through `set_state` / `set_act` / `physics_step`, all from the same states: flags 0 for 1
and for 10 substeps (the separating-direction history of the convex pairs carries across substeps), FFE_NO_NOSLIP | FFE_NO_ADHESION
for 1.  Kept per run: qpos, qvel, act, the task-state ints and reals, the validity ints.
Env run: `reset()`, then three `step()` calls with the stored actions.  Kept: obs, reward, discount and step_type of the reset and of
the third step, and after it the state, the task-state ints and reals and validity.

All ints are kept whole for all 32 envs, so that the fixture's coverage can be read from it; of the float arrays the first RAW_ROWS
envs are kept whole, so that a difference can be read, and the others as one 16-byte BLAKE2b digest per env row."""
import argparse
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NO_NOSLIP, NO_ADHESION = 128, 256
# run name: (flags, substeps)
PHYSICS_RUNS = {"all_n1": (0, 1), "all_n10": (0, 10), "no_noslip_no_adhesion_n1": (NO_NOSLIP | NO_ADHESION, 1)}
ENV_RUNS = ("env",)
RUNS = list(PHYSICS_RUNS) + list(ENV_RUNS)
GROUPS = {"fly_fly": slice(0, 20), "primitive": slice(20, 26), "convex": slice(26, 32)}
NC, OVER, FEW = 16, 20, 12  # the tile's contact slots; contacts of an overflow row by the oracle's count; primitive ones of a `convex` row
BALL_MOST = 14              # ball contacts of a `primitive` row: two slots and more are free when the primitive pass begins
FLY_FLY_SEED, POSE_SEED, BASE_SEED, CTRL_SEED, ACTION_SEED = 3, 17, 3, 11, 12
B = 32
POOL = 16  # touching poses of each kind that are tried for its five rows
RAW_ROWS = 4
ENV_STEPS = 3


def make_inputs():
    """{in_qpos, in_qvel, in_act, in_ctrl, in_actions} of the 32 envs, built with the oracle (CPU)."""
    import json

    sys.path.insert(0, os.path.join(ROOT, "tests"))
    try:
        import ball_fly_fly_states as F
    finally:
        sys.path.pop(0)
    from flybody_amd.model.blob import read_blob
    from oracle import oracle as O

    m, _, pool = F.fly_fly_states(4 * POOL, seed=FLY_FLY_SEED)  # POOL of each kind, in the order claw, mouth, convex, other
    t = read_blob(F.BALL_BLOB)
    names = json.load(open(F.BALL_BLOB.replace(".ffmb", ".json")))["geom_name"]
    gtype = np.asarray(t["geom_type"])
    d = O.OracleData(m)
    rs = np.random.RandomState(CTRL_SEED)
    ctrl = np.stack([rs.uniform(-0.5, 0.5, 59).astype(np.float32) for _ in range(B)])

    def counts():
        """(ball contacts, sphere / capsule pairs, convex pairs) among the contacts that take a slot, at the oracle's position stage"""
        ball = prim = cvx = 0
        for r in d.contacts():
            g1, g2 = int(r[0]), int(r[1])
            if int(r[3]) != 0 and "claw" not in names[g1] and "claw" not in names[g2]:
                continue  # inside the margin, outside margin - gap, no adhesion actuator: no slot
            if "ball" in names[g1] or "ball" in names[g2]:
                ball += 1
            elif gtype[g1] < 4 and gtype[g2] < 4:
                prim += 1
            else:
                cvx += 1
        assert ball + prim + cvx == d.ncon_matter
        return ball, prim, cvx

    def at(q, v, a):
        d.qpos[:], d.qvel[:], d.act[:] = q, v, a
        d.ctrl[:] = 0
        d.forward()
        return counts()

    def stays_touching(s, c):
        """The fly still touches itself after every physics run (the kernel reports the contacts of the state it ends on)."""
        for flags, nsteps in PHYSICS_RUNS.values():
            m.set_flags(flags)
            d.qpos[:], d.qvel[:], d.act[:] = s[:3]
            d.ctrl[:] = c.astype(np.float64)
            d.step1()
            for _ in range(nsteps):
                d.step2()
                d.step1()
            ball, prim, cvx = counts()
            m.set_flags(0)
            if prim + cvx == 0 or ball + prim + cvx > NC:
                return False
        return True

    states = []
    for kind in range(4):
        for s in pool[kind * POOL:(kind + 1) * POOL]:
            if len(states) < 5 * (kind + 1) and sum(at(*s[:3])) <= NC and stays_touching(s, ctrl[len(states)]):
                states.append((s[0].copy(), s[1].copy(), s[2].copy()))
        assert len(states) == 5 * (kind + 1), (kind, len(states))
    # the base state of test_forced_capacity_overflow_stays_finite: an oracle rollout's third control step under small random actions
    env = O.OracleBallEnv(m)
    env.reset()
    rs = np.random.RandomState(BASE_SEED)
    for _ in range(3):
        env.step(rs.uniform(-0.2, 0.2, 59))
    base = env.data.qpos.copy(), np.zeros_like(env.data.qvel), env.data.act.copy()
    lo, hi = np.asarray(t["jnt_range"])[:, 0], np.asarray(t["jnt_range"])[:, 1]
    adr = np.asarray(t["jnt_qposadr"])
    hinge = [j for j in range(len(adr)) if int(t["jnt_type"][j]) == 3 and hi[j] > lo[j]]
    rng = np.random.RandomState(POSE_SEED)
    want = {k: GROUPS[k].stop - GROUPS[k].start for k in ("primitive", "convex")}
    found = {"primitive": [], "convex": []}
    for _ in range(60000):
        if all(len(found[k]) == want[k] for k in want):
            break
        q = base[0].copy()
        for j in hinge:
            q[int(adr[j])] = rng.uniform(lo[j], hi[j])
        ball, prim, cvx = at(q, base[1], base[2])
        # (`primitive`: the ball contacts leave slots, or the tile is full before the primitive pass and nothing is replaced)
        kind = "primitive" if ball <= BALL_MOST and ball + prim >= OVER else ("convex" if ball + prim <= FEW and ball + prim + cvx >= OVER else None)
        if kind and len(found[kind]) < want[kind]:
            found[kind].append(((q, base[1].copy(), base[2].copy()), (ball, prim, cvx)))
    assert all(len(found[k]) == want[k] for k in want), {k: len(v) for k, v in found.items()}
    for k in ("primitive", "convex"):
        print(k, "rows: (ball, sphere / capsule, convex) contacts by the oracle", [c for _, c in found[k]])
        states += [s for s, _ in found[k]]
    assert len(states) == B
    rs = np.random.RandomState(ACTION_SEED)
    actions = np.stack([rs.uniform(-0.5, 0.5, (B, 59)).astype(np.float32) for _ in range(ENV_STEPS)])
    return {"in_qpos": np.stack([s[0] for s in states]).astype(np.float64), "in_qvel": np.stack([s[1] for s in states]).astype(np.float64),
            "in_act": np.stack([s[2] for s in states]).astype(np.float64), "in_ctrl": ctrl, "in_actions": actions}


def _rows(a):
    a = np.ascontiguousarray(a).reshape(B, -1)
    dig = np.stack([np.frombuffer(hashlib.blake2b(a[i].tobytes(), digest_size=16).digest(), dtype=np.uint8) for i in range(RAW_ROWS, B)])
    return a[:RAW_ROWS].copy(), dig


def _keep(out, name, floats, ints):
    for k, x in floats.items():
        out[f"{name}_{k}_raw"], out[f"{name}_{k}_digest"] = _rows(x.cpu().numpy())
    for k, x in ints.items():
        out[f"{name}_{k}"] = np.ascontiguousarray(x.cpu().numpy()).reshape(B, -1)


def _report(torch, env):
    """(qpos, qvel, act, task-state ints, task-state reals, validity ints) of a handle"""
    from flybody_amd import _capi

    q, v = env.get_state()
    a = env.get_act()
    ints, reals = env.get_task_state()
    info = torch.full((B, 4), -1, dtype=torch.int32, device="cuda")
    assert _capi.lib().ffe_get_validity(env._h, info.data_ptr(), env._stream()) == 0
    torch.cuda.synchronize()
    return {"qpos": q, "qvel": v, "act": a, "reals": reals}, {"ints": ints, "validity": info}


def _run_physics(torch, inputs, name):
    from flybody_amd.batched_env import BatchedBallEnv

    flags, nsteps = PHYSICS_RUNS[name]
    env = BatchedBallEnv(batch_size=B, physics_flags=flags)
    dev = lambda a, dt: torch.tensor(a, dtype=dt, device="cuda")
    env.reset()
    env.set_state(dev(inputs["in_qpos"], torch.float64), dev(inputs["in_qvel"], torch.float64))
    env.set_act(dev(inputs["in_act"], torch.float64))
    env.physics_step(dev(inputs["in_ctrl"], torch.float32), nsteps)
    out = {}
    _keep(out, name, *_report(torch, env))
    env.close()
    return out


def _run_env(torch, inputs, name):
    from flybody_amd.batched_env import BatchedBallEnv

    env = BatchedBallEnv(batch_size=B)
    out = {}

    def timestep(ts, tag):
        _keep(out, f"{name}_{tag}", {"obs": env.flat_observation, "reward": ts.reward, "discount": ts.discount}, {"step_type": ts.step_type})

    timestep(env.reset(), "reset")
    for k in range(ENV_STEPS):
        ts = env.step(torch.tensor(inputs["in_actions"][k], dtype=torch.float32, device="cuda"))
    timestep(ts, "step")
    _keep(out, name, *_report(torch, env))
    env.close()
    return out


def run(inputs, name):
    """{entry name: array} of run `name` on the library the package loads."""
    import torch

    return (_run_env if name in ENV_RUNS else _run_physics)(torch, inputs, name)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--commit", required=True, help="hash of the commit whose library records (kept in the file)")
    ap.add_argument("--inputs", help="an .npz with the in_* arrays of an earlier `--inputs-only` call, instead of building them")
    ap.add_argument("--inputs-only", action="store_true", help="build the inputs with the oracle, write them to --out and stop (no GPU)")
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    if args.inputs:
        with np.load(args.inputs) as f:
            rec = {k: f[k] for k in f.files if k.startswith("in_")}
    else:
        rec = make_inputs()
    if not args.inputs_only:
        for name in RUNS:
            rec.update(run(rec, name))
            ints = rec[f"{name}_ints"]
            print(name, "contacts", ints[:, 5].tolist(), "fly-fly", ints[:, 3].tolist(), "iterations", ints[:, 6].tolist(),
                  "bits", rec[f"{name}_validity"][:, 0].tolist(), flush=True)
        rec["commit"] = np.array(args.commit)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    np.savez_compressed(args.out, **rec)
    print(f"wrote {args.out}: {len(rec)} entries, {os.path.getsize(args.out)} bytes")


if __name__ == "__main__":
    main()
