"""Records what the joint-limit kernel of the free-root walking fly (`walk_limits_kernel`, `BatchedWalkPhysics(joint_limits=True)`)
returns on a fixed batch of 32 states, so that a change that must not move a single bit of its results (the constraint solve moved
into row_newton.hpp and shared with the tethered kernel) can be pinned against the library that came before it.

    python tools/record_walk_limits_digest.py --out tests/golden/walk_limits_parent_digest.npz --commit <hash of the tree that is run>

Run it in a checkout of the commit whose results are to be kept (its own built library is what records), on an MI355X.
tests/test_gpu_walk_limits_bytes_vs_parent.py replays `run()` below on the current library and compares every entry byte for byte.

The batch (one wavefront is one env, so 32 envs in one batch of 32 reach everything), from tests/walk_limit_sets.py on the machine
that records; the states and the controls are stored in the file, so the replay never depends on the oracle reproducing them:
  rows  0-23  all of set C: 1 ... 32 hinges pushed out of range (the solver's 8-, 16- and 32-row instantiations),
  rows 24-27  pushed(A[:4], [36, 40, 44, 48], PUSH_SEED): the 48-row instantiation,
  rows 28-29  pushed(A[:2], [70, 70], OVER_SEED): more limits than rows - the rest is dropped, bit value 2,
  rows 30-31  clamped A[:2]: no row at all, the branch that skips the constraint block.
Controls: RandomState(CTRL_SEED).uniform(-0.5, 0.5, 59) per env, as tests/test_gpu_walk_limits.py draws them.

Four runs from the same states: FFE_NO_CONTACT | FFE_WALK_JOINT_LIMITS alone ("lim") and with the five force switches of
ONLY_LIMITS ("only": the stopping scale is ~0 and the solver runs to its cap of 20), each for 1 and for 10 substeps.  Kept per run:
qpos, qvel, act, the eight task-state ints and the four validity ints.  The ints (row counts, iteration counts, overflow bits) are
kept whole for all 32 envs, so that the fixture's coverage can be read from it; of the float arrays the first RAW_ROWS envs are kept
whole, so that a difference can be read, and the others as one 16-byte BLAKE2b digest per env row (any differing byte of a row
changes its digest, and the row index says which env)."""
import argparse
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NO_FLUID, NO_DAMPER, NO_SPRING, NO_GRAVITY, NO_ACTUATION, NO_CONTACT, WALK_JOINT_LIMITS = 1, 4, 8, 16, 32, 64, 512
LIM = NO_CONTACT | WALK_JOINT_LIMITS
ONLY_LIMITS = NO_FLUID | NO_GRAVITY | NO_ACTUATION | NO_SPRING | NO_DAMPER
RUNS = {"lim_n1": (LIM, 1), "lim_n10": (LIM, 10), "only_n1": (LIM | ONLY_LIMITS, 1), "only_n10": (LIM | ONLY_LIMITS, 10)}
BIG_COUNTS, OVER_COUNTS = [36, 40, 44, 48], [70, 70]
PUSH_SEED, OVER_SEED, CTRL_SEED = 13, 9, 11
GROUPS = {"C": slice(0, 24), "big": slice(24, 28), "over": slice(28, 30), "clamped": slice(30, 32)}
B = 32
RAW_ROWS = 4
FLOATS, INTS = ("qpos", "qvel", "act"), ("ints", "validity")


def make_inputs():
    """{in_qpos, in_qvel, in_act, in_ctrl} of the 32 envs, built with the oracle (CPU)."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    try:
        import walk_limit_sets as S
    finally:
        sys.path.pop(0)
    _, A, C = S.sets()
    states = list(C) + S.pushed(A[:4], BIG_COUNTS, PUSH_SEED) + S.pushed(A[:2], OVER_COUNTS, OVER_SEED)
    states += [(S.clamp_inside(q), v.copy(), a.copy()) for q, v, a in A[:2]]
    assert len(states) == B
    rs = np.random.RandomState(CTRL_SEED)
    ctrl = np.stack([rs.uniform(-0.5, 0.5, 59).astype(np.float32) for _ in range(B)])
    return {"in_qpos": np.stack([s[0] for s in states]).astype(np.float64), "in_qvel": np.stack([s[1] for s in states]).astype(np.float64),
            "in_act": np.stack([s[2] for s in states]).astype(np.float64), "in_ctrl": ctrl}


def _rows(a):
    a = np.ascontiguousarray(a).reshape(B, -1)
    dig = np.stack([np.frombuffer(hashlib.blake2b(a[i].tobytes(), digest_size=16).digest(), dtype=np.uint8) for i in range(RAW_ROWS, B)])
    return a[:RAW_ROWS].copy(), dig


def run(inputs, name):
    """{entry name: array} of run `name` on the library the package loads."""
    import torch

    from flybody_amd import _capi
    from flybody_amd.batched_env import BatchedWalkPhysics

    flags, nsteps = RUNS[name]
    env = BatchedWalkPhysics(batch_size=B, physics_flags=flags)
    dev = lambda a, dt: torch.tensor(a, dtype=dt, device="cuda")
    env.set_state(dev(inputs["in_qpos"], torch.float64), dev(inputs["in_qvel"], torch.float64))
    env.set_act(dev(inputs["in_act"], torch.float64))
    env.physics_step(dev(inputs["in_ctrl"], torch.float32), nsteps)
    q, v = env.get_state()
    a = env.get_act()
    ints, _ = env.get_task_state()
    info = torch.full((B, 4), -1, dtype=torch.int32, device="cuda")
    assert _capi.lib().ffe_get_validity(env._h, info.data_ptr(), env._stream()) == 0
    torch.cuda.synchronize()
    out = {}
    for k, x in zip(FLOATS, (q, v, a)):
        out[f"{name}_{k}_raw"], out[f"{name}_{k}_digest"] = _rows(x.cpu().numpy())
    out[f"{name}_ints"] = np.ascontiguousarray(ints.cpu().numpy()).reshape(B, -1)
    out[f"{name}_validity"] = np.ascontiguousarray(info.cpu().numpy()).reshape(B, -1)
    env.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--commit", required=True, help="hash of the commit whose library records (kept in the file)")
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    rec = make_inputs()
    for name in RUNS:
        rec.update(run(rec, name))
        print(name, "rows", rec[f"{name}_ints"][:, 4].tolist(), "iterations", rec[f"{name}_ints"][:, 6].tolist(),
              "bits", rec[f"{name}_validity"][:, 0].tolist(), flush=True)
    rec["commit"] = np.array(args.commit)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    np.savez_compressed(args.out, **rec)
    print(f"wrote {args.out}: {len(rec)} entries, {os.path.getsize(args.out)} bytes")


if __name__ == "__main__":
    main()
