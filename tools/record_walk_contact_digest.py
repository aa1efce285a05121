"""Records what the contact kernels of the free-root walking fly return on a fixed batch of 32 states, so that a change that must not
move a single bit of their results (one constraint block `contact_forces` and one sensor pass for the floor and for the fly's own
contacts, csrc/walk_substeps.hpp) can be pinned against the library that came before it.

    python tools/record_walk_contact_digest.py --out tests/golden/walk_contact_parent_digest.npz --commit <hash of the tree that is run>

Run it in a checkout of the commit whose results are to be kept (its own built library is what records), on an MI355X.
tests/test_gpu_walk_contact_bytes_vs_parent.py replays `run()` below on the current library and compares every entry byte for byte.

The batch (one wavefront is one env), built once with the helpers of tests/walk_self_sets.py, tests/walk_floor_sets.py and
tests/walk_limit_sets.py on the machine that records; states, controls and actions are stored in the file, so the replay needs neither
the oracle nor the reference:
  rows  0-1   FAR: two crafted poses of XL, the root 1 cm above the reset pose: higher than any geom reaches, the far branch of `floor_step`,
  rows  2-5   HOVER: standing states with the root 0.03 / 0.05 / 0.08 / 0.12 cm above its height in the reset pose of clip 0 (0.13 cm), 6
              hinges pushed out of range: within reach of the floor (the reach bound is 0.32 cm) but, the higher ones, without a floor
              contact - the cone solver with limit rows and no cone block,
  rows  6-7   two more poses of XL (far on the floor handle; on the self handle the fly-fly rows alone),
  rows  8-11  four crafted standing poses of XS: floor and fly-fly contacts mixed,
  rows 12-31  states standing on the floor, from R10, XS and F10 in turn, every limited hinge clamped inside its range and then 0, 6, 12, 20
              and 30 hinges pushed out of it (four states each, `pushed`).  Of the pool only states that the oracle sees touching
              themselves, with at most MAX_CONTACTS contacts, are taken: every env has a fly-fly row on the self handle.  A pushed hinge adds exactly one row, so with three
              rows per floor contact the row count reaches every instantiation of the solver: <= 12, <= 18, <= 24, <= 32 and RMAX.
Controls: RandomState(CTRL_SEED).uniform(-0.5, 0.5, 59) per env; actions of the env runs: RandomState(ACTION_SEED) likewise, three rows.

Physics runs, all from the same states, on the floor handle (`BatchedWalkPhysics(floor_contacts=True)`) and on the self handle
(`self_contacts=True` on top): default flags for 1 and for 10 substeps, FFE_NO_NOSLIP and FFE_NO_FLUID | FFE_NO_ADHESION for 1 substep.
Kept per run: qpos, qvel, act, the task-state ints and reals, the validity ints.
Env runs, on `BatchedWalkEnv(floor_contacts=True)` without and with `self_contacts=True` (three synthetic clips, as
tests/test_gpu_walk_self_env.py builds them): a reset (env i on clip i % 3), then three steps with the stored actions.  Kept: obs,
reward, discount and step_type of the reset and of the third step, and after it the state, the task-state ints and reals and validity.

All ints are kept whole for all 32 envs, so that the fixture's coverage can be read from it; of the float arrays the first RAW_ROWS
envs are kept whole, so that a difference can be read, and the others as one 16-byte BLAKE2b digest per env row."""
import argparse
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NO_FLUID, NO_NOSLIP, NO_ADHESION = 1, 128, 256
FLAG_SETS = {"all": 0, "no_noslip": NO_NOSLIP, "no_fluid_no_adhesion": NO_FLUID | NO_ADHESION}
# run name: (fly's own contacts, extra flags, substeps)
PHYSICS_RUNS = {f"{h}_{fs}_n{n}": (h == "self", FLAG_SETS[fs], n)
                for h in ("floor", "self") for fs, n in (("all", 1), ("all", 10), ("no_noslip", 1), ("no_fluid_no_adhesion", 1))}
ENV_RUNS = {"env_floor": False, "env_self": True}
RUNS = list(PHYSICS_RUNS) + list(ENV_RUNS)
HOVER_LIFTS, HOVER_PUSHED = [0.03, 0.05, 0.08, 0.12], 6
MAX_CONTACTS = 12  # of a pushed state, by the oracle's count: the device keeps up to 16
PUSH_COUNTS = [0] * 4 + [6] * 4 + [12] * 4 + [20] * 4 + [30] * 4
PUSH_SEED, HOVER_SEED, CTRL_SEED, ACTION_SEED = 13, 17, 11, 12
GROUPS = {"far": slice(0, 2), "hover": slice(2, 6), "lifted": slice(6, 8), "standing": slice(8, 12), "pushed": slice(12, 32)}
ROW_CLASSES = ((1, 12), (13, 18), (19, 24), (25, 32), (33, 48))  # the row counts each instantiation of the solver takes
B = 32
RAW_ROWS = 4
ENV_STEPS = 3


def make_inputs():
    """{in_qpos, in_qvel, in_act, in_ctrl, in_actions} of the 32 envs, built with the oracle (CPU)."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    try:
        import walk_floor_sets as F
        import walk_limit_sets as L
        import walk_self_sets as S
    finally:
        sys.path.pop(0)
    from oracle import oracle as O

    R10, XL, XS, F10 = S.r10(), S.x_lifted(), S.x_standing(), F.sets()[2]
    three = lambda s: (s[0].copy(), s[1].copy(), s[2].copy())
    m, d = S.model(), O.OracleData(S.model())

    def contacts(state):
        """(contacts that take a slot, the fly-fly ones among them) of the oracle's collision pass at `state`"""
        d.qpos[:], d.qvel[:], d.act[:] = state
        d.ctrl[:] = 0
        d.forward()
        return d.ncon_matter, S._matter_self(m, d)

    # a pushed state is taken when the fly touches itself somewhere (clamping the hinges inside their ranges opens the mouth parts'
    # standing contacts, so not every state does) and its contacts leave slots free: the next state of the pool is tried otherwise
    pool, cursor = [three(s) for trio in zip(R10[:12], XS, F10[:12]) for s in trio], 0

    stand = F.reset_pose()[2]  # the root's height in the reset pose of clip 0

    def push(n, seed, lift=None):
        nonlocal cursor
        while True:
            q, v, a = three(pool[cursor % len(pool)])
            cursor += 1
            assert cursor < 4 * len(pool)
            if lift is not None:
                q[2] = stand + lift
            st = L.pushed([(q, v, a)], [n], seed + cursor)[0]
            ncon, nself = contacts(st)
            if nself >= 1 and ncon <= MAX_CONTACTS:
                return st

    states = [three(XL[0]), three(XL[3])] + [push(HOVER_PUSHED, HOVER_SEED, lift) for lift in HOVER_LIFTS] + [three(XL[6]), three(XL[9])]
    states += [three(XS[k]) for k in (0, 3, 6, 9)] + [push(n, PUSH_SEED) for n in PUSH_COUNTS]
    assert len(states) == B
    rs = np.random.RandomState(CTRL_SEED)
    ctrl = np.stack([rs.uniform(-0.5, 0.5, 59).astype(np.float32) for _ in range(B)])
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
    from flybody_amd.batched_env import BatchedWalkPhysics

    self_contacts, flags, nsteps = PHYSICS_RUNS[name]
    env = BatchedWalkPhysics(batch_size=B, physics_flags=flags, floor_contacts=True, self_contacts=self_contacts)
    dev = lambda a, dt: torch.tensor(a, dtype=dt, device="cuda")
    env.set_state(dev(inputs["in_qpos"], torch.float64), dev(inputs["in_qvel"], torch.float64))
    env.set_act(dev(inputs["in_act"], torch.float64))
    env.physics_step(dev(inputs["in_ctrl"], torch.float32), nsteps)
    out = {}
    _keep(out, name, *_report(torch, env))
    env.close()
    return out


def _run_env(torch, inputs, name):
    from flybody_amd.batched_env import BatchedWalkEnv
    from flybody_amd.tasks import walking as W

    view = W.WalkModelView()
    refs = W.WalkRefSet(W.synthetic_snippets(view, n=3, length=100))
    env = BatchedWalkEnv(refs, view, batch_size=B, floor_contacts=True, self_contacts=ENV_RUNS[name])
    out = {}

    def timestep(ts, tag):
        _keep(out, f"{name}_{tag}", {"obs": env.flat_observation, "reward": ts.reward, "discount": ts.discount}, {"step_type": ts.step_type})

    env.set_next_trajectory_index(np.arange(B) % 3)
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


def row_counts(rec, name):
    """Rows of the last substep's constraint block per env of a physics run: three per floor contact, one per fly-fly contact and limit."""
    ints = rec[f"{name}_ints"]
    return 3 * (ints[:, 5] - ints[:, 3]) + ints[:, 3] + ints[:, 4]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--commit", required=True, help="hash of the commit whose library records (kept in the file)")
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    rec = make_inputs()
    for name in RUNS:
        rec.update(run(rec, name))
        ints = rec[f"{name}_ints"]
        print(name, "contacts", ints[:, 5].tolist(), "fly-fly", (rec[f"{name}_reals_raw"][:, 2] if name in ENV_RUNS else ints[:, 3]).tolist(),
              "limit rows", ints[:, 4].tolist(), "iterations", ints[:, 6].tolist(), "bits", rec[f"{name}_validity"][:, 0].tolist(), flush=True)
    rec["commit"] = np.array(args.commit)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    np.savez_compressed(args.out, **rec)
    print(f"wrote {args.out}: {len(rec)} entries, {os.path.getsize(args.out)} bytes")


if __name__ == "__main__":
    main()
