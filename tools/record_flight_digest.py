"""Records what flight_imitation returns over a short, fixed rollout, so that a change that must not move a single bit of the flight
step kernel's results (register allocation, addressing, scheduling) can be pinned against the library that came before it.

    python tools/record_flight_digest.py --out tests/golden/flight_parent_digest.npz --commit <hash of the tree that is run>

Run it in a checkout of the commit whose results are to be kept (its own built library is what records), on an MI355X.
tests/test_gpu_flight_bytes_vs_parent.py replays `rollout()` below on the current library and compares every entry byte for byte.

The rollout, per batch size (130, 5) and contact capacity (6, 12): `flight_imitation(random_state=0, env_id_base=0)`, `reset()`, 40
control steps with actions uniform over the whole (canonical) action spec from numpy's `default_rng(ACTION_SEED)`, and one
`reset_envs` of a fixed mask after step 20.  Kept: observation, reward, discount and step_type of steps 10, 20, 21, 30 and 40, the
row that `reset_envs` returned, and `get_state()` after the last step.

To stay a small fixture the B = 130 rollouts keep every per-env row as a 16-byte BLAKE2b digest of its bytes (`<name>` of shape
[B, 16], uint8: any differing byte of a row changes its digest, and the row index says which env); the B = 5 rollouts keep the
arrays themselves, so a difference there can be read."""
import argparse
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

BATCHES = (130, 5)
CAPACITIES = (6, 12)
STEPS = 40
KEEP = (10, 20, 21, 30, 40)
RESET_AFTER = 20
ACTION_SEED = 20240
RAW_MAX_BATCH = 8  # batches up to this size keep whole arrays, larger ones a digest per row


def reset_mask(B):
    """Every third env, and the last one."""
    m = (np.arange(B) % 3 == 1)
    m[B - 1] = True
    return m


def _rows(a, B):
    a = np.ascontiguousarray(a)
    a = a.reshape(B, -1)
    if B <= RAW_MAX_BATCH:
        return a
    return np.stack([np.frombuffer(hashlib.blake2b(a[i].tobytes(), digest_size=16).digest(), dtype=np.uint8) for i in range(B)])


def rollout(B, capacity):
    """{entry name: array} of one rollout on the library the package loads."""
    import torch

    from flybody_amd import fly_envs

    env = fly_envs.flight_imitation(batch_size=B, random_state=0, env_id_base=0, contact_capacity=capacity)
    spec = env.action_spec()
    lo = np.broadcast_to(np.asarray(spec.minimum, np.float32), spec.shape)
    hi = np.broadcast_to(np.asarray(spec.maximum, np.float32), spec.shape)
    rng = np.random.default_rng(ACTION_SEED)
    out = {}

    def keep(tag, ts):
        torch.cuda.synchronize()
        out[f"{tag}_observation"] = _rows(env.flat_observation.cpu().numpy(), B)
        out[f"{tag}_reward"] = _rows(ts.reward.cpu().numpy(), B)
        out[f"{tag}_discount"] = _rows(ts.discount.cpu().numpy(), B)
        out[f"{tag}_step_type"] = _rows(ts.step_type.cpu().numpy(), B)

    env.reset()
    for k in range(1, STEPS + 1):
        u = rng.random((B, spec.shape[0]), dtype=np.float32)
        a = torch.from_numpy((lo + (hi - lo) * u).astype(np.float32)).cuda().contiguous()
        ts = env.step(a)
        if k in KEEP:
            keep(f"step{k}", ts)
        if k == RESET_AFTER:
            keep("reset_envs", env.reset_envs(torch.from_numpy(reset_mask(B)).cuda()))
    qpos, qvel = env.get_state()
    torch.cuda.synchronize()
    out["final_qpos"], out["final_qvel"] = _rows(qpos.cpu().numpy(), B), _rows(qvel.cpu().numpy(), B)
    env.close()
    return out


def record_all():
    rec = {}
    for B in BATCHES:
        for cap in CAPACITIES:
            for k, v in rollout(B, cap).items():
                rec[f"b{B}_c{cap}_{k}"] = v
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--commit", required=True, help="hash of the commit whose library records (kept in the file)")
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    rec = record_all()
    rec["commit"] = np.array(args.commit)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    np.savez_compressed(args.out, **rec)
    print(f"wrote {args.out}: {len(rec)} entries, {os.path.getsize(args.out)} bytes")


if __name__ == "__main__":
    main()
