"""`order_by_cost` (flybody_amd/csrc/launch_order.hpp: one 1024-thread workgroup, 16 keys per thread in registers, a re-reading
loop above 16 384 envs) at ragged and large batches.  The order must be a permutation of the envs: a skipped env keeps its old
outputs, a doubly visited one is stepped twice, and either shows as soon as every env's outputs are compared with a run that does
not depend on the order.  Everything is `torch.equal`.  Run with `-m gpu -s` on an MI355X."""
import numpy as np
import pytest

from test_gpu_parity import torch_mod  # noqa: F401

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("B", [2, 1023, 1025, 8191, 8192])
def test_flight_sorted_against_index_order(torch_mod, wb_tables, ref_traj, B):
    """Flight sorts its launches for 2 <= B <= 8192; physics_flags = 1 << 24 steps in plain index order.  Same seed, same full-range
    actions: observation, reward, discount, step_type after every step and the task state at the end are equal bit for bit, with
    episodes ending and restarting inside the run and the constraint solver at work."""
    from flybody_amd.batched_env import BatchedFlyEnv

    torch = torch_mod
    steps = 300
    a_env = BatchedFlyEnv(wb_tables, *ref_traj, batch_size=B, seed=11)
    b_env = BatchedFlyEnv(wb_tables, *ref_traj, batch_size=B, seed=11, physics_flags=1 << 24)
    g = torch.Generator(device="cuda").manual_seed(5)
    lo, hi = (torch.tensor(x, device="cuda") for x in a_env.raw_action_bounds())
    ta, tb = a_env.reset(), b_env.reset()
    firsts = torch.zeros(B, dtype=torch.int64, device="cuda")
    for k in range(steps):
        assert torch.equal(a_env.flat_observation, b_env.flat_observation), k
        assert torch.equal(ta.reward, tb.reward) and torch.equal(ta.step_type, tb.step_type) and torch.equal(ta.discount, tb.discount), k
        a = (lo + (hi - lo) * torch.rand(B, 12, device="cuda", generator=g)).contiguous()
        ta, tb = a_env.step(a), b_env.step(a)
        firsts += (ta.step_type == 0)
    assert torch.equal(a_env.flat_observation, b_env.flat_observation)
    ia, ra = a_env.get_task_state()
    ib, rb = b_env.get_task_state()
    assert torch.equal(ia, ib)
    restarted = int((firsts > 0).sum())
    print(f"\nflight B {B}: {steps} steps, {int(firsts.sum())} auto-resets in {restarted} envs, envs with solver passes at the end {int((ia[:, 6] > 0).sum())}")
    assert int(firsts.sum()) >= B and restarted >= 1      # episodes ended and restarted within the run, one per env on average
    assert int((ia[:, 6] > 0).sum()) > 0                  # the constraint solver was exercised
    a_env.close(); b_env.close()


def test_flight_above_the_sorted_range(torch_mod, wb_tables, ref_traj):
    """Above FFE_ORDER_MAX_BATCH = 8192 flight steps in index order and the flag changes nothing, so the check is the one of
    test_shards_reproduce_the_single_handle: one handle of 32 768 envs against four (sorted) handles of 8 192 with env_id_base,
    bit for bit across auto-resets."""
    from flybody_amd.batched_env import BatchedFlyEnv

    torch = torch_mod
    B, H, steps = 32768, 8192, 150
    full = BatchedFlyEnv(wb_tables, *ref_traj, batch_size=B, seed=6)
    parts = [BatchedFlyEnv(wb_tables, *ref_traj, batch_size=H, seed=6, env_id_base=b) for b in range(0, B, H)]
    g = torch.Generator(device="cuda").manual_seed(9)
    lo, hi = (torch.tensor(x, device="cuda") for x in full.raw_action_bounds())
    t_full = full.reset()
    t_parts = [p.reset() for p in parts]
    firsts = torch.zeros(B, dtype=torch.int64, device="cuda")
    for k in range(steps):
        if k:
            a = (lo + (hi - lo) * torch.rand(B, 12, device="cuda", generator=g)).contiguous()
            t_full = full.step(a)
            t_parts = [p.step(a[i * H:(i + 1) * H].contiguous()) for i, p in enumerate(parts)]
            firsts += (t_full.step_type == 0)
        for i, (p, t) in enumerate(zip(parts, t_parts)):
            sl = slice(i * H, (i + 1) * H)
            assert torch.equal(p.flat_observation, full.flat_observation[sl]), (k, i)
            assert torch.equal(t.reward, t_full.reward[sl]) and torch.equal(t.discount, t_full.discount[sl]), (k, i)
            assert torch.equal(t.step_type, t_full.step_type[sl]), (k, i)
    n_first, restarted = int(firsts.sum()), int((firsts > 0).sum())
    print(f"\nflight B {B} against 4 x {H}: {steps} steps, {n_first} auto-resets in {restarted} envs")
    # under full-range actions the wings end an episode within about 130 steps: most envs restart within 150
    assert restarted > B // 2
    for e in (full, *parts):
        e.close()


K_CLASSES = 7


@pytest.mark.parametrize("B", [2, 1025, 16384, 16385, 20001])
def test_walk_on_ball_every_env_follows_its_action_stream(torch_mod, B):
    """walk_on_ball sorts at every batch above 1 and has neither an index-order switch nor per-env randomness: an env's outputs
    depend on its action stream alone.  Seven streams of different amplitude (+-0.2 .. +-1.0 canonical, so that contacts, hence
    cost keys, differ between the classes); env i of the batch gets the stream of class perm[i] % 7 for a fixed scrambling perm.
    After every step every env equals its class's row in a handle of 7 envs fed the 7 streams, bit for bit - a skipped or doubly
    visited env would not."""
    from flybody_amd.batched_env import BatchedBallEnv

    torch = torch_mod
    K, steps = K_CLASSES, 30
    env = BatchedBallEnv(batch_size=B, canonical_actions=True, clip_actions=True)
    ref = BatchedBallEnv(batch_size=K, canonical_actions=True, clip_actions=True)
    A = env.spec.action_dim
    perm = np.random.RandomState(B).permutation(B)
    cls_h = perm % K if B >= K else perm * (K - 1) // (B - 1)          # (two envs: the weakest and the strongest stream)
    cls = torch.tensor(cls_h, device="cuda")
    assert len(set(cls_h.tolist())) == min(B, K)
    amp = torch.linspace(0.2, 1.0, K, device="cuda")[:, None]
    g = torch.Generator(device="cuda").manual_seed(3)
    te, tr = env.reset(), ref.reset()
    contacts_differ, key_spread, flagged = 0, 0, 0
    for k in range(steps + 1):
        assert torch.equal(env.flat_observation, ref.flat_observation[cls]), k
        assert torch.equal(te.reward, tr.reward[cls]) and torch.equal(te.discount, tr.discount[cls]) and torch.equal(te.step_type, tr.step_type[cls]), k
        if k == steps:
            break
        a_k = (amp * (torch.rand(K, A, device="cuda", generator=g) * 2 - 1)).contiguous()
        te, tr = env.step(a_k[cls].contiguous()), ref.step(a_k)
        ncon = ref.get_task_state()[0][:, 5]
        big = env.get_task_state()[0][:, 5]
        assert torch.equal(big, ncon[cls]), k                          # the contact count an env ends its step with
        classes_here = ncon[torch.unique(cls)]
        contacts_differ += int(classes_here.min() != classes_here.max())
        key_spread = max(key_spread, int(classes_here.max() - classes_here.min()))
        flagged += int((env.validity().step_bits != 0).sum())
    print(f"\nwalk_on_ball B {B}: {steps} steps, the classes' contact counts differed after {contacts_differ} of them (largest spread {key_spread}); "
          f"env-steps with step_bits != 0: {flagged}")
    assert contacts_differ > 0          # otherwise every cost key ties and the sort is trivial
    env.close(); ref.close()
