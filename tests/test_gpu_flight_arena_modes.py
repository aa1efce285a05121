"""The two paths of the flight step kernel that the byte-identity rollouts (test_gpu_flight_bytes_vs_parent.py) do not run, on a
handle from the shipped blob whose tables the kernel reads at fixed arena offsets: bare physics (`ffe_physics_step`, mode 2) and a
step with FFE_NO_CONTACT.  B = 5, both contact capacities; the results are finite and the same, byte for byte, on two handles made
one after the other in the same process (each handle uploads an arena of its own).  Run with `-m gpu` on an MI355X."""
import numpy as np
import pytest

from test_gpu_parity import torch_mod  # noqa: F401

pytestmark = pytest.mark.gpu

B = 5


def _run(torch, capacity):
    from flybody_amd import fly_envs
    from flybody_amd.batched_env import FFE_NO_CONTACT

    out = {}
    env = fly_envs.flight_imitation(batch_size=B, random_state=0, env_id_base=0, contact_capacity=capacity)
    env.reset()
    rng = np.random.default_rng(7)
    for k in range(3):  # three calls of bare physics: controls taken verbatim, 1, 2 and 5 substeps
        ctrl = torch.from_numpy(rng.uniform(-0.3, 0.3, (B, env.spec.nu)).astype(np.float32)).cuda().contiguous()
        env.physics_step(ctrl, (1, 2, 5)[k])
        qpos, qvel = env.get_state()
        torch.cuda.synchronize()
        out[f"phys{k}_qpos"], out[f"phys{k}_qvel"] = qpos.cpu().numpy().copy(), qvel.cpu().numpy().copy()
    env.close()
    env = fly_envs.flight_imitation(batch_size=B, random_state=0, env_id_base=0, contact_capacity=capacity, physics_flags=FFE_NO_CONTACT)
    env.reset()
    spec = env.action_spec()
    lo, hi = np.broadcast_to(np.asarray(spec.minimum, np.float32), spec.shape), np.broadcast_to(np.asarray(spec.maximum, np.float32), spec.shape)
    a = torch.from_numpy((lo + (hi - lo) * rng.random((B, spec.shape[0]), dtype=np.float32)).astype(np.float32)).cuda().contiguous()
    ts = env.step(a)
    torch.cuda.synchronize()
    out["nc_observation"] = env.flat_observation.cpu().numpy().copy()
    out["nc_reward"], out["nc_step_type"] = ts.reward.cpu().numpy().copy(), ts.step_type.cpu().numpy().copy()
    qpos, qvel = env.get_state()
    out["nc_qpos"], out["nc_qvel"] = qpos.cpu().numpy().copy(), qvel.cpu().numpy().copy()
    # no collision pass ran: the position stage holds no contact
    out["nc_contacts"] = (env.get_task_state()[0].cpu().numpy()[:, 7] & 0xff).copy()
    env.close()
    return out


@pytest.mark.parametrize("capacity", [6, 12])
def test_bare_physics_and_no_contact_step(torch_mod, capacity):
    first, second = _run(torch_mod, capacity), _run(torch_mod, capacity)
    assert (first["nc_contacts"] == 0).all(), first["nc_contacts"]
    for k, v in first.items():
        assert np.isfinite(v.astype(np.float64)).all(), k
        assert v.tobytes() == second[k].tobytes(), k
    # the physics moved: bare physics with non-zero controls changes the joint velocities from call to call
    assert not np.array_equal(first["phys0_qvel"], first["phys2_qvel"])
    assert (first["nc_step_type"] != 0).all(), first["nc_step_type"]  # not FIRST rows: the step ran a control step of the episode
