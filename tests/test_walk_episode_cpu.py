"""CPU-side checks of the walk_imitation environment with the floor off (csrc/walk_env.hip `imitation_step_kernel`, DESIGN.md section 12
step 4b): the opt-in bit and the factory's keyword exist, the default factory call still raises, the third step kernel sits inside the
resource targets while the two bare-physics kernels keep their figures, and the closed-form thorax IMU (csrc/walk_imu.hpp) agrees with
the float64 oracle's sensors.  The IMU runs in a stand-alone program under AddressSanitizer and UBSan (tests/walk_imu_host.cpp)."""
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

BLOB = os.path.join(ROOT, "flybody_amd", "assets", "fly_walk.ffmb")
FO_NO_CONTACT = 64

# Worst float32 errors of the closed forms the host program measured on the 30 states below, relative to max(1, max |reference|) of the
# group (gyro 6.3 rad/s, velocimeter 19 cm/s, accelerometer 114 cm/s^2: the fly falls freely, so the accelerometer reads the root's
# motion about the centre of mass alone): gyro 3.6e-8, velocimeter 9.4e-8, accelerometer 2.7e-7.  Asserted at 3x, never above 1e-5.  In
# float64 the same program gives at most 3.5e-16 (bound 1e-12).
IMU_F32_MEASURED = {"gyro": 3.6e-8, "velocimeter": 9.4e-8, "accelerometer": 2.7e-7}
# `build.kernel_resource_usage` of the two bare-physics kernels at the parent commit: (VGPRs, ScratchSize, LDS Size, Occupancy)
PARENT_FIGURES = {"walk_limits_kernel": (256, 112, 18800, 2), "walk_step_kernel": (168, 0, 18240, 2)}


def test_header_bit_and_factory_keyword():
    from flybody_amd import batched_env, fly_envs

    hdr = open(os.path.join(ROOT, "include", "flybody_env.h")).read()
    assert re.search(r"\bFFE_WALK_EPISODES\s*=\s*1024\b", hdr)
    assert batched_env.FFE_WALK_EPISODES == 1024
    for field in ("const ffe_walk_task *task", "env_id_base", "time_limit_steps", "pad_first_obs", "canonical_actions", "clip_actions"):
        assert field in hdr.split("} ffe_walk_physics_task;")[0].rsplit("typedef struct", 1)[1], field
    sig = inspect.signature(fly_envs.walk_imitation)
    assert list(sig.parameters)[:3] == ["ref_path", "random_state", "terminal_com_dist"]
    assert sig.parameters["floor_contacts"].default is True and sig.parameters["floor_contacts"].kind is inspect.Parameter.KEYWORD_ONLY
    assert sig.parameters["batch_size"].default == 1 and sig.parameters["device"].default == 0
    assert issubclass(batched_env.BatchedWalkEnv, batched_env.BatchedFlyEnv) and batched_env.BatchedWalkEnv.task_kind == "walk_imitation"


def test_default_factory_call_still_raises():
    from flybody_amd import fly_envs

    for kw in ({}, {"floor_contacts": True}, {"floor_contacts": True, "batch_size": 4}):
        with pytest.raises(NotImplementedError, match="floor contacts"):
            fly_envs.walk_imitation(**kw)


@pytest.fixture(scope="module")
def walk_kernels():
    from flybody_amd import build

    return build.kernel_resource_usage("walk_env.hip", "_kernel")


def test_episode_kernel_inside_the_resource_targets(walk_kernels):
    """The third kernel with an LDS tile; its name carries no `walk_`, so the counts the two older test files pin stay as they are."""
    tiles = {k: u for k, u in walk_kernels.items() if u["LDS Size"] > 0}
    assert len(tiles) == 3, sorted(tiles)
    (name, u), = [(k, u) for k, u in tiles.items() if "imitation_step_kernel" in k]
    print(name, u)
    assert "walk_" not in name
    assert u["LDS Size"] <= 20480 and u["Occupancy"] == 2 and u["VGPRs Spill"] == 0


def test_bare_physics_kernels_keep_the_parents_figures(walk_kernels):
    for key, want in PARENT_FIGURES.items():
        (name, u), = [(k, u) for k, u in walk_kernels.items() if key in k]
        print(name, u)
        assert (u["VGPRs"], u["ScratchSize"], u["LDS Size"], u["Occupancy"]) == want, name


@pytest.fixture(scope="module")
def imu_report(tmp_path_factory):
    """tests/walk_imu_host.cpp built with -fsanitize=address,undefined and run on its own (never loaded into Python) on 30 root states of
    a contacts-off oracle rollout at +-1.0 actions."""
    from oracle import oracle as O
    from flybody_amd.model.blob import read_blob
    from flybody_amd.tasks import walking as W

    tmp = tmp_path_factory.mktemp("walk_imu")
    exe, states = str(tmp / "walk_imu_host"), str(tmp / "states.bin")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(ROOT, "tests", "walk_imu_host.cpp")])
    t = read_blob(BLOB)
    site = np.asarray(t["site"], dtype=np.float64).ravel()
    view = W.WalkModelView()
    refs = W.WalkRefSet(W.synthetic_snippets(view, n=3, length=100))
    m = O.OracleModel(BLOB)
    m.set_flags(FO_NO_CONTACT)
    env = O.OracleWalkEnv(m, refs, view.mocap_jnt, view.mocap_site, (view.retract_qadr, view.retract_val), terminal_com_dist=np.inf)
    d = O.OracleData(m)
    rng = np.random.RandomState(7)
    rows = []
    for clip in range(3):
        env.force_next(clip)
        env.reset()
        for _ in range(10):
            act = rng.choice([-1.0, 1.0], env.naction)
            env.step(act)
            # the same state through mj_forward, so that every sensor and qacc belong to one state
            d.qpos[:], d.qvel[:], d.act[:], d.ctrl[:] = env.data.qpos, env.data.qvel, env.data.act, env.data.ctrl
            d.forward()
            rows.append(np.concatenate([d.qpos[3:7], d.qvel[:6], d.qacc[:6], d.sensors]))
    assert len(rows) == 30
    head = np.concatenate([[float(len(rows))], site[1:4], site[4:8], [float(t["opt"][5])]])
    np.concatenate([head] + rows).astype(np.float64).tofile(states)
    r = subprocess.run([exe, states], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr  # a sanitizer report ends the program with a non-zero status
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr
    print(r.stdout)
    return {k: float(v) for k, v in (line.split(None, 1) for line in r.stdout.splitlines())}


def test_imu_closed_forms_equal_the_oracles_sensors_in_float64(imu_report):
    assert imu_report["states"] == 30
    for g in ("gyro", "velocimeter", "accelerometer"):
        assert imu_report["scale_" + g] > 1.0, g  # the states move: no group is compared at zero
        assert imu_report["f64_" + g] <= 1e-12, (g, imu_report["f64_" + g])


def test_imu_closed_forms_in_float32(imu_report):
    for g, measured in IMU_F32_MEASURED.items():
        print(f"{g}: float32 relative error {imu_report['f32_' + g]:.3e} (measured {measured:.1e})")
        assert 3 * measured <= 1e-5
        assert imu_report["f32_" + g] <= 3 * measured, g
