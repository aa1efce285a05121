"""Environment factories with the reference's names and keyword meaning (`vnl_ray/fly_envs.py`), returning
batched MI355X environments instead of single-instance `composer.Environment`s.

Built so far: `flight_imitation` (`fly_envs.py:29-72`), `walk_on_ball` (`fly_envs.py:125-157`) and `walk_imitation` without its
floor (`floor_contacts=False`), on the floor plane (`floor_contacts="primitives"`) and there with the fly's own contacts
(`self_contacts=True`) and with the plane against the fly's ellipsoids and cylinders (`floor_convex=True`); the default call still
raises (see `walk_imitation`).  `vision_guided_flight` and `template_task` are
later rows of SURVEY.md section 8 and raise `NotImplementedError`.
"""

from __future__ import annotations

import numpy as np

from .batched_env import BatchedBallEnv, BatchedFlyEnv
from .tasks import synthetic, trajectories, wbpg


def flight_imitation(wpg_pattern_path: str | None = None, ref_path: str | None = None, random_state=None,
                     terminal_com_dist: float = 2.0, *, batch_size: int = 1, device: int = 0, env_id_base: int = 0,
                     **env_kwargs) -> BatchedFlyEnv:
    """Requires a fruitfly to track a flying reference (`fly_envs.py:29-72`).

    Args:
        wpg_pattern_path: `.npy` with one wing-beat cycle, shape (timesteps, 3) [yaw, roll, pitch], as the
            reference's WingBeatPatternGenerator expects.  None = the build's synthetic cycle.
        ref_path: `.npz` written by `tools/convert_hdf5_to_npz.py` from the reference's HDF5 layout
            (`tasks/trajectory_loaders.py:90-96`; h5py is unavailable here): `com_qpos (rows,7)`, `com_qvel (rows,6)`,
            `traj_off (N+1,)`, `timestep_seconds` - every trajectory keeps its own length, as in the reference.
            None = synthetic trajectories.
        random_state: int seed or `np.random.RandomState`; seeds the per-env counter-based generators that draw the
            trajectory index and the initial wing-beat phase of every episode.
        terminal_com_dist: episode terminates when the model-to-ghost CoM distance exceeds this (cm).
        batch_size, device, env_id_base: batching (env `i` of this handle is global env `env_id_base + i`).
    """
    if wpg_pattern_path is None:
        tables = wbpg.build_tables(synthetic.base_wing_pattern())
    else:
        tables = wbpg.load_tables(wpg_pattern_path)
    if ref_path is None:
        refs = trajectories.as_refset(*trajectories.preprocess(*synthetic.flight_trajectories()))
    else:
        com_qpos, com_qvel, dt = trajectories.load_npz(ref_path)
        if abs(dt - tables.dt_ctrl) > 1e-12:
            raise ValueError(f"trajectory timestep {dt} != control timestep {tables.dt_ctrl}")
        refs = trajectories.preprocess_ragged(com_qpos, com_qvel)
    if isinstance(random_state, np.random.RandomState):
        seed = int(random_state.randint(0, 2**31 - 1))
    else:
        seed = 0 if random_state is None else int(random_state)
    # fly_envs.py:54-65: time_limit 0.6 s, joint_filter 0 (compiled into the model), future_steps 5, initialize_qvel
    return BatchedFlyEnv(tables, refs, batch_size=batch_size, device=device, seed=seed, env_id_base=env_id_base,
                         future_steps=5, time_limit=0.6, terminal_com_dist=terminal_com_dist, **env_kwargs)


def walk_on_ball(random_state=None, *, batch_size: int = 1, device: int = 0, **env_kwargs) -> BatchedBallEnv:
    """Requires a tethered fruitfly to walk on a floating ball (`fly_envs.py:125-157`).

    The arena (ball at (-0.05, 0, -0.419), radius 0.454, density 0.0025), `joint_filter=0.01`, `adhesion_filter=0.007`
    and the claw friction are compiled into `assets/fly_ball.ffmb`; `time_limit` is 2.0 s.  Episodes carry no randomness
    (`walk_on_ball.py:48-54`), so `random_state` is accepted for signature parity and ignored."""
    del random_state
    return BatchedBallEnv(batch_size=batch_size, device=device, time_limit=2.0, **env_kwargs)


def walk_imitation(ref_path=None, random_state=None, terminal_com_dist: float = 0.3, *, floor_contacts=True, self_contacts: bool = False,
                   floor_convex: bool = False, batch_size: int = 1, device: int = 0, **env_kwargs):
    """Requires a fruitfly to track a reference walking fly (`fly_envs.py:75-122`).

    Built: the compiled model (`assets/fly_walk.ffmb`: free root, floor plane, Walking
    configuration), the snippet layout and walker features (`tasks/walking.py`), the DeepMimic reward maths (`tasks/rewards.py`), the
    task layer on the device (`tasks/walk_tracker.py`: features, reward, termination, observation columns), the free-root smooth
    dynamics with the joint limits of the 102 hinges (`batched_env.BatchedWalkPhysics`), and around them the sensors and the episode
    protocol of the step kernel (`batched_env.BatchedWalkEnv`), with the floor plane under the fly's 48 sphere / capsule geoms and the
    force and touch sensors on it and, opt-in, the fly's own contacts (leg against leg, leg against body) and the plane against the
    fly's 16 ellipsoid and 6 cylinder geoms (section 12 step 4e); the float64 CPU restatement of the whole task that the tests check
    against is test infrastructure, outside this package.  With both opt-ins the environment carries all floor contacts and all
    fly-fly contacts of the reference's task (`tasks/base.py:331-364`).

    The default call (`floor_contacts=True`, the reference's task with every contact) still raises `NotImplementedError`, for two
    reasons.  Switching it is a change of behaviour that existing tests pin, so it belongs to a follow-up that edits those tests.  And
    a handle keeps NC = 16 contacts per substep: 40 % of the placed fallen poses measured for step 3d exceed 16, so the capacity is the
    open question for a default that is faithful to the reference.  This package has no CPU path and the factory fails instead of
    returning a slow or a different environment.  The explicit opt-ins to what exists: `floor_contacts="primitives"` returns a
    `BatchedWalkEnv` that stands and walks on the floor (plane against spheres and capsules; the fly's own contacts off unless
    `self_contacts=True` switches them on, the plane against ellipsoids and cylinders off unless `floor_convex=True` does, which needs
    `self_contacts=True`), and `floor_contacts=False` one whose fly falls freely under gravity (or floats with
    `physics_flags=FFE_NO_GRAVITY`), with force and touch reading zero.

    Args:
        ref_path: `.npz` written by `tasks.walking.save_npz` (clips of individual lengths with their tracked features).  None = the
            build's synthetic snippets.
        random_state: int seed or `np.random.RandomState`; seeds the per-env counter-based generator that draws every episode's clip.
        terminal_com_dist: an episode terminates when the root is further than this from the reference root (cm).
        floor_contacts: True (the default) raises; "primitives" returns the environment on the floor plane (sphere / capsule geoms only);
            False returns the environment without the floor.
        self_contacts: with `floor_contacts="primitives"`, True adds the fly's own contacts (`BatchedWalkEnv(self_contacts=True)`).
        floor_convex: with `floor_contacts="primitives", self_contacts=True`, True adds the plane against the fly's ellipsoids and
            cylinders (`BatchedWalkEnv(floor_convex=True)`); `ValueError` with anything else.
        batch_size, device: batching.  `env_kwargs` go to `BatchedWalkEnv` (`inference_mode`, `env_id_base`, `pad_first_obs`,
            `physics_flags`, `canonical_actions`, `clip_actions`, `double_buffer`)."""
    if isinstance(floor_contacts, str) and floor_contacts != "primitives":
        raise ValueError(f"walk_imitation: floor_contacts must be True, False or \"primitives\", not {floor_contacts!r}")
    if floor_convex and not (floor_contacts == "primitives" and self_contacts):
        raise ValueError("walk_imitation: floor_convex=True is accepted only with floor_contacts=\"primitives\", self_contacts=True")
    if floor_contacts and floor_contacts != "primitives":
        raise NotImplementedError("walk_imitation: the default call is not switched to the full contact set yet.  Every part exists as an "
                                  "explicit opt-in (DESIGN.md section 12): the floor contacts of the HIP step kernel for the floor plane "
                                  "against the fly's sphere and capsule geoms (floor_contacts=\"primitives\"), the fly's own contacts "
                                  "(self_contacts=True) and the plane against its ellipsoid and cylinder geoms (floor_convex=True, with the "
                                  "other two), around the model, the device task layer (WalkTracker), the free-root smooth dynamics with "
                                  "their joint limits (BatchedWalkPhysics), the sensors and the episode protocol (BatchedWalkEnv).  The "
                                  "default stays refused for two reasons: switching it changes behaviour that existing tests pin and "
                                  "belongs to a follow-up that edits them, and a handle keeps NC = 16 contacts per substep while 40 % of the "
                                  "placed fallen poses exceed 16, so the capacity is open for a faithful default.  "
                                  "walk_imitation(floor_contacts=\"primitives\", self_contacts=True, floor_convex=True) returns the "
                                  "environment with every contact kind, walk_imitation(floor_contacts=False) the one without a floor")
    from .batched_env import BatchedWalkEnv
    from .tasks import walking

    view = walking.WalkModelView()
    if ref_path is None:
        refs = walking.WalkRefSet(walking.synthetic_snippets(view))
    else:
        refs, joint_names, site_names, dt = walking.load_npz(ref_path)
        if abs(dt - 2e-3) > 1e-12:
            raise ValueError(f"trajectory timestep {dt} != control timestep 0.002")
        if list(joint_names) != list(view.meta["mocap_joints"]) or list(site_names) != list(view.meta["mocap_sites"]):
            raise ValueError("the file's tracked joints / sites are not the model's (assets/fly_walk.json: mocap_joints, mocap_sites)")
    if isinstance(random_state, np.random.RandomState):
        seed = int(random_state.randint(0, 2**31 - 1))
    else:
        seed = 0 if random_state is None else int(random_state)
    # fly_envs.py:100-118: time_limit 10 s, future_steps 64, joint_filter / adhesion_filter compiled into the model
    return BatchedWalkEnv(refs, view, batch_size=batch_size, device=device, seed=seed, future_steps=64, time_limit=10.0,
                          terminal_com_dist=terminal_com_dist, floor_contacts=floor_contacts == "primitives", self_contacts=bool(self_contacts),
                          floor_convex=bool(floor_convex), **env_kwargs)


def vision_guided_flight(*args, **kwargs):
    raise NotImplementedError("vision-guided flight needs rendering + heightfield collision; out of scope (SURVEY.md 8f)")


def template_task(*args, **kwargs):
    raise NotImplementedError("template_task is a reference test scaffold; out of scope (SURVEY.md section 2 row 12)")
