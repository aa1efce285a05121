/*
 * flybody_env.h - C ABI of the MI355X-native batched fruit-fly environment.
 *
 * The reference has no FFI on this path: its boundary is the Python dm_env.Environment protocol
 * (SURVEY.md section 8b).  Each entry point below therefore names the reference *Python* interface
 * it stands in for; the ctypes binding a maintainer adds on the reference side is shown in
 * INTEGRATION.md, and flybody_amd/batched_env.py is that binding in this repo.
 *
 * Conventions
 *   - every function returns 0 on success, <0 on error (ffe_last_error() has the text); nothing throws;
 *   - all "dev" pointers are device (HBM) buffers owned by the caller; the library owns env state;
 *   - `stream` is a hipStream_t passed as void*; calls are asynchronous on it and never synchronise;
 *   - one handle per (device, stream); handles are not thread-safe; every entry point runs on the handle's device
 *     whatever the caller's current device is, and leaves the caller's current device as it found it;
 *   - layouts are row-major with the env index leading: act[B][A], obs[B][O].
 *
 * Return codes of the env-handle calls (csrc/capi.hip maps them in one place; tests/test_gpu_capi_contract.py pins them)
 *    0  done (asynchronously on `stream`).
 *   -1  refused, nothing was launched: a NULL handle (the only case without a text: there is no handle to keep one), a NULL or
 *       otherwise bad argument ("ffe_get_state: null buffer", "null device buffer" from a flight step,
 *       "null reset mask", an `info_dev` that is not 16-byte aligned, a trajectory index out of range), every failure of a create
 *       function (text in ffe_last_error(NULL), *out = NULL), or a call this kind of handle does not have:
 *         flight        ffe_get_act, ffe_set_act
 *         walk_on_ball  ffe_force_next_episode ("no per-episode randomness")
 *         walk physics  ffe_reset, ffe_reset_envs, ffe_step, ffe_force_next_episode, ffe_time_steps, ffe_time_kernel
 *                       ("... not available on a walk physics handle"; a FFE_WALK_EPISODES handle has all six);
 *                       ffe_get_task_state / ffe_get_validity zero-fill (a FFE_WALK_JOINT_LIMITS or FFE_WALK_EPISODES handle: see
 *                       ffe_create_walk_physics).
 *   -2  a HIP call failed (text: the call and hipGetErrorString).  For historical reasons also walk_on_ball's NULL-buffer
 *       checks of ffe_step / ffe_reset ("walk_on_ball: null output buffer" / "null action buffer").
 *   Since the calls moved into csrc/capi.hip every -1 / -2 on a non-NULL handle sets ffe_last_error(h) (NULL-argument -1s and some
 *   -2 paths used to leave it stale), and a HIP failure inside a flight handle's ffe_force_next_episode is -2 (it was -1).
 *
 * The other four handle families (ffe_nstep_*, ffe_sampler_*, ffe_eplog_*, ffe_walktask_*) use the same codes through the same layer
 * (csrc/handle.hpp): -1 refused with a text, -2 a launch or HIP call failed ("<function>: <hipGetErrorString>"), the text in the
 * family's last_error(h); a create function's text and "<function>: null handle" for a call on a NULL handle are in last_error(NULL).
 * Since the families moved onto that layer their return codes and texts are as before, with these additions to ffe_nstep_*, which
 * used to leave ffe_nstep_last_error stale or empty there: a NULL handle ("ffe_nstep_observe: null handle"), a NULL argument
 * ("ffe_nstep_create: null out", "ffe_nstep_observe: a null input", "ffe_nstep_taint_buffer: null taint") have a text; the -2 text
 * starts with the function's name; the device refusal reads "ffe_nstep_create: no such HIP device: ..." (it had no prefix).
 * ffe_pack_timestep, ffe_episode_stats and ffe_validity_stats have no handle and no text: -1 bad arguments, -2 launch refused.
 */
#ifndef FLYBODY_ENV_H_
#define FLYBODY_ENV_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ffe_env *ffe_handle;

enum { FFE_STEP_FIRST = 0, FFE_STEP_MID = 1, FFE_STEP_LAST = 2 }; /* dm_env.StepType */

/* physics switches (tests / BASELINE config 2 "constraints off"); 0 = everything on */
enum {
  FFE_NO_FLUID = 1, FFE_NO_LIMIT = 2, FFE_NO_DAMPER = 4, FFE_NO_SPRING = 8, FFE_NO_GRAVITY = 16, FFE_NO_ACTUATION = 32,
  FFE_NO_CONTACT = 64, FFE_NO_NOSLIP = 128, FFE_NO_ADHESION = 256 /* walk_on_ball only */,
  /* ffe_create_walk_physics only: joint limits on (the second step kernel of csrc/walk_env.hip).  An opt-in bit and provisional: it
   * exists because plain FFE_NO_CONTACT is a pinned refusal of that create call while floor contacts are missing; when the step
   * kernel lands it folds into "FFE_NO_LIMIT absent". */
  FFE_WALK_JOINT_LIMITS = 512,
  /* ffe_create_walk_physics only: the handle is the walk_imitation environment (sensors, episode protocol, task layer): with the floor
   * off as FFE_NO_CONTACT | FFE_WALK_JOINT_LIMITS | FFE_WALK_EPISODES plus force switches (the third step kernel of csrc/walk_env.hip),
   * on the floor plane with FFE_WALK_FLOOR on top of that (csrc/walk_floor_env.hip), and there with the fly's own contacts with
   * FFE_WALK_SELF | FFE_WALK_SELF_EPISODES on top of both (csrc/walk_imit_self_env.hip).  An opt-in bit and provisional for the same reason: it goes when every
   * contact of the reference's task is built. */
  FFE_WALK_EPISODES = 1024,
  /* ffe_create_walk_physics only: the floor plane against the fly's sphere and capsule geoms, on the bare-physics handle (the fourth
   * step kernel of csrc/walk_env.hip) or, with FFE_WALK_EPISODES and the task, under the environment (csrc/walk_floor_env.hip).  Accepted
   * only as FFE_NO_CONTACT | FFE_WALK_JOINT_LIMITS | FFE_WALK_FLOOR [| FFE_WALK_EPISODES] plus force switches, FFE_NO_NOSLIP and
   * FFE_NO_ADHESION; on such a handle FFE_NO_CONTACT keeps meaning "the fly's own contacts are off" unless FFE_WALK_SELF switches them
   * on.  An opt-in bit and provisional as the two above. */
  FFE_WALK_FLOOR = 2048,
  /* ffe_create_walk_physics only: the fly's own contacts (its 48 sphere / capsule geoms against each other, and every candidate pair
   * with an ellipsoid or a cylinder on one side) on the bare-physics floor handle (csrc/walk_self_env.hip) or, with FFE_WALK_EPISODES and
   * the task (and FFE_WALK_SELF_EPISODES, below), under the environment on the floor (csrc/walk_imit_self_env.hip).  Accepted only as
   * FFE_NO_CONTACT | FFE_WALK_JOINT_LIMITS | FFE_WALK_FLOOR | FFE_WALK_SELF [| FFE_WALK_EPISODES | FFE_WALK_SELF_EPISODES] plus force switches, FFE_NO_NOSLIP and
   * FFE_NO_ADHESION;
   * FFE_NO_CONTACT is then only the marker every accepted set of that create call carries (plain "contacts on" stays a pinned refusal
   * while the floor against ellipsoids and cylinders is missing): the contacts that are built are all on.  With FFE_WALK_EPISODES the
   * bit needs FFE_WALK_FLOOR, the task and FFE_WALK_SELF_EPISODES: a handle without a task does not carry the episode protocol and is
   * refused.  An opt-in bit and provisional as the three above. */
  FFE_WALK_SELF = 4096,
  /* ffe_create_walk_physics only: asks for FFE_WALK_SELF under the environment.  It exists because FFE_WALK_EPISODES | FFE_WALK_FLOOR |
   * FFE_WALK_SELF by themselves are a pinned refusal of that create call, as plain FFE_NO_CONTACT is (see FFE_WALK_JOINT_LIMITS):
   * accepted only together with exactly those three and the task, refused in every other set.  Provisional as the four above. */
  FFE_WALK_SELF_EPISODES = 8192,
  /* ffe_create_walk_physics only: the floor plane against the fly's remaining geoms too - its 16 ellipsoids (two on the thorax, head,
   * rostrum, haustellum halves, four wing blades, six coxae) and 6 cylinders (the abdomen segments) - on the bare-physics handle that
   * carries the floor and the fly's own contacts (csrc/walk_full_env.hip).  With it every geom of fruitfly.xml that the reference's
   * Walking task collides with its floor (tasks/base.py:331-364) does so here.  Accepted only as FFE_NO_CONTACT | FFE_WALK_JOINT_LIMITS |
   * FFE_WALK_FLOOR | FFE_WALK_SELF | FFE_WALK_FLOOR_CONVEX plus force switches, FFE_NO_NOSLIP and FFE_NO_ADHESION, bare physics, or as
   * that set | FFE_WALK_EPISODES | FFE_WALK_SELF_EPISODES with the task: the walk_imitation environment with every contact of the
   * reference's task (csrc/walk_imit_full_env.hip).  Every other set with it - with only one of FFE_WALK_EPISODES and
   * FFE_WALK_SELF_EPISODES, with both and a null `task`, without FFE_WALK_SELF - is refused with a text naming the bit.  (16384 is not
   * used: a set with it is a pinned refusal.)  Provisional as the five above. */
  FFE_WALK_FLOOR_CONVEX = 32768
};

typedef struct ffe_walk_task_s ffe_walk_task; /* the walk_imitation task layer's inputs, defined with ffe_walktask_create below */

/* Task inputs of fly_envs.flight_imitation (vnl_ray/fly_envs.py:29-72).  All host pointers, float64,
 * copied during ffe_create. */
typedef struct {
  /* WingBeatPatternGenerator tables (vnl_ray/tasks/pattern_generators.py:18-119), built by the host */
  int32_t wb_nfreq;            /* number of beat frequencies (201) */
  const double *wb_beat_freqs; /* [nfreq] */
  const int32_t *wb_tab_off;   /* [nfreq+1] row offsets */
  const double *wb_traj;       /* [rows][6] wing angles */
  const double *wb_phase;      /* [rows] */
  double wb_base_freq, wb_rel_range, wb_rate, wb_dt_ctrl;
  /* reference trajectories after the per-episode preprocessing of flight_imitation.py:97-104.  The reference serves
   * trajectories of different lengths (trajectory_loaders.py:98-100,124-129): rows of all trajectories are concatenated
   * and `traj_off[ntraj + 1]` holds the first row of each; traj_off == NULL means every trajectory has `traj_len` rows. */
  int32_t ntraj, traj_len;
  const double *ref_qpos; /* [rows][7] ghost root pose */
  const double *ref_qvel; /* [rows][6] */
  const int32_t *traj_off; /* [ntraj + 1] or NULL */
  int32_t future_steps;     /* fly_envs.py:65 (5) */
  int32_t time_limit_steps; /* round(time_limit / control_timestep), fly_envs.py:54 (3000): caps `_traj_timesteps`
                               (flight_imitation.py:107-108: min(len(trajectory), this) - (future_steps + 1)) */
  int32_t episode_limit_steps; /* control steps after which composer.Environment's `physics.time() >= time_limit` fires;
                                  MuJoCo's time is a float64 running sum of the physics timestep, so this is 3001, not
                                  3000, for 0.6 s at 5e-5 s (flybody_amd/batched_env.py:time_limit_control_steps);
                                  <= 0 means time_limit_steps */
  double terminal_com_dist; /* fly_envs.py:33 (2.0) */
  double ghost_accel_z;     /* gravity felt by the armature-1 ghost, cm/s^2 */
  int32_t pad_first_obs;    /* 0 = dm_control zero-padded sensor buffers at reset */
  int32_t physics_flags;    /* FFE_NO_* */
  /* acme.wrappers.CanonicalSpecWrapper folded in (train_dmpo_ray.py:128-129; same map as tasks/task_utils.py:53-76
   * canonical2real): actions arrive in [-1,1] and are mapped to lo + (a+1)/2 (hi-lo); optional clip to [-1,1] first */
  int32_t canonical_actions;
  int32_t clip_actions;
  /* simultaneous self-contacts the solver carries per env: 0 or 6 = 6 (the default and the benchmarked configuration), 12 = the
   * larger step kernel (same physics up to six contacts, rows for up to twelve); anything else fails ffe_create_flight.  Beyond the
   * capacity the deepest are kept and the env is flagged (ffe_get_task_state, int 7 bits 8-15) */
  int32_t contact_capacity;
} ffe_flight_task;

/* Task inputs of fly_envs.walk_on_ball (vnl_ray/fly_envs.py:125-157).  The arena (ball position / radius / density,
 * tasks/arenas/ball.py:61-69), the actuator filters (joint_filter 0.01, adhesion_filter 0.007) and the claw friction
 * (tasks/walk_on_ball.py:21,41-42) are compiled into the model blob (flybody_amd/assets/fly_ball.ffmb). */
typedef struct {
  double control_timestep;  /* tasks/constants.py:17 (2e-3 s; the model carries the 2e-4 s physics step) */
  int32_t time_limit_steps; /* control steps after which `physics.time() >= time_limit` fires (fly_envs.py:144, 2.0 s):
                               1001 - ten thousand float64 additions of 2e-4 give 1.9999999999998 - see
                               flybody_amd/batched_env.py:time_limit_control_steps */
  int32_t pad_first_obs;    /* 0 = dm_control zero-padded sensor buffers at reset */
  int32_t physics_flags;    /* FFE_NO_* */
  int32_t canonical_actions, clip_actions; /* acme.wrappers.CanonicalSpecWrapper folded in, as in ffe_flight_task */
} ffe_ball_task;

typedef struct {
  int32_t batch, nq, nv, nu, action_dim, obs_dim, nsub;
  double physics_timestep, control_timestep;
  /* observation layout: offsets into the obs row, in the order dm_control emits the walker observables */
  int32_t off_accelerometer, off_gyro, off_joints_pos, off_joints_vel, off_velocimeter, off_world_zaxis,
      off_ref_displacement, off_ref_root_quat, n_obs_joints, n_ref;
} ffe_spec_t;

/* fly_envs.flight_imitation(...) -> composer.Environment (fly_envs.py:29-72); environment_factory() call
 * site agents/ray_distributed_dmpo.py:314.  `model_blob` is the compiled model (flybody_amd/assets). */
int ffe_create_flight(const void *model_blob, size_t blob_size, const ffe_flight_task *task, int batch, int device,
                      uint64_t seed, uint64_t env_id_base, ffe_handle *out);
/* fly_envs.walk_on_ball(...) -> composer.Environment (fly_envs.py:125-157): tethered fly walking on a floating ball
 * (tasks/walk_on_ball.py:16-95; physics via MuJoCo mj_step with contacts, elliptic cones, noslip).  The returned handle
 * works with ffe_spec / ffe_action_bounds / ffe_reset / ffe_step / ffe_physics_step / ffe_get_state / ffe_set_state /
 * ffe_get_task_state / ffe_time_steps / ffe_destroy.  Observation row (289 floats): accelerometer 3 |
 * actuator_activation 59 | appendages_pos 21 | ball_qvel 3 | force 18 | gyro 3 | joints_pos 85 | joints_vel 85 |
 * touch 6 | velocimeter 3 | world_zaxis 3.  State layout: qpos[106] = ball quaternion, then the 102 hinges;
 * qvel[105] = ball angular velocity (body frame), then the hinges. */
int ffe_create_walk_on_ball(const void *model_blob, size_t blob_size, const ffe_ball_task *task, int batch, int device,
                            ffe_handle *out);
/* The walking fly of fly_envs.walk_imitation (fly_envs.py:75-122; flybody_amd/assets/fly_walk.ffmb: free thorax, 6 + 102 dofs, 59
 * filtered actuators) as bare physics: smooth dynamics on the device with constraints off ("dynamics only", as ffe_physics_step offers
 * for the other two tasks), or with the joint limits of its 102 hinges on (FFE_WALK_JOINT_LIMITS); and, with FFE_WALK_EPISODES on top
 * of that, the walk_imitation environment itself with the floor off: sensors, observation row, reward, termination and the episode
 * protocol on the device, a fly that falls freely (or floats with FFE_NO_GRAVITY).  FFE_WALK_FLOOR adds the floor plane against the
 * fly's 48 sphere / capsule geoms (elliptic cones, noslip, adhesion) to the bare-physics handle or, together with FFE_WALK_EPISODES,
 * to the environment, whose force and touch columns are then live; FFE_WALK_SELF adds the fly's own contacts to the bare-physics floor
 * handle or, together with FFE_WALK_EPISODES | FFE_WALK_FLOOR | FFE_WALK_SELF_EPISODES, to the environment on the floor.  FFE_WALK_FLOOR_CONVEX adds
 * the floor against the fly's ellipsoids and cylinders to the bare-physics handle with both or, with FFE_WALK_EPISODES |
 * FFE_WALK_SELF_EPISODES and the task on top, to the environment with both. */
typedef struct {
  /* FFE_NO_CONTACT and exactly one of FFE_NO_LIMIT (smooth dynamics alone) or FFE_WALK_JOINT_LIMITS (joint limits on: up to 48 limit
   * rows per env and substep), plus any of the force switches FFE_NO_FLUID / _DAMPER / _SPRING / _GRAVITY / _ACTUATION; every other
   * set is refused (the text names FFE_WALK_JOINT_LIMITS when that bit was passed).  FFE_WALK_EPISODES is accepted only together with
   * FFE_NO_CONTACT | FFE_WALK_JOINT_LIMITS (plus force switches); every other set with it is refused with a text naming it.
   * FFE_WALK_FLOOR is accepted only as FFE_NO_CONTACT | FFE_WALK_JOINT_LIMITS | FFE_WALK_FLOOR plus force switches, FFE_NO_NOSLIP and
   * FFE_NO_ADHESION (meaningful only with this bit), with or without FFE_WALK_EPISODES; every other set with it - with FFE_NO_LIMIT,
   * without FFE_WALK_JOINT_LIMITS, with FFE_WALK_EPISODES and a null `task` - is refused with a text naming FFE_WALK_FLOOR (and
   * FFE_WALK_EPISODES when that bit was passed too).  FFE_WALK_SELF is accepted only as FFE_NO_CONTACT | FFE_WALK_JOINT_LIMITS |
   * FFE_WALK_FLOOR | FFE_WALK_SELF plus the same switches, bare physics, or with FFE_WALK_EPISODES | FFE_WALK_SELF_EPISODES and the
   * task on top of exactly that; every other set with it - without FFE_WALK_FLOOR, with FFE_NO_LIMIT, with FFE_WALK_EPISODES and a null
   * `task` (a handle without the task does not carry the episode protocol), with only one of FFE_WALK_EPISODES and
   * FFE_WALK_SELF_EPISODES - is refused with a text naming FFE_WALK_SELF.  FFE_WALK_FLOOR_CONVEX is accepted only on top of exactly
   * those two sets with FFE_WALK_SELF (see the bit).  The accepted sets:
   *   FFE_NO_CONTACT | FFE_NO_LIMIT                                                   smooth dynamics
   *   FFE_NO_CONTACT | FFE_WALK_JOINT_LIMITS                                          + joint limits
   *   FFE_NO_CONTACT | FFE_WALK_JOINT_LIMITS | FFE_WALK_FLOOR                         + the floor plane (bare physics)
   *   FFE_NO_CONTACT | FFE_WALK_JOINT_LIMITS | FFE_WALK_FLOOR | FFE_WALK_SELF         + the fly's own contacts (bare physics)
   *   FFE_NO_CONTACT | FFE_WALK_JOINT_LIMITS | FFE_WALK_FLOOR | FFE_WALK_SELF | FFE_WALK_FLOOR_CONVEX
   *                                                                                   + the floor against ellipsoids and cylinders (bare physics)
   *   FFE_NO_CONTACT | FFE_WALK_JOINT_LIMITS | FFE_WALK_EPISODES                      walk_imitation, floor off
   *   FFE_NO_CONTACT | FFE_WALK_JOINT_LIMITS | FFE_WALK_EPISODES | FFE_WALK_FLOOR     walk_imitation on the floor plane
   *   FFE_NO_CONTACT | FFE_WALK_JOINT_LIMITS | FFE_WALK_EPISODES | FFE_WALK_FLOOR | FFE_WALK_SELF | FFE_WALK_SELF_EPISODES
   *                                                                                   + the fly's own contacts
   *   FFE_NO_CONTACT | FFE_WALK_JOINT_LIMITS | FFE_WALK_EPISODES | FFE_WALK_FLOOR | FFE_WALK_SELF | FFE_WALK_SELF_EPISODES |
   *   FFE_WALK_FLOOR_CONVEX                                                           + the floor against ellipsoids and cylinders */
  int32_t physics_flags;
  /* read only when physics_flags has FFE_WALK_EPISODES (a caller without the bit may pass the one int above alone) */
  const ffe_walk_task *task;  /* clips, tracked joints / sites, reward and termination constants: a float32 task layer of the env's
                                 own is created from it (host pointers, copied during the create call); control_timestep must be 10
                                 physics steps */
  uint64_t seed, env_id_base; /* clip of an episode: rng(seed, env_id_base + env, episode, 0) % ntraj, the generator of ffe_create_flight */
  int32_t time_limit_steps;   /* control steps after which the time limit ends an episode, the count ffe_ball_task carries; 10 s: 5001 */
  int32_t pad_first_obs;      /* 0 = dm_control zero-padded sensor buffers at reset */
  int32_t canonical_actions, clip_actions; /* as in ffe_ball_task */
} ffe_walk_physics_task;
/* The handle starts at the blob's qpos0 with zero velocity and zero activation and works with ffe_spec (nq 109, nv 108, nu 59,
 * action_dim 59, obs_dim 0, nsub 10, every observation offset -1) / ffe_action_bounds / ffe_physics_step (ctrl[B][59], clamped to
 * ctrlrange) / ffe_get_state / ffe_set_state / ffe_get_act / ffe_set_act / ffe_get_task_state / ffe_get_validity (zeros on a plain handle) /
 * ffe_last_error / ffe_destroy.  State layout (MuJoCo's): qpos[109] = root position 3 (float64 on the device too), root quaternion
 * 4, the 102 hinges; qvel[108] = root linear velocity in the world frame 3, root angular velocity in the body frame 3, the hinges.
 * ffe_set_state normalises the quaternion as the position stage does.  Refused with rc < 0 and a text (ffe_last_error): flags
 * other than the sets named above (both limit bits together included), a blob that is not the walk model; on either kind of handle
 * ffe_reset, ffe_reset_envs, ffe_step, ffe_time_steps, ffe_time_kernel and ffe_force_next_episode.
 * A handle created with FFE_WALK_JOINT_LIMITS reports instead of the zeros (there is no episode protocol, so nothing is sticky):
 *   ffe_get_validity    column 0 = the overflow bits of the last ffe_physics_step call: bit value 2 = some substep instantiated more
 *                       joint limits than the kernel carries rows (48; walk_on_ball's bit for the same cause) - the rows that did not
 *                       fit were dropped for that substep; columns 1-3 zero
 *   ffe_get_task_state  int 4 = limit rows instantiated in the last substep, int 6 = solver iterations of the last substep, int 7 =
 *                       the same overflow bits; every other int and every real zero
 * and all of them are zero until the first ffe_physics_step.
 * A handle created with FFE_WALK_FLOOR reports the same and on top of it:
 *   ffe_get_validity    column 0 also carries walk_on_ball's other two bits: 1 = more floor contacts than slots (16; the deepest were
 *                       kept), 4 = more rows in one block of the inertia than columns (24; the rows without a column were switched
 *                       off for that substep); bit value 2 counts contact and limit rows together (48)
 *   ffe_get_task_state  int 5 = floor contacts kept in the last substep, real 0 = the sum of their normal forces, real 1 = the
 *                       smallest contact distance (0 without a contact)
 * A handle created with FFE_WALK_SELF reports what a floor handle reports, every column keeping its meaning, with these additions:
 *   ffe_get_validity    column 0 bit value 1 = more contacts, floor and fly-fly together, than slots (16; the floor's keep the first
 *                       slots, the deepest fly-fly ones were kept behind them); bit value 8 = a convex candidate pair was left out of a
 *                       substep because one of its pair lists was full (192 pairs past the bounding spheres, 24 into the narrow phase)
 *   ffe_get_task_state  int 5 = all contacts kept in the last substep, floor and fly-fly (a contact inside its margin but outside
 *                       margin - gap is kept only where an adhesion actuator counts it), int 3 = the fly-fly contacts among them,
 *                       real 0 = the sum of the floor contacts' normal forces as before, real 1 = the smallest distance over both kinds
 * A handle created with FFE_WALK_FLOOR_CONVEX reports what a FFE_WALK_SELF handle reports, every column keeping its meaning: int 5 counts
 * all contacts kept (floor contacts of both kinds and fly-fly), int 3 the fly-fly ones, real 0 sums the normal forces of the floor
 * contacts of both kinds, real 1 is the smallest distance over all three kinds, bit value 1 = more contacts than slots (the 16 deepest
 * floor contacts of both kinds keep the first slots).  The plane-ellipsoid / plane-cylinder contacts among int 5 are reported in real 2:
 * that column is zero on every other bare-physics handle, whereas every int is taken.  On an environment real 2 is the fly-fly count, so
 * an environment created with FFE_WALK_FLOOR_CONVEX reports the plane-ellipsoid / plane-cylinder contacts in real 3 (see below).
 * A handle created with FFE_WALK_EPISODES is an environment (everything above still works on it): ffe_reset, ffe_reset_envs, ffe_step,
 * ffe_force_next_episode (the clip; the phase array is ignored), ffe_time_steps and ffe_time_kernel work as on a walk_on_ball handle,
 * and ffe_spec reports obs_dim 741 with the offsets of the row: accelerometer 3 | actuator_activation 59 | appendages_pos 21 |
 * force 18 | gyro 3 | joints_pos 85 | joints_vel 85 | ref_displacement 195 | ref_root_quat 260 | touch 6 | velocimeter 3 |
 * world_zaxis 3.  Force and touch are zero without FFE_WALK_FLOOR (no contacts); with it force is the interaction force on each
 * tarsus in its site's frame (inertial when nothing touches, so not zero) and touch the sum of the positive normal forces on each claw,
 * both sampled in every substep's acceleration stage and averaged like the accelerometer.  A step is five launches on `stream` (episode bookkeeping, the reset pose,
 * the step kernel, the task layer, the closing rule), with no allocation and no synchronisation, so it can be captured into a HIP
 * graph.  Episode rules (walk_imitation.py:89-177): a reset takes the forced clip or draws one, starts at row 0 of it with zero
 * velocity and activation; a step ends the episode when |velocimeter| > 50, |gyro| > 200, the root is further than terminal_com_dist
 * from the clip's, sqrt(sum qacc^2) > 1e14 or NaN (discount 0), or at the end of the clip (discount 1), or at the time limit.
 *   ffe_get_validity    {step_bits, episode_flagged_steps, episode_bits, episode_steps}, the limit-overflow bit (value 2) sticky over
 *                       the episode in episode_bits, as on a walk_on_ball handle
 *   ffe_get_task_state  int 0 = clip, int 1 = step counter, int 2 = episodes started (low 32 bits), int 3 = needs_reset (the next
 *                       ffe_step resets this env), ints 4, 6, 7 as on a limits handle, int 5 and every real zero; with FFE_WALK_FLOOR
 *                       int 5, real 0 and real 1 as on a floor handle, and the floor's bits 1 / 4 in step_bits and episode_bits too
 *                       with FFE_WALK_SELF on top of that (the force and touch columns then carry the fly-fly contacts' forces on both
 *                       of their links) every column keeps its meaning and: int 5 = all contacts kept in the last substep, floor
 *                       and fly-fly, real 2 = the fly-fly contacts among them (int 3 is needs_reset here; real 2 is zero on every other
 *                       handle), real 1 = the smallest distance over both kinds, and bit value 8 (a convex candidate pair left out)
 *                       joins bits 1 / 2 / 4 in step_bits, sticky per episode in episode_bits
 *                       with FFE_WALK_FLOOR_CONVEX on top of that every column keeps its meaning again: int 5 = all contacts kept,
 *                       floor contacts of both kinds and fly-fly, real 2 = the fly-fly ones, real 0 = the sum of the normal forces of
 *                       the floor contacts of both kinds, real 1 = the smallest distance over all three kinds, and real 3 = the
 *                       plane-ellipsoid / plane-cylinder contacts among int 5 (real 3 is zero on every other handle); bits 1 / 2 / 4 /
 *                       8 unchanged.  Such a contact is a floor cone block: its force enters the force sensor of a tarsus only if its
 *                       geom's link lies below that tarsus (none of the shipped model's does) and touch only on a claw's link; the
 *                       accelerometer and the inertial half of the force sensors see it through qacc
 * A failure of the env's task layer is the env handle's error text. */
int ffe_create_walk_physics(const void *model_blob, size_t blob_size, const ffe_walk_physics_task *task, int batch, int device,
                            ffe_handle *out);
/* physics.data.act (actuator activations, [B][nu] float64 device buffers) of a walk_on_ball or walk physics handle */
int ffe_get_act(ffe_handle h, double *act_dev, void *stream);
int ffe_set_act(ffe_handle h, const double *act_dev, void *stream);
int ffe_destroy(ffe_handle h);

/* observation_spec()/action_spec()/reward_spec()/discount_spec() (ray_distributed_dmpo.py:315) */
int ffe_spec(ffe_handle h, ffe_spec_t *spec);
/* FruitFly.get_action_spec bounds (fruitfly/fruitfly.py:496-526); host arrays of action_dim floats */
int ffe_action_bounds(ffe_handle h, float *minimum, float *maximum);

/* Environment.reset() (acme loop, ray_distributed_dmpo.py:404): every env starts a new episode and reports
 * FIRST.  Outputs as in ffe_step. */
int ffe_reset(ffe_handle h, float *obs_dev, float *reward_dev, float *discount_dev, int32_t *step_type_dev,
              void *stream);
/* Environment.reset() of a subset (one composer.Environment per actor in the reference, each reset on its own:
 * ray_distributed_dmpo.py:401-404; evaluators restart episodes at will): envs with mask_dev[i] != 0 start a new
 * episode and report FIRST; the state and the output rows of the other envs are left untouched. */
int ffe_reset_envs(ffe_handle h, const uint8_t *mask_dev, float *obs_dev, float *reward_dev, float *discount_dev,
                   int32_t *step_type_dev, void *stream);
/* Environment.step(action) (ray_distributed_dmpo.py:404 via acme.EnvironmentLoop.run_episode): one control step of
 * every env = before_step, nsub physics substeps, reward, discount, termination, observation
 * (tasks/flight_imitation.py:149-220, tasks/base.py:190-217).  An env that returned LAST performs its reset on
 * this call instead and returns FIRST (reward 0, discount 1), exactly as dm_control auto-resets.
 * act_dev[B][action_dim] is in the raw action spec and is not modified. */
int ffe_step(ffe_handle h, const float *act_dev, float *obs_dev, float *reward_dev, float *discount_dev,
             int32_t *step_type_dev, void *stream);

/* physics.set_control(ctrl) + nsteps x physics.step() with no task layer (fruitfly/fruitfly.py:492 reaching MuJoCo's mj_step):
 * advances every env's (qpos, qvel) by `nsteps` physics steps under ctrl_dev[B][nu] (clamped to ctrlrange).  BASELINE config 2
 * ("free-flight, dynamics only"); combine with FFE_NO_LIMIT for "constraints off".  Produces no observation. */
int ffe_physics_step(ffe_handle h, const float *ctrl_dev, int nsteps, void *stream);

/* FlightImitationWBPG.set_next_trajectory_index (flight_imitation.py:87-91), plus the initial wing-beat phase
 * the reference draws from its RandomState (flight_imitation.py:137).  Host arrays [B]; traj_idx<0 keeps the
 * counter-based draw.  Applies to each env's next reset only.  The host arrays are staged on `stream` and may be reused
 * as soon as the call returns. */
int ffe_force_next_episode(ffe_handle h, const int32_t *traj_idx_host, const double *phase_host, void *stream);

/* physics.get_state()/set_state() analogue for parity tests: qpos[B][nq] (root position first), qvel[B][nv],
 * float64 device buffers.  set_state leaves task counters untouched. */
int ffe_get_state(ffe_handle h, double *qpos_dev, double *qvel_dev, void *stream);
int ffe_set_state(ffe_handle h, const double *qpos_dev, const double *qvel_dev, void *stream);
/* task-side state per env: {wbpg_step, wbpg_freq_idx, step_counter, traj_idx, needs_reset, n_active_limits,
 * solver_iters, contacts} int32[B][8] and {wbpg_ctrl_freq, ghost_pos[3], ghost_quat[4]} float64[B][8].
 * flight handles, int 7 (the fly's own contacts, for the parity tests): bits 0-7 contacts of the current position stage; bits
 * 8-15 non-zero when a position stage of the last control step met more contacts than the solver carries (the
 * handle's contact_capacity, 6 or 12; the deepest are kept); bits 16-31 the contacts each of the last step's four substeps used, 4 bits each.
 * walk_on_ball handles: {contact history lo, hi, step_counter, fly-fly contacts, needs_reset, contacts, solver_iters, overflow
 * (sticky over the episode; bit 0 more than 16 contacts, bit 1 more than 48 constraint rows, bit 2 more than 24 columns in one
 * block of M)} - the contact history holds, 4 bits per substep for the first 16 substeps of the last control step, the number of
 * contacts that received constraint rows; real 0 holds, 5 bits per substep for the first 12 substeps, the number of contacts
 * DETECTED inside their margin (adhesion is shared over those); the other reals are zero */
int ffe_get_task_state(ffe_handle h, int32_t *ints_dev, double *reals_dev, void *stream);

/* Validity of the physics behind each env's current timestep.  Stands in for what MuJoCo tells a dm_control user through its
 * warnings (mjWARN_CONTACTFULL / mjWARN_CNSTRFULL in physics.data.warning, surfaced by dm_control's Physics.check_invalid_state,
 * mujoco/engine.py): the step kernels carry a fixed number of simultaneous contacts / constraint rows, keep the deepest when a
 * state needs more, and go on - that env-step ran physics the reference would not have run.  info_dev is int32[B][4], 16-byte
 * aligned:
 *   0 step_bits              what went wrong in the launch that produced the current timestep (0 = nothing).  flight: bit 0 a
 *                            position stage of the launch met more contacts than the handle's contact_capacity (exactly int 7 bits
 *                            8-15 != 0 of the task state), bit 1 the constraint solve left its active-set loop on the iteration
 *                            cap (8) with a changed set that got no re-solve.  walk_on_ball: this launch's overflow bits 0-2 as
 *                            documented for int 7 of the task state
 *   1 episode_flagged_steps  control steps of the current episode with step_bits != 0
 *   2 episode_bits           OR of step_bits over those steps (walk_on_ball: the sticky int 7)
 *   3 episode_steps          control steps of the current episode so far (the task state's step_counter)
 * The call that returns FIRST (auto-reset, ffe_reset, a masked row of ffe_reset_envs) sets fields 1-3 to 0; its step_bits describe
 * the start state's position stage and are not counted, so the values read after a LAST timestep are that episode's totals.
 * ffe_physics_step updates step_bits only (walk_on_ball: and ORs into the sticky int 7, as before); ffe_set_state touches none.
 * One small launch on `stream`; the step kernels maintain the fields in the state record they write anyway. */
int ffe_get_validity(ffe_handle h, int32_t *info_dev, void *stream);

/* name and duration helper for bench.py's roofline: launches `iters` steps bracketed by HIP events on `stream`
 * and returns the mean milliseconds per ffe_step launch (synchronises the stream). */
int ffe_time_steps(ffe_handle h, const float *act_dev, float *obs_dev, float *reward_dev, float *discount_dev,
                   int32_t *step_type_dev, int iters, void *stream, float *ms_per_step);
/* the same for the step kernel alone (bench.py's roofline.kernel_ms; what rocprofv3 --kernel-trace reports for it): HIP events
 * immediately around each of `iters` launches of the step kernel, without the launch-order kernel that follows it; synchronises
 * after every launch */
int ffe_time_kernel(ffe_handle h, const float *act_dev, float *obs_dev, float *reward_dev, float *discount_dev,
                    int32_t *step_type_dev, int iters, void *stream, float *ms_per_kernel);

/* device unit test of the in-kernel quaternion helpers against vnl_ray/quaternions.py goldens:
 * op 0 mult_quat(a,b) 1 reciprocal_quat(a) 2 rotate_vec_with_quat(a.xyz,b) 3 quat_dist_short_arc(a,b)
 * 4 get_dquat_local(a,b); a,b,out are device float[n][4] */
int ffe_test_quat(int op, const float *a_dev, const float *b_dev, float *out_dev, int n, void *stream);

const char *ffe_last_error(ffe_handle h);
const char *ffe_version(void);

/* ---- bulk n-step transition writer: the adder the reference's actors feed, batched and device-resident.
 * Replaces acme.adders.reverb.NStepTransitionAdder(n_step, discount) as built at agents/ray_distributed_dmpo.py:514-521
 * (n_step = 50, train_dmpo_ray.py:236) and driven through actor.observe_first / actor.observe (agents/actors.py:91-101).
 * One call per env step with the action that was applied and the timestep ffe_step returned; FIRST rows start an episode
 * (their action is ignored).  Per env each call writes the transition from the oldest held entry (at most n steps back) to the
 * new observation, (o_s, a_s, R, D, o_t+1) with R = r_0 + g d_0 r_1 + g^2 d_0 d_1 r_2 + ... and D = g^(m-1) d_0 ... d_(m-1) over the
 * m <= n entries spanned - like acme's adder it does not wait for n entries, so an episode's first n - 1 steps yield the short
 * transitions (o_0 -> o_1), (o_0 -> o_2), ...; LAST also flushes the shorter tails (an episode of T steps leaves T + min(T, n) - 1).
 * Transitions go to a device replay ring of `capacity` slots (slot = count mod capacity).  capacity >= batch * n_step, the rows one
 * call can write (every env on LAST with a full ring): both constructors refuse a smaller ring with a text in
 * ffe_nstep_last_error(NULL), because two transitions of one launch would then share a slot and a row's arrays are stored by
 * different wavefronts.  Calls are stream-ordered, the envs of one call are not: after W rows the ring holds the last
 * min(W, capacity) claimed rows, each of them whole, in no particular order inside a call.  acme is not in the reference tree:
 * these semantics restate its published behaviour (parity unpinned; the kernel is pinned to a numpy restatement of them at the
 * deployed shapes, tests/test_gpu_nstep_shapes.py). */
typedef struct ffe_nstep *ffe_nstep_handle;
int ffe_nstep_create(int batch, int obs_dim, int act_dim, int n_step, float discount, long long capacity, int device, ffe_nstep_handle *out);
int ffe_nstep_observe(ffe_nstep_handle h, const float *action_dev, const int32_t *step_type_dev, const float *reward_dev,
                      const float *discount_dev, const float *obs_dev, void *stream);
/* device pointers of the replay ring: obs[capacity][O], act[capacity][A], n-step return[capacity], discount[capacity],
 * next_obs[capacity][O], and the running count of transitions written */
int ffe_nstep_buffers(ffe_nstep_handle h, float **obs, float **act, float **ret, float **disc, float **next_obs, unsigned long long **written_dev);
int ffe_nstep_destroy(ffe_nstep_handle h);
/* Validity tracking of the writer - no counterpart in acme's adder, which sees MuJoCo's unbounded contact list: the replay ring
 * gains a taint column so that a learner can drop or down-weight transitions that span truncated physics.  A writer made by the
 * _tracked constructor (same arguments as the plain one) is fed step_bits with every call: element i at step_bits_dev[i * stride_ints],
 * so that column 0 of the ffe_get_validity buffer is passed as it lies with stride_ints = 4.  The position stage a launch ends with
 * is carried into the first substep of the next launch, so a flag raised at step t can reach the physics of step t + 1: the entry
 * appended at step t is marked when bits_t | bits_(t-1) != 0 (the bits passed with a FIRST row count as bits_(t-1) of the episode's
 * first entry), and a transition is tainted (taint[slot] = 1, written with the row) when any entry it spans is marked.  Fed through
 * the plain observe call, a tracked writer takes the bits as zero; the flagged call on an untracked writer, and the taint buffer of
 * one, fail with a text. */
int ffe_nstep_create_tracked(int batch, int obs_dim, int act_dim, int n_step, float discount, long long capacity, int device, ffe_nstep_handle *out);
int ffe_nstep_observe_flagged(ffe_nstep_handle h, const float *action_dev, const int32_t *step_type_dev, const float *reward_dev,
                              const float *discount_dev, const float *obs_dev, const int32_t *step_bits_dev, int stride_ints, void *stream);
int ffe_nstep_taint_buffer(ffe_nstep_handle h, uint8_t **taint /* [capacity] */);
/* The unit the per-step gather to a central learner moves (the reference has no collective - its actors
 * push transitions through Reverb, agents/ray_distributed_dmpo.py:106-115): one fused launch packs (obs, reward, discount,
 * step_type) of the current device into packed_dev[B][obs_dim + 3] (flybody_amd/distributed.py:TimestepGather). */
int ffe_pack_timestep(const float *obs_dev, const float *reward_dev, const float *discount_dev, const int32_t *step_type_dev,
                      float *packed_dev, int batch, int obs_dim, void *stream);

/* episode statistics of a batched actor loop, the ones the reference's EnvironmentLoop logs (agents/ray_distributed_dmpo.py:401-440:
 * episode_return, episode_length): per env the running return [B] float32 and length [B] int64 (a FIRST row adds nothing), and for
 * rows reporting LAST the batch totals {finished episodes, sum of their lengths} (int64[2]) and the sum of their returns (float64[1]);
 * the finished env's counters restart.  One launch per step, nothing read back. */
int ffe_episode_stats(const int32_t *step_type_dev, const float *reward_dev, float *episode_return_dev, long long *episode_length_dev,
                      long long *totals_i64_dev, double *total_return_dev, int batch, void *stream);
/* batch totals of the validity records, accumulated on the device like the episode statistics above (the reference logs nothing of
 * the kind: MuJoCo's warning counters stay inside each actor process): totals_dev int64[3] += {env-steps with step_bits != 0 on
 * MID / LAST rows, episodes finished in this call (LAST rows) with episode_flagged_steps > 0, sum of their episode_flagged_steps}.
 * info_dev is the int32[B][4] buffer of ffe_get_validity for the same timestep as step_type_dev; no per-env running state is needed,
 * the step kernels keep it. */
int ffe_validity_stats(const int32_t *step_type_dev, const int32_t *info_dev, long long *totals_dev, int batch, void *stream);
const char *ffe_nstep_last_error(ffe_nstep_handle h);

/* ---- device replay sampler: uniform minibatches from the writers' replay rings, the read side of the table the writers feed.
 * Replaces the reverb.Table(sampler=reverb.selectors.Uniform(), remover=reverb.selectors.Fifo(), max_size=max_replay_size,
 * rate_limiter=MinSize(min_replay_size) | SampleToInsertRatio(...)) of agents/ray_distributed_dmpo.py:85-113 and the batching of the
 * dataset the learner iterates (batch_size = 256).  The ring is already the Fifo remover and max_size; this adds the Uniform
 * sampler (with replacement), the MinSize gate and the batch, over 1 .. 8 rings (one per env group).  Reverb is not in the reference
 * tree: these semantics restate its published behaviour (parity unpinned; the kernel is pinned to a numpy restatement of the draw
 * below, tests/test_gpu_replay_sampler.py).
 * Lifetime and ordering: the sampler keeps raw pointers into the writers' rings, so every writer must outlive it (destroy the
 * sampler first); and a sample must be stream-ordered after every ffe_nstep_observe / ffe_nstep_observe_flagged whose rows it may
 * see - the same stream, or an event wait - because a writer claims a slot before it stores the row: a row that is being
 * overwritten would otherwise be read torn.  The sample calls on one handle must be stream-ordered among themselves as well (one
 * stream, or event waits between them): the control block the prologue writes and the gather reads, the counters and info are one
 * per handle, so two calls in flight at once on unordered streams would race on them.  Use one sampler per consumer stream. */
typedef struct ffe_sampler *ffe_sampler_handle;
enum { FFE_SAMPLE_SKIP_TAINTED = 1 };
/* reverb.Table(...) + the learner's batch: n_writers 1 .. 8, all on `device` with equal obs_dim and act_dim and a capacity below
 * 2^40; batch (K) 1 .. 2^20; min_size >= 1 (MinSize(min_replay_size)); flags 0 or FFE_SAMPLE_SKIP_TAINTED, which needs every writer
 * tracked.  Anything else fails with rc < 0 and a text in ffe_sampler_last_error(NULL). */
int ffe_sampler_create(const ffe_nstep_handle *writers, int n_writers, int batch, uint64_t seed, long long min_size, int flags, int device,
                       ffe_sampler_handle *out);
/* one item of the learner's iterator (next(dataset) on reverb.TrajectoryDataset batched to K, sampler Uniform): two launches on
 * `stream`, no host synchronisation and no host read, so the call can be captured into a HIP graph and replayed.  With
 * N_r = min(written_r, capacity_r), total = sum N_r: when total < min_size nothing is written (the outputs keep what they held);
 * otherwise row k of obs_dev[K][O], act_dev[K][A], ret_dev[K], disc_dev[K], next_obs_dev[K][O], taint_dev[K], index_dev[K] is the
 * ring row g (rings concatenated in the order given, index = (ring << 40) | slot), drawn exactly as
 *   key = splitmix64(splitmix64(seed ^ 0x5A3B1E) + call), u(k,t) = splitmix64(key + (k << 3) + t), g(k,t) = (u(k,t) * total) >> 64
 * with call = the number of earlier sample calls on this handle, ready or not (kept on the device).  Without
 * FFE_SAMPLE_SKIP_TAINTED row k is g(k,0); with it the first try t = 0 .. 7 whose row has taint 0, the eighth when all are tainted
 * (counted in info[3]).  A non-NULL taint_dev needs every writer tracked. */
int ffe_sampler_sample(ffe_sampler_handle s, float *obs_dev, float *act_dev, float *ret_dev, float *disc_dev, float *next_obs_dev,
                       uint8_t *taint_dev /* may be NULL */, int64_t *index_dev /* may be NULL */, void *stream);
/* reverb.Table.info / the rate limiter's counters: *info_dev = library-owned device int64[8], rewritten by every sample call:
 * 0 ready, 1 total (rows eligible at this call), 2 call (the index this call used), 3 draws of this call that stayed tainted,
 * 4 samples_drawn (cumulative rows of ready calls: with the writers' counts the sample-to-insert ratio SampleToInsertRatio
 * enforces - the host can throttle on it, the device never blocks), 5-7 zero. */
int ffe_sampler_info(ffe_sampler_handle s, long long **info_dev);
/* reverb.Client / Table teardown; the writers are left as they are */
int ffe_sampler_destroy(ffe_sampler_handle s);
const char *ffe_sampler_last_error(ffe_sampler_handle s);

/* ---- per-episode log on the device: one 32-byte record per finished episode, in a ring in HBM.  Replaces what the reference's
 * EnvironmentLoop keeps per episode - the row `run_episode` returns to its logger after every episode (episode_length,
 * episode_return: agents/ray_distributed_dmpo.py:401-440) and the list `self._stats` of the last eval_average_over of them that
 * the evaluator's `_eval_agg_stat` aggregates into avg_ / var_ / max_ / min_ (:408-440; eval_average_over: :81) - for B envs per
 * call.  The aggregation itself stays on the host (flybody_amd.actor_loop.summarize).  acme's loop is not in the reference tree:
 * the per-episode rule restates its published behaviour (parity unpinned; the kernel is pinned to a numpy restatement of the rule,
 * tests/test_gpu_episode_log.py).
 * Record (32 bytes, 32-byte aligned):
 *   int32 env            env index in the handle
 *   int32 tag            the caller's tag of the env, read on the LAST row (flight imitation: the clip, task-state int 3)
 *   int32 length         control steps of the episode
 *   float ret            running float32 sum of the rewards in step order, exactly as ffe_episode_stats accumulates it
 *   int64 call           index of the observe call that closed the episode (the first call on the handle is 0)
 *   int32 flagged_steps  info[i][1] on the LAST row (ffe_get_validity: episode_flagged_steps); 0 without info_dev
 *   int32 bits           bits 0-7 info[i][2] & 255 (episode_bits); bit 8 set when the LAST row's discount is 0: the episode
 *                        terminated and was not cut by the time limit
 * Per env: a FIRST row restarts the running return and length and adds nothing, so an episode abandoned by an explicit reset leaves
 * no record (as in the reference's loop, which only logs at the end of run_episode); a MID row adds its reward and one step; a LAST
 * row does the same, then emits the record and restarts the counters.
 * Ring: the slot of a record is count mod capacity; count, the call counter and armed_left live on the device in the info block
 * int64[4] = {records written, calls, armed_left, reserved}.  capacity >= batch, the records one call can emit: the constructor
 * refuses a smaller ring with a text in the last-error string of the NULL handle.  Calls are stream-ordered; the records of one call are
 * in no particular order among themselves but occupy one contiguous range of count. */
typedef struct ffe_eplog *ffe_eplog_handle;
enum { FFE_EPLOG_ONE_SHOT = 1 };
/* the evaluator's / actor's per-episode bookkeeping (EnvironmentLoop.__init__, agents/ray_distributed_dmpo.py:342-352, where
 * `self._stats = []` is set up): flags 0 or FFE_EPLOG_ONE_SHOT - only armed envs emit, and an env disarms on its LAST: the "first
 * episode of every env" an evaluation round wants */
int ffe_eplog_create(int batch, long long capacity, int flags /* bit 0: one-shot */, int device, ffe_eplog_handle *out);
/* starting an evaluation round (the evaluator's run_episode entered once per env, :401-404): armed[i] = mask_dev[i] != 0, or every env
 * when mask_dev is NULL, and armed_left = their number.  One launch on `stream`, nothing read back.  Fails with a text on a plain log */
int ffe_eplog_arm(ffe_eplog_handle h, const uint8_t *mask_dev /* [B] or NULL = all */, void *stream);
/* the loop body's bookkeeping of one timestep (episode_return += reward, episode_steps += 1, and at the end of the episode the
 * logged row: agents/ray_distributed_dmpo.py:401-415) for every env: one launch on `stream`, no host read, capturable into a HIP
 * graph (the call index lives on the device, so every replay is its own call).  The pointers are read on the handle's device */
int ffe_eplog_observe(ffe_eplog_handle h, const int32_t *step_type_dev, const float *reward_dev, const float *discount_dev,
                      const int32_t *info_dev   /* ffe_get_validity buffer int32[B][4], or NULL */,
                      const int32_t *tag_dev, int tag_stride_ints /* element i at tag_dev[i*stride]; NULL = tag 0 */,
                      void *stream);
/* `self._stats` itself (:408-412): *records_dev = the library-owned ring of `capacity` records, *info_dev = the int64[4] info block */
int ffe_eplog_buffers(ffe_eplog_handle h, void **records_dev, long long **info_dev /* int64[4] */);
/* the loop's teardown */
int ffe_eplog_destroy(ffe_eplog_handle h);
const char *ffe_eplog_last_error(ffe_eplog_handle h);

/* ---- walk_imitation task layer: features, reward factors, termination bits and the kinematic observation columns of
 * fly_envs.walk_imitation (vnl_ray/fly_envs.py:75-122, tasks/walk_imitation.py:24-191, tasks/rewards.py:9-111, tasks/base.py:237-261)
 * as a pure function of (qpos, qvel, clip, step) - no physics.  Stands in for get_walker_features / reward_factors_deep_mimic, for
 * the task observables ref_displacement / ref_root_quat and the walker observables appendages_pos / joints_pos / joints_vel /
 * world_zaxis, and for the pose initialize_episode writes at reset.  The reference's walking dataset is not in its repository: which
 * joints and sites are tracked comes from the caller (parity unpinned on that choice).  One wavefront per state row; no call
 * allocates, reads back or synchronises, so every call can be captured into a HIP graph.  States come in the ffe_get_state layout:
 * qpos double [N][nq], qvel double [N][nv]. */
typedef struct ffe_walktask *ffe_walktask_handle;
enum { FFE_WALKTASK_FLOAT64 = 1 };
/* all host pointers, copied during create */
struct ffe_walk_task_s { /* (typedef ffe_walk_task, declared above ffe_walk_physics_task) */
  int32_t n_joints; const int32_t *joints;   /* tracked hinge joints (model joint indices); may be 0 */
  int32_t n_sites; const int32_t *sites;     /* tracked sites (model site indices); may be 0 */
  /* reference clips of individual lengths, rows concatenated (HDF5WalkingTrajectoryLoader.get_trajectory, trajectory_loaders.py:163-215);
   * ntraj = 0: no reference, only ffe_walktask_features works */
  int32_t ntraj; const int32_t *traj_off;    /* [ntraj + 1], traj_off[0] = 0 */
  const double *ref_qpos;                    /* [rows][7 + n_joints] */
  const double *ref_qvel;                    /* [rows][6 + n_joints] */
  const double *ref_root2site;               /* [rows][n_sites][3] */
  const double *ref_joint_quat;              /* [rows][n_joints][4] */
  int32_t future_steps;                      /* fly_envs.py (64): preview rows after the current one */
  double control_timestep, time_limit, terminal_com_dist;
  double std[4], weights[4];                 /* com, qvel, root2site, joint_quat (rewards.py:96-102; walk_imitation.py: 20,1,1,1) */
  int32_t n_overrides; const int32_t *override_qadr; const double *override_val; /* qpos written after the reference pose at reset
                                                                                    (retract_wings, task_utils.py:117-122) */
  int32_t inference_mode;                    /* walk_imitation.py:148-151: the reward is the constant 1 */
};
/* flags: 0 = float32 kinematics and outputs, FFE_WALKTASK_FLOAT64 = the float64 instantiation (dataset featurisation).  The root
 * position and every difference against it are float64 in both.  Refused with rc < 0 and a text in ffe_walktask_last_error(NULL):
 * a null required pointer, a tracked joint that is not a hinge, a joint / site / override index out of range, a clip shorter than
 * future_steps + 2 rows, a non-positive std or control_timestep, unknown flags, no such device. */
int ffe_walktask_create(const void *model_blob, size_t blob_size, const ffe_walk_task *task, int flags, int device, ffe_walktask_handle *out);
/* get_walker_features (rewards.py:36-61) of n states: com double [n][3], qvel [n][6 + J], root2site [n][S][3], joint_quat [n][1 + J][4]
 * (the root quaternion heads it); the three typed outputs are float or double as the handle was created.  Any output may be NULL
 * (skipped); qvel_dev may be NULL when qvel_out_dev is */
int ffe_walktask_features(ffe_walktask_handle h, const double *qpos_dev, const double *qvel_dev, int n, double *com_dev, void *qvel_out_dev,
                          void *root2site_dev, void *joint_quat_dev, void *stream);
/* reward_factors_deep_mimic against get_reference_features(clip, step) and check_termination's task rules, for n states with their
 * clip[n] and step[n] (int32): factors [n][4], reward [n] (their product, NaN -> 0; 1 in inference mode), term_bits int32 [n]
 * (bit 0: |ref_root[step] - root| > terminal_com_dist; bit 1: step == episode_steps; bit 2: step outside [0, episode_steps] or clip
 * outside [0, ntraj)), and the kinematic columns of the observation row written into obs_dev[n][obs_stride] at the offsets
 * ffe_walktask_info reports (appendages_pos, joints_pos, joints_vel, ref_displacement, ref_root_quat, world_zaxis); the other columns
 * of the row (sensors, activations) are left untouched.  Every reference row index is clamped to the clip's own rows.  Typed
 * outputs are float or double as the handle; any output may be NULL.  obs_stride (elements) must be at least obs_dim */
int ffe_walktask_evaluate(ffe_walktask_handle h, const double *qpos_dev, const double *qvel_dev, const int32_t *clip_dev, const int32_t *step_dev,
                          int n, void *factors_dev, void *reward_dev, int32_t *term_bits_dev, void *obs_dev, int obs_stride, void *stream);
/* the state initialize_episode builds (walk_imitation.py:112-121): qpos0, the root pose and the tracked joints of row `step` of the
 * clip, then the overrides; zero velocity.  qpos double [n][nq], qvel double [n][nv]: exact copies, the root quaternion q / |q| as the
 * position stage leaves it in qpos (mj_kinematics normalises it in place), rounded as that code rounds it; either may be NULL */
int ffe_walktask_reference_pose(ffe_walktask_handle h, const int32_t *clip_dev, const int32_t *step_dev, int n, double *qpos_dev, double *qvel_dev,
                                void *stream);
/* dims int32[16]: 0 nq, 1 nv, 2 J, 3 S, 4 ntraj, 5 future_steps, 6 obs_dim, 7 off appendages_pos, 8 off joints_pos, 9 off joints_vel,
 * 10 off ref_displacement, 11 off ref_root_quat, 12 off world_zaxis, 13 appendages, 14 observed joints, 15 float64 handle.
 * episode_steps int32[ntraj] (host; may be NULL): min(len - future_steps - 1, round(time_limit / control_timestep) + 1) */
int ffe_walktask_info(ffe_walktask_handle h, int32_t *dims, int32_t *episode_steps);
int ffe_walktask_destroy(ffe_walktask_handle h);
const char *ffe_walktask_last_error(ffe_walktask_handle h);

#ifdef __cplusplus
}
#endif
#endif /* FLYBODY_ENV_H_ */
