// walk_env.hip - MI355X (gfx950) batched free-root dynamics of the walking fly (walk_imitation).
//
// ball_env.hip's design with the thorax on a free joint: ONE 64-lane wavefront per environment, lane = link, the leg code of
// leg_dyn.hpp / leg_stage1.inc compiled with FREE_ROOT = true.  This translation unit holds the free-root kernel alone, so that the
// tethered kernel of ball_env.hip is compiled exactly as it was.  Per substep (mj: mj_step restated, constraints off):
//   stage 1  root frame: V0 = (w_b, R' v_w); the leg code in the root body frame about the root origin; whole-tree spatial inertia and
//            bias force (the root rows) WITHOUT gravity; block factorisation of M_jj and M_jj + h B;
//   stage 2  filtered actuators, smooth joint forces; the arrowhead solve of (M + h B) x = f with the six root dofs eliminated last:
//            z = A^-1 f_j and Y = A^-1 M_jr by two four-wide block solves (A = M_jj + h B), S = M_rr - M_rj Y (6 x 6, Cholesky in
//            registers, the same on every lane), x_r = S^-1 (f_r - M_rj z), x_j = z - Y x_r; implicit-in-damping Euler; free joint:
//            qacc = (R (vdot_b + w_b x v_b) + g, wdot_b), position in float64, quaternion as mju_quatIntegrate.
// Gravity: the fictitious base acceleration -R' g of every link is the bias force M e_r (0, -R' g), and B is zero on the root, so the
// solution with it is the solution without it plus (0, R' g) on the root alone.  It is added there, in the world frame, after the
// solve: free fall is exact, and no gravity torque about the root origin is rounded in float32 and divided by the small rotational
// inertias of S (which cost 2e-3 rad/s^2 of root angular acceleration when gravity went through the solve).
// The device code of the substep lives in walk_substeps.hpp (stage 1 is the text fragment `#include "leg_stage1.inc"` inside its `stage1`),
// shared with walk_floor_env.hip, walk_self_env.hip and walk_imit_self_env.hip, one kernel each: there the constraint block of every floor
// tile is the one `contact_forces` and the sensor pass the one `contact_sense`, what the fly's own contacts add under `Tile::kSelf`.
// On the host one table names the handle kinds `walk_create` accepts, and one kernel (`walk_report_kernel`) reports for all of them.
// Four kernels of this file share that code: three of bare physics (`ffe_physics_step`; the third, `floor_step`, collides the floor plane with
// the fly's sphere / capsule geoms and is described where its code starts: "floor contacts") and
// the walk_imitation environment with the floor off (`imitation_step_kernel`, at the end of the kernel section).  `walk_step_kernel` is the smooth dynamics alone (a handle created with FFE_NO_CONTACT |
// FFE_NO_LIMIT).  `walk_limits_kernel` (FFE_NO_CONTACT | FFE_WALK_JOINT_LIMITS) adds the joint-limit
// rows and the constraint solve on the arrowhead matrix between the smooth forces and the Euler solve of stage 2:
//   rows     mj_instantiateLimit with margin 0 (sign, D, aref per hinge slot), compacted by ballots in (slot, lane) order, at most RMAX;
//   M^-1     through M's own factor (not M + h B): z_m = M_jj^-1 f_j, Y_m = M_jj^-1 M_jr, S_m = M_rr - M_rj Y_m = L L',
//            x_r = S_m^-1 (b_r - M_rj z_m), a_s = z_m - Y_m x_r on the hinges;
//   G        G_ik = s_i s_k [(M_jj^-1)_{f_i f_k} + (L^-1 Y_m[f_i]) . (L^-1 Y_m[f_k])]: the block part four columns per block solve, rows
//            of different blocks sharing a column; the rank-6 part from each row lane's own 6-vector, the others' by v_readlane;
//   solve    the dual Newton in row space that the tethered kernel runs, scalar rows only (row_newton.hpp, `row_newton<RB, ScalarRows>`,
//            out of line, a leaf);
//   forces   qfrc_constraint = s f on the hinge right-hand side of the Euler solve; the root's is unchanged (J_r = 0): the root
//            feels a limit through M_rj alone.
// A substep that instantiates no row skips all of it by a wave-uniform branch.
// Parity tests: tests/test_gpu_walk_physics.py, tests/test_gpu_walk_limits.py, tests/test_gpu_walk_episode.py.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>
#include <memory>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <vector>

#include "walk_env.hpp"
#include "walk_model.hpp"
#include "walk_self_model.hpp"
#include "leg_dyn.hpp"
#include "row_newton.hpp"
#include "walk_imu.hpp"
#include "walk_floor.hpp"
#include "walk_substeps.hpp"

namespace ffw {
using namespace dm;
using namespace ffb;

// smooth dynamics alone (FFE_NO_CONTACT | FFE_NO_LIMIT)
__global__ __launch_bounds__(64, 2) void walk_step_kernel(const WalkModel *__restrict__ Wp, int flags, WState *__restrict__ states,
                                                         const float *__restrict__ ctrl, int batch, int nphys) {
  if ((int)blockIdx.x >= batch) return;
  __shared__ WTile T;
  walk_substeps<false>(T, Wp, flags, states, ctrl, nphys);
}

// smooth dynamics + joint limits (FFE_NO_CONTACT | FFE_WALK_JOINT_LIMITS)
__global__ __launch_bounds__(64, 2) void walk_limits_kernel(const WalkModel *__restrict__ Wp, int flags, WState *__restrict__ states,
                                                           const float *__restrict__ ctrl, int batch, int nphys) {
  if ((int)blockIdx.x >= batch) return;
  __shared__ WTileL T;
  walk_substeps<true>(T, Wp, flags, states, ctrl, nphys);
}

// smooth dynamics + joint limits + the floor plane against the fly's sphere / capsule geoms (FFE_NO_CONTACT | FFE_WALK_JOINT_LIMITS |
// FFE_WALK_FLOOR: the fly's own contacts stay off).  Its name carries neither of the two substrings by
// which the older tests count the tile-owning kernels of this file.
__global__ __launch_bounds__(64, 2) void floor_step(const WalkModel *__restrict__ Wp, int flags, WState *__restrict__ states,
                                                   const float *__restrict__ ctrl, FloorRec *__restrict__ rec, int batch, int nphys) {
  if ((int)blockIdx.x >= batch) return;
  __shared__ WTileF T;
  // One substep per pass, the state going through `states` between the passes (float32 and float64 as the registers hold it: nothing is
  // rounded).  While the root origin is higher over the plane than any geom can reach (WalkExtra::f_reach: a bound over all joint
  // angles), the substep is walk_limits_kernel's - the same code of walk_substeps on the same tile layout - so that a floor
  // handle with no floor in reach gives the bits of a limits handle; otherwise it is the floor's.
  const int env = blockIdx.x, lane = threadIdx.x;
  const WalkExtra FFE_GLOBAL &X = *(const WalkExtra FFE_GLOBAL *)&Wp->x;
  WState &S = states[env];
  if (lane == 0) T.step_bits = 0;
#pragma unroll 1
  for (int s = 0; s < nphys; s++) {
    const double height = (double)X.f_frame[0] * S.pos[0] + (double)X.f_frame[1] * S.pos[1] + (double)X.f_frame[2] * S.pos[2] - (double)X.f_off;
    const bool far = __builtin_amdgcn_readfirstlane(height > (double)X.f_reach ? 1 : 0) != 0;
    if (far) {
      walk_substeps<true>(*reinterpret_cast<WTileFar *>(&T), Wp, flags, states, ctrl, 1);
      if (lane == 0) rec[env] = FloorRec{0, 0.f, 0.f, 0};
    } else {
      walk_substeps<true>(T, Wp, flags, states, ctrl, 1, FloorCall{rec});
    }
    if (lane == 0) T.step_bits |= S.step_bits;  // (lane 0 wrote it: its own store)
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");  // the next pass reads what other lanes of this wave stored
    DM_SYNC();
  }
  if (lane == 0) S.step_bits = T.step_bits;
}

// ------------------------------------------------------------------------------------------------ walk_imitation, floor off
// One control step of fly_envs.walk_imitation per wave (FFE_WALK_EPISODES), or the reset of an env that
// episode_begin_kernel flagged: the limits kernel's substeps, the action row in front of them, the sensor sums, the physics columns
// of the observation row and the state for the task layer behind them.  A step is five launches on the caller's stream:
//   episode_begin_kernel           who resets, the clip draw, the step counters
//   ffe_walktask_reference_pose    the pose a reset row starts from (row 0 of its clip)
//   imitation_step_kernel          this one
//   ffe_walktask_evaluate          reward, termination bits and the kinematic observation columns of (qpos, qvel, clip, step)
//   episode_close_kernel           reward, discount, step_type; who resets next
// (its name carries no `walk_`: the two kernels above are the bare-physics step kernels the older tests count)
__global__ __launch_bounds__(64, 2) void imitation_step_kernel(const WalkModel *__restrict__ Wp, int flags, WState *__restrict__ states,
                                                              const ImitArgs *__restrict__ args, const float *__restrict__ action,
                                                              float *__restrict__ obs, int batch) {
  if ((int)blockIdx.x >= batch) return;
  __shared__ WTileE T;
  walk_substeps<true>(T, Wp, flags, states, nullptr, 0, ImitCall{args, action, obs});
}

// Episode record of an env (the oracle's fo_walk_env counters)
struct EpState {
  unsigned long long episode;  // episodes started so far: the counter of the clip draw
  int clip, step, needs_reset, forced;  // forced: clip of the next reset (-1: draw)
  int episode_steps;           // min(len - future_steps - 1, round(time_limit / dt) + 1) of the clip
  int ep_flagged, ep_bits;     // validity: flagged control steps of the episode, OR of their step_bits
  int pad;
};

__device__ __forceinline__ unsigned long long splitmix64(unsigned long long x) {
  x += 0x9E3779B97F4A7C15ULL;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ULL;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBULL;
  return x ^ (x >> 31);
}
// the counter-based generator of fly_env.hip (include/flybody_env.h)
__device__ __forceinline__ unsigned long long env_rng(unsigned long long seed, unsigned long long env, unsigned long long episode, unsigned long long stream) {
  return splitmix64(splitmix64(splitmix64(seed ^ 0xF1B0D7ULL) + env) + (episode << 2) + stream);
}

// mode 0 step, 1 reset all, 3 reset the envs whose mask byte is set.  ref: walk_imitation.py:89-110 (the clip of a new episode),
// base.py: step_counter.  `zero`: the row index ffe_walktask_reference_pose reads the pose from.
__global__ void episode_begin_kernel(EpState *eps, const unsigned char *mask, int mode, unsigned long long seed, unsigned long long env_id_base,
                                     int ntraj, const int *clip_steps, int *flag, int *clip, int *step, int *zero, int batch) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= batch) return;
  EpState &e = eps[i];
  const bool skip = mode == 3 && !mask[i];
  const bool reset = mode == 1 || (mode == 3 && !skip) || (mode == 0 && e.needs_reset != 0);
  if (reset) {
    if (e.forced >= 0) { e.clip = e.forced; e.forced = -1; }
    else e.clip = (int)(env_rng(seed, env_id_base + (unsigned long long)i, e.episode, 0) % (unsigned long long)ntraj);
    e.episode++;
    e.episode_steps = clip_steps[e.clip];
    e.step = 0;
  } else if (!skip) {
    e.step++;
  }
  flag[i] = skip ? 2 : (reset ? 1 : 0);
  clip[i] = e.clip; step[i] = e.step; zero[i] = 0;
}

// ref: walk_imitation.py:148-177 get_reward_factors / check_termination, composer.Environment's time limit.  `reward_in` and `bits`
// are ffe_walktask_evaluate's (the product of the four factors with NaN -> 0, 1 in inference mode; bit 0 distance, bit 1 end of clip).
__global__ void episode_close_kernel(EpState *eps, const WState *states, const int *flag, const float *term, const float *reward_in, const int *bits,
                                     int time_limit_steps, float *rew, float *disc, int *st, int batch) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= batch) return;
  if (flag[i] == 2) return;
  EpState &e = eps[i];
  if (flag[i] == 1) {
    rew[i] = 0.f; disc[i] = 1.f; st[i] = 0;
    e.needs_reset = 0; e.ep_flagged = 0; e.ep_bits = 0;
    return;
  }
  const float *t = term + (size_t)i * 4;
  const bool end = (bits[i] & 2) != 0;
  const bool fatal = t[0] > 50.f || t[1] > 200.f || (bits[i] & 1) != 0 || !(t[2] == t[2]) || !(sqrtf(t[2]) <= 1e14f);
  const bool stop = fatal || end;
  const bool timeup = e.step >= time_limit_steps;
  const float r = reward_in[i];
  rew[i] = r == r ? r : 0.f;
  disc[i] = (stop && !end) ? 0.f : 1.f;
  st[i] = (stop || timeup) ? 2 : 1;
  e.needs_reset = (stop || timeup) ? 1 : 0;
  const int sb = states[i].step_bits;
  e.ep_flagged += sb ? 1 : 0; e.ep_bits |= sb;
}

__global__ void episode_force_kernel(EpState *eps, const int *traj, int batch) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < batch && traj[i] >= 0) eps[i].forced = traj[i];
}
__global__ void episode_init_kernel(EpState *eps, int batch) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= batch) return;
  EpState z{};
  z.needs_reset = 1; z.forced = -1;
  eps[i] = z;
}
// Task state and validity of every handle with limit rows; `eps` is null without FFE_WALK_EPISODES, `rec` without FFE_WALK_FLOOR.
//   ints      {clip, step counter, episode (low 32 bits), needs_reset} of the episode record, zeros without one - but int 3 of a
//             bare-physics floor handle is the fly-fly contacts among int 5 (0 without FFE_WALK_SELF); limit rows of the last substep;
//             contacts kept in the last substep (floor and, with FFE_WALK_SELF, fly-fly), 0 off the floor; solver iterations of the last
//             substep; overflow bits of the last launch
//   reals     on the floor the sum of the contacts' normal forces and the smallest contact distance (0 without a contact; with
//             FFE_WALK_SELF over both kinds), and on an episode handle, where int 3 is taken, the fly-fly count in real 2; on a bare-physics
//             handle with FFE_WALK_FLOOR_CONVEX real 2 is the plane-ellipsoid / plane-cylinder contacts among int 5 (bits 8 .. 15 of the
//             record's nself, zero from every other kernel), on an episode handle with that bit, where real 2 is taken, they are real 3;
//             zeros otherwise
//   validity  {overflow bits of the last launch (1 more contacts than slots, 2 more rows than RMAX, 4 more rows in a block than columns,
//             8 a convex candidate pair left out because a pair list of the substep was full), episode_flagged_steps, episode_bits,
//             episode_steps}, the last three zero without an episode record
__global__ void walk_report_kernel(const EpState *eps, const WState *states, const FloorRec *rec, int *ints, double *reals, int *info, int batch) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= batch) return;
  const WState &S = states[i];
  if (ints) {
    int *o = ints + (size_t)i * 8;
    o[0] = eps ? eps[i].clip : 0; o[1] = eps ? eps[i].step : 0; o[2] = eps ? (int)(unsigned)eps[i].episode : 0;
    o[3] = eps ? eps[i].needs_reset : (rec ? (rec[i].nself & 0xff) : 0);
    o[4] = S.nlim; o[5] = rec ? rec[i].ncon : 0; o[6] = S.iters; o[7] = S.step_bits;
    double *r = reals + (size_t)i * 8;
    for (int k = 0; k < 8; k++) r[k] = 0.0;
    if (rec) { r[0] = (double)rec[i].fsum; r[1] = (double)rec[i].mind; r[2] = eps ? (double)(rec[i].nself & 0xff) : (double)(rec[i].nself >> 8); if (eps) r[3] = (double)(rec[i].nself >> 8); }
  }
  if (info) *reinterpret_cast<int4 *>(info + (size_t)i * 4) = eps ? make_int4(S.step_bits, eps[i].ep_flagged, eps[i].ep_bits, eps[i].step) : make_int4(S.step_bits, 0, 0, 0);
}

// mj: mj_normalizeQuat as the position stage applies it (float32, a null quaternion becomes the identity)
__device__ __forceinline__ void store_quat(WState &S, double w, double x, double y, double z) {
  const Q4 q = qnormalize(Q4{(float)w, (float)x, (float)y, (float)z});
  S.quat[0] = q.w; S.quat[1] = q.x; S.quat[2] = q.y; S.quat[3] = q.z;
}
__global__ void walk_init_states(WState *states, const WalkModel *Wp, int batch) {
  const int env = blockIdx.x, t = threadIdx.x;
  if (env >= batch) return;
  WState &S = states[env];
  for (int k = t; k < NDP; k += blockDim.x) { S.q[k] = k < ND ? Wp->b.qpos0[k] : 0.f; S.v[k] = 0.f; }
  for (int k = t; k < 64; k += blockDim.x) S.act[k] = 0.f;
  if (t == 0) {
    for (int k = 0; k < 3; k++) { S.pos[k] = (double)Wp->x.qpos0[k]; S.vlin[k] = 0.f; S.wb[k] = 0.f; }
    store_quat(S, Wp->x.qpos0[3], Wp->x.qpos0[4], Wp->x.qpos0[5], Wp->x.qpos0[6]);
    S.nlim = S.iters = S.step_bits = S.pad = 0;
  }
}
__global__ void walk_get_state_kernel(const WState *states, double *qpos, double *qvel, int batch) {
  const int env = blockIdx.x, t = threadIdx.x;
  if (env >= batch) return;
  const WState &S = states[env];
  for (int k = t; k < 109; k += blockDim.x) qpos[(size_t)env * 109 + k] = k < 3 ? S.pos[k] : (k < 7 ? (double)S.quat[k - 3] : (double)S.q[k - 7]);
  for (int k = t; k < 108; k += blockDim.x) qvel[(size_t)env * 108 + k] = k < 3 ? (double)S.vlin[k] : (k < 6 ? (double)S.wb[k - 3] : (double)S.v[k - 6]);
}
__global__ void walk_set_state_kernel(WState *states, const double *qpos, const double *qvel, int batch) {
  const int env = blockIdx.x, t = threadIdx.x;
  if (env >= batch) return;
  WState &S = states[env];
  const double *qp = qpos + (size_t)env * 109, *qv = qvel + (size_t)env * 108;
  for (int k = t; k < ND; k += blockDim.x) { S.q[k] = (float)qp[7 + k]; S.v[k] = (float)qv[6 + k]; }
  if (t < 3) { S.pos[t] = qp[t]; S.vlin[t] = (float)qv[t]; S.wb[t] = (float)qv[3 + t]; }
  if (t == 0) store_quat(S, qp[3], qp[4], qp[5], qp[6]);
}
__global__ void walk_act_kernel(WState *states, double *act, int batch, int set) {
  const int env = blockIdx.x, t = threadIdx.x;
  if (env >= batch || t >= NU) return;
  if (set) states[env].act[t] = (float)act[(size_t)env * NU + t];
  else act[(size_t)env * NU + t] = (double)states[env].act[t];
}

// ================================================================================================ host side
// Bare physics (reset, step, forced episodes and the timers are refused) or, created with FFE_WALK_EPISODES, the walk_imitation
// environment with the floor off or, with FFE_WALK_FLOOR too, on the floor (step 4c: the third of the five
// launches is then `imitation_floor_step` of walk_floor_env.hip; step 4d, with FFE_WALK_SELF on top: `imitation_self_step` of
// walk_imit_self_env.hip; step 4e, with FFE_WALK_FLOOR_CONVEX on top: `imitation_full_step` of walk_imit_full_env.hip).
struct WalkEnv final : ffe::EnvBackend {
  int flags = 0;
  bool limits = false;    // FFE_WALK_JOINT_LIMITS: walk_limits_kernel steps this handle
  bool episodes = false;  // FFE_WALK_EPISODES: ffe_step / ffe_reset / ... work, imitation_step_kernel steps them
  bool floor = false;     // FFE_WALK_FLOOR: floor_step steps this handle (with `episodes`: imitation_floor_step)
  bool self = false;      // FFE_WALK_SELF (with `floor`): floor_self_step of walk_self_env.hip steps this handle (with `episodes`:
                          // imitation_self_step of walk_imit_self_env.hip)
  FloorRec *rec = nullptr;  // floor handle only: contacts, normal-force sum and smallest distance of the last substep
  WalkHost host;
  ffe::DeviceBuffers mem{"ffe_create_walk_physics"};  // everything below lives here
  WalkModel *model_dev = nullptr;
  WalkModelFull *full_dev = nullptr;  // FFE_WALK_FLOOR_CONVEX only: the model with the second floor table behind it (model_dev = &full_dev->m);
                                      // floor_full_step of walk_full_env.hip steps this handle (with `episodes`: imitation_full_step
                                      // of walk_imit_full_env.hip)
  WState *states = nullptr;
  // episode handle only
  ffe_walktask_handle task = nullptr;  // the float32 task layer of this env
  ImitArgs args{};
  ImitArgs *args_dev = nullptr;  // its copy on the device
  EpState *eps = nullptr;
  int *flag = nullptr, *clip = nullptr, *step = nullptr, *zero = nullptr, *clip_steps = nullptr, *bits = nullptr, *forced_dev = nullptr;
  float *reward_tmp = nullptr;
  unsigned long long seed = 0, env_id_base = 0;
  int ntraj = 0, time_limit_steps = 0, n_obs_joints = 0, n_ref = 0, off_jpos = -1, off_jvel = -1, off_disp = -1, off_rquat = -1, off_zaxis = -1;
  ffe::KernelTimer tm;

  ~WalkEnv() override {
    if (task) (void)ffe_walktask_destroy(task);
  }

  [[noreturn]] void refuse(const char *what) const override {
    throw ffe::Refused(std::string(what) + ": not available on a walk physics handle (bare physics only: limits, floor contacts, sensors and the episode protocol are not built yet)");
  }
  // a failure of the task layer becomes this handle's error
  void task_ok(int rc, const char *what) const {
    if (rc != 0) throw std::runtime_error(std::string(what) + ": " + ffe_walktask_last_error(task));
  }

  void spec(ffe_spec_t &s) const override {  // bare physics: no observation row, every offset is -1
    s = ffe_spec_t{};
    s.batch = batch; s.nq = host.nq; s.nv = host.nv; s.nu = NU; s.action_dim = NACT; s.obs_dim = 0; s.nsub = host.m.b.nsub;
    s.physics_timestep = host.m.b.h; s.control_timestep = (double)host.m.b.nsub * (double)host.m.b.h;
    s.off_accelerometer = s.off_gyro = s.off_joints_pos = s.off_joints_vel = s.off_velocimeter = s.off_world_zaxis = -1;
    s.off_ref_displacement = -1; s.off_ref_root_quat = -1;
    if (episodes) {
      // accelerometer 3 | actuator_activation 59 | appendages_pos | force 18 | gyro 3 | joints_pos | joints_vel | ref_displacement |
      // ref_root_quat | touch 6 | velocimeter 3 | world_zaxis 3
      s.obs_dim = args.obs_dim; s.off_accelerometer = 0; s.off_gyro = args.off_gyro; s.off_joints_pos = off_jpos; s.off_joints_vel = off_jvel;
      s.off_velocimeter = args.off_velocimeter; s.off_world_zaxis = off_zaxis; s.off_ref_displacement = off_disp; s.off_ref_root_quat = off_rquat;
      s.n_obs_joints = n_obs_joints; s.n_ref = n_ref;
    }
  }
  void action_bounds(float *mn, float *mx) const override {
    for (int k = 0; k < NACT; k++) { mn[k] = host.action_min[k]; mx[k] = host.action_max[k]; }
  }
  ffe::KernelTimer *timer() override { return episodes ? &tm : nullptr; }

  void launch(const float *act, float *obs, float *rew, float *disc, int32_t *st, void *stream, int mode, int nphys, const uint8_t *mask) override {
    hipStream_t s = (hipStream_t)stream;
    if (mode == 2) {  // bare physics: act = ctrl[B][59]
      if (!act || nphys <= 0) throw std::runtime_error("walk physics: null control buffer or no steps");
      if (full_dev) launch_floor_full_step(full_dev, flags, states, act, rec, batch, nphys, s);
      else if (self) launch_floor_self_step(model_dev, flags, states, act, rec, batch, nphys, s);
      else if (floor) hipLaunchKernelGGL(floor_step, dim3(batch), dim3(64), 0, s, model_dev, flags, states, act, rec, batch, nphys);
      else if (limits) hipLaunchKernelGGL(walk_limits_kernel, dim3(batch), dim3(64), 0, s, model_dev, flags, states, act, batch, nphys);
      else hipLaunchKernelGGL(walk_step_kernel, dim3(batch), dim3(64), 0, s, model_dev, flags, states, act, batch, nphys);
      HIP_OK(hipGetLastError());
      return;
    }
    if (!episodes) refuse("ffe_reset / ffe_reset_envs / ffe_step");
    ffe::need(mode != 0 || act, "walk_imitation: null action buffer");
    ffe::need(obs && rew && disc && st, "walk_imitation: null output buffer");
    const dim3 grid((batch + 63) / 64), block(64);
    hipLaunchKernelGGL(episode_begin_kernel, grid, block, 0, s, eps, mask, mode, seed, env_id_base, ntraj, clip_steps, flag, clip, step, zero, batch);
    HIP_OK(hipGetLastError());
    task_ok(ffe_walktask_reference_pose(task, clip, zero, batch, const_cast<double *>(args.pose), nullptr, stream), "walk_imitation");
    const ImitArgs &a = args;
    tm.start(s);
    if (full_dev) launch_imitation_full_step(full_dev, flags, states, args_dev, act, obs, batch, s);
    else if (self) launch_imitation_self_step(model_dev, flags, states, args_dev, act, obs, batch, s);
    else if (floor) launch_imitation_floor_step(model_dev, flags, states, args_dev, act, obs, batch, s);
    else hipLaunchKernelGGL(imitation_step_kernel, dim3(batch), dim3(64), 0, s, model_dev, flags, states, args_dev, act, obs, batch);
    HIP_OK(hipGetLastError());
    tm.stop(s);
    task_ok(ffe_walktask_evaluate(task, a.qpos, a.qvel, clip, step, batch, nullptr, reward_tmp, bits, obs, a.obs_dim, stream), "walk_imitation");
    hipLaunchKernelGGL(episode_close_kernel, grid, block, 0, s, eps, states, flag, a.term, reward_tmp, bits, time_limit_steps, rew, disc, st, batch);
    HIP_OK(hipGetLastError());
    tm.collect();
  }
  void force_next_episode(const int32_t *traj, const double *, void *stream) override {  // (walk_imitation draws no phase)
    if (!episodes) refuse("ffe_force_next_episode");
    for (int i = 0; i < batch; i++)
      if (traj[i] >= ntraj) throw ffe::Refused("ffe_force_next_episode: trajectory index out of range");
    hipStream_t s = (hipStream_t)stream;
    // pageable host memory: the copy is staged before the call returns, ordered on `s` with the kernel below; the stream is
    // synchronised once so that a second call cannot overwrite the staging buffer under a pending kernel (as the flight handle)
    HIP_OK(hipMemcpyAsync(forced_dev, traj, sizeof(int) * (size_t)batch, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(episode_force_kernel, dim3((batch + 63) / 64), dim3(64), 0, s, eps, forced_dev, batch);
    HIP_OK(hipGetLastError());
    HIP_OK(hipStreamSynchronize(s));
  }
  void get_state(double *qpos, double *qvel, void *stream) override {  // qpos[B][109], qvel[B][108]: MuJoCo's free-joint layout
    hipLaunchKernelGGL(walk_get_state_kernel, dim3(batch), dim3(128), 0, (hipStream_t)stream, states, qpos, qvel, batch);
    HIP_OK(hipGetLastError());
  }
  void set_state(const double *qpos, const double *qvel, void *stream) override {
    hipLaunchKernelGGL(walk_set_state_kernel, dim3(batch), dim3(128), 0, (hipStream_t)stream, states, qpos, qvel, batch);
    HIP_OK(hipGetLastError());
  }
  void get_act(double *act, void *stream) override {
    hipLaunchKernelGGL(walk_act_kernel, dim3(batch), dim3(64), 0, (hipStream_t)stream, states, act, batch, 0);
    HIP_OK(hipGetLastError());
  }
  void set_act(const double *act, void *stream) override {
    hipLaunchKernelGGL(walk_act_kernel, dim3(batch), dim3(64), 0, (hipStream_t)stream, states, const_cast<double *>(act), batch, 1);
    HIP_OK(hipGetLastError());
  }
  void report(int *ints, double *reals, int *info, void *stream) {
    hipLaunchKernelGGL(walk_report_kernel, dim3((batch + 63) / 64), dim3(64), 0, (hipStream_t)stream, eps, states, rec, ints, reals, info, batch);
    HIP_OK(hipGetLastError());
  }
  void get_task_state(int32_t *ints, double *reals, void *stream) override {  // int32[B][8] and float64[B][8]: zeros on a plain handle
    if (limits) return report(ints, reals, nullptr, stream);
    HIP_OK(hipMemsetAsync(ints, 0, sizeof(int32_t) * 8 * (size_t)batch, (hipStream_t)stream));
    HIP_OK(hipMemsetAsync(reals, 0, sizeof(double) * 8 * (size_t)batch, (hipStream_t)stream));
  }
  void get_validity(int32_t *info, void *stream) override {  // int32[B][4]: zeros on a plain handle
    if (limits) return report(nullptr, nullptr, info, stream);
    HIP_OK(hipMemsetAsync(info, 0, sizeof(int32_t) * 4 * (size_t)batch, (hipStream_t)stream));
  }
};

// what FFE_WALK_EPISODES adds to a limits handle: the task layer, the episode records and the buffers between the launches of a step
static void make_episodes(WalkEnv &e, const Blob &b, const void *blob, size_t blob_size, const ffe_walk_physics_task &t) {
  const int B = e.batch;
  if (ffe_walktask_create(blob, blob_size, t.task, 0, e.device, &e.task) != 0)
    throw std::runtime_error(std::string("ffe_create_walk_physics: FFE_WALK_EPISODES: ") + ffe_walktask_last_error(nullptr));
  int32_t dims[16];
  e.task_ok(ffe_walktask_info(e.task, dims, nullptr), "ffe_create_walk_physics");
  e.ntraj = dims[4];
  if (e.ntraj <= 0) throw std::runtime_error("ffe_create_walk_physics: FFE_WALK_EPISODES needs reference clips in the task");
  if (dims[0] != e.host.nq || dims[1] != e.host.nv) throw std::runtime_error("ffe_create_walk_physics: FFE_WALK_EPISODES: the task layer's model is not the walk model");
  if (llround(t.task->control_timestep / (double)e.host.m.b.h) != e.host.m.b.nsub)
    throw std::runtime_error("ffe_create_walk_physics: FFE_WALK_EPISODES: the task's control_timestep must be 10 physics steps");
  if (t.time_limit_steps <= 0) throw std::runtime_error("ffe_create_walk_physics: FFE_WALK_EPISODES: time_limit_steps must be positive");
  std::vector<int32_t> ep((size_t)e.ntraj);
  e.task_ok(ffe_walktask_info(e.task, dims, ep.data()), "ffe_create_walk_physics");
  // the row: accelerometer 3 | actuator_activation 59 | appendages_pos | force 18 | gyro 3 | joints_pos | joints_vel | ref_displacement |
  // ref_root_quat | touch 6 | velocimeter 3 | world_zaxis 3; the kinematic offsets are the task layer's
  ImitArgs &a = e.args;
  const int F1 = dims[5] + 1;
  a.obs_dim = dims[6]; a.off_act = 3; a.off_force = dims[7] + 3 * dims[13]; a.off_gyro = a.off_force + 18;
  a.off_touch = dims[11] + 4 * F1; a.off_velocimeter = a.off_touch + 6;
  e.off_jpos = dims[8]; e.off_jvel = dims[9]; e.off_disp = dims[10]; e.off_rquat = dims[11]; e.off_zaxis = dims[12];
  e.n_obs_joints = dims[14]; e.n_ref = F1;
  if (dims[7] != 3 + NU || dims[8] != a.off_gyro + 3 || dims[12] != a.off_velocimeter + 3 || a.obs_dim != dims[12] + 3)
    throw std::runtime_error("ffe_create_walk_physics: FFE_WALK_EPISODES: the task layer's observation row leaves no room for the 92 physics columns");
  a.canonical = t.canonical_actions; a.clip = t.clip_actions; a.pad_first_obs = t.pad_first_obs;
  {
    const Tensor &site = b.get("site");  // body, position 3, quaternion 4 of the IMU site (the thorax is the root: already its frame)
    for (int k = 0; k < 3; k++) a.site_pos[k] = (float)site.f(1 + k);
    for (int k = 0; k < 4; k++) a.site_quat[k] = (float)site.f(4 + k);
  }
  e.seed = t.seed; e.env_id_base = t.env_id_base; e.time_limit_steps = t.time_limit_steps;
  a.pose = e.mem.zeroed<double>((size_t)B * 109);
  a.qpos = e.mem.zeroed<double>((size_t)B * 109); a.qvel = e.mem.zeroed<double>((size_t)B * 108);
  a.term = e.mem.zeroed<float>((size_t)B * 4);
  e.eps = e.mem.zeroed<EpState>((size_t)B);
  e.flag = e.mem.zeroed<int>((size_t)B); e.clip = e.mem.zeroed<int>((size_t)B); e.step = e.mem.zeroed<int>((size_t)B);
  e.zero = e.mem.zeroed<int>((size_t)B); e.bits = e.mem.zeroed<int>((size_t)B); e.forced_dev = e.mem.zeroed<int>((size_t)B);
  e.reward_tmp = e.mem.zeroed<float>((size_t)B);
  e.clip_steps = e.mem.zeroed<int>((size_t)e.ntraj);
  a.flag = e.flag;
  a.rec = e.rec;  // (null without FFE_WALK_FLOOR)
  e.args_dev = e.mem.zeroed<ImitArgs>(1);
  HIP_OK(hipMemcpy(e.args_dev, &a, sizeof(ImitArgs), hipMemcpyHostToDevice));
  HIP_OK(hipMemcpy(e.clip_steps, ep.data(), sizeof(int32_t) * (size_t)e.ntraj, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(episode_init_kernel, dim3((B + 63) / 64), dim3(64), 0, 0, e.eps, B);
  HIP_OK(hipGetLastError());
  e.tm.create();
}

// The handle kinds without the fly's own contacts.  A set of flags belongs to the first kind whose `key` it shows under `key_mask`; it is
// accepted when, the kind's `switches` aside, it is exactly `bits`, and when the task is there where `task` asks for it.
constexpr int kForceSwitches = BF_NO_FLUID | BF_NO_DAMPER | BF_NO_SPRING | BF_NO_GRAVITY | BF_NO_ACTUATION;
constexpr int kSwitches = kForceSwitches | BF_NO_NOSLIP | BF_NO_ADHESION;
constexpr int kLimitBits = BF_NO_CONTACT | BF_NO_LIMIT | BF_WALK_JOINT_LIMITS;  // all a handle off the floor and without episodes is judged by
struct WalkKind { int key_mask, key, bits, switches; bool task; const char *bad_flags, *no_task; };
static const WalkKind kWalkKinds[] = {
  {BF_WALK_FLOOR | BF_WALK_EPISODES, BF_WALK_FLOOR | BF_WALK_EPISODES, BF_NO_CONTACT | BF_WALK_JOINT_LIMITS | BF_WALK_EPISODES | BF_WALK_FLOOR, kSwitches, true,
   "ffe_create_walk_physics: FFE_WALK_EPISODES | FFE_WALK_FLOOR (the walk_imitation environment on the floor plane) needs "
   "FFE_NO_CONTACT | FFE_WALK_JOINT_LIMITS and takes the force switches, FFE_NO_NOSLIP and FFE_NO_ADHESION only: it excludes "
   "FFE_NO_LIMIT",
   "ffe_create_walk_physics: FFE_WALK_EPISODES | FFE_WALK_FLOOR needs the task (a null ffe_walk_task pointer); FFE_WALK_FLOOR "
   "without FFE_WALK_EPISODES is the bare-physics floor handle"},
  {BF_WALK_FLOOR | BF_WALK_EPISODES, BF_WALK_FLOOR, BF_NO_CONTACT | BF_WALK_JOINT_LIMITS | BF_WALK_FLOOR, kSwitches, false,
   "ffe_create_walk_physics: FFE_WALK_FLOOR (the floor plane against the fly's sphere and capsule geoms, bare physics) needs "
   "FFE_NO_CONTACT | FFE_WALK_JOINT_LIMITS and takes the force switches, FFE_NO_NOSLIP and FFE_NO_ADHESION only: it excludes "
   "FFE_NO_LIMIT and FFE_WALK_EPISODES",
   nullptr},
  {BF_WALK_FLOOR | BF_WALK_EPISODES, BF_WALK_EPISODES, BF_NO_CONTACT | BF_WALK_JOINT_LIMITS | BF_WALK_EPISODES, kForceSwitches, true,
   "ffe_create_walk_physics: FFE_WALK_EPISODES (the walk_imitation environment with the floor off) needs FFE_NO_CONTACT | "
   "FFE_WALK_JOINT_LIMITS and takes the force switches only: floor contacts are not built yet",
   "ffe_create_walk_physics: FFE_WALK_EPISODES needs the task (a null ffe_walk_task pointer)"},
  // without the bit the text is the one the C ABI contract pins; with it the text names the bit
  {BF_WALK_JOINT_LIMITS, BF_WALK_JOINT_LIMITS, BF_NO_CONTACT | BF_WALK_JOINT_LIMITS, ~kLimitBits, false,
   "ffe_create_walk_physics: floor contacts and joint limits are not built yet as a step kernel: FFE_WALK_JOINT_LIMITS needs "
   "FFE_NO_CONTACT and excludes FFE_NO_LIMIT",
   nullptr},
  {0, 0, BF_NO_CONTACT | BF_NO_LIMIT, ~kLimitBits, false,
   "ffe_create_walk_physics: floor contacts and joint limits are not built yet: physics_flags must contain FFE_NO_CONTACT | FFE_NO_LIMIT", nullptr},
};

std::unique_ptr<ffe::EnvBackend> walk_create(const void *blob, size_t blob_size, const ffe_walk_physics_task &task, int batch, int device) {
  const int physics_flags = task.physics_flags;
  if (!blob || batch <= 0) throw std::runtime_error("ffe_create_walk_physics: bad arguments");
  const bool limits = (physics_flags & BF_WALK_JOINT_LIMITS) != 0;
  const bool episodes = (physics_flags & BF_WALK_EPISODES) != 0, floor = (physics_flags & BF_WALK_FLOOR) != 0;
  const bool self = (physics_flags & BF_WALK_SELF) != 0, self_env = (physics_flags & BF_WALK_SELF_EPISODES) != 0;
  const bool convex = (physics_flags & BF_WALK_FLOOR_CONVEX) != 0;
  if (convex) {  // the floor against ellipsoids and cylinders: two accepted sets, bare physics and the environment with the task
    constexpr int kFull = BF_NO_CONTACT | BF_WALK_JOINT_LIMITS | BF_WALK_FLOOR | BF_WALK_SELF | BF_WALK_FLOOR_CONVEX;
    if (episodes != self_env)
      throw std::runtime_error("ffe_create_walk_physics: FFE_WALK_FLOOR_CONVEX under the environment is asked for with FFE_WALK_EPISODES | "
                               "FFE_WALK_SELF_EPISODES together (on FFE_NO_CONTACT | FFE_WALK_JOINT_LIMITS | FFE_WALK_FLOOR | FFE_WALK_SELF | "
                               "FFE_WALK_FLOOR_CONVEX and with the task): one of the two bits without the other is refused");
    if ((physics_flags & ~(kSwitches | BF_WALK_EPISODES | BF_WALK_SELF_EPISODES)) != kFull)
      throw std::runtime_error("ffe_create_walk_physics: FFE_WALK_FLOOR_CONVEX (the floor plane against the fly's ellipsoids and cylinders) is "
                               "accepted only as FFE_NO_CONTACT | FFE_WALK_JOINT_LIMITS | FFE_WALK_FLOOR | FFE_WALK_SELF | FFE_WALK_FLOOR_CONVEX "
                               "(bare physics) or as that set | FFE_WALK_EPISODES | FFE_WALK_SELF_EPISODES with the task (the walk_imitation "
                               "environment), each plus the force switches, FFE_NO_NOSLIP and FFE_NO_ADHESION: it excludes FFE_NO_LIMIT");
    if (episodes && !task.task)
      throw std::runtime_error("ffe_create_walk_physics: FFE_WALK_FLOOR_CONVEX with FFE_WALK_EPISODES | FFE_WALK_SELF_EPISODES needs the task (a "
                               "null ffe_walk_task pointer): a handle without one does not carry the episode protocol; without the two bits "
                               "FFE_WALK_FLOOR_CONVEX makes the bare-physics handle");
  } else if (self || self_env) {  // the fly's own contacts: refusals of their own, which the table does not express
    if (episodes && !floor)
      throw std::runtime_error("ffe_create_walk_physics: FFE_WALK_SELF (the fly's own contacts) with FFE_WALK_EPISODES needs FFE_WALK_FLOOR: the "
                               "walk_imitation environment with the floor off does not carry the fly's own contacts");
    if (episodes && !task.task)
      throw std::runtime_error("ffe_create_walk_physics: FFE_WALK_SELF (the fly's own contacts) with FFE_WALK_EPISODES needs the task (a null "
                               "ffe_walk_task pointer): a handle without one does not carry the episode protocol; without FFE_WALK_EPISODES the bit "
                               "makes the bare-physics floor handle");
    if ((physics_flags & ~(kSwitches | BF_WALK_EPISODES | BF_WALK_SELF_EPISODES)) != (BF_NO_CONTACT | BF_WALK_JOINT_LIMITS | BF_WALK_FLOOR | BF_WALK_SELF))
      throw std::runtime_error("ffe_create_walk_physics: FFE_WALK_SELF (the fly's own contacts on the bare-physics floor handle) is accepted only as "
                               "FFE_NO_CONTACT | FFE_WALK_JOINT_LIMITS | FFE_WALK_FLOOR | FFE_WALK_SELF plus the force switches, FFE_NO_NOSLIP and "
                               "FFE_NO_ADHESION, and with FFE_WALK_EPISODES | FFE_WALK_SELF_EPISODES and the task on top of exactly that");
    // FFE_WALK_EPISODES | FFE_WALK_FLOOR | FFE_WALK_SELF alone is a refusal the C ABI contract pins: the environment takes its own bit too
    if (episodes != self_env)
      throw std::runtime_error("ffe_create_walk_physics: FFE_WALK_SELF under the environment (FFE_WALK_EPISODES | FFE_WALK_FLOOR and the task) is asked "
                               "for with FFE_WALK_SELF_EPISODES on top: the three bits without it are refused, and so is FFE_WALK_SELF_EPISODES "
                               "without FFE_WALK_EPISODES | FFE_WALK_FLOOR | FFE_WALK_SELF");
  } else {
    const WalkKind *kind = kWalkKinds;
    while ((physics_flags & kind->key_mask) != kind->key) kind++;  // (the last kind's mask is empty: it takes what is left)
    if ((physics_flags & ~kind->switches) != kind->bits) throw std::runtime_error(kind->bad_flags);
    if (kind->task && !task.task) throw std::runtime_error(kind->no_task);
  }
  std::unique_ptr<WalkEnv> e(new WalkEnv());  // frees the device allocations made so far if a later step throws
  Blob b(blob, blob_size);
  e->host = build_walk_model(b);
  e->device = device; e->batch = batch; e->flags = physics_flags & ~(BF_WALK_EPISODES | BF_WALK_SELF_EPISODES); e->limits = limits; e->episodes = episodes; e->floor = floor; e->self = self;
  if (self) build_walk_self(b, e->host);  // (before the model goes to the device)
  if (floor && !e->host.m.x.f_ok)
    throw std::runtime_error("ffe_create_walk_physics: FFE_WALK_FLOOR: the floor's contacts are expected to be condim 3 with one solimp");
  if (convex) {
    build_walk_floor_convex(b, e->host);
    if (!e->host.xc.ok)
      throw std::runtime_error("ffe_create_walk_physics: FFE_WALK_FLOOR_CONVEX: the floor's contacts with the ellipsoids and cylinders are expected to "
                               "be condim 3 with the solimp of its other contacts");
  }
  e->host.m.b.nsub = 10;  // the reference's control step of 2 ms over the model's 0.2 ms (bare physics: ffe_spec's figure alone)
  // one place decides the allocation, from `convex` alone and before any kernel is chosen: every launch of a kernel with the second
  // floor pass goes through `full_dev`, whose type a plain WalkModel allocation does not have
  if (convex) {
    e->full_dev = e->mem.zeroed<WalkModelFull>(1);
    e->model_dev = &e->full_dev->m;
    HIP_OK(hipMemcpy(&e->full_dev->xc, &e->host.xc, sizeof(WalkFloorConvex), hipMemcpyHostToDevice));
  } else {
    e->model_dev = e->mem.zeroed<WalkModel>(1);
  }
  HIP_OK(hipMemcpy(e->model_dev, &e->host.m, sizeof(WalkModel), hipMemcpyHostToDevice));
  e->states = e->mem.zeroed<WState>((size_t)batch);
  hipLaunchKernelGGL(walk_init_states, dim3(batch), dim3(64), 0, 0, e->states, e->model_dev, batch);
  HIP_OK(hipGetLastError());
  if (floor) e->rec = e->mem.zeroed<FloorRec>((size_t)batch);
  if (episodes) make_episodes(*e, b, blob, blob_size, task);
  HIP_OK(hipDeviceSynchronize());
  return e;
}

}  // namespace ffw
