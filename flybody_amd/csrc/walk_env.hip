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
// Collision, contact and limit rows, the constraint solver, sensors, observation, reward and reset are not compiled into this
// kernel: only bare physics (`ffe_physics_step`) exists, and a handle is only created with FFE_NO_CONTACT | FFE_NO_LIMIT.
// Parity tests: tests/test_gpu_walk_physics.py.
#include <hip/hip_runtime.h>

#include <cmath>
#include <memory>
#include <stdexcept>
#include <string>

#include "walk_env.hpp"
#include "walk_model.hpp"
#include "leg_dyn.hpp"

namespace ffw {
using namespace dm;
using namespace ffb;

// State record of the free-root handle (the tethered handle's BState is untouched).  MuJoCo's free-joint conventions: position and
// linear velocity in the world frame, angular velocity in the body frame.
struct alignas(16) WState {
  double pos[3];
  float quat[4];
  float vlin[3], wb[3];
  float q[NDP], v[NDP], act[64];
  int pad[2];
};

struct alignas(16) WTile {
  union {
    struct { float Q[NDP], V[NDP]; };  // joint state staged for the actuators (start of stage 2)
    float4 X4[NDP];                     // right-hand sides / solutions of the block solves
  };
  float dadd[NDP];                      // h * damping: only read by the stage-1 factorisation
  float Mq[NMMAX];                      // joint-space inertia of the hinges: only read by the stage-1 factorisation
  union {
    float F[NDP][6];                    // crb * cdof = the hinge's column of M_rj: written by the assembly, read by stage 2
    float lk[NL][12];                   // link exchange of the tree passes (dead once the assembly starts)
  };
  float Lm[NMMAX], Lh[NMMAX];           // factors of M_jj and of M_jj + h B
  float dinv_m[NDP], dinv_h[NDP];
  float C[NDP][6];
  float frc[64];
  float Y[NDP][6];                      // (M_jj + h B)^-1 M_jr
};
static_assert(sizeof(WTile) <= 20480, "the tile must leave room for 8 waves per CU");

struct Ctx {
  const BallModel *M;
  const WalkExtra FFE_GLOBAL *X;
  WTile *T;
  int lane, flags;
  unsigned lpack;
  int sdof[3];
  float q[3], v[3], fnb[3];
  int xh;
  V3 xp, xip;
  Q4 xq;
  S6 cvel, caccb;
  float mass;
  // root
  Q4 rq;        // orientation
  V3 vw, wb;    // linear velocity in the world frame, angular velocity in the body frame
  double pos[3];
  S6 V0;        // (w_b, R' v_w)
  I10 Itree;    // spatial inertia of the whole tree about the root origin = M_rr
  S6 Ftot;      // bias force of the whole tree without gravity = -(root rows of the smooth force)
};

// ------------------------------------------------------------------------------------------------ stage 1
template <class C>  // (a template so that the fragment's tethered branches are discarded, not compiled)
__device__ __forceinline__ void stage1(C &c) {
  constexpr bool FREE_ROOT = true;
  WTile &T = *c.T;
  const BallModel FFE_GLOBAL &M = model(c);
  {
    const M3 R = q2m(c.rq);
    c.V0 = mk6(c.wb, mtv(R, c.vw));
  }
#include "leg_stage1.inc"
  (void)xmat;
  // the root link itself: uniform across the wave
  {
    const WalkExtra FFE_GLOBAL &X = *c.X;
    const I10 I0 = {X.r_cin[0], X.r_cin[1], X.r_cin[2], X.r_cin[3], X.r_cin[4], X.r_cin[5], X.r_cin[6], X.r_cin[7], X.r_cin[8], X.r_cin[9]};
    S6 f0 = cross_force(c.V0, mul_inert(I0, c.V0));
    if (!(c.flags & BF_NO_FLUID)) {
      float fl[8];
#pragma unroll
      for (int k = 0; k < 8; k++) fl[k] = X.r_fl[k];
      f0 = f0 - box_drag(fl, q2m(Q4{X.r_iquat[0], X.r_iquat[1], X.r_iquat[2], X.r_iquat[3]}), V3{X.r_ipos[0], X.r_ipos[1], X.r_ipos[2]}, c.V0);
    }
    c.Itree = add10(c.Itree, I0);
    c.Ftot = c.Ftot + f0;
  }
}

// ------------------------------------------------------------------------------------------------ stage 2
template <class C>
__device__ __forceinline__ void stage2(C &c, float act_reg, float ctrl_reg, float &act_out) {
  WTile &T = *c.T;
  const BallModel FFE_GLOBAL &M = model(c);
  const int lane = c.lane;
  const float h = M.h;
#pragma unroll
  for (int s = 0; s < 3; s++) if (slot_on(c, s)) { T.Q[opq(c.sdof[s])] = c.q[s]; T.V[opq(c.sdof[s])] = c.v[s]; }
  DM_SYNC();
  // ---- mj: mj_fwdActuation: first-order activation filter, affine position servo on the activation (as ball_env.hip; an adhesion
  //      actuator has nothing to pull on without contacts)
  float act_dot = 0.f;
  if (lane < NU) {
    float force = 0.f;
    if (!(c.flags & BF_NO_ACTUATION)) {
      float ctrl = ctrl_reg;
      if (M.a_climited[lane]) ctrl = fminf(fmaxf(ctrl, M.a_clo[lane]), M.a_chi[lane]);
      act_dot = (ctrl - act_reg) * frcp(M.a_tau[lane]);
      float length = 0.f, vel = 0.f;
      const int nw = M.a_nwrap[lane];
      for (int w = 0; w < nw; w++) { const int f = M.a_wdof[w][lane]; const float cf = M.a_wcoef[w][lane]; length += cf * T.Q[f]; vel += cf * T.V[f]; }
      force = M.a_gain[lane] * act_reg + M.a_b0[lane] + M.a_b1[lane] * length + M.a_b2[lane] * vel;
      if (M.a_flimited[lane]) force = fminf(fmaxf(force, M.a_flo[lane]), M.a_fhi[lane]);
    }
    T.frc[lane] = force;
  }
  act_out = act_reg + h * act_dot;
  DM_SYNC();
  // ---- smooth forces of the hinges (mj: mj_fwdAcceleration's right-hand side)
  float qs[3];
#pragma unroll
  for (int s = 0; s < 3; s++) {
    qs[s] = 0.f;
    if (slot_on(c, s)) {
      float f = c.fnb[s];
      const int a0 = M.s_act[0][s][lane], a1 = M.s_act[1][s][lane];
      if (a0 >= 0) f += M.s_actcoef[0][s][lane] * T.frc[a0];
      if (a1 >= 0) f += M.s_actcoef[1][s][lane] * T.frc[a1];
      qs[s] = f;
    }
  }
  // ---- z = A^-1 f_j and Y = A^-1 M_jr, A = M_jj + h B: seven right-hand sides through two four-wide block solves.  M_jr's column of
  //      hinge f is T.F[f] (the 6-vector crb * cdof of the assembly: the root's motion axes are the unit vectors of this frame).
  S6 mrj[3], y[3];
  float z[3];
#pragma unroll
  for (int s = 0; s < 3; s++) mrj[s] = slot_on(c, s) ? ld6(T.F[opq(c.sdof[s])]) : zero6();
  DM_SYNC();  // (Q / V have been read: X4 lies over them)
#pragma unroll
  for (int s = 0; s < 3; s++) if (slot_on(c, s)) T.X4[opq(c.sdof[s])] = make_float4(qs[s], mrj[s].a0, mrj[s].a1, mrj[s].a2);
  DM_SYNC();
  solve4(c, T.Lh, T.dinv_h);
#pragma unroll
  for (int s = 0; s < 3; s++) {
    const float4 x = slot_on(c, s) ? T.X4[opq(c.sdof[s])] : make_float4(0.f, 0.f, 0.f, 0.f);
    z[s] = x.x; y[s].a0 = x.y; y[s].a1 = x.z; y[s].a2 = x.w;
  }
  DM_SYNC();
#pragma unroll
  for (int s = 0; s < 3; s++) if (slot_on(c, s)) T.X4[opq(c.sdof[s])] = make_float4(mrj[s].l0, mrj[s].l1, mrj[s].l2, 0.f);
  DM_SYNC();
  solve4(c, T.Lh, T.dinv_h);
#pragma unroll
  for (int s = 0; s < 3; s++) {
    const float4 x = slot_on(c, s) ? T.X4[opq(c.sdof[s])] : make_float4(0.f, 0.f, 0.f, 0.f);
    y[s].l0 = x.x; y[s].l1 = x.y; y[s].l2 = x.z;
  }
  DM_SYNC();
#pragma unroll
  for (int s = 0; s < 3; s++) if (slot_on(c, s)) st6(T.Y[opq(c.sdof[s])], y[s]);  // kept for the constraint rows of step 3 (rank-6 term of G)
  // ---- Schur complement S = M_rr - M_rj Y and right-hand side f_r - M_rj z: wave sums of the lanes' own hinges
  auto comp = [](const S6 &v, int k) { return k == 0 ? v.a0 : (k == 1 ? v.a1 : (k == 2 ? v.a2 : (k == 3 ? v.l0 : (k == 4 ? v.l1 : v.l2)))); };
  float Sm[6][6], br[6];
  {
    // M_rr from the tree's spatial inertia: column k = I e_k
#pragma unroll
    for (int k = 0; k < 6; k++) {
      const S6 e = {k == 0 ? 1.f : 0.f, k == 1 ? 1.f : 0.f, k == 2 ? 1.f : 0.f, k == 3 ? 1.f : 0.f, k == 4 ? 1.f : 0.f, k == 5 ? 1.f : 0.f};
      const S6 col = mul_inert(c.Itree, e);
#pragma unroll
      for (int r = 0; r < 6; r++) Sm[r][k] = comp(col, r);
    }
#pragma unroll
    for (int a = 0; a < 6; a++) {
#pragma unroll
      for (int b = 0; b <= a; b++) {
        float p = 0.f;
#pragma unroll
        for (int s = 0; s < 3; s++) p += comp(mrj[s], a) * comp(y[s], b);
        Sm[a][b] -= wave_sum(p);
      }
      float p = 0.f;
#pragma unroll
      for (int s = 0; s < 3; s++) p += comp(mrj[s], a) * z[s];
      br[a] = -comp(c.Ftot, a) - wave_sum(p);
    }
  }
  // ---- 6 x 6 Cholesky S = L L' (lower triangle, in registers, uniform), x_r = S^-1 b_r
  float xr[6];
  {
    float id[6];
#pragma unroll
    for (int j = 0; j < 6; j++) {
      float d = Sm[j][j];
#pragma unroll
      for (int k = 0; k < j; k++) d -= Sm[j][k] * Sm[j][k];
      const float r = __builtin_amdgcn_rsqf(d);
      const float ir = r * (1.5f - 0.5f * d * r * r);  // 1 / sqrt(d), one Newton step
      id[j] = ir;
      Sm[j][j] = d * ir;
#pragma unroll
      for (int i = j + 1; i < 6; i++) {
        float e = Sm[i][j];
#pragma unroll
        for (int k = 0; k < j; k++) e -= Sm[i][k] * Sm[j][k];
        Sm[i][j] = e * ir;
      }
    }
#pragma unroll
    for (int i = 0; i < 6; i++) {  // L w = b
      float w = br[i];
#pragma unroll
      for (int k = 0; k < i; k++) w -= Sm[i][k] * xr[k];
      xr[i] = w * id[i];
    }
#pragma unroll
    for (int i = 5; i >= 0; i--) {  // L' x = w
      float w = xr[i];
#pragma unroll
      for (int k = i + 1; k < 6; k++) w -= Sm[k][i] * xr[k];
      xr[i] = w * id[i];
    }
  }
  // ---- back substitution of the hinges, integration (mj: mj_Euler, implicit in the joint damping)
#pragma unroll
  for (int s = 0; s < 3; s++) {
    if (slot_on(c, s)) {
      float a = z[s];
#pragma unroll
      for (int k = 0; k < 6; k++) a -= comp(y[s], k) * xr[k];
      c.v[s] += h * a;
      c.q[s] += h * c.v[s];
    }
  }
  {
    // free joint: qacc = (R (vdot_b + w_b x v_b) + g, wdot_b), gravity added here (see the head of this file); mj_integratePos: position with the new velocity, quaternion by mju_quatIntegrate
    const M3 R = q2m(c.rq);
    const V3 wd = {xr[0], xr[1], xr[2]}, vd = {xr[3], xr[4], xr[5]};
    V3 aw = mv(R, vd + cross(ang(c.V0), lin(c.V0)));
    if (!(c.flags & BF_NO_GRAVITY)) aw.z += M.gz;
    c.vw = c.vw + h * aw;
    c.wb = c.wb + h * wd;
    c.pos[0] += (double)h * (double)c.vw.x; c.pos[1] += (double)h * (double)c.vw.y; c.pos[2] += (double)h * (double)c.vw.z;
    const float wn = fsqrt(dot(c.wb, c.wb));
    Q4 q = qnormalize(c.rq);
    if (wn >= 1e-15f) q = qnormalize(qmul(q, axis_angle(frcp(wn) * c.wb, wn * h)));
    c.rq = q;
  }
}

// ------------------------------------------------------------------------------------------------ kernel
__global__ __launch_bounds__(64, 2) void walk_step_kernel(const WalkModel *__restrict__ Wp, int flags, WState *__restrict__ states,
                                                         const float *__restrict__ ctrl, int batch, int nphys) {
  const int env = blockIdx.x, lane = threadIdx.x;
  if (env >= batch) return;
  __shared__ WTile T;
  const BallModel &M = Wp->b;
  WState &S = states[env];
  Ctx c;
  c.M = &Wp->b; c.X = (const WalkExtra FFE_GLOBAL *)&Wp->x; c.T = &T; c.lane = lane; c.flags = flags;
  c.lpack = M.l_pack[lane]; c.xh = M.x_on[lane];
#pragma unroll
  for (int s = 0; s < 3; s++) c.sdof[s] = M.s_dof[s][lane];
#pragma unroll
  for (int s = 0; s < 3; s++) { c.q[s] = slot_on(c, s) ? S.q[c.sdof[s]] : 0.f; c.v[s] = slot_on(c, s) ? S.v[c.sdof[s]] : 0.f; }
  c.rq = {S.quat[0], S.quat[1], S.quat[2], S.quat[3]};
  c.vw = {S.vlin[0], S.vlin[1], S.vlin[2]}; c.wb = {S.wb[0], S.wb[1], S.wb[2]};
  c.pos[0] = S.pos[0]; c.pos[1] = S.pos[1]; c.pos[2] = S.pos[2];
  float act_reg = lane < NU ? S.act[lane] : 0.f;
  const float ctrl_reg = lane < NU ? ctrl[(size_t)env * NU + lane] : 0.f;
#pragma unroll 1
  for (int s = 0; s < nphys; s++) {
    stage1(c);
    float act_new;
    stage2(c, act_reg, ctrl_reg, act_new);
    act_reg = act_new;
  }
#pragma unroll
  for (int s = 0; s < 3; s++) if (slot_on(c, s)) { S.q[c.sdof[s]] = c.q[s]; S.v[c.sdof[s]] = c.v[s]; }
  if (lane < NU) S.act[lane] = act_reg;
  if (lane == 0) {
    S.quat[0] = c.rq.w; S.quat[1] = c.rq.x; S.quat[2] = c.rq.y; S.quat[3] = c.rq.z;
    S.vlin[0] = c.vw.x; S.vlin[1] = c.vw.y; S.vlin[2] = c.vw.z;
    S.wb[0] = c.wb.x; S.wb[1] = c.wb.y; S.wb[2] = c.wb.z;
    S.pos[0] = c.pos[0]; S.pos[1] = c.pos[1]; S.pos[2] = c.pos[2];
  }
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
    S.pad[0] = S.pad[1] = 0;
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
// Bare physics is all that is built: reset, step, forced episodes and the timers are refused.
struct WalkEnv final : ffe::EnvBackend {
  int flags = 0;
  WalkHost host;
  WalkModel *model_dev = nullptr;
  WState *states = nullptr;

  ~WalkEnv() override {
    (void)hipFree(model_dev); (void)hipFree(states);
  }

  [[noreturn]] void refuse(const char *what) const override {
    throw ffe::Refused(std::string(what) + ": not available on a walk physics handle (bare physics only: limits, floor contacts, sensors and the episode protocol are not built yet)");
  }

  void spec(ffe_spec_t &s) const override {  // no observation row: every offset is -1
    s = ffe_spec_t{};
    s.batch = batch; s.nq = host.nq; s.nv = host.nv; s.nu = NU; s.action_dim = NACT; s.obs_dim = 0; s.nsub = host.m.b.nsub;
    s.physics_timestep = host.m.b.h; s.control_timestep = (double)host.m.b.nsub * (double)host.m.b.h;
    s.off_accelerometer = s.off_gyro = s.off_joints_pos = s.off_joints_vel = s.off_velocimeter = s.off_world_zaxis = -1;
    s.off_ref_displacement = -1; s.off_ref_root_quat = -1;
  }
  void action_bounds(float *mn, float *mx) const override {
    for (int k = 0; k < NACT; k++) { mn[k] = host.action_min[k]; mx[k] = host.action_max[k]; }
  }
  void launch(const float *ctrl, float *, float *, float *, int32_t *, void *stream, int mode, int nphys, const uint8_t *) override {  // ctrl[B][59]
    if (mode != 2) refuse("ffe_reset / ffe_reset_envs / ffe_step");
    if (!ctrl || nphys <= 0) throw std::runtime_error("walk physics: null control buffer or no steps");
    hipLaunchKernelGGL(walk_step_kernel, dim3(batch), dim3(64), 0, (hipStream_t)stream, model_dev, flags, states, ctrl, batch, nphys);
    HIP_OK(hipGetLastError());
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
  void get_task_state(int32_t *ints, double *reals, void *stream) override {  // int32[B][8] and float64[B][8]: zeros
    HIP_OK(hipMemsetAsync(ints, 0, sizeof(int32_t) * 8 * (size_t)batch, (hipStream_t)stream));
    HIP_OK(hipMemsetAsync(reals, 0, sizeof(double) * 8 * (size_t)batch, (hipStream_t)stream));
  }
  void get_validity(int32_t *info, void *stream) override {  // int32[B][4]: zeros
    HIP_OK(hipMemsetAsync(info, 0, sizeof(int32_t) * 4 * (size_t)batch, (hipStream_t)stream));
  }
};

std::unique_ptr<ffe::EnvBackend> walk_create(const void *blob, size_t blob_size, int physics_flags, int batch, int device) {
  if (!blob || batch <= 0) throw std::runtime_error("ffe_create_walk_physics: bad arguments");
  if ((physics_flags & (BF_NO_CONTACT | BF_NO_LIMIT)) != (BF_NO_CONTACT | BF_NO_LIMIT))
    throw std::runtime_error("ffe_create_walk_physics: floor contacts and joint limits are not built yet: physics_flags must contain FFE_NO_CONTACT | FFE_NO_LIMIT");
  std::unique_ptr<WalkEnv> e(new WalkEnv());  // frees the device allocations made so far if a later step throws
  Blob b(blob, blob_size);
  e->host = build_walk_model(b);
  e->device = device; e->batch = batch; e->flags = physics_flags;
  e->host.m.b.nsub = 10;  // ffe_spec's figure: the reference's control step of 2 ms over the model's 0.2 ms (nothing here steps by it)
  HIP_OK(hipMalloc((void **)&e->model_dev, sizeof(WalkModel)));
  HIP_OK(hipMemcpy(e->model_dev, &e->host.m, sizeof(WalkModel), hipMemcpyHostToDevice));
  HIP_OK(hipMalloc((void **)&e->states, sizeof(WState) * (size_t)batch));
  hipLaunchKernelGGL(walk_init_states, dim3(batch), dim3(64), 0, 0, e->states, e->model_dev, batch);
  HIP_OK(hipGetLastError());
  HIP_OK(hipDeviceSynchronize());
  return e;
}

}  // namespace ffw
