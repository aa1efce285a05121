// ball_env.hip - MI355X (gfx950) batched walk_on_ball environment (ref: fly_envs.py:125-157, tasks/walk_on_ball.py).
//
// ONE 64-lane wavefront per environment, one launch = one control step (10 physics substeps of 2e-4 s, dm_control's
// legacy mj_step2;mj_step1 order, buffered sensors, observation, reward, termination, auto-reset).  Lane mapping and
// the model tables are described in ball_model.hpp.  Per substep (mj: mj_step restated):
//   stage 1  kinematics, velocities / bias accelerations (root-to-leaf passes by pointer jumping), spatial inertias about the
//            fixed thorax origin, inertia-box drag, composite inertias and subtree forces (gathers over depth-first lane
//            ranges), joint-space inertia (582 entries across the lanes), block factorisation of M and M + hB together,
//            ball-capsule collision;
//   stage 2  filtered actuators (+ adhesion through the contact normals), smooth acceleration, joint-limit and
//            elliptic-cone contact rows, the constraint solve in the space of those rows (G = J M^-1 J' from block solves,
//            the dense Newton of row_newton.hpp with the exact cone Hessian in registers, lane = row, noslip sweeps on the same G),
//            touch / force sensors, implicit-in-damping Euler integration.
// Parity tests: tests/test_gpu_ball.py.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <memory>
#include <stdexcept>
#include <vector>

#include "ball_env.hpp"
#include "launch_order.hpp"
#include "ball_model.hpp"
#include "dev_math.hpp"
#include "convex.hpp"

namespace ffb {
using namespace dm;

#ifdef FFB_STAMPS
__device__ unsigned long long g_bstamps[24];
#define BSTAMP(k) do { const unsigned long long t_ = __builtin_amdgcn_s_memtime(); c.st_acc[k] += t_ - c.st_t0; c.st_t0 = t_; } while (0)
#else
#define BSTAMP(k) do { } while (0)
#endif
// Diagnostic build only (-DFFE_TRACE): start / end shader clock and hardware slot of every wave of the last launch (tools/wave_timeline.py)
#ifdef FFE_TRACE
__device__ unsigned long long g_btrace[32768][4];
#endif

struct alignas(16) BState {
  float q[NDP], v[NDP], act[64];
  float ballq[4], ballw[4];
  float qacc_ws[NDP], wsc[NL][3];  // warm start of the constraint solver: last limit force per dof, last contact force per link
  int step_counter, needs_reset, overflow, iters, ncon, have_ws, nself;
  int step_bits;  // validity (ffe_get_validity): the overflow bits of the last launch alone (`overflow` is their OR over the episode)
  unsigned con_hist[2];  // active (inside includemargin) contacts of each of the control step's first 16 substeps, 4 bits each: parity tooling
  unsigned det_hist[2];  // detected (inside margin) contacts of its first 12 substeps, 5 bits each
  float sd_n[NSD][4];    // separating-direction cache of the convex pairs (convex_pairs)
  unsigned short sd_pid[NSD];
  int sd_cnt, ws_n;
  int ep_flagged, pad2;  // control steps of the current episode whose launch raised an overflow bit
  float ws_f[NC];        // forces of the fly-fly contacts of the last substep, by pair id (warm start)
  unsigned short ws_pid[NC];
};

struct BTaskDev {
  int time_limit_steps, pad_first_obs, flags, canonical, clip;
};

struct alignas(16) BTile {
  // One scratch region, used by the phases of a substep in turn (7 488 B):
  //   stage 1:    X4 / dadd / Mq (inertia, factorisation), F then lk (assembly, tree passes)
  //   collision:  gc / gq / lp (geom frames, link poses) over the dead X4 .. Mq; primitive geom slots + the pair list in lk
  //   stage 2:    Q, V / X4 (block solves) | G over the dead Mq and lk | Newton: S over everything (G is in registers by then)
  union {
    struct {
      union {
        struct { float Q[NDP], V[NDP]; };  // joint state staged for the actuators / contact rows (start of stage 2) and the observation
        float4 X4[NDP];                     // right-hand sides / solutions of the block solves
      };
      float dadd[NDP];                      // h * damping: only read by the stage-1 factorisation
      union {
        struct {
          float Mq[NMMAX];                  // joint-space inertia: only read by the stage-1 factorisation
          union {
            float F[NDP][6];                // crb * cdof during the inertia assembly
            float lk[NL][12];               // link exchange of the tree passes: pose (7) | motion vector (6) | crb (10) | force (6)
            struct { float pg[NPG * 9]; unsigned short cl1[CL1], cl2[CL2], tc_pid[NSD]; float tc_n[NSD][4], cl2n[CL2][5]; };  // collision: primitive geom slots, pair lists, next cache
          };
        };
        float G[RMAX * (RMAX + 1) / 2];     // stage 2: G = J M^-1 J' over the constraint rows, lower triangle packed by rows (lane r owns row r)
      };
    };
    float S[RMAX * (RMAX + 1) / 2];         // Newton: the factor of I + L' G L, transposed through here (packed lower triangle)
    struct { float4 gc[NG], gq[NG]; float lp[NL][8]; };  // collision: geom centre | bounding radius, geom quaternion; link pose
  };
  float Lm[NMMAX], Lh[NMMAX];               // factors of M and of M + h B (Euler), made together in stage 1
  float dinv_m[NDP], dinv_h[NDP];
  float C[NDP][6];
  float frc[64];
  int c_link[NC], c_blk[NC], c_excl[NC], c_nch[NC], c_adh[NC];
  unsigned c_amask[NC], c_bmask[NBLK];  // c_bmask[b]: contacts whose chain lies in block b
  unsigned char c_chain[NC][16];
  float c_par[NC][5];  // K, B, invweight, friction, includemargin
  float c_pos[NC][3], c_frame[NC][9], c_dist[NC];
  float c_D[NC], c_mu[NC], c_aref[NC][3], c_f[NC][3], c_w[NC][3];
  // constraint rows: 3 per contact (normal, two tangents), then the instantiated joint limits
  float r_y0[RMAX], r_lam[RMAX], r_f[RMAX];
  float r_sgn[RMAX], r_D[RMAX];
  unsigned char r_blk[RMAX], r_col[RMAX], r_dof[RMAX], rowof[NBLK][KCOL];
  float sens[24];  // running sums of the buffered sensors: force 18, touch 6
  // separating directions of the convex pairs that reached the narrow phase, kept from substep to substep (convex_pairs)
  float sd_n[NSD][4];  // direction | the capsule's axis parameter of a capsule - convex pair
  unsigned short sd_pid[NSD];
  int sd_cnt;
  // fly-fly contacts: pair id of each slot, and the pairs' forces of the last substep (warm start of their rows)
  unsigned short c_pid[NC], ws_pid[NC];
  float ws_f[NC];
  int ws_n;
};

// ------------------------------------------------------------------------------------------------ per-lane context
// Only what must survive between the stages lives here; model constants are re-read from the (L2-resident) tables
// where they are used, through a laundered pointer so the compiler does not hoist them back into registers.
struct Ctx {
  const BallModel *M;
  BTile *T;
  int lane, flags;
  unsigned lpack;         // parent + 1 | depth << 8 | ndof << 12
  int sdof[3];
  unsigned sbl[3];        // block | local index << 8 of each slot's dof
  float q[3], v[3], fnb[3];
  int xh;                 // this lane carries a haltere in slot 2 (closed-form single hinge, see ball_model.hpp)
  V3 xp, xip;
  Q4 xq;
  S6 cvel, caccb;         // link velocity and bias acceleration (gravity + velocity products) about the thorax origin
  float mass;
  Q4 bq;
  V3 bw, btau;
  int nc, nact;           // ball contacts detected / of those, the ones inside includemargin (they get constraint rows)
  int nsc;                // fly-fly contacts of this substep: slots nc .. nc + nsc - 1 of the contact arrays (see prim_pairs)
  int ndrop;              // detected fly-fly contacts without a slot (inactive, no adhesion actuator involved)
  float wsl[3], wsc[3];   // warm start of the constraint solver: last substep's limit force per slot, contact force of this link
  int have_ws, overflow;
#ifdef FFB_STAMPS
  unsigned long long st_t0, st_acc[24];
#endif
};


}  // namespace ffb

#include "leg_dyn.hpp"  // BF_* flags, slot_on / l_parent / l_ndof / model, impedance, factor2 / solve4 / solve_dual
#include "row_newton.hpp"  // the constraint solve (row_newton<RB, ConeRows>), cone_force, qcqp2
#include "self_pairs.hpp"  // prim_pairs, convex_pairs, load_geom

namespace ffb {


// ------------------------------------------------------------------------------------------------ fly-fly collision
// The two passes of self_pairs.hpp on the ball's tile.  The primitive geom slots are in T.lk (stage 1 publishes them), the geom frames in
// T.gc / T.gq (`ball_convex` makes them), the pair lists beside the slots; the convex pass keeps its separating directions in T.sd_*.
struct BallPairs {
  static constexpr bool kSyncAtEnd = false, kHistory = true;
  static constexpr int kFullBit = 8;
  static __device__ __forceinline__ const float4 *slots(const BTile &T) { return reinterpret_cast<const float4 *>(&T.lk[0][0]); }
  static __device__ __forceinline__ const float *radii(const BTile &T) { return reinterpret_cast<const float *>(slots(T) + 2 * NPG); }
  static __device__ __forceinline__ const float4 *centres(const BTile &T) { return T.gc; }
  static __device__ __forceinline__ Q4 quat(const BTile &T, const BallModel FFE_GLOBAL &, int g) { const float4 qq = T.gq[g]; return Q4{qq.x, qq.y, qq.z, qq.w}; }
  static __device__ __forceinline__ unsigned short *cl1(BTile &T) { return T.cl1; }
  static __device__ __forceinline__ unsigned short *cl2(BTile &T) { return T.cl2; }
  __device__ __forceinline__ void fill_slots(BTile &, int) const {}                                     // (stage 1 has made them)
  static __device__ __forceinline__ void fill_centres(BTile &, const BallModel FFE_GLOBAL &, int) {}  // (`ball_convex` has)
  // A fly-fly contact in the layout of the ball contacts' arrays: c_link = link of geom1 | link of geom2 << 8, c_frame[0..2] = normal from
  // geom1 to geom2, c_par = {K, B, invweight, 0, margin - gap}.  A geom of the thorax (fixed to the world) has no link: the moving
  // geom's link is stored first and the normal turned, so that it still points from the first link's geom to the second's.
  static __device__ __forceinline__ void put(BTile &T, const BallModel FFE_GLOBAL &M, int at, int la, int lb, int pid, V3 nrm, V3 cpos, float dist, float margin, float invw) {
    if (la < 0) { la = lb; lb = 255; nrm = V3{-nrm.x, -nrm.y, -nrm.z}; }
    else if (lb < 0) lb = 255;
    const float incl = margin - (margin != 0.f ? M.sc_gap : 0.f);
    T.c_link[at] = la | (lb << 8);
    T.c_pid[at] = (unsigned short)pid;
    T.c_excl[at] = dist >= incl ? 1 : 0;
    T.c_dist[at] = dist;
    T.c_pos[at][0] = cpos.x; T.c_pos[at][1] = cpos.y; T.c_pos[at][2] = cpos.z;
    T.c_frame[at][0] = nrm.x; T.c_frame[at][1] = nrm.y; T.c_frame[at][2] = nrm.z;
    T.c_par[at][0] = M.sc_K; T.c_par[at][1] = M.sc_B; T.c_par[at][2] = invw; T.c_par[at][3] = 0.f;
    T.c_par[at][4] = incl;
  }
};

// ------------------------------------------------------------------------------------------------ convex pairs
// mj: mjc_Convex for the pairs with an ellipsoid or a cylinder on one side (thorax, head, rostrum, labrum, wings, coxae, abdomen
// segments; fruitfly.xml:323-443), restated in csrc/convex.hpp.  The geoms' world frames are made once per substep from the link
// poses the lanes publish (`T.lp`) into `T.gc` (centre | bounding radius) / `T.gq` (orientation).
//
// Ball (geom1, a sphere) against the ellipsoids / cylinders that can reach it (abdomen segments: mjc_SphereCylinder; labrum, wings:
// the sphere's centre against the ellipsoid's signed distance): condim-3 ball contacts like the leg capsules', appended to the
// `nc0` ball contacts stage 1 has just stored.  Also makes the geom frames for `convex_pairs`.  Returns the number appended
// | overflow << 8.
__device__ __noinline__ int ball_convex(BTile *Tp, ModelPtr Mp, const int lane, const int nc0) {
  BTile &T = *Tp;
  const BallModel FFE_GLOBAL &M = *Mp;
  const int ncg = M.ncg;
  for (int g = lane; g < ncg; g += 64) {
    const int l = M.cg_link[g];
    V3 gp = {M.cg_pos[0][g], M.cg_pos[1][g], M.cg_pos[2][g]};
    Q4 gq = {M.cg_quat[0][g], M.cg_quat[1][g], M.cg_quat[2][g], M.cg_quat[3][g]};
    if (l >= 0) {
      const float *lp = T.lp[l];
      const Q4 xq = {lp[3], lp[4], lp[5], lp[6]};
      gp = V3{lp[0], lp[1], lp[2]} + qrot(xq, gp);
      gq = qnormalize(qmul(xq, gq));
    }
    T.gc[g] = make_float4(gp.x, gp.y, gp.z, M.cg_brad[g]);
    T.gq[g] = make_float4(gq.w, gq.x, gq.y, gq.z);
  }
  DM_SYNC();
  bool hit = false;
  float dist = 0.f, incl = 0.f;
  V3 nrm = {1.f, 0.f, 0.f}, cpos = {0.f, 0.f, 0.f};
  const int nxb = M.nxb;
  int g = 0;
  if (lane < nxb) {
    g = M.xb_geom[lane];
    const cvx::Geom ball = {V3{M.b_center[0], M.b_center[1], M.b_center[2]}, Q4{1.f, 0.f, 0.f, 0.f}, M.b_radius, 0.f, 0.f, cvx::SPHERE};
    const float4 cc = T.gc[g];
    const float dx = cc.x - ball.c.x, dy = cc.y - ball.c.y, dz = cc.z - ball.c.z, reach = M.b_radius + cc.w + M.xb_margin[lane];
    if (dx * dx + dy * dy + dz * dz <= reach * reach) {  // mj: the bounding-sphere test of mj_collision
      const cvx::PResult r = cvx::prim_convex<1>(ball, load_geom<BallPairs>(T, M, g));
      dist = r.dist; nrm = r.n; cpos = r.pos;
      hit = dist <= M.xb_margin[lane];
      incl = M.xb_margin[lane] - M.xb_gap[lane];
    }
  }
  const unsigned long long bal = __ballot(hit);
  const int n = __popcll(bal), idx = nc0 + __popcll(bal & ((1ull << lane) - 1ull));
  if (hit && idx < NC) {
    const int link = M.cg_link[g], nch = M.l_nchain[link], last = M.l_chain[nch - 1][link];
    T.c_link[idx] = link;
    T.c_blk[idx] = M.d_blk[last]; T.c_amask[idx] = M.d_amask[last];
    T.c_excl[idx] = dist >= incl ? 1 : 0;
    T.c_dist[idx] = dist;
    T.c_pos[idx][0] = cpos.x; T.c_pos[idx][1] = cpos.y; T.c_pos[idx][2] = cpos.z;
    T.c_nch[idx] = nch;
    for (int p = 0; p < NCH; p++) T.c_chain[idx][p] = (unsigned char)(p < nch ? M.l_chain[p][link] : 0);
    T.c_par[idx][0] = M.xb_K[lane]; T.c_par[idx][1] = M.xb_B[lane]; T.c_par[idx][2] = M.xb_invw[lane]; T.c_par[idx][3] = M.xb_fric[lane];
    T.c_par[idx][4] = incl;
    T.c_adh[idx] = M.l_adh[link];
    V3 t1 = (nrm.y < 0.5f && nrm.y > -0.5f) ? V3{0.f, 1.f, 0.f} : V3{0.f, 0.f, 1.f};  // mj: mju_makeFrame
    t1 = t1 - dot(nrm, t1) * nrm;
    t1 = frcp(fsqrt(dot(t1, t1))) * t1;
    const V3 t2 = cross(nrm, t1);
    float *fr = T.c_frame[idx];
    fr[0] = nrm.x; fr[1] = nrm.y; fr[2] = nrm.z; fr[3] = t1.x; fr[4] = t1.y; fr[5] = t1.z; fr[6] = t2.x; fr[7] = t2.y; fr[8] = t2.z;
  }
  DM_SYNC();
  return min(n, NC - nc0) | ((nc0 + n > NC ? 1 : 0) << 8);
}

// Fly-fly contact slots keep the dofs of geom2's chain (14 bytes), and the block-local solve column of that chain (byte 14),
// in the slot's unused ball Jacobian.
__device__ __forceinline__ unsigned char *sc_chain_b(BTile &T, int k) { return reinterpret_cast<unsigned char *>(&T.c_frame[k][3]); }  // (a fly-fly slot uses row 0 of its frame only: 24 spare bytes)
__device__ __forceinline__ const unsigned char *sc_chain_b(const BTile &T, int k) { return reinterpret_cast<const unsigned char *>(&T.c_frame[k][3]); }

// The contact rows' Jacobian entries are evaluated where they are used, from the dof's motion axes (T.C) and the contact's point and
// frame.  As a table (16 contacts x 3 rows x 14 chain dofs, plus the ball's 3 x 3 per contact) they took 3.2 KB of the tile - the
// difference between 6 and 8 resident waves per CU, i.e. between three rounds of waves per launch and two (walk_on_ball +39 %).
// cj_u: velocity of contact k's point per unit rate of fly dof f (about the fixed thorax origin c0).
__device__ __forceinline__ V3 cj_u(const BTile &T, int k, int f, V3 c0) {
  const S6 cd = ld6(T.C[f]);
  const V3 r = V3{T.c_pos[k][0], T.c_pos[k][1], T.c_pos[k][2]} - c0;
  return lin(cd) + cross(ang(cd), r);
}
__device__ __forceinline__ float cj_row(const BTile &T, int k, int r, V3 u) { const float *fr = &T.c_frame[k][3 * r]; return fr[0] * u.x + fr[1] * u.y + fr[2] * u.z; }
// the ball's three entries of row r of ball contact k (geom1 = the ball, rates = its angular velocity in body axes; Rb = its rotation)
__device__ __forceinline__ V3 cj_ball(const BTile &T, int k, int r, const M3 &Rb, V3 bc) {
  const V3 rr = V3{T.c_pos[k][0], T.c_pos[k][1], T.c_pos[k][2]} - bc;
  const float *fr = &T.c_frame[k][3 * r];
  const V3 u0 = cross(V3{Rb.m0, Rb.m3, Rb.m6}, rr), u1 = cross(V3{Rb.m1, Rb.m4, Rb.m7}, rr), u2 = cross(V3{Rb.m2, Rb.m5, Rb.m8}, rr);
  return V3{-(fr[0] * u0.x + fr[1] * u0.y + fr[2] * u0.z), -(fr[0] * u1.x + fr[1] * u1.y + fr[2] * u1.z), -(fr[0] * u2.x + fr[1] * u2.y + fr[2] * u2.z)};
}

// mj: mj_makeConstraint rows of the fly-fly contacts (condim 1: one frictionless row each, J = n . (jacp2 - jacp1) at the
// contact point), mj_makeImpedance, mj_referenceConstraint; and mj_transmission mjTRN_BODY for the adhesion actuators: an
// adhesion force is spread evenly over ALL contacts of its body (ball and fly-fly, also the ones inside the gap), which
// rewrites the weights the ball-only path set.  Slot k = nc + j: c_J[k][0] / c_J[k][1] = the row over the chain dofs of
// geom1's / geom2's link, c_chain[k] / sc_chain_b = those dofs, c_nch / c_blk = counts / blocks (second << 8),
// c_amask = chain masks (second << 16), c_adh = adhesion actuators of the two links (255 = none).
__device__ __noinline__ void self_rows(BTile *Tp, ModelPtr Mp, const int lane, const int nc, const int nsc) {
  BTile &T = *Tp;
  const BallModel FFE_GLOBAL &M = *Mp;
  const V3 c0 = {M.thorax_pos[0], M.thorax_pos[1], M.thorax_pos[2]};
  for (int j = 0; j < nsc; j++) {
    const int k = nc + j, la = T.c_link[k] & 255, lb = T.c_link[k] >> 8;
    const int half = lane >> 4, p = lane & 15, link = half == 0 ? la : lb;
    const int nch = (half < 2 && link != 255) ? M.l_nchain[link] : 0;  // (link 255: a geom of the thorax, fixed to the world - no chain)
    float jv = 0.f, vv = 0.f;
    int f = 0;
    if (half < 2 && p < nch) {
      f = M.l_chain[p][link];
      const S6 cd = ld6(T.C[f]);
      const V3 r = V3{T.c_pos[k][0], T.c_pos[k][1], T.c_pos[k][2]} - c0;
      const V3 u = lin(cd) + cross(ang(cd), r);
      jv = (T.c_frame[k][0] * u.x + T.c_frame[k][1] * u.y + T.c_frame[k][2] * u.z) * (half == 0 ? -1.f : 1.f);
      vv = T.V[f];
    }
    if (half < 2 && p < NCH) {
      if (half == 0) T.c_chain[k][p] = (unsigned char)f; else sc_chain_b(T, k)[p] = (unsigned char)f;
    }
    const float vel = wave_sum(jv * vv);
    if (lane == 0) {
      const int na = M.l_nchain[la], nb = lb != 255 ? M.l_nchain[lb] : 0, fa = M.l_chain[na - 1][la], fb = lb != 255 ? M.l_chain[nb - 1][lb] : fa;
      T.c_nch[k] = na | (nb << 8);
      T.c_blk[k] = (int)M.d_blk[fa] | ((int)M.d_blk[fb] << 8);
      T.c_amask[k] = (unsigned)M.d_amask[fa] | ((lb != 255 ? (unsigned)M.d_amask[fb] : 0u) << 16);
      T.c_adh[k] = (M.l_adh[la] & 255) | (((lb != 255 ? M.l_adh[lb] : -1) & 255) << 8);
      const float K = T.c_par[k][0], B = T.c_par[k][1], invw = T.c_par[k][2], incl = T.c_par[k][4], dist = T.c_dist[k];
      float si_[5];
#pragma unroll
      for (int q2 = 0; q2 < 5; q2++) si_[q2] = M.sc_solimp[q2];
      const float imp = impedance(si_, fabsf(dist - incl));
      const float R0 = fmaxf(1e-15f, (1.f - imp) * invw * frcp(imp));
      T.c_D[k] = T.c_excl[k] ? 0.f : frcp(R0);
      T.c_mu[k] = 0.f;
      T.c_aref[k][0] = -B * vel - K * imp * (dist - incl);
      T.c_aref[k][1] = T.c_aref[k][2] = 0.f;
    }
  }
  DM_SYNC();
  // adhesion weights over all contacts of the claw's body
  if (lane < nc + nsc) {
    const int k = lane;
    auto ids = [&](int kk, int &a1, int &a2) {
      if (kk < nc) { a1 = T.c_adh[kk] >= 0 ? T.c_adh[kk] : 255; a2 = 255; }
      else { a1 = T.c_adh[kk] & 255; a2 = (T.c_adh[kk] >> 8) & 255; }
    };
    int a1, a2;
    ids(k, a1, a2);
    int n1 = 0, n2 = 0;
    for (int kk = 0; kk < nc + nsc; kk++) {
      int b1, b2;
      ids(kk, b1, b2);
      n1 += (a1 != 255 && (b1 == a1 || b2 == a1)) ? 1 : 0;
      n2 += (a2 != 255 && (b1 == a2 || b2 == a2)) ? 1 : 0;
    }
    float w = 0.f;
    if (a1 != 255) w -= T.frc[a1] / (float)n1;
    if (a2 != 255 && a2 != a1) w -= T.frc[a2] / (float)n2;
    T.c_w[k][0] = w; T.c_w[k][1] = 0.f; T.c_w[k][2] = 0.f;
  }
  DM_SYNC();
}

// J' of the fly-fly rows into the right-hand sides of a block solve: over geom1's chain, then (the chains may share dofs)
// accumulated over geom2's chain.  X4 has been zeroed and filled by the other rows; columns as assigned in stage 2.
__device__ __noinline__ void self_rhs(BTile *Tp, const int lane, const int nc, const int nsc, const int nrc, const int cb, const float c0x, const float c0y, const float c0z) {
  BTile &T = *Tp;
  const V3 c0 = {c0x, c0y, c0z};
#pragma unroll 1
  for (int half = 0; half < 2; half++) {
    DM_SYNC();
    for (int item = lane; item < nsc * 16; item += 64) {
      const int j = item >> 4, p = item & 15, k = nc + j;
      const int nch = (T.c_nch[k] >> (8 * half)) & 0xff;
      const int col = (half == 0 ? (int)T.r_col[nrc + j] : (int)sc_chain_b(T, k)[14]) + 1 - cb;
      if (p < nch && col >= 0 && col < 4) {
        const int f = half == 0 ? (int)T.c_chain[k][p] : (int)sc_chain_b(T, k)[p];
        (&T.X4[f].x)[col] += (half == 0 ? -1.f : 1.f) * cj_row(T, k, 0, cj_u(T, k, f, c0));
      }
    }
  }
}
// rows of G owned by fly-fly contacts: J over each of the two chains against the solved columns of that chain's block
__device__ __noinline__ void self_gacc(BTile *Tp, const int lane, const int nc, const int nsc, const int nrc, const int cb, const float c0x, const float c0y, const float c0z) {
  BTile &T = *Tp;
  const V3 c0 = {c0x, c0y, c0z};
  if (lane < nrc || lane >= nrc + nsc) return;
  const int k = nc + lane - nrc, gtri = lane * (lane + 1) / 2;
#pragma unroll 1
  for (int half = 0; half < 2; half++) {
    const int nch = (T.c_nch[k] >> (8 * half)) & 0xff, b = (T.c_blk[k] >> (8 * half)) & 0xff;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int p = 0; p < nch; p++) {
      const int f = half == 0 ? (int)T.c_chain[k][p] : (int)sc_chain_b(T, k)[p];
      const float jv = (half == 0 ? -1.f : 1.f) * cj_row(T, k, 0, cj_u(T, k, f, c0));
      const float4 y = T.X4[f];
      acc.x += jv * y.x; acc.y += jv * y.y; acc.z += jv * y.z; acc.w += jv * y.w;
    }
#pragma unroll
    for (int q2 = 0; q2 < 4; q2++) {
      const int gc = cb + q2;
      const float av = q2 == 0 ? acc.x : (q2 == 1 ? acc.y : (q2 == 2 ? acc.z : acc.w));
      if (gc == 0) T.r_y0[lane] += av;  // J a_s
      else if (gc - 1 < KCOL) {
        const int r2 = T.rowof[b][gc - 1];
        if (r2 <= lane) T.G[gtri + r2] += av;  // (255 = no such row)
      }
    }
  }
}

// sum over the fly-fly contacts whose row touches fly dof (blk, li) of J[c][p] * w[c][0]
__device__ __forceinline__ float self_gather(const Ctx &c, unsigned sbl, int f, V3 c0, const float (*w)[3]) {
  const BTile &T = *c.T;
  const unsigned li = sbl >> 8, blk = sbl & 0xffu;
  float acc = 0.f;
  for (int k = c.nc; k < c.nc + c.nsc; k++) {
    const unsigned bl = (unsigned)T.c_blk[k], am = T.c_amask[k];
    const bool in1 = (bl & 0xffu) == blk && ((am >> li) & 1u), in2 = (bl >> 8) == blk && ((am >> (16 + li)) & 1u);
    if (in1 || in2) {  // (dof f lies on geom1's chain: -n . u, on geom2's: +n . u, on both: they cancel)
      const float jn = cj_row(T, k, 0, cj_u(T, k, f, c0));
      acc += ((in2 ? jn : 0.f) - (in1 ? jn : 0.f)) * w[k][0];
    }
  }
  return acc;
}

// ------------------------------------------------------------------------------------------------ stage 1
template <class C>  // (a template so that the fragment's free-root branches are discarded, not compiled)
__device__ __forceinline__ void stage1(C &c) {
  constexpr bool FREE_ROOT = false;
  BTile &T = *c.T;
  const BallModel FFE_GLOBAL &M = model(c);
#include "leg_stage1.inc"
  // ---- mj: mj_collision, ball (geom1, sphere) against this link's capsule: mjc_SphereCapsule
  bool hit = false;
  float dist = 0.f, margin = 0.f, gap = 0.f;
  V3 nrm = {1.f, 0.f, 0.f}, cpos = {0.f, 0.f, 0.f};
  if (M.g_has[lane] && !(c.flags & BF_NO_CONTACT)) {
    const V3 bc = {M.b_center[0], M.b_center[1], M.b_center[2]};
    const V3 gp = c.xp + mv(xmat, V3{M.g_pos[0][lane], M.g_pos[1][lane], M.g_pos[2][lane]});
    const V3 ax = mv(xmat, V3{M.g_axis[0][lane], M.g_axis[1][lane], M.g_axis[2][lane]});
    const float half = M.g_half[lane], rad = M.g_rad[lane], x = fminf(fmaxf(dot(ax, bc - gp), -half), half);
    {  // publish the geom for the fly-fly pair tests below (the link-exchange area is free between the factorisation and stage 2)
      // two float4 arrays (centre | radius, axis | half length), slot-major: consecutive lanes read consecutive 16-byte words
      float4 *o = reinterpret_cast<float4 *>(&T.lk[0][0]);
      const int sl = M.g_slot[lane];
      o[sl] = make_float4(gp.x, gp.y, gp.z, half + rad);  // bounding radius: all the broad phase reads of a partner
      o[NPG + sl] = make_float4(ax.x, ax.y, ax.z, half);
      reinterpret_cast<float *>(o + 2 * NPG)[sl] = rad;
    }
    margin = M.g_margin[lane]; gap = M.g_gap[lane];
    const V3 dif = gp + x * ax - bc;
    const float cd = fsqrt(dot(dif, dif));
    dist = cd - M.b_radius - rad;
    hit = cd <= margin + M.b_radius + rad;
    if (cd >= 1e-15f) nrm = frcp(cd) * dif;
    cpos = bc + (M.b_radius + 0.5f * dist) * nrm;
  }
  BSTAMP(5);  // collision: the ball against the leg capsules
  unsigned long long bal = __ballot(hit);
  if (__popcll(bal) > NC) {
    // more contacts than the tile holds: the env is flagged and the NC DEEPEST are kept (dropping a deep one lets the leg sink in
    // until a later substep answers with an enormous force: tools/soak.py saw such envs blow up at saturated actions)
    c.overflow |= 1;
    int rank = 0;
    for (unsigned long long m = bal; m; m &= m - 1) {
      const int j = __ffsll((long long)m) - 1;
      const float dj = __shfl(dist, j);
      if (dj < dist || (dj == dist && j < lane)) rank++;
    }
    hit = hit && rank < NC;
    bal = __ballot(hit);
  }
  const int idx = __popcll(bal & ((1ull << lane) - 1ull));
  c.nc = min(__popcll(bal), NC);
  c.nact = __popcll(__ballot(hit && idx < NC && !(dist >= margin - gap)));
  if (hit && idx < NC) {
    T.c_link[idx] = lane;
    const int last = ndof == 1 ? c.sdof[0] : (ndof == 2 ? c.sdof[1] : c.sdof[2]);
    T.c_blk[idx] = M.d_blk[last]; T.c_amask[idx] = M.d_amask[last];
    T.c_excl[idx] = dist >= margin - gap ? 1 : 0;
    T.c_dist[idx] = dist;
    T.c_pos[idx][0] = cpos.x; T.c_pos[idx][1] = cpos.y; T.c_pos[idx][2] = cpos.z;
    const int nch = M.l_nchain[lane];
    T.c_nch[idx] = nch;
    for (int p = 0; p < NCH; p++) T.c_chain[idx][p] = (unsigned char)(p < nch ? M.l_chain[p][lane] : 0);
    T.c_par[idx][0] = M.g_K[lane]; T.c_par[idx][1] = M.g_B[lane]; T.c_par[idx][2] = M.g_invw[lane]; T.c_par[idx][3] = M.g_fric[lane];
    T.c_par[idx][4] = margin - gap;
    T.c_adh[idx] = M.l_adh[lane];
    // mj: mju_makeFrame
    V3 t1 = (nrm.y < 0.5f && nrm.y > -0.5f) ? V3{0.f, 1.f, 0.f} : V3{0.f, 0.f, 1.f};
    t1 = t1 - dot(nrm, t1) * nrm;
    t1 = frcp(fsqrt(dot(t1, t1))) * t1;
    const V3 t2 = cross(nrm, t1);
    float *fr = T.c_frame[idx];
    fr[0] = nrm.x; fr[1] = nrm.y; fr[2] = nrm.z; fr[3] = t1.x; fr[4] = t1.y; fr[5] = t1.z; fr[6] = t2.x; fr[7] = t2.y; fr[8] = t2.z;
  }
  DM_SYNC();
  // ---- the ball against the ellipsoids / cylinders that can reach it (more condim-3 ball contacts), and the geom frames of the
  //      convex pairs below, from the link poses published here
  if (!(c.flags & BF_NO_CONTACT)) {
    float *o = T.lp[lane];
    o[0] = c.xp.x; o[1] = c.xp.y; o[2] = c.xp.z; o[3] = c.xq.w; o[4] = c.xq.x; o[5] = c.xq.y; o[6] = c.xq.z;
    DM_SYNC();
    const int xb = __builtin_amdgcn_readfirstlane(ball_convex(c.T, (ModelPtr)c.M, lane, c.nc));
    if (xb >> 8) c.overflow |= 1;
    for (int k = c.nc; k < c.nc + (xb & 0xff); k++) c.nact += T.c_excl[k] ? 0 : 1;
    c.nc += xb & 0xff;
  }
  BSTAMP(10);  // geom frames + the ball against its convex partners
  if (lane < NBLK) {
    unsigned bm = 0u;
    for (int k = 0; k < c.nc; k++) if (T.c_blk[k] == lane) bm |= 1u << k;
    T.c_bmask[lane] = bm;
  }
  // ---- mj: mj_collision over the fly's own sphere / capsule pairs (condim 1).  Every link publishes its primitive geoms
  //      (world centre, axis, half length, radius) into the link-exchange area, which is free between the factorisation and
  //      stage 2; the pair tests read them back from there.
  c.nsc = 0; c.ndrop = 0;
  if (!(c.flags & BF_NO_CONTACT)) {
    if (lane == M.pg2_lane) {  // the rostrum's second capsule
      const V3 gc = c.xp + mv(xmat, V3{M.pg2_pos[0], M.pg2_pos[1], M.pg2_pos[2]});
      const V3 ga = mv(xmat, V3{M.pg2_axis[0], M.pg2_axis[1], M.pg2_axis[2]});
      float4 *o = reinterpret_cast<float4 *>(&T.lk[0][0]);
      o[M.pg2_slot] = make_float4(gc.x, gc.y, gc.z, M.pg2_half + M.pg2_rad);
      o[NPG + M.pg2_slot] = make_float4(ga.x, ga.y, ga.z, M.pg2_half);
      reinterpret_cast<float *>(o + 2 * NPG)[M.pg2_slot] = M.pg2_rad;
    }
    DM_SYNC();
    const int sc = __builtin_amdgcn_readfirstlane(prim_pairs(c.T, (ModelPtr)c.M, BallPairs{}, lane, c.nc));  // wave-uniform by construction
    c.nsc = sc & 0xff;
    if ((sc >> 8) & 0xff) c.overflow |= 1;
    c.ndrop = sc >> 16;
    BSTAMP(11);  // sphere / capsule pairs
    // ---- and over its pairs with an ellipsoid or cylinder on one side
    const int cc = __builtin_amdgcn_readfirstlane(convex_pairs<BallPairs>(c.T, (ModelPtr)c.M, lane, c.nc + c.nsc));
    c.nsc += cc & 0xff;
    if ((cc >> 8) & 0xff) c.overflow |= 1;
    c.ndrop += cc >> 16;
    for (int k = c.nc; k < c.nc + c.nsc; k++) c.nact += T.c_excl[k] ? 0 : 1;
  }
  DM_SYNC();
  BSTAMP(12);  // convex pairs
}

// sum over the contacts whose chain contains fly dof (blk, li) of  sum_r J[c][r][p] * w[c][r]
__device__ __forceinline__ float contact_gather(const Ctx &c, unsigned sbl, int f, V3 c0, const float (*w)[3]) {
  const BTile &T = *c.T;
  const unsigned li = sbl >> 8;
  unsigned bm = T.c_bmask[sbl & 0xffu];
  float acc = 0.f;
  while (bm) {
    const int k = __ffs(bm) - 1;
    bm &= bm - 1u;
    const unsigned am = T.c_amask[k];
    if ((am >> li) & 1u) {
      const V3 u = cj_u(T, k, f, c0);
      acc += cj_row(T, k, 0, u) * w[k][0] + cj_row(T, k, 1, u) * w[k][1] + cj_row(T, k, 2, u) * w[k][2];
    }
  }
  return acc;
}

// ------------------------------------------------------------------------------------------------ stage 2
__device__ __forceinline__ void stage2(Ctx &c, float act_reg, float ctrl_reg, float &act_out, bool integrate, int &iters_out, float *qacc_norm2) {
  BTile &T = *c.T;
  const BallModel FFE_GLOBAL &M = model(c);
  const int lane = c.lane;
  const int nc = c.nc;
  const float h = M.h;
  const V3 c0 = {M.thorax_pos[0], M.thorax_pos[1], M.thorax_pos[2]};
  const V3 bc = {M.b_center[0], M.b_center[1], M.b_center[2]};
#pragma unroll
  for (int s = 0; s < 3; s++) if (slot_on(c, s)) { T.Q[opq(c.sdof[s])] = c.q[s]; T.V[opq(c.sdof[s])] = c.v[s]; }
  DM_SYNC();
  // ---- mj: mj_fwdActuation: first-order activation filter, affine position servo on the activation
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
      if (M.a_trn[lane] == 2 && (c.flags & BF_NO_ADHESION)) force = 0.f;
    }
    T.frc[lane] = force;
  }
  act_out = act_reg + h * act_dot;
  // ---- contact rows: Jacobians over the chain dofs (jac2 - jac1, geom1 = ball), impedance, reference acceleration
  const M3 Rb = q2m(c.bq);
  DM_SYNC();
  DM_SYNC();
  // per-contact parameters and the adhesion pull (mj: mj_transmission mjTRN_BODY: -force along the normal row).
  // Row-parallel: a row of 16 lanes handles one contact, lane p of the row the p-th dof of its chain.
  for (int base = 0; base < nc; base += 4) {
    const int k = base + (lane >> 4), p = lane & 15;
    const bool on = k < nc;
    const bool pv = on && p < T.c_nch[k];
    const float vv = pv ? T.V[T.c_chain[k][p]] : 0.f;
    const V3 uj = pv ? cj_u(T, k, T.c_chain[k][p], c0) : V3{0.f, 0.f, 0.f};
    float vel[3];
#pragma unroll
    for (int r = 0; r < 3; r++) {
      vel[r] = row_sum(pv ? cj_row(T, k, r, uj) * vv : 0.f);
      if (on) { const V3 jb = cj_ball(T, k, r, Rb, bc); vel[r] += jb.x * c.bw.x + jb.y * c.bw.y + jb.z * c.bw.z; }
    }
    if (on && p == 0) {
      const float K = T.c_par[k][0], B = T.c_par[k][1], invw = T.c_par[k][2], incl = T.c_par[k][4], dist = T.c_dist[k];
      float si_[5];
#pragma unroll
      for (int q2 = 0; q2 < 5; q2++) si_[q2] = M.c_solimp[q2];
      const float imp = impedance(si_, fabsf(dist - incl));
      const float R0 = fmaxf(1e-15f, (1.f - imp) * invw * frcp(imp));
      T.c_D[k] = T.c_excl[k] ? 0.f : frcp(R0);
      T.c_mu[k] = T.c_par[k][3];
      T.c_aref[k][0] = -B * vel[0] - K * imp * (dist - incl);
      T.c_aref[k][1] = -B * vel[1];
      T.c_aref[k][2] = -B * vel[2];
      const int adh = T.c_adh[k];
      T.c_w[k][0] = adh >= 0 ? -T.frc[adh] : 0.f; T.c_w[k][1] = 0.f; T.c_w[k][2] = 0.f;
    }
  }
  DM_SYNC();
#ifdef FFB_SC_NOSTAGE2
  const int nsc = 0;
#else
  const int nsc = c.nsc;
#endif
  if (nsc) self_rows(c.T, (ModelPtr)c.M, lane, nc, nsc);  // fly-fly contacts (rare): rows, impedance, adhesion shares
  BSTAMP(6);  // actuation + contact rows
  // ---- smooth forces (mj: mj_fwdAcceleration); the smooth acceleration a_s = M^-1 qfrc_smooth rides as column 0 of the
  //      first block solve of the G build below
  float qs[3], am[3];
#pragma unroll
  for (int s = 0; s < 3; s++) {
    qs[s] = 0.f; am[s] = 0.f;
    if (slot_on(c, s)) {
      float f = c.fnb[s];
      const int a0 = M.s_act[0][s][lane], a1 = M.s_act[1][s][lane];
      if (a0 >= 0) f += M.s_actcoef[0][s][lane] * T.frc[a0];
      if (a1 >= 0) f += M.s_actcoef[1][s][lane] * T.frc[a1];
      if (nc) f += contact_gather(c, opq(c.sbl[s]), opq(c.sdof[s]), c0, T.c_w);
      if (nsc) f += self_gather(c, opq(c.sbl[s]), opq(c.sdof[s]), c0, T.c_w);
      qs[s] = f;
    }
  }
  V3 qsb = c.btau;
  for (int k = 0; k < nc; k++) {
    const V3 jb = cj_ball(T, k, 0, Rb, bc);
    qsb.x += jb.x * T.c_w[k][0]; qsb.y += jb.y * T.c_w[k][0]; qsb.z += jb.z * T.c_w[k][0];
  }
  const float Ib = M.b_I;
  const V3 amb = frcp(Ib) * qsb;
  BSTAMP(7);  // smooth forces
  // ---- joint-limit rows (mj: mj_instantiateLimit, margin 0): sign, D, aref per slot
  float lsgn[3], lD[3], laref[3];
#pragma unroll
  for (int s = 0; s < 3; s++) {
    lsgn[s] = 0.f; lD[s] = 0.f; laref[s] = 0.f;
    if (slot_on(c, s) && M.s_limited[s][lane] && !(c.flags & BF_NO_LIMIT)) {
      const float dlo = c.q[s] - M.s_lo[s][lane], dhi = M.s_hi[s][lane] - c.q[s];
      float dist = 0.f;
      if (dlo < 0.f) { lsgn[s] = 1.f; dist = dlo; }
      else if (dhi < 0.f) { lsgn[s] = -1.f; dist = dhi; }
      if (lsgn[s] != 0.f) {
        float si_[5];
#pragma unroll
        for (int q2 = 0; q2 < 5; q2++) si_[q2] = M.j_solimp[q2];
        const float imp = impedance(si_, fabsf(dist));
        lD[s] = frcp(fmaxf(1e-15f, (1.f - imp) * M.s_invw[s][lane] * frcp(imp)));
        laref[s] = -M.s_B[s][lane] * (lsgn[s] * c.v[s]) - M.s_K[s][lane] * imp * dist;
      }
    }
  }
  // ---- mj: mj_fwdConstraint in the space of the constraint rows.  With Y = M^-1 J', G = J Y and a = a_s + Y lambda the
  //      primal cost 1/2 (a - a_s)' M (a - a_s) + s(J a - aref) becomes 1/2 lambda' G lambda + s(y0 + G lambda), y0 = J a_s - aref;
  //      its Newton step is  d = -(I + W G)^-1 (lambda - f),  W = d2s/dy2 (3x3 per contact, scalar per limit).  M is factorised
  //      once per substep (stage 1); the rows' columns of G come four per block solve, rows of different blocks sharing a
  //      column because M^-1 is block diagonal; every Newton iteration is then dense work on <= 32 rows.
  int lrow[3] = {-1, -1, -1};
  const int nrc = 3 * nc;
  int R = nrc;
  if (nsc) {  // fly-fly contact rows: one unilateral row each (condim 1), handled by the solver like a joint-limit row
    if (lane < nsc) {
      const int row = nrc + lane, k = nc + lane;
      T.r_sgn[row] = 0.f; T.r_D[row] = T.c_D[k]; T.r_dof[row] = (unsigned char)k; T.r_blk[row] = (unsigned char)(T.c_blk[k] & 0xff);
      T.r_y0[row] = -T.c_aref[k][0];
      float l0 = 0.f;  // the same pair's force of the last substep
      if (c.have_ws) { const int nw = T.ws_n; const unsigned pid = T.c_pid[k]; for (int j = 0; j < nw; j++) if (T.ws_pid[j] == pid) l0 = T.ws_f[j]; }
      T.r_lam[row] = l0;
    }
    R += nsc;
  }
  {  // limit rows: one per instantiated limit, in (slot, lane) order; y0 starts as -aref, J a_s is added by the first solve
#pragma unroll
    for (int s = 0; s < 3; s++) {
      const bool on = lsgn[s] != 0.f;
      const unsigned long long bal = __ballot(on);
      const int idx = R + __popcll(bal & ((1ull << lane) - 1ull));
      if (on && idx < RMAX) {
        lrow[s] = idx;
        T.r_sgn[idx] = lsgn[s]; T.r_D[idx] = lD[s]; T.r_dof[idx] = (unsigned char)opq(c.sdof[s]); T.r_blk[idx] = (unsigned char)(opq(c.sbl[s]) & 0xffu);
        T.r_y0[idx] = -laref[s];
        T.r_lam[idx] = c.have_ws ? c.wsl[s] : 0.f;
      }
      R += __popcll(bal);
    }
    if (R > RMAX) { R = RMAX; c.overflow |= 2; }
  }
  const bool constrained = R > 0;
  int iters = 0;
  if (lane < nrc) {  // contact rows: the ball's share of J a_s minus aref; the fly's share comes with the first solve
    const int k = lane / 3, r = lane - 3 * k;
    T.r_blk[lane] = (unsigned char)T.c_blk[k];
    const V3 jb = cj_ball(T, k, r, Rb, bc);
    T.r_y0[lane] = jb.x * amb.x + jb.y * amb.y + jb.z * amb.z - T.c_aref[k][r];
  }
  for (int k = lane; k < NBLK * KCOL; k += 64) (&T.rowof[0][0])[k] = 255;
  // warm start from the force this link's contact carried last substep
  if (c.have_ws) { for (int k = 0; k < nc; k++) if (T.c_link[k] == lane) { T.r_lam[3 * k] = c.wsc[0]; T.r_lam[3 * k + 1] = c.wsc[1]; T.r_lam[3 * k + 2] = c.wsc[2]; } }
  else if (lane < nrc) T.r_lam[lane] = 0.f;
  DM_SYNC();
  // columns: a row's column is its rank among the rows of its block
  int ncol;
  {
    int mycol = 0, mycol2 = 0;
    const int myb = lane < R ? (int)T.r_blk[lane] : -1;
    int myb2 = -1;  // a fly-fly row whose two chains sit in different blocks needs a column in each of them
    if (nsc && lane >= nrc && lane < nrc + nsc) { myb2 = T.c_blk[nc + lane - nrc] >> 8; if (myb2 == myb) myb2 = -1; }
    for (int b = 0; b < NBLK; b++) {  // rank among the lower rows of the same block, by ballots
      const unsigned long long mb = __ballot(myb == b || myb2 == b);
      if (myb == b) mycol = __popcll(mb & ((1ull << lane) - 1ull));
      if (myb2 == b) mycol2 = __popcll(mb & ((1ull << lane) - 1ull));
    }
    if (lane < R) {
      const int b = myb;
      T.r_col[lane] = (unsigned char)mycol;
      if (mycol < KCOL) T.rowof[b][mycol] = (unsigned char)lane;
      if (myb2 >= 0) {
        sc_chain_b(T, nc + lane - nrc)[14] = (unsigned char)mycol2;
        if (mycol2 < KCOL) T.rowof[myb2][mycol2] = (unsigned char)lane;
        mycol = max(mycol, mycol2);
      } else if (nsc && lane >= nrc && lane < nrc + nsc) sc_chain_b(T, nc + lane - nrc)[14] = (unsigned char)mycol;
      mycol += 1;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) mycol = max(mycol, __shfl_xor(mycol, off));
    if (mycol > KCOL) c.overflow |= 4;  // more than KCOL rows in one block of M: the env is flagged
                                     // (wave-uniform here: lane 0 reports it) and the rows without a column exert no force (below)
    ncol = min(mycol, KCOL);
    if (mycol > KCOL) {
      // A row without a column would keep its force law but lose its own response (its row of G stays empty): an explicit spring
      // of stiffness D - the blow-ups tools/soak.py saw at saturated actions.  Such rows are switched off for this substep
      // instead: a contact as a whole (all three rows), a limit or fly-fly row through D = 0.
      DM_SYNC();
      const bool nocol = lane < R && ((int)T.r_col[lane] >= KCOL || (myb2 >= 0 && mycol2 >= KCOL));
      if (nocol) { if (lane < nrc) T.c_excl[lane / 3] = 1; else T.r_D[lane] = 0.f; }
    }
  }
  DM_SYNC();
  // G: ball coupling between contact rows, then the fly part M_blk^-1 from the block solves
  const float iIb = frcp(Ib);
  const int gtri = lane * (lane + 1) / 2;  // G is symmetric: row `lane` keeps its columns r2 <= lane
  {
    V3 ja = {0.f, 0.f, 0.f};  // this row's ball Jacobian (zero for limit rows); the other rows' come by v_readlane
    if (lane < nrc) { const V3 jp = cj_ball(T, lane / 3, lane % 3, Rb, bc); ja = {jp.x * iIb, jp.y * iIb, jp.z * iIb}; }
    for (int r2 = 0; r2 < R; r2++) {
      const float gv = (ja.x * rl_f(ja.x, r2) + ja.y * rl_f(ja.y, r2) + ja.z * rl_f(ja.z, r2)) * Ib;
      if (lane < R && r2 <= lane) T.G[gtri + r2] = gv;
    }
  }
  // solve columns: 0 = qfrc_smooth, 1 + c = the rows whose block-local column is c
#pragma unroll 1
  for (int cb = 0; cb < ncol + 1; cb += 4) {
    for (int f = lane; f < ND; f += 64) T.X4[f] = make_float4(0.f, 0.f, 0.f, 0.f);
    DM_SYNC();
    if (cb == 0) {
#pragma unroll
      for (int s = 0; s < 3; s++) if (slot_on(c, s)) T.X4[opq(c.sdof[s])].x = qs[s];
    }
    for (int item = lane; item < nrc * NCH; item += 64) {  // contact rows: J' over the chain
      const int r = item / NCH, p = item - r * NCH, k = r / 3, col = (int)T.r_col[r] + 1 - cb;
      if (col >= 0 && col < 4 && p < T.c_nch[k]) { const int f = T.c_chain[k][p]; (&T.X4[f].x)[col] = cj_row(T, k, r - 3 * k, cj_u(T, k, f, c0)); }
    }
    if (lane >= nrc + nsc && lane < R) {
      const int col = (int)T.r_col[lane] + 1 - cb;
      if (col >= 0 && col < 4) (&T.X4[T.r_dof[lane]].x)[col] = T.r_sgn[lane];
    }
    if (nsc) self_rhs(c.T, lane, nc, nsc, nrc, cb, c0.x, c0.y, c0.z);
    DM_SYNC();
    solve4(c, T.Lm, T.dinv_m);
    if (cb == 0) {
#pragma unroll
      for (int s = 0; s < 3; s++) if (slot_on(c, s)) am[s] = T.X4[opq(c.sdof[s])].x;
    }
    if (lane < R) {
      float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
      if (lane < nrc) {
        const int k = lane / 3, r = lane - 3 * k, nch = T.c_nch[k];
        for (int p = 0; p < nch; p++) {
          const int f = T.c_chain[k][p];
          const float jv = cj_row(T, k, r, cj_u(T, k, f, c0));
          const float4 y = T.X4[f];
          acc.x += jv * y.x; acc.y += jv * y.y; acc.z += jv * y.z; acc.w += jv * y.w;
        }
      } else if (lane < nrc + nsc) {  // fly-fly row: self_gacc below
      } else {
        const float sg = T.r_sgn[lane];
        const float4 y = T.X4[T.r_dof[lane]];
        acc = make_float4(sg * y.x, sg * y.y, sg * y.z, sg * y.w);
      }
      const int b = T.r_blk[lane];
#pragma unroll
      for (int q2 = 0; q2 < 4; q2++) {
        const int gc = cb + q2;
        const float av = q2 == 0 ? acc.x : (q2 == 1 ? acc.y : (q2 == 2 ? acc.z : acc.w));
        if (gc == 0) T.r_y0[lane] += av;  // J a_s
        else if (gc - 1 < KCOL) {
          const int r2 = T.rowof[b][gc - 1];
          if (r2 <= lane) T.G[gtri + r2] += av;  // (255 = no such row)
        }
      }
    }
    if (nsc) self_gacc(c.T, lane, nc, nsc, nrc, cb, c0.x, c0.y, c0.z);
    DM_SYNC();
  }
  BSTAMP(8);  // constraint rows + G
  const float scale2 = [&]() { float sq = 0.f;
#pragma unroll
    for (int s = 0; s < 3; s++) if (slot_on(c, s)) sq += qs[s] * am[s];
    return wave_sum(sq) + dot(qsb, amb); }();
  if (constrained) {
    int nact_ = 0;
    for (int k = 0; k < nc; k++) nact_ += T.c_excl[k] ? 0 : 1;
    const int nslip = (nact_ > 0 && !(c.flags & BF_NO_NOSLIP)) ? M.noslip_iterations : 0;
    ModelPtr mp_ = (ModelPtr)c.M;
    // the dense solver's cost grows with the square of its register-resident size: sizes around the common row counts (3 rows per
    // contact + ~5 joint limits: 17, 20, 23, 26) are instantiated more finely (+1.1 % env-steps/s; every even size: no further gain)
    if (R <= 12) iters = row_newton<12, ConeRows>(c.T, mp_, lane, R, nrc, scale2, nslip, c.have_ws);
    else if (R <= 16) iters = row_newton<16, ConeRows>(c.T, mp_, lane, R, nrc, scale2, nslip, c.have_ws);
    else if (R <= 18) iters = row_newton<18, ConeRows>(c.T, mp_, lane, R, nrc, scale2, nslip, c.have_ws);
    else if (R <= 20) iters = row_newton<20, ConeRows>(c.T, mp_, lane, R, nrc, scale2, nslip, c.have_ws);
    else if (R <= 22) iters = row_newton<22, ConeRows>(c.T, mp_, lane, R, nrc, scale2, nslip, c.have_ws);
    else if (R <= 24) iters = row_newton<24, ConeRows>(c.T, mp_, lane, R, nrc, scale2, nslip, c.have_ws);
    else if (R <= 28) iters = row_newton<28, ConeRows>(c.T, mp_, lane, R, nrc, scale2, nslip, c.have_ws);
    else if (R <= 32) iters = row_newton<32, ConeRows>(c.T, mp_, lane, R, nrc, scale2, nslip, c.have_ws);
    else if (R <= 40) iters = row_newton<40, ConeRows>(c.T, mp_, lane, R, nrc, scale2, nslip, c.have_ws);
    else iters = row_newton<RMAX, ConeRows>(c.T, mp_, lane, R, nrc, scale2, nslip, c.have_ws);
    BSTAMP(9);  // newton + noslip (dense, in registers)
  }
  iters_out += iters;
  BSTAMP(16);  // noslip
  // ---- constraint forces in joint space, final acceleration a = a_s + M^-1 J' f
  if (lane < nrc) T.c_f[lane / 3][lane % 3] = constrained ? T.r_f[lane] : 0.f;
  if (nsc && lane < nsc) {
    T.c_f[nc + lane][0] = T.r_f[nrc + lane]; T.c_f[nc + lane][1] = 0.f; T.c_f[nc + lane][2] = 0.f;
    T.ws_pid[lane] = T.c_pid[nc + lane]; T.ws_f[lane] = constrained ? T.r_f[nrc + lane] : 0.f;
  }
  if (lane == 0) T.ws_n = nsc;
  DM_SYNC();
  float qc[3], a[3];
#pragma unroll
  for (int s = 0; s < 3; s++) {
    qc[s] = 0.f;
    if (slot_on(c, s)) {
      if (lrow[s] >= 0) { const float lf_ = T.r_f[lrow[s]]; qc[s] = lsgn[s] * lf_; c.wsl[s] = lf_; } else c.wsl[s] = 0.f;
      if (nc) qc[s] += contact_gather(c, opq(c.sbl[s]), opq(c.sdof[s]), c0, T.c_f);
      if (nsc) qc[s] += self_gather(c, opq(c.sbl[s]), opq(c.sdof[s]), c0, T.c_f);
    }
  }
  c.wsc[0] = c.wsc[1] = c.wsc[2] = 0.f;
  for (int k = 0; k < nc; k++) if (T.c_link[k] == lane) { c.wsc[0] = T.c_f[k][0]; c.wsc[1] = T.c_f[k][1]; c.wsc[2] = T.c_f[k][2]; }
  V3 qcb = {0.f, 0.f, 0.f};
  for (int k = 0; k < nc; k++) {
    const float f0 = T.c_f[k][0], f1 = T.c_f[k][1], f2 = T.c_f[k][2];
    const V3 b0 = cj_ball(T, k, 0, Rb, bc), b1 = cj_ball(T, k, 1, Rb, bc), b2 = cj_ball(T, k, 2, Rb, bc);
    qcb.x += b0.x * f0 + b1.x * f1 + b2.x * f2;
    qcb.y += b0.y * f0 + b1.y * f1 + b2.y * f2;
    qcb.z += b0.z * f0 + b1.z * f1 + b2.z * f2;
  }
  // final acceleration a = a_s + M^-1 J' f and the Euler acceleration (M + h B)^-1 (qfrc_smooth + J' f) (mj: mj_Euler, implicit in
  // the joint damping) in one pass: component x through M's factor, component y through the factor of M + h B
  V3 ab = amb + frcp(Ib) * qcb;
  float qe[3];
#pragma unroll
  for (int s = 0; s < 3; s++) if (slot_on(c, s)) T.X4[opq(c.sdof[s])] = make_float4(qc[s], qs[s] + qc[s], 0.f, 0.f);
  DM_SYNC();
  solve_dual(c, T.Lm, T.dinv_m, T.Lh, T.dinv_h);
#pragma unroll
  for (int s = 0; s < 3; s++) {
    const float4 x = slot_on(c, s) ? T.X4[opq(c.sdof[s])] : make_float4(0.f, 0.f, 0.f, 0.f);
    a[s] = am[s] + x.x; qe[s] = x.y;
  }
  DM_SYNC();
  {
    float n2 = 0.f;
#pragma unroll
    for (int s = 0; s < 3; s++) if (slot_on(c, s)) n2 += a[s] * a[s];
    *qacc_norm2 = wave_sum(n2) + dot(ab, ab);
    c.have_ws = 1;
  }
  BSTAMP(17);  // constraint forces, final acceleration
  // ---- sensors (mj: mj_rnePostConstraint + mj_sensorAcc): touch = normal force on the claw, force = interaction
  //      force on the tarsus from its parent, in the tarsus site frame.  Only the linear part of the spatial force is
  //      needed: m (a_lin + alpha x r + w x (v_lin + w x r)) with r = CoM - origin.
  {
    const int parent = l_parent(c), ndof = l_ndof(c);
    const unsigned tree = M.l_tree[lane];
    const int sub = (int)(tree & 0xffu), anc2 = (int)((tree >> 8) & 0xffu) - 1, anc4 = (int)((tree >> 16) & 0xffu) - 1;
    V3 fext = {0.f, 0.f, 0.f};
    float touch = 0.f;
    for (int k = 0; k < nc; k++) {
      if (T.c_link[k] == lane && !T.c_excl[k]) {
        const float *fr = T.c_frame[k];
        const float f0 = T.c_f[k][0], f1 = T.c_f[k][1], f2 = T.c_f[k][2];
        fext = fext + V3{fr[0] * f0 + fr[3] * f1 + fr[6] * f2, fr[1] * f0 + fr[4] * f1 + fr[7] * f2, fr[2] * f0 + fr[5] * f1 + fr[8] * f2};
        if (f0 > 0.f) touch += f0;
      }
    }
    for (int k = nc; k < nc + nsc; k++) {  // fly-fly contacts: -n f on geom1's link, +n f on geom2's (mj_rnePostConstraint's cfrc_ext)
      const int la = T.c_link[k] & 255, lb = T.c_link[k] >> 8;
      if ((la == lane || lb == lane) && !T.c_excl[k]) {
        const float f0 = T.c_f[k][0] * (lb == lane ? 1.f : -1.f);
        fext = fext + V3{T.c_frame[k][0] * f0, T.c_frame[k][1] * f0, T.c_frame[k][2] * f0};
        if (T.c_f[k][0] > 0.f) touch += T.c_f[k][0];  // the contact point lies inside the claw's (larger) touch site
      }
    }
    S6 dacc = zero6();  // sum over the dofs of the ancestor path of cdof * qacc (path sum by pointer jumping, as in stage 1)
#pragma unroll
    for (int s = 0; s < 3; s++) if (s < ndof) dacc = dacc + a[s] * ld6(T.C[opq(c.sdof[s])]);
#pragma unroll
    for (int r = 0; r < 3; r++) {
      const int an = r == 0 ? parent : (r == 1 ? anc2 : anc4);
      st6(T.lk[lane], dacc);
      DM_SYNC();
      if (an >= 0) dacc = dacc + ld6(T.lk[an]);
      DM_SYNC();
    }
    const S6 cacc = c.caccb + dacc;
    const V3 r = c.xip - V3{M.thorax_pos[0], M.thorax_pos[1], M.thorax_pos[2]};
    const V3 w = ang(c.cvel);
    V3 fint = c.mass * (lin(cacc) + cross(ang(cacc), r) + cross(w, lin(c.cvel) + cross(w, r))) - fext;
    {  // subtree sum over the link's depth-first lane range
      float *o = T.lk[lane];
      o[0] = fint.x; o[1] = fint.y; o[2] = fint.z;
      DM_SYNC();
      const int maxsub = M.maxsub;
#pragma unroll 1
      for (int t = 1; t < maxsub; t++) if (t < sub) { const float *p = T.lk[lane + t]; fint = fint + V3{p[0], p[1], p[2]}; }
      DM_SYNC();
    }
    const int fi = M.l_force[lane], ti = M.l_touch[lane];
    if (fi >= 0) {
      const Q4 sq = qmul(c.xq, Q4{M.l_fsite[0][lane], M.l_fsite[1][lane], M.l_fsite[2][lane], M.l_fsite[3][lane]});
      const V3 fl_ = mtv(q2m(sq), fint);
      T.sens[3 * fi] += fl_.x; T.sens[3 * fi + 1] += fl_.y; T.sens[3 * fi + 2] += fl_.z;
    }
    if (ti >= 0) T.sens[18 + ti] += touch;
    DM_SYNC();
  }
  BSTAMP(18);  // sensors
  if (!integrate) return;  // mj_forward: state untouched
  // ---- integrate with the Euler acceleration computed above
#pragma unroll
  for (int s = 0; s < 3; s++) {
    if (slot_on(c, s)) { c.v[s] += h * qe[s]; c.q[s] += h * c.v[s]; }
  }
  // ball: no damping, so its Euler acceleration is ab = (tau_smooth + J_b' f) / I
  c.bw = c.bw + h * ab;
  {
    const float wn = fsqrt(dot(c.bw, c.bw));
    if (wn >= 1e-15f) {
      const Q4 dq = axis_angle(frcp(wn) * c.bw, wn * h);
      c.bq = qnormalize(qmul(qnormalize(c.bq), dq));
    }
  }
  BSTAMP(19);  // Euler
}

// ------------------------------------------------------------------------------------------------ kernel
__global__ __launch_bounds__(64, 2) void ball_step_kernel(const BallModel *__restrict__ Mp, BTaskDev K, BState *__restrict__ states,
                                                         const float *__restrict__ act, float *__restrict__ obs, float *__restrict__ rew,
                                                         float *__restrict__ disc, int *__restrict__ st, int batch, int mode, int nphys,
                                                         const int *__restrict__ order, int *__restrict__ cost,
                                                         const unsigned char *__restrict__ reset_mask) {
  // Workgroups are dispatched in index order; `order` lists the envs by decreasing cost of their previous control step, so the
  // expensive ones (more contacts, more Newton iterations) start first and the launch does not end on a few long waves
  // running alone at low occupancy (launch_order.hpp; walk_on_ball, B = 4 096: -3 % launch time).
  if ((int)blockIdx.x >= batch) return;
#ifdef FFE_TRACE
  const unsigned long long tr_t0 = __builtin_amdgcn_s_memrealtime();
  const int tr_prev = cost[order[blockIdx.x]];
#endif
  const int env = order[blockIdx.x], lane = threadIdx.x;
  if (mode == 3) {  // ffe_reset_envs: only the masked envs start a new episode; the others keep state and output rows
    if (!reset_mask[env]) return;
    mode = 1;
  }
  __shared__ BTile T;
  const BallModel &M = *Mp;
  BState &S = states[env];
  Ctx c;
  c.M = Mp; c.T = &T; c.lane = lane; c.flags = K.flags; c.overflow = 0;
#ifdef FFB_STAMPS
  c.st_t0 = __builtin_amdgcn_s_memtime();
  for (int k = 0; k < 24; k++) c.st_acc[k] = 0;
#endif
  c.lpack = M.l_pack[lane]; c.xh = M.x_on[lane];
#pragma unroll
  for (int s = 0; s < 3; s++) {
    const int f = M.s_dof[s][lane];
    c.sdof[s] = f;
    c.sbl[s] = f >= 0 ? ((unsigned)M.d_blk[f] | ((unsigned)M.d_li[f] << 8)) : 0u;
  }
  const bool do_reset = (mode == 1) || (mode == 0 && S.needs_reset != 0);
  const bool phys_only = (mode == 2);
  float act_reg = 0.f, ctrl_reg = 0.f;
  int step_counter = S.step_counter, iters = 0;
  if (do_reset) {
    // ref: walk_on_ball.py:52-54 + fruitfly.py:330-340: qpos0, zero velocity / activation, wings folded to their spring reference
#pragma unroll
    for (int s = 0; s < 3; s++) { c.q[s] = 0.f; c.v[s] = 0.f; }
#pragma unroll
    for (int s = 0; s < 3; s++)
      if (slot_on(c, s)) for (int w = 0; w < M.nwing; w++) if (M.wing_dof[w] == c.sdof[s]) c.q[s] = M.qspring[c.sdof[s]];
    c.bq = {1.f, 0.f, 0.f, 0.f}; c.bw = {0.f, 0.f, 0.f};
    c.have_ws = 0;
#pragma unroll
    for (int s = 0; s < 3; s++) { c.wsl[s] = 0.f; c.wsc[s] = 0.f; }
    step_counter = 0;
  } else {
#pragma unroll
    for (int s = 0; s < 3; s++) { c.q[s] = slot_on(c, s) ? S.q[c.sdof[s]] : 0.f; c.v[s] = slot_on(c, s) ? S.v[c.sdof[s]] : 0.f; }
    c.bq = {S.ballq[0], S.ballq[1], S.ballq[2], S.ballq[3]}; c.bw = {S.ballw[0], S.ballw[1], S.ballw[2]};
    c.have_ws = S.have_ws;
#pragma unroll
    for (int s = 0; s < 3; s++) { c.wsl[s] = slot_on(c, s) ? S.qacc_ws[c.sdof[s]] : 0.f; c.wsc[s] = S.wsc[lane][s]; }
    act_reg = lane < NU ? S.act[lane] : 0.f;
    if (lane < NU) {
      if (phys_only) ctrl_reg = act[(size_t)env * NU + lane];
      else {
        // ref: fruitfly.py:480-492 apply_action (+ the CanonicalSpecWrapper the reference wraps every env in)
        const int ai = M.a_action[lane];
        float av = ai >= 0 ? act[(size_t)env * NACT + ai] : 0.f;
        if (!(av == av)) av = 0.f;
        if (K.canonical && ai >= 0) {
          if (K.clip) av = fminf(fmaxf(av, -1.f), 1.f);
          av = M.act_lo[ai] + 0.5f * (av + 1.f) * (M.act_hi[ai] - M.act_lo[ai]);
        }
        ctrl_reg = av;
      }
    }
    if (!phys_only) step_counter++;
  }
  if (lane < 24) T.sens[lane] = 0.f;
  if (lane < NSD) { T.sd_pid[lane] = S.sd_pid[lane]; T.sd_n[lane][0] = S.sd_n[lane][0]; T.sd_n[lane][1] = S.sd_n[lane][1]; T.sd_n[lane][2] = S.sd_n[lane][2]; T.sd_n[lane][3] = S.sd_n[lane][3]; }
  if (lane == 0) { T.sd_cnt = do_reset ? 0 : S.sd_cnt; T.ws_n = do_reset ? 0 : S.ws_n; }
  if (lane < NC) { T.ws_pid[lane] = S.ws_pid[lane]; T.ws_f[lane] = S.ws_f[lane]; }
  DM_SYNC();
  const int nsub = phys_only ? nphys : M.nsub;
  float qn2 = 0.f;
  // one copy of each stage: stage1 ; [stage2 ; stage1] x nsub.  A reset is stage1 ; stage2 without actuation and without
  // integrating (mj_forward, dm_control's after_reset); its sensors are the first sample of the buffers.
  if (do_reset) c.flags |= BF_NO_ACTUATION;
  unsigned long long con_hist = 0ull, det_hist = 0ull;
#pragma unroll 1
  for (int s = 0;; s++) {
    stage1(c);
    if (!do_reset && s == nsub) break;
    if (s < 16) con_hist |= (unsigned long long)min(c.nact, 15) << (4 * s);
    if (s < 12) det_hist |= (unsigned long long)min(c.nc + c.nsc, 31) << (5 * s);
    float act_new;
    stage2(c, act_reg, ctrl_reg, act_new, !do_reset, iters, &qn2);
    if (do_reset) break;
    act_reg = act_new;
  }
  c.flags = K.flags;
  // ---- store state
#pragma unroll
  for (int s = 0; s < 3; s++) if (slot_on(c, s)) { S.q[c.sdof[s]] = c.q[s]; S.v[c.sdof[s]] = c.v[s]; S.qacc_ws[c.sdof[s]] = c.wsl[s]; }
#pragma unroll
  for (int s = 0; s < 3; s++) S.wsc[lane][s] = c.wsc[s];
  if (lane < NU) S.act[lane] = do_reset ? 0.f : act_reg;
  if (lane < NSD) { S.sd_pid[lane] = T.sd_pid[lane]; S.sd_n[lane][0] = T.sd_n[lane][0]; S.sd_n[lane][1] = T.sd_n[lane][1]; S.sd_n[lane][2] = T.sd_n[lane][2]; S.sd_n[lane][3] = T.sd_n[lane][3]; }
  if (lane == 0) { S.sd_cnt = T.sd_cnt; S.ws_n = T.ws_n; }
  if (lane < NC) { S.ws_pid[lane] = T.ws_pid[lane]; S.ws_f[lane] = T.ws_f[lane]; }
  if (lane == 0) {
    S.ballq[0] = c.bq.w; S.ballq[1] = c.bq.x; S.ballq[2] = c.bq.y; S.ballq[3] = c.bq.z;
    S.ballw[0] = c.bw.x; S.ballw[1] = c.bw.y; S.ballw[2] = c.bw.z;
    S.step_counter = step_counter; S.iters = iters; S.ncon = c.nc + c.nsc; S.nself = c.nsc;  // (contacts that take part in something: an inactive one without an adhesion actuator on either body is not kept)
    S.con_hist[0] = (unsigned)con_hist; S.con_hist[1] = (unsigned)(con_hist >> 32);
    S.det_hist[0] = (unsigned)det_hist; S.det_hist[1] = (unsigned)(det_hist >> 32);
    // key of the next launch's order: what a wave's lifetime varies with - Newton iterations over the step's substeps (4 us each)
    // and the number of contacts (40 us each; least-squares fit of the lifetimes in tools/wave_timeline.py's trace)
    cost[env] = min(255, iters + 10 * (c.nc + c.nsc));
    if (do_reset) S.overflow = 0; else S.overflow |= c.overflow;  // sticky over the episode: 1 contacts > 10, 2 constraint rows > 32, 4 rows of one block > 12
    S.have_ws = do_reset ? 0 : c.have_ws;
    // validity: bare physics reports its own launch and leaves the episode's count alone; a FIRST row starts it at zero
    S.step_bits = c.overflow;
    if (!phys_only) S.ep_flagged = do_reset ? 0 : S.ep_flagged + (c.overflow ? 1 : 0);
  }
#ifdef FFB_STAMPS
  BSTAMP(20);  // prologue + state store
  if (lane == 0) for (int k = 0; k < 24; k++) atomicAdd(&g_bstamps[k], c.st_acc[k]);
#endif
  if (phys_only) return;
  // ---- observation (ref: SURVEY App. A order): accelerometer 3 | actuator_activation 59 | appendages_pos 21 | ball_qvel 3 |
  //      force 18 | gyro 3 | joints_pos 85 | joints_vel 85 | touch 6 | velocimeter 3 | world_zaxis 3
#pragma unroll
  for (int s = 0; s < 3; s++) if (slot_on(c, s)) { T.Q[c.sdof[s]] = c.q[s]; T.V[c.sdof[s]] = c.v[s]; }
  {
    float *o = T.lk[lane];
    o[0] = c.xp.x; o[1] = c.xp.y; o[2] = c.xp.z; o[3] = c.xq.w; o[4] = c.xq.x; o[5] = c.xq.y; o[6] = c.xq.z;
  }
  DM_SYNC();
  float *ob = obs + (size_t)env * NOBS;
  const float inv = (do_reset && K.pad_first_obs) ? 1.f : 1.f / (float)M.nsub;
  const int nsamp = do_reset ? 1 : M.nsub;
  const M3 Rt = q2m(Q4{M.thorax_quat[0], M.thorax_quat[1], M.thorax_quat[2], M.thorax_quat[3]});
  const M3 Rs = q2m(Q4{M.site_quat[0], M.site_quat[1], M.site_quat[2], M.site_quat[3]});
  if (lane < 3) {
    // the thorax is welded to the world: accelerometer = R_site' (0, 0, -g), gyro = velocimeter = 0
    const V3 g = mtv(Rs, V3{0.f, 0.f, (c.flags & BF_NO_GRAVITY) ? 0.f : -M.gz});
    ob[lane] = (lane == 0 ? g.x : (lane == 1 ? g.y : g.z)) * (float)nsamp * inv;
    ob[3 + NU + 21 + 3 + 18 + lane] = 0.f;                       // gyro
    ob[3 + NU + 21 + 3 + 18 + 3 + 2 * NOBSJ + 6 + lane] = 0.f;   // velocimeter
    ob[3 + NU + 21 + 3 + 18 + 3 + 2 * NOBSJ + 6 + 3 + lane] = lane == 0 ? Rt.m6 : (lane == 1 ? Rt.m7 : Rt.m8);  // world_zaxis = xmat[6:9]
    ob[3 + NU + 21 + lane] = lane == 0 ? c.bw.x : (lane == 1 ? c.bw.y : c.bw.z);  // ball_qvel
  }
  if (lane < NU) ob[3 + lane] = do_reset ? 0.f : act_reg;
  if (lane < 7) {  // appendages_pos: (x_site - x_thorax) . R_thorax (ref: fruitfly.py:629-638)
    const int l = M.app_link[lane];
    const float *p = T.lk[l];
    const V3 sp = V3{p[0], p[1], p[2]} + qrot(Q4{p[3], p[4], p[5], p[6]}, V3{M.app_pos[lane][0], M.app_pos[lane][1], M.app_pos[lane][2]});
    const V3 rel = mtv(Rt, sp - V3{M.thorax_pos[0], M.thorax_pos[1], M.thorax_pos[2]});
    ob[3 + NU + 3 * lane] = rel.x; ob[3 + NU + 3 * lane + 1] = rel.y; ob[3 + NU + 3 * lane + 2] = rel.z;
  }
  if (lane < 18) ob[3 + NU + 21 + 3 + lane] = T.sens[lane] * inv;
  if (lane < 6) ob[3 + NU + 21 + 3 + 18 + 3 + 2 * NOBSJ + lane] = T.sens[18 + lane] * inv;
  for (int k = lane; k < NOBSJ; k += 64) {
    ob[3 + NU + 21 + 3 + 18 + 3 + k] = T.Q[M.obs_dof[k]];
    ob[3 + NU + 21 + 3 + 18 + 3 + NOBSJ + k] = T.V[M.obs_dof[k]];
  }
  // ---- reward / termination (ref: walk_on_ball.py:61-79, base.py:213-217)
  if (lane == 0) {
    if (do_reset) { rew[env] = 0.f; disc[env] = 1.f; st[env] = 0; S.needs_reset = 0; }
    else {
      float r = fmaxf(0.f, 1.f - fabsf(c.bw.x) / 6.f) * fmaxf(0.f, 1.f - fabsf(c.bw.y + 5.f) / 6.f) * fmaxf(0.f, 1.f - fabsf(c.bw.z) / 6.f);
      const bool bad = !(qn2 == qn2) || !(sqrtf(qn2) <= 1e14f);
      const bool timeup = step_counter >= K.time_limit_steps;
      if (bad && !(r == r)) r = 0.f;
      rew[env] = r; disc[env] = bad ? 0.f : 1.f; st[env] = (bad || timeup) ? 2 : 1;
      S.needs_reset = (bad || timeup) ? 1 : 0;
    }
  }
#ifdef FFE_TRACE
  __builtin_amdgcn_s_waitcnt(0);
  if (lane == 0 && blockIdx.x < 32768) {
    g_btrace[blockIdx.x][0] = tr_t0; g_btrace[blockIdx.x][1] = __builtin_amdgcn_s_memrealtime();
    g_btrace[blockIdx.x][2] = __builtin_amdgcn_s_getreg((31 << 11) | 4); g_btrace[blockIdx.x][3] = (__builtin_amdgcn_s_getreg((31 << 11) | 20) & 0xf) | ((unsigned long long)((unsigned)(iters & 0xff) | ((unsigned)((c.nc + c.nsc) & 0xff) << 8) | ((unsigned)(tr_prev & 0xffff) << 16)) << 8);
  }
#endif
}

__global__ void ball_init_states(BState *states, int *order, int *cost, int batch) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= batch) return;
  BState z;
  memset(&z, 0, sizeof(z));
  z.needs_reset = 1; z.ballq[0] = 1.f;
  states[i] = z;
  order[i] = i;
  cost[i] = 0;
}
__global__ void ball_get_state_kernel(const BState *states, double *qpos, double *qvel, int batch) {
  const int env = blockIdx.x, t = threadIdx.x;
  if (env >= batch) return;
  const BState &S = states[env];
  for (int k = t; k < 106; k += blockDim.x) qpos[(size_t)env * 106 + k] = k < 4 ? (double)S.ballq[k] : (double)S.q[k - 4];
  for (int k = t; k < 105; k += blockDim.x) qvel[(size_t)env * 105 + k] = k < 3 ? (double)S.ballw[k] : (double)S.v[k - 3];
}
__global__ void ball_set_state_kernel(BState *states, const double *qpos, const double *qvel, int batch) {
  const int env = blockIdx.x, t = threadIdx.x;
  if (env >= batch) return;
  BState &S = states[env];
  for (int k = t; k < 106; k += blockDim.x) { if (k < 4) S.ballq[k] = (float)qpos[(size_t)env * 106 + k]; else S.q[k - 4] = (float)qpos[(size_t)env * 106 + k]; }
  for (int k = t; k < 105; k += blockDim.x) { if (k < 3) S.ballw[k] = (float)qvel[(size_t)env * 105 + k]; else S.v[k - 3] = (float)qvel[(size_t)env * 105 + k]; }
  if (t == 0) { S.have_ws = 0; S.sd_cnt = 0; S.ws_n = 0; }
}
__global__ void ball_act_kernel(BState *states, double *act, int batch, int set) {
  const int env = blockIdx.x, t = threadIdx.x;
  if (env >= batch || t >= NU) return;
  if (set) states[env].act[t] = (float)act[(size_t)env * NU + t];
  else act[(size_t)env * NU + t] = (double)states[env].act[t];
}
__global__ void ball_task_state_kernel(const BState *states, int *ints, double *reals, int batch) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= batch) return;
  const BState &S = states[i];
  int *o = ints + (size_t)i * 8;
  o[0] = (int)S.con_hist[0]; o[1] = (int)S.con_hist[1]; o[2] = S.step_counter; o[3] = S.nself; o[4] = S.needs_reset; o[5] = S.ncon; o[6] = S.iters; o[7] = S.overflow;
  for (int k = 0; k < 8; k++) reals[(size_t)i * 8 + k] = 0.0;
  reals[(size_t)i * 8] = (double)((unsigned long long)S.det_hist[0] | ((unsigned long long)S.det_hist[1] << 32));  // (60 bits used: exact up to 10 substeps)
}

// ffe_get_validity: {step_bits, episode_flagged_steps, episode_bits, episode_steps} per env
__global__ void ball_validity_kernel(const BState *states, int *info, int batch) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= batch) return;
  const BState &S = states[i];
  *reinterpret_cast<int4 *>(info + (size_t)i * 4) = make_int4(S.step_bits, S.ep_flagged, S.overflow, S.step_counter);
}

// ================================================================================================ host side
struct BallEnv final : ffe::EnvBackend {
  BallHost host;
  BTaskDev task{};
  BallModel *model_dev = nullptr;
  BState *states = nullptr;
  int *order = nullptr, *cost = nullptr;  // launch order of the envs and its sort keys (launch_order.hpp)
  ffe::KernelTimer tm;
  double control_timestep = 0;

  ~BallEnv() override {
    (void)hipFree(model_dev); (void)hipFree(states); (void)hipFree(order); (void)hipFree(cost);
  }

  void spec(ffe_spec_t &s) const override {
    s = ffe_spec_t{};
    s.batch = batch; s.nq = 106; s.nv = 105; s.nu = NU; s.action_dim = NACT; s.obs_dim = NOBS; s.nsub = host.m.nsub;
    s.physics_timestep = host.m.h; s.control_timestep = control_timestep;
    // walk_on_ball row: accelerometer 3 | actuator_activation 59 | appendages_pos 21 | ball_qvel 3 | force 18 | gyro 3 |
    //                   joints_pos 85 | joints_vel 85 | touch 6 | velocimeter 3 | world_zaxis 3
    s.off_accelerometer = 0; s.off_gyro = 104; s.off_joints_pos = 107; s.off_joints_vel = 192; s.off_velocimeter = 283; s.off_world_zaxis = 286;
    s.off_ref_displacement = -1; s.off_ref_root_quat = -1; s.n_obs_joints = NOBSJ; s.n_ref = 0;
  }
  void action_bounds(float *mn, float *mx) const override {
    for (int k = 0; k < NACT; k++) { mn[k] = host.action_min[k]; mx[k] = host.action_max[k]; }
  }
  ffe::KernelTimer *timer() override { return &tm; }

  void launch(const float *act, float *obs, float *rew, float *disc, int32_t *st, void *stream, int mode, int nphys, const uint8_t *mask) override {
    // (not ffe::Refused: these two have always come out as -2, and the header's table says so)
    if (mode != 1 && mode != 3 && !act) throw std::runtime_error("walk_on_ball: null action buffer");
    if (mode != 2 && (!obs || !rew || !disc || !st)) throw std::runtime_error("walk_on_ball: null output buffer");
    hipStream_t s = (hipStream_t)stream;
    tm.start(s);
    hipLaunchKernelGGL(ball_step_kernel, dim3(batch), dim3(64), 0, s, model_dev, task, states, act, obs, rew, disc, st, batch, mode, nphys, order, cost, mask);
    HIP_OK(hipGetLastError());
    tm.stop(s);
    if (mode == 0 && batch > 1) {
      hipLaunchKernelGGL(ffe_order::order_by_cost, dim3(1), dim3(1024), 0, s, cost, order, batch);
      HIP_OK(hipGetLastError());
    }
    tm.collect();
  }
  void force_next_episode(const int32_t *, const double *, void *) override { throw ffe::Refused("walk_on_ball episodes have no per-episode randomness"); }

  void get_state(double *qpos, double *qvel, void *stream) override {
    hipLaunchKernelGGL(ball_get_state_kernel, dim3(batch), dim3(128), 0, (hipStream_t)stream, states, qpos, qvel, batch);
    HIP_OK(hipGetLastError());
  }
  void set_state(const double *qpos, const double *qvel, void *stream) override {
    hipLaunchKernelGGL(ball_set_state_kernel, dim3(batch), dim3(128), 0, (hipStream_t)stream, states, qpos, qvel, batch);
    HIP_OK(hipGetLastError());
  }
  void get_act(double *act, void *stream) override {
    hipLaunchKernelGGL(ball_act_kernel, dim3(batch), dim3(64), 0, (hipStream_t)stream, states, act, batch, 0);
    HIP_OK(hipGetLastError());
  }
  void set_act(const double *act, void *stream) override {
    hipLaunchKernelGGL(ball_act_kernel, dim3(batch), dim3(64), 0, (hipStream_t)stream, states, const_cast<double *>(act), batch, 1);
    HIP_OK(hipGetLastError());
  }
  void get_task_state(int32_t *ints, double *reals, void *stream) override {
    hipLaunchKernelGGL(ball_task_state_kernel, dim3((batch + 63) / 64), dim3(64), 0, (hipStream_t)stream, states, ints, reals, batch);
    HIP_OK(hipGetLastError());
  }
  void get_validity(int32_t *info, void *stream) override {
    hipLaunchKernelGGL(ball_validity_kernel, dim3((batch + 63) / 64), dim3(64), 0, (hipStream_t)stream, states, info, batch);
    HIP_OK(hipGetLastError());
  }
};

std::unique_ptr<ffe::EnvBackend> ball_create(const void *blob, size_t blob_size, const BallTaskHost &task, int batch, int device) {
  if (!blob || batch <= 0) throw std::runtime_error("ffe_create_walk_on_ball: bad arguments");
  std::unique_ptr<BallEnv> e(new BallEnv());  // frees the device allocations made so far if a later step throws
  Blob b(blob, blob_size);
  e->host = build_ball_model(b);
  e->device = device; e->batch = batch;
  e->control_timestep = task.control_timestep;
  e->host.m.nsub = (int)llround(task.control_timestep / (double)e->host.m.h);
  if (e->host.m.nsub < 1 || e->host.m.nsub > 64) throw std::runtime_error("walk_on_ball: bad control timestep");
  e->task.time_limit_steps = task.time_limit_steps; e->task.pad_first_obs = task.pad_first_obs; e->task.flags = task.physics_flags;
  e->task.canonical = task.canonical_actions; e->task.clip = task.clip_actions;
  HIP_OK(hipMalloc((void **)&e->model_dev, sizeof(BallModel)));
  HIP_OK(hipMemcpy(e->model_dev, &e->host.m, sizeof(BallModel), hipMemcpyHostToDevice));
  HIP_OK(hipMalloc((void **)&e->states, sizeof(BState) * (size_t)batch));
  HIP_OK(hipMalloc((void **)&e->order, sizeof(int) * (size_t)batch));
  HIP_OK(hipMalloc((void **)&e->cost, sizeof(int) * (size_t)batch));
  hipLaunchKernelGGL(ball_init_states, dim3((batch + 63) / 64), dim3(64), 0, 0, e->states, e->order, e->cost, batch);
  HIP_OK(hipGetLastError());
  HIP_OK(hipDeviceSynchronize());
  e->tm.create();
  return e;
}
#ifdef FFE_TRACE
extern "C" int ffb_debug_read_trace(unsigned long long *out, int nrows) {
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_btrace), (size_t)nrows * 4 * sizeof(unsigned long long)) == hipSuccess ? 0 : -1;
}
#endif
#ifdef FFB_STAMPS
extern "C" int ffb_debug_read_stamps(unsigned long long *out24, int reset) {
  if (hipMemcpyFromSymbol(out24, HIP_SYMBOL(g_bstamps), 24 * sizeof(unsigned long long)) != hipSuccess) return -1;
  if (reset) { unsigned long long z[24] = {0}; if (hipMemcpyToSymbol(HIP_SYMBOL(g_bstamps), z, sizeof(z)) != hipSuccess) return -1; }
  return 0;
}
#endif

}  // namespace ffb
