// leg_dyn.hpp - the leg code both fly step kernels run: per-lane helpers, the constraint impedance, the block factorisation and the
// triangular solves of the joint-space inertia, and - as the text fragment leg_stage1.inc, included into the body of each kernel's stage 1 - the dynamics half
// of stage 1 (kinematics, velocities / bias accelerations, body forces, subtree sums, smooth joint forces, inertia assembly,
// factorisation).  Written once, compiled per translation unit:
//   ball_env.hip  FREE_ROOT = false: the thorax is welded to the world (walk_on_ball);
//   walk_env.hip  FREE_ROOT = true:  the thorax hangs on a free joint (walk_imitation).  Everything is expressed
//                 in the root body frame about the root origin, where the legs' kinematics are the tethered fly's: the root adds its
//                 spatial velocity `c.V0 = (w_b, R' v_w)` to every path sum; the halteres become ordinary single-hinge links of the root
//                 (`c.X`, walk_model.hpp); `c.Itree` / `c.Ftot` return the spatial inertia and bias force of all links together (the
//                 root's own excluded).  Gravity is not in these bias forces: the fictitious base acceleration -R' g of every link
//                 is M e_r (-R' g), so the caller solves without it and adds g to the root's linear acceleration (walk_env.hip).
// The two kernels live in separate translation units on purpose: instantiations of one kernel template compiled together share a
// register-allocation context, and the benchmarked tethered kernel must not move when the free-root one changes.
// The context type C carries what the Ctx of ball_env.hip carries (M, T, lane, flags, lpack, sdof, q, v, fnb, xh, xp, xip, xq, cvel,
// caccb, mass); the tile type behind c.T the arrays X4, dadd, Mq, F, lk, Lm, Lh, dinv_m, dinv_h, C.
#pragma once
#include <hip/hip_runtime.h>

#include "ball_model.hpp"
#include "dev_math.hpp"

namespace ffb {
using namespace dm;

enum { BF_NO_FLUID = 1, BF_NO_LIMIT = 2, BF_NO_DAMPER = 4, BF_NO_SPRING = 8, BF_NO_GRAVITY = 16, BF_NO_ACTUATION = 32,
       BF_NO_CONTACT = 64, BF_NO_NOSLIP = 128, BF_NO_ADHESION = 256 };

// Keeps the fully unrolled per-entry loops from being interleaved into one huge basic block of loads: without it the
// scheduler hoists every entry's LDS reads to the top and the kernel needs > 500 VGPRs.
#define ENTRY_FENCE() __builtin_amdgcn_sched_barrier(0)
// Loop-invariant code motion otherwise precomputes every LDS address derived from the per-lane entry / slot words once per
// launch and keeps ~150 of them alive across the substep loop; an opaque copy forces the (cheap) address math to stay local.
__device__ __forceinline__ unsigned opq(unsigned x) { asm volatile("" : "+v"(x)); return x; }
__device__ __forceinline__ int opq(int x) { asm volatile("" : "+v"(x)); return x; }
#ifndef BSTAMP
#define BSTAMP(k) do { } while (0)
#endif

template <class C>
__device__ __forceinline__ bool slot_on(const C &c, int s) { return c.sdof[s] >= 0; }
template <class C>
__device__ __forceinline__ int l_parent(const C &c) { return (int)(c.lpack & 0xffu) - 1; }
template <class C>
__device__ __forceinline__ int l_ndof(const C &c) { return (int)((c.lpack >> 12) & 0x3u); }
// The tables are read through an address-space-1 pointer: a generic pointer makes every table read a FLAT load, which
// counts against the LDS wait counter as well, so each LDS wait would also wait for the schedule prefetch.
typedef const BallModel FFE_GLOBAL *ModelPtr;
template <class C>
__device__ __forceinline__ const BallModel FFE_GLOBAL &model(const C &c) {
  ModelPtr m = (ModelPtr)c.M;
  asm volatile("" : "+s"(m));
  return *m;
}

// ------------------------------------------------------------------------------------------------ impedance
// mj: getimpedance (margin folded into `x` by the caller: x = |pos - margin|)
__device__ __forceinline__ float impedance(const float *si, float x) {
  float d0 = fminf(fmaxf(si[0], 1e-4f), 0.9999f), d1 = fminf(fmaxf(si[1], 1e-4f), 0.9999f);
  const float width = fmaxf(0.f, si[2]), mid = fminf(fmaxf(si[3], 1e-4f), 0.9999f), power = fmaxf(1.f, si[4]);
  if (d0 == d1 || width <= 1e-15f) return 0.5f * (d0 + d1);
  x = x * frcp(width);
  if (x >= 1.f) return d1;
  if (x <= 0.f) return d0;
  float y;
  if (power == 1.f) y = x;
  else if (power == 2.f) y = x <= mid ? x * x * frcp(mid) : 1.f - (1.f - x) * (1.f - x) * frcp(1.f - mid);
  else if (x <= mid) y = powf(x, power) / powf(mid, power - 1.f);
  else y = 1.f - powf(1.f - x, power) / powf(1.f - mid, power - 1.f);
  return d0 + y * (d1 - d0);
}

// ------------------------------------------------------------------------------------------------ block factorisation
// mj: mj_factorI on M's 12 independent blocks, all blocks in lock step (step s eliminates every block's s-th pivot from the
// leaf end).  The matrix lives in LDS, so any lane can apply any update: the host lays the ~2300 updates
//   L[e] -= L[ki] * L[kj] / L[kk]        (e = (i, j), i a proper ancestor of the pivot k; values stay unscaled until the end)
// out in step order as `nfs` slots of 64 independent updates (ball_model.hpp), read coalesced and one slot ahead.
// LDS operations of a wave complete in issue order, which is all the ordering the steps need.
template <class C>
__device__ __forceinline__ void factor2(C &c) {
  // factorises M into T.Lm and M + diag(T.dadd) into T.Lh in one pass over the schedule (same elimination order, so the
  // schedule words, address arithmetic and control flow are shared)
  auto &T = *c.T;
  const BallModel FFE_GLOBAL &M = model(c);
  const int lane = c.lane;
#pragma unroll
  for (int t = 0; t < ECAP; t++) {
    const unsigned ea = M.ent_a[t][lane];
    if (ea >> 31) {
      const unsigned i = ea & 0xffu, j = (ea >> 8) & 0xffu, adr = (ea >> 16) & 0x3ffu;
      const float vv = T.Mq[adr];
      T.Lm[adr] = vv;
      T.Lh[adr] = i == j ? vv + T.dadd[i] : vv;
    }
  }
  DM_SYNC();
  // Schedule words are fetched one group of four slots ahead (tables are zero padded past nfs).  No fence inside the loop:
  // the LDS accesses of consecutive slots may alias, so the compiler keeps their order, and the hardware executes a
  // wave's LDS operations in issue order.
  const int nfs = M.nfs;
  unsigned wa[4], wb[4];
#pragma unroll
  for (int q = 0; q < 4; q++) { wa[q] = M.fac_a[q][lane]; wb[q] = M.fac_b[q][lane]; }
#pragma unroll 1
  for (int base = 0; base < nfs; base += 4) {
    unsigned ca[4], cb[4];
#pragma unroll
    for (int q = 0; q < 4; q++) { ca[q] = wa[q]; cb[q] = wb[q]; }
#pragma unroll
    for (int q = 0; q < 4; q++) { wa[q] = M.fac_a[base + 4 + q][lane]; wb[q] = M.fac_b[base + 4 + q][lane]; }
#pragma unroll
    for (int q = 0; q < 4; q++) {
      const unsigned a = ca[q], b = cb[q];
      if (a >> 31) {
        const unsigned akk = (a >> 10) & 0x3ffu, aki = (a >> 20) & 0x3ffu, akj = b & 0x3ffu, ae = a & 0x3ffu;
        const float mkk = T.Lm[akk], mki = T.Lm[aki], mkj = T.Lm[akj], hkk = T.Lh[akk], hki = T.Lh[aki], hkj = T.Lh[akj];
        T.Lm[ae] -= mki * mkj * frcp(mkk);
        T.Lh[ae] -= hki * hkj * frcp(hkk);
      }
    }
  }
  DM_SYNC();
#pragma unroll
  for (int t = 0; t < ECAP; t++) {
    const unsigned ea = M.ent_a[t][lane];
    if ((ea >> 31) && (ea & 0xffu) == ((ea >> 8) & 0xffu)) {
      T.dinv_m[ea & 0xffu] = frcp(T.Lm[(ea >> 16) & 0x3ffu]);
      T.dinv_h[ea & 0xffu] = frcp(T.Lh[(ea >> 16) & 0x3ffu]);
    }
  }
  DM_SYNC();
#pragma unroll
  for (int t = 0; t < ECAP; t++) {
    const unsigned ea = M.ent_a[t][lane];
    if ((ea >> 31) && (ea & 0xffu) != ((ea >> 8) & 0xffu)) {
      T.Lm[(ea >> 16) & 0x3ffu] *= T.dinv_m[ea & 0xffu];
      T.Lh[(ea >> 16) & 0x3ffu] *= T.dinv_h[ea & 0xffu];
    }
  }
  DM_SYNC();
}

// mj: mj_solveLD on T.X4 (four right-hand sides at once): rows leaf -> root, D^-1, columns root -> leaf, from the two
// schedules p1 / p2 (slots of 64 independent updates in step order)
template <class C>
__device__ __forceinline__ void solve4(C &c, const float *L, const float *dinv) {
  auto &T = *c.T;
  const BallModel FFE_GLOBAL &M = model(c);
  const int lane = c.lane;
  {
    const int n = M.np1;
    unsigned wq[4];
#pragma unroll
    for (int q = 0; q < 4; q++) wq[q] = M.p1[q][lane];
#pragma unroll 1
    for (int base = 0; base < n; base += 4) {
      unsigned cw[4];
#pragma unroll
      for (int q = 0; q < 4; q++) cw[q] = wq[q];
#pragma unroll
      for (int q = 0; q < 4; q++) wq[q] = M.p1[base + 4 + q][lane];
#pragma unroll
      for (int q = 0; q < 4; q++) {
        const unsigned w = cw[q];
        if (w >> 31) {
          const unsigned i = (w >> 10) & 0x7fu, j = (w >> 17) & 0x7fu;
          const float l = L[w & 0x3ffu];
          const float4 xi = T.X4[i];
          float4 xj = T.X4[j];
          xj.x -= l * xi.x; xj.y -= l * xi.y; xj.z -= l * xi.z; xj.w -= l * xi.w;
          T.X4[j] = xj;
        }
      }
    }
    DM_SYNC();
  }
  for (int f = lane; f < ND; f += 64) {
    const float dv = dinv[f];
    float4 x = T.X4[f];
    x.x *= dv; x.y *= dv; x.z *= dv; x.w *= dv;
    T.X4[f] = x;
  }
  DM_SYNC();
  {
    const int n = M.np2;
    unsigned wq[4];
#pragma unroll
    for (int q = 0; q < 4; q++) wq[q] = M.p2[q][lane];
#pragma unroll 1
    for (int base = 0; base < n; base += 4) {
      unsigned cw[4];
#pragma unroll
      for (int q = 0; q < 4; q++) cw[q] = wq[q];
#pragma unroll
      for (int q = 0; q < 4; q++) wq[q] = M.p2[base + 4 + q][lane];
#pragma unroll
      for (int q = 0; q < 4; q++) {
        const unsigned w = cw[q];
        if (w >> 31) {
          const unsigned i = (w >> 10) & 0x7fu, j = (w >> 17) & 0x7fu;
          const float l = L[w & 0x3ffu];
          const float4 xj = T.X4[j];
          float4 xi = T.X4[i];
          xi.x -= l * xj.x; xi.y -= l * xj.y; xi.z -= l * xj.z; xi.w -= l * xj.w;
          T.X4[i] = xi;
        }
      }
    }
    DM_SYNC();
  }
}

// Two single-right-hand-side solves with two factors of the same structure in one pass over the schedules:
// T.X4[.].x <- (L_A D_A L_A')^-1 x, T.X4[.].y <- (L_B D_B L_B')^-1 y   (final acceleration with M, Euler with M + h B)
template <class C>
__device__ __forceinline__ void solve_dual(C &c, const float *LA, const float *dinvA, const float *LB, const float *dinvB) {
  auto &T = *c.T;
  const BallModel FFE_GLOBAL &M = model(c);
  const int lane = c.lane;
  {
    const int n = M.np1;
    unsigned wq[4];
#pragma unroll
    for (int q = 0; q < 4; q++) wq[q] = M.p1[q][lane];
#pragma unroll 1
    for (int base = 0; base < n; base += 4) {
      unsigned cw[4];
#pragma unroll
      for (int q = 0; q < 4; q++) cw[q] = wq[q];
#pragma unroll
      for (int q = 0; q < 4; q++) wq[q] = M.p1[base + 4 + q][lane];
#pragma unroll
      for (int q = 0; q < 4; q++) {
        const unsigned w = cw[q];
        if (w >> 31) {
          const unsigned i = (w >> 10) & 0x7fu, j = (w >> 17) & 0x7fu;
          const float la = LA[w & 0x3ffu], lb = LB[w & 0x3ffu];
          const float4 xi = T.X4[i];
          float4 xj = T.X4[j];
          xj.x -= la * xi.x; xj.y -= lb * xi.y;
          T.X4[j] = xj;
        }
      }
    }
    DM_SYNC();
  }
  for (int f = lane; f < ND; f += 64) {
    float4 x = T.X4[f];
    x.x *= dinvA[f]; x.y *= dinvB[f];
    T.X4[f] = x;
  }
  DM_SYNC();
  {
    const int n = M.np2;
    unsigned wq[4];
#pragma unroll
    for (int q = 0; q < 4; q++) wq[q] = M.p2[q][lane];
#pragma unroll 1
    for (int base = 0; base < n; base += 4) {
      unsigned cw[4];
#pragma unroll
      for (int q = 0; q < 4; q++) cw[q] = wq[q];
#pragma unroll
      for (int q = 0; q < 4; q++) wq[q] = M.p2[base + 4 + q][lane];
#pragma unroll
      for (int q = 0; q < 4; q++) {
        const unsigned w = cw[q];
        if (w >> 31) {
          const unsigned i = (w >> 10) & 0x7fu, j = (w >> 17) & 0x7fu;
          const float la = LA[w & 0x3ffu], lb = LB[w & 0x3ffu];
          const float4 xj = T.X4[j];
          float4 xi = T.X4[i];
          xi.x -= la * xj.x; xi.y -= lb * xj.y;
          T.X4[i] = xi;
        }
      }
    }
    DM_SYNC();
  }
}

// ------------------------------------------------------------------------------------------------ stage 1
// mj: mj_inertiaBoxFluidModel for one body: the wrench (about the reference origin) of the drag on a body whose inertial frame has
// orientation `ximat` and sits at `r` from that origin, moving with the spatial velocity `vel` (about the same origin)
__device__ __forceinline__ S6 box_drag(const float *fl, const M3 &ximat, V3 r, S6 vel) {
  const V3 wl = mtv(ximat, ang(vel)), vl = mtv(ximat, lin(vel) + cross(ang(vel), r));
  const V3 Tl = {-fl[0] * wl.x - fl[5] * fabsf(wl.x) * wl.x, -fl[0] * wl.y - fl[6] * fabsf(wl.y) * wl.y, -fl[0] * wl.z - fl[7] * fabsf(wl.z) * wl.z};
  const V3 Fl = {-fl[1] * vl.x - fl[2] * fabsf(vl.x) * vl.x, -fl[1] * vl.y - fl[3] * fabsf(vl.y) * vl.y, -fl[1] * vl.z - fl[4] * fabsf(vl.z) * vl.z};
  const V3 Tw = mv(ximat, Tl), Fw = mv(ximat, Fl);
  return mk6(Tw + cross(r, Fw), Fw);
}

// Free root only: the haltere this lane carries in slot 2, as a single-hinge link of the root (frame, axis and inertia from c.X, all in
// the root frame about the root origin).  Stores the dof's motion axis (T.C) and its column of the inertia (T.F), returns the link's
// spatial inertia and bias force for the tree totals, and the dof's smooth force without actuation.
template <class C>
__device__ __forceinline__ float haltere_link(C &c, I10 &cin, S6 &frc) {
  auto &T = *c.T;
  const BallModel FFE_GLOBAL &M = model(c);
  const auto &X = *c.X;
  const int lane = c.lane, f = c.sdof[2];
  const V3 xp = {X.hx_pos[0][lane], X.hx_pos[1][lane], X.hx_pos[2][lane]}, axis = {X.hx_axis[0][lane], X.hx_axis[1][lane], X.hx_axis[2][lane]};
  const Q4 quat = {X.hx_quat[0][lane], X.hx_quat[1][lane], X.hx_quat[2][lane], X.hx_quat[3][lane]};
  float sn, cs;
  fsincos(0.5f * c.q[2], &sn, &cs);
  const Q4 xq = qnormalize(qmul(quat, Q4{cs, axis.x * sn, axis.y * sn, axis.z * sn}));
  const V3 axw = qrot(quat, axis);
  const S6 cdof = mk6(axw, cross(xp, axw));  // about the root origin: axis x (origin - anchor)
  const M3 xmat = q2m(xq);
  const V3 xip = xp + mv(xmat, V3{X.hx_ipos[0][lane], X.hx_ipos[1][lane], X.hx_ipos[2][lane]});
  const M3 ximat = q2m(qmul(xq, Q4{X.hx_iquat[0][lane], X.hx_iquat[1][lane], X.hx_iquat[2][lane], X.hx_iquat[3][lane]}));
  cin = inert_com(V3{X.hx_inertia[0][lane], X.hx_inertia[1][lane], X.hx_inertia[2][lane]}, ximat, xip, X.hx_mass[lane]);
  const S6 vel = c.V0 + c.v[2] * cdof;
  const S6 acc = c.v[2] * cross_motion(c.V0, cdof);
  frc = mul_inert(cin, acc) + cross_force(vel, mul_inert(cin, vel));
  if (!(c.flags & BF_NO_FLUID)) {
    float fl[8];
#pragma unroll
    for (int k = 0; k < 8; k++) fl[k] = X.hx_fl[k][lane];
    frc = frc - box_drag(fl, ximat, xip, vel);
  }
  st6(T.C[f], cdof);
  st6(T.F[f], mul_inert(cin, cdof));
  float g = -dot6(cdof, frc);
  if (!(c.flags & BF_NO_SPRING)) g -= M.s_stiff[2][lane] * (c.q[2] - M.s_sref[2][lane]);
  if (!(c.flags & BF_NO_DAMPER)) g -= M.s_damp[2][lane] * c.v[2];
  return g;
}


}  // namespace ffb
