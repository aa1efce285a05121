// walk_task.hpp - task layer of fly_envs.walk_imitation (stage 4): forward kinematics of the walking fly in
// its root body frame, the walker features of tasks/rewards.py:36-61, the four DeepMimic reward factors, the termination bits and
// the kinematic columns of the observation row - a pure function of (qpos, qvel, clip, step).
//
// The maths is templated on the scalar type T (float, double) and compiles for the host with -DWT_HOST (tests/walk_task_host.cpp),
// where the 64 lanes of a wavefront become a loop; walk_task.hip holds the kernels and the C ABI only.  One wavefront works on one
// state row.  The root position qpos[0:3] and every difference taken against it stay float64 whatever T is (DESIGN.md sections 5
// and 12: 20 cm of walking against features of 1e-4 cm).
//
// Root frame: the thorax is at the origin with the identity orientation, so root2site, the joint axes "rotated by the inverse
// root quaternion" and appendages_pos come out of the kinematics directly; the only world quantities are world_zaxis and the
// reference displacements.
#pragma once

#include <cmath>
#include <cstdint>
#include <cstring>
#include <map>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/flybody_env.h"

#if defined(WT_HOST)
#define WT_FN inline
#define WT_SYNC() ((void)0)
#define WT_LANE_FIRST 0
#define WT_LANE_STEP 1
#define WT_ACC 64
#ifndef WT_RECORD_ROW  // the host harness records every reference row index the code forms: (row, first row of the clip, one past its last)
#define WT_RECORD_ROW(row, lo, hi) ((void)0)
#endif
#else
#define WT_FN __device__ __forceinline__
#define WT_SYNC() __syncthreads()
#define WT_LANE_FIRST ((int)threadIdx.x)
#define WT_LANE_STEP 64
#define WT_ACC 1
#define WT_RECORD_ROW(row, lo, hi) ((void)0)
#endif
// the body runs once per lane: on the device for this thread, on the host for lanes 0 .. 63 in turn
#define WT_LANES(lane) for (int lane = WT_LANE_FIRST; lane < 64; lane += WT_LANE_STEP)

namespace wt {

constexpr int kJntFree = 0, kJntHinge = 3;

// Device (or host) view of everything a row needs.  Per-body / per-joint / per-site tables are field-major ("[field][index]") so
// that the lanes of a wave, one body or joint each, read consecutive words.
template <class T>
struct Tables {
  int nbody, njnt, nq, nv, nsite, maxdepth;
  const int *b_parent, *b_depth, *b_jntadr, *b_jntnum;  // [nbody]
  const T *b_pos, *b_quat;                               // [3][nbody], [4][nbody]
  const int *j_qadr;                                     // [njnt]
  const double *j_q0;                                    // [njnt] qpos0 at the joint's address
  const T *j_pos, *j_axis;                               // [3][njnt]
  const int *s_body;                                     // [nsite]
  const T *s_pos;                                        // [3][nsite]
  int J, S, nappend, nobsj;
  const int *t_jnt, *t_qadr, *t_dadr, *t_site;           // tracked joints [J] (index, qpos address, dof address), sites [S]
  const int *app_site, *obs_qadr, *obs_dadr;             // appendages_pos sites, joints_pos / joints_vel addresses
  // reference clips, rows concatenated
  int ntraj, future, inference;
  const int *traj_off, *ep_steps;                        // [ntraj + 1], [ntraj]
  const double *r_root7, *r_jang;                        // [rows][7] root pose, [rows][J] tracked joint angles (exact copies)
  const T *r_qvel, *r_r2s, *r_jq;                        // [rows][6 + J], [rows][3 S], [rows][4 J]
  // reference_pose: qpos[a] = pose_src[a] < 0 ? pose_const[a] : column pose_src[a] of (root7 | jang)
  const int *pose_src;                                   // [nq]
  const double *pose_const;                              // [nq]
  double term_dist;
  T coef[4], weight[4];                                  // factor k = weight[k] exp(coef[k] diff[k]), coef = -0.5 / std^2
  int off_app, off_jpos, off_jvel, off_disp, off_rquat, off_zaxis, obs_dim;

  template <class F>
  void each_ptr(F f) {
    f(b_parent); f(b_depth); f(b_jntadr); f(b_jntnum); f(b_pos); f(b_quat); f(j_qadr); f(j_q0); f(j_pos); f(j_axis); f(s_body); f(s_pos);
    f(t_jnt); f(t_qadr); f(t_dadr); f(t_site); f(app_site); f(obs_qadr); f(obs_dadr); f(traj_off); f(ep_steps); f(r_root7); f(r_jang);
    f(r_qvel); f(r_r2s); f(r_jq); f(pose_src); f(pose_const);
  }
};

// ------------------------------------------------------------------------------------------------ scalar helpers
WT_FN float sqrt_(float x) { return sqrtf(x); }
WT_FN double sqrt_(double x) { return sqrt(x); }
WT_FN float sin_(float x) { return sinf(x); }
WT_FN double sin_(double x) { return sin(x); }
WT_FN float cos_(float x) { return cosf(x); }
WT_FN double cos_(double x) { return cos(x); }
WT_FN float exp_(float x) { return expf(x); }
WT_FN double exp_(double x) { return exp(x); }
WT_FN float asin_(float x) { return asinf(x); }
WT_FN double asin_(double x) { return asin(x); }

// mju_rotVecQuat as model/quat.py::rot evaluates it (the unnormalised sandwich product through the matrix)
template <class T>
WT_FN void rot(T *r, const T *v, const T *q) {
  const T w = q[0], x = q[1], y = q[2], z = q[3];
  const T r0 = (w * w + x * x - y * y - z * z) * v[0] + 2 * (x * y - w * z) * v[1] + 2 * (x * z + w * y) * v[2];
  const T r1 = 2 * (x * y + w * z) * v[0] + (w * w - x * x + y * y - z * z) * v[1] + 2 * (y * z - w * x) * v[2];
  const T r2 = 2 * (x * z - w * y) * v[0] + 2 * (y * z + w * x) * v[1] + (w * w - x * x - y * y + z * z) * v[2];
  r[0] = r0; r[1] = r1; r[2] = r2;
}
template <class T>
WT_FN void qmul(T *r, const T *a, const T *b) {
  const T w = a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3];
  const T x = a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2];
  const T y = a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1];
  const T z = a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0];
  r[0] = w; r[1] = x; r[2] = y; r[3] = z;
}
template <class T>
WT_FN void qnormalize(T *q) {  // model/quat.py::normalize
  const T n = sqrt_(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  if (n < T(1e-15)) { q[0] = 1; q[1] = 0; q[2] = 0; q[3] = 0; return; }
  const T s = 1 / n;
  q[0] *= s; q[1] *= s; q[2] *= s; q[3] *= s;
}

// quaternions.py:205-249 quat_z2vec: the rotation taking the z axis to `vec`.  The reference forms (cos(a/2), sin(a/2) axis) with
// a = acos(v_z) and axis = (-v_y, v_x, 0) / |.|; since cos(a/2) = sqrt((1 + v_z)/2) and sin(a/2) / |(-v_y, v_x)| = 1 / sqrt(2 (1 + v_z))
// that is (1 + v_z, -v_y, v_x, 0) / sqrt(2 (1 + v_z)): the same quaternion without the acos, whose float32 value next to
// v_z = +-1 is ill-conditioned.  The exact-zero edge branch (v_x == v_y == 0) is the reference's.
template <class T>
WT_FN void quat_z2vec(T *q, const T *vec) {
  T v0 = vec[0], v1 = vec[1], v2 = vec[2];
  const bool edge = v0 == T(0) && v1 == T(0);
  if (edge) v0 = 1;  // the reference's placeholder; only the sign of v_z is read below
  const T inv = 1 / sqrt_(v0 * v0 + v1 * v1 + v2 * v2);
  v0 *= inv; v1 *= inv; v2 *= inv;
  if (edge) {
    q[0] = v2 < 0 ? T(0) : T(1); q[1] = v2 < 0 ? T(1) : T(0); q[2] = 0; q[3] = 0;
    return;
  }
  const T s = 1 / sqrt_(2 * (1 + v2));
  q[0] = (1 + v2) * s; q[1] = -v1 * s; q[2] = v0 * s; q[3] = 0;
}
// quaternions.py:298-321 joint_orientation_quat = axis_angle_to_quat(xaxis, qpos) * quat_z2vec(xaxis)
template <class T>
WT_FN void joint_orientation_quat(T *out, const T *xaxis, T qpos) {
  T q1[4], q2[4];
  quat_z2vec(q1, xaxis);
  const T inv = 1 / sqrt_(xaxis[0] * xaxis[0] + xaxis[1] * xaxis[1] + xaxis[2] * xaxis[2]);
  const T h = qpos * T(0.5), s = sin_(h) * inv;
  q2[0] = cos_(h); q2[1] = s * xaxis[0]; q2[2] = s * xaxis[1]; q2[3] = s * xaxis[2];
  qmul(out, q2, q1);
}
// quaternions.py:273-295 quat_dist_short_arc, squared: theta = acos(min(1, 2 (a.b)^2 - 1)) on normalised a, b.  With c = |a.b| and
// c = cos(phi), theta = 2 phi, and |a - sign(a.b) b|^2 = 2 - 2 c = 4 sin^2(phi/2), so theta = 4 asin(|a - sign(a.b) b| / 2): the
// difference is formed element-wise and stays well-conditioned where acos of a value next to 1 is not.  min(1, .) survives as the
// clamp of the asin argument and as theta -> 0, never NaN, when rounding puts c above 1.
template <class T>
WT_FN T short_arc_sq(const T *a, const T *b) {
  const T ia = 1 / sqrt_(a[0] * a[0] + a[1] * a[1] + a[2] * a[2] + a[3] * a[3]);
  const T ib = 1 / sqrt_(b[0] * b[0] + b[1] * b[1] + b[2] * b[2] + b[3] * b[3]);
  const T a0 = a[0] * ia, a1 = a[1] * ia, a2 = a[2] * ia, a3 = a[3] * ia;
  T b0 = b[0] * ib, b1 = b[1] * ib, b2 = b[2] * ib, b3 = b[3] * ib;
  if (a0 * b0 + a1 * b1 + a2 * b2 + a3 * b3 < 0) { b0 = -b0; b1 = -b1; b2 = -b2; b3 = -b3; }
  const T d0 = a0 - b0, d1 = a1 - b1, d2 = a2 - b2, d3 = a3 - b3;
  T h = T(0.5) * sqrt_(d0 * d0 + d1 * d1 + d2 * d2 + d3 * d3);
  if (h > 1) h = 1;
  const T th = 4 * asin_(h);
  return th * th;
}

// sum over the wave; every lane (the host: element 0) ends with the total, added in the same butterfly order on both sides
template <class T>
WT_FN T wave_sum(T *a) {
#if defined(WT_HOST)
  for (int o = 32; o > 0; o >>= 1) {
    T n[64];
    for (int l = 0; l < 64; l++) n[l] = a[l] + a[l ^ o];
    for (int l = 0; l < 64; l++) a[l] = n[l];
  }
  return a[0];
#else
  T v = a[0];
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
#endif
}

// reference row `k` of clip `c`, clamped to the clip's own rows
template <class T>
WT_FN int ref_row(const Tables<T> &t, int c, long long k) {
  const int lo = t.traj_off[c], hi = t.traj_off[c + 1];
  long long r = k < 0 ? 0 : k;
  if (r > (long long)(hi - lo - 1)) r = hi - lo - 1;
  const int row = lo + (int)r;
  WT_RECORD_ROW(row, lo, hi);
  return row;
}
template <class T>
WT_FN int clamp_clip(const Tables<T> &t, int c) { return c < 0 ? 0 : (c >= t.ntraj ? t.ntraj - 1 : c); }

// ------------------------------------------------------------------------------------------------ kinematics
// Pose of body b from its parent's, model/pyref.py::kinematics: the k-th hinge's anchor and axis are taken in the body frame
// after the hinges before k have been applied.  P [7][nbody] (pos, quat), AX [3][njnt], both in the root frame.
template <class T>
WT_FN void body_pose(const Tables<T> &t, int b, const double *qpos, T *P, T *AX) {
  const int NB = t.nbody, NJ = t.njnt, p = t.b_parent[b];
  const T pp[3] = {P[p], P[NB + p], P[2 * NB + p]}, pq[4] = {P[3 * NB + p], P[4 * NB + p], P[5 * NB + p], P[6 * NB + p]};
  const T bp[3] = {t.b_pos[b], t.b_pos[NB + b], t.b_pos[2 * NB + b]};
  const T bq[4] = {t.b_quat[b], t.b_quat[NB + b], t.b_quat[2 * NB + b], t.b_quat[3 * NB + b]};
  T pos[3], quat[4];
  rot(pos, bp, pq);
  pos[0] += pp[0]; pos[1] += pp[1]; pos[2] += pp[2];
  qmul(quat, pq, bq);
  const int adr = t.b_jntadr[b], num = t.b_jntnum[b];
  for (int j = adr; j < adr + num; j++) {
    const T jp[3] = {t.j_pos[j], t.j_pos[NJ + j], t.j_pos[2 * NJ + j]}, ja[3] = {t.j_axis[j], t.j_axis[NJ + j], t.j_axis[2 * NJ + j]};
    T anchor[3], ax[3], r[3], qa[4];
    rot(anchor, jp, quat);
    anchor[0] += pos[0]; anchor[1] += pos[1]; anchor[2] += pos[2];
    rot(ax, ja, quat);
    AX[j] = ax[0]; AX[NJ + j] = ax[1]; AX[2 * NJ + j] = ax[2];
    const T h = T(qpos[t.j_qadr[j]] - t.j_q0[j]) * T(0.5), s = sin_(h);
    qa[0] = cos_(h); qa[1] = ja[0] * s; qa[2] = ja[1] * s; qa[3] = ja[2] * s;
    qmul(quat, quat, qa);
    rot(r, jp, quat);
    pos[0] = anchor[0] - r[0]; pos[1] = anchor[1] - r[1]; pos[2] = anchor[2] - r[2];
  }
  qnormalize(quat);
  P[b] = pos[0]; P[NB + b] = pos[1]; P[2 * NB + b] = pos[2];
  P[3 * NB + b] = quat[0]; P[4 * NB + b] = quat[1]; P[5 * NB + b] = quat[2]; P[6 * NB + b] = quat[3];
}

// bodies 0 (world, unused) and 1 (the root) are the identity; links 2 .. nbody-1 go level by level, lane l taking bodies 2 + l and
// 2 + l + 64 (66 links on 64 lanes: lanes 0 and 1 carry two)
template <class T>
WT_FN void kinematics(const Tables<T> &t, const double *qpos, T *P, T *AX) {
  const int NB = t.nbody;
  WT_LANES(lane) if (lane < 2) {
    for (int c = 0; c < 7; c++) P[c * NB + lane] = c == 3 ? T(1) : T(0);
  }
  WT_SYNC();
  for (int d = 2; d <= t.maxdepth; d++) {
    WT_LANES(lane) for (int b = 2 + lane; b < NB; b += 64)
      if (t.b_depth[b] == d) body_pose(t, b, qpos, P, AX);
    WT_SYNC();
  }
}

template <class T>
WT_FN void site_root(const Tables<T> &t, int s, const T *P, T *out) {
  const int NB = t.nbody, NS = t.nsite, b = t.s_body[s];
  const T sp[3] = {t.s_pos[s], t.s_pos[NS + s], t.s_pos[2 * NS + s]};
  const T q[4] = {P[3 * NB + b], P[4 * NB + b], P[5 * NB + b], P[6 * NB + b]};
  rot(out, sp, q);
  out[0] += P[b]; out[1] += P[NB + b]; out[2] += P[2 * NB + b];
}

// ------------------------------------------------------------------------------------------------ the row
// Outputs of one row, already offset to it; any may be NULL (skipped).
template <class T>
struct RowOut {
  double *com;            // [3]
  T *qvel, *r2s, *jq;     // [6 + J], [S][3], [1 + J][4]
  T *factors, *reward;    // [4], [1]
  int *term;              // [1]
  T *obs;                 // [obs_dim]: only the kinematic columns are written
};

// features (kEval false: com / qvel / r2s / jq) or evaluate (kEval true: factors / reward / term / obs) of one state.
// P, AX: scratch of the wave (LDS on the device).
template <class T, bool kEval>
WT_FN void row_task(const Tables<T> &t, const double *qpos, const double *qvel, int clip, int step, const RowOut<T> &o, T *P, T *AX) {
  kinematics(t, qpos, P, AX);
  const int J = t.J, S = t.S;
  const T rq[4] = {T(qpos[3]), T(qpos[4]), T(qpos[5]), T(qpos[6])};
  int row = 0;
  bool bad_clip = false;
  if (kEval) { bad_clip = clip < 0 || clip >= t.ntraj; clip = clamp_clip(t, clip); row = ref_row(t, clip, step); }
  const bool diffs = kEval && !t.inference;
  T a1[WT_ACC], a2[WT_ACC], a3[WT_ACC];
  WT_LANES(lane) {
    T s1 = 0, s2 = 0, s3 = 0;
    if (o.jq || diffs) {
      for (int i = lane; i < 1 + J; i += 64) {
        T q[4];
        if (i == 0) { q[0] = rq[0]; q[1] = rq[1]; q[2] = rq[2]; q[3] = rq[3]; }
        else {
          const int j = t.t_jnt[i - 1];
          const T ax[3] = {AX[j], AX[t.njnt + j], AX[2 * t.njnt + j]};
          joint_orientation_quat(q, ax, T(qpos[t.t_qadr[i - 1]]));
        }
        if (o.jq) { o.jq[4 * i] = q[0]; o.jq[4 * i + 1] = q[1]; o.jq[4 * i + 2] = q[2]; o.jq[4 * i + 3] = q[3]; }
        if (diffs) {
          T r[4];
          if (i == 0) { const double *p = t.r_root7 + (size_t)row * 7 + 3; r[0] = T(p[0]); r[1] = T(p[1]); r[2] = T(p[2]); r[3] = T(p[3]); }
          else { const T *p = t.r_jq + ((size_t)row * J + (i - 1)) * 4; r[0] = p[0]; r[1] = p[1]; r[2] = p[2]; r[3] = p[3]; }
          s3 += short_arc_sq(q, r);
        }
      }
    }
    if (o.r2s || diffs) {
      for (int i = lane; i < S; i += 64) {
        T x[3];
        site_root(t, t.t_site[i], P, x);
        if (o.r2s) { o.r2s[3 * i] = x[0]; o.r2s[3 * i + 1] = x[1]; o.r2s[3 * i + 2] = x[2]; }
        if (diffs) {
          const T *p = t.r_r2s + ((size_t)row * S + i) * 3;
          const T d0 = x[0] - p[0], d1 = x[1] - p[1], d2 = x[2] - p[2];
          s2 += d0 * d0 + d1 * d1 + d2 * d2;
        }
      }
    }
    if (o.qvel || diffs) {
      for (int i = lane; i < 6 + J; i += 64) {
        const T v = T(qvel[i < 6 ? i : t.t_dadr[i - 6]]);
        if (o.qvel) o.qvel[i] = v;
        if (diffs) { const T d = v - t.r_qvel[(size_t)row * (6 + J) + i]; s1 += d * d; }
      }
    }
    if (!kEval && o.com && lane < 3) o.com[lane] = qpos[lane];
    if (kEval && o.obs) {
      T qn[4] = {rq[0], rq[1], rq[2], rq[3]};
      qnormalize(qn);  // the root body's xquat (pyref normalises the free joint's quaternion)
      const T qc[4] = {qn[0], -qn[1], -qn[2], -qn[3]};
      for (int i = lane; i < t.nappend; i += 64) {  // fruitfly.py:629-638 appendages_pos: (x_site - x_root) . R_root
        T x[3];
        site_root(t, t.app_site[i], P, x);
        T *w = o.obs + t.off_app + 3 * i;
        w[0] = x[0]; w[1] = x[1]; w[2] = x[2];
      }
      for (int i = lane; i < t.nobsj; i += 64) {
        o.obs[t.off_jpos + i] = T(qpos[t.obs_qadr[i]]);
        o.obs[t.off_jvel + i] = T(qvel[t.obs_dadr[i]]);
      }
      // tasks/base.py:237-261: rows step .. step + future_steps of the clip, in the walker's frame
      const T n2 = rq[0] * rq[0] + rq[1] * rq[1] + rq[2] * rq[2] + rq[3] * rq[3];
      const T qi[4] = {rq[0] / n2, -rq[1] / n2, -rq[2] / n2, -rq[3] / n2};
      for (int f = lane; f <= t.future; f += 64) {
        const double *p = t.r_root7 + (size_t)ref_row(t, clip, (long long)step + f) * 7;
        const T dv[3] = {T(p[0] - qpos[0]), T(p[1] - qpos[1]), T(p[2] - qpos[2])};
        T e[3], rr[4];
        rot(e, dv, qc);
        T *w = o.obs + t.off_disp + 3 * f;
        w[0] = e[0]; w[1] = e[1]; w[2] = e[2];
        const T pq[4] = {T(p[3]), T(p[4]), T(p[5]), T(p[6])};
        qmul(rr, qi, pq);
        w = o.obs + t.off_rquat + 4 * f;
        w[0] = rr[0]; w[1] = rr[1]; w[2] = rr[2]; w[3] = rr[3];
      }
      if (lane == 0) {  // third row of the root rotation
        const T w_ = qn[0], x = qn[1], y = qn[2], z = qn[3];
        T *w = o.obs + t.off_zaxis;
        w[0] = 2 * (x * z - w_ * y); w[1] = 2 * (y * z + w_ * x); w[2] = w_ * w_ - x * x - y * y + z * z;
      }
    }
    a1[lane & (WT_ACC - 1)] = s1; a2[lane & (WT_ACC - 1)] = s2; a3[lane & (WT_ACC - 1)] = s3;
  }
  if (!kEval) return;
  const T d1 = wave_sum(a1), d2 = wave_sum(a2), d3 = wave_sum(a3);
  WT_LANES(lane) if (lane == 0) {
    const double *p = t.r_root7 + (size_t)row * 7;
    const double e0 = qpos[0] - p[0], e1 = qpos[1] - p[1], e2 = qpos[2] - p[2];
    const double d0 = e0 * e0 + e1 * e1 + e2 * e2;
    T f[4] = {1, 1, 1, 1}, r = 1;
    if (diffs) {
      f[0] = t.weight[0] * exp_(T(double(t.coef[0]) * d0));
      f[1] = t.weight[1] * exp_(t.coef[1] * d1);
      f[2] = t.weight[2] * exp_(t.coef[2] * d2);
      f[3] = t.weight[3] * exp_(t.coef[3] * d3);
      r = f[0] * f[1] * f[2] * f[3];
      if (!(r == r)) r = 0;  // walk_imitation.py: NaN rewards are scrubbed
    }
    if (o.factors) { o.factors[0] = f[0]; o.factors[1] = f[1]; o.factors[2] = f[2]; o.factors[3] = f[3]; }
    if (o.reward) *o.reward = r;
    if (o.term) {
      const int ep = t.ep_steps[clip];
      int bits = sqrt(d0) > t.term_dist ? 1 : 0;  // walk_imitation.py:161-177: |ref_displacement[0]|
      if (step == ep) bits |= 2;
      if (step < 0 || step > ep || bad_clip) bits |= 4;
      *o.term = bits;
    }
  }
}

// The position stage normalises the free joint's quaternion inside qpos (mj_kinematics; the oracle's fo_kinematics), so the state a
// reset leaves holds q / |q|, not the row's q.  Component k, rounded exactly as that C code rounds it: no contraction into FMAs.
WT_FN double normalized_component(const double *q, int k) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double n = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  if (n < 1e-15) return k == 0 ? 1.0 : 0.0;  // mjMINVAL
  return q[k] / n;
}

// the state walk_reset builds: qpos0, the root pose and the tracked joints from the row, then the overrides; the root quaternion as the
// position stage leaves it; zero velocity
template <class T>
WT_FN void row_reference_pose(const Tables<T> &t, int clip, int step, double *qpos, double *qvel) {
  clip = clamp_clip(t, clip);
  const int row = ref_row(t, clip, step);
  WT_LANES(lane) {
    if (qpos)
      for (int a = lane; a < t.nq; a += 64) {
        const int c = t.pose_src[a];
        double v = c < 0 ? t.pose_const[a] : (c < 7 ? t.r_root7[(size_t)row * 7 + c] : t.r_jang[(size_t)row * t.J + (c - 7)]);
        if (a >= 3 && a < 7) v = normalized_component(t.r_root7 + (size_t)row * 7 + 3, a - 3);
        qpos[a] = v;
      }
    if (qvel)
      for (int a = lane; a < t.nv; a += 64) qvel[a] = 0.0;
  }
}

// ------------------------------------------------------------------------------------------------ host: tables from the blob
// (model/blob.py layout).  Everything is packed into one arena; the pointers of `tab` hold byte offsets into it until
// rebase() turns them into addresses of wherever the arena lives (host vector or HBM).
struct BlobView {
  struct Ten { int dtype; size_t count; const unsigned char *data; };
  std::map<std::string, Ten> ten;
  bool parse(const void *p, size_t n, std::string &err) {
    const unsigned char *b = static_cast<const unsigned char *>(p);
    if (n < 12 || std::memcmp(b, "FFMB", 4) != 0) { err = "model blob: bad magic"; return false; }
    uint32_t ver, cnt;
    std::memcpy(&ver, b + 4, 4); std::memcpy(&cnt, b + 8, 4);
    if (ver != 1) { err = "model blob: unsupported version"; return false; }
    size_t off = 12;
    for (uint32_t k = 0; k < cnt; k++) {
      uint16_t nl;
      if (off + 2 > n) { err = "model blob: truncated"; return false; }
      std::memcpy(&nl, b + off, 2); off += 2;
      if (off + nl + 2 > n) { err = "model blob: truncated"; return false; }
      std::string name(reinterpret_cast<const char *>(b + off), nl); off += nl;
      Ten t; t.dtype = b[off]; const int ndim = b[off + 1]; off += 2; t.count = 1;
      if (off + 4 * (size_t)ndim > n) { err = "model blob: truncated"; return false; }
      for (int d = 0; d < ndim; d++) { uint32_t v; std::memcpy(&v, b + off, 4); off += 4; t.count *= v; }
      off += (8 - off % 8) % 8;
      t.data = b + off;
      off += t.count * (t.dtype == 0 ? 8 : 4);
      if (off > n) { err = "model blob: truncated tensor " + name; return false; }
      ten[name] = t;
    }
    return true;
  }
  bool ints(const std::string &name, std::vector<int> &out, std::string &err, bool optional = false) const {
    auto it = ten.find(name);
    out.clear();
    if (it == ten.end()) { if (optional) return true; err = "model blob: missing tensor " + name; return false; }
    if (it->second.dtype != 1) { err = "model blob: tensor " + name + " is not int32"; return false; }
    out.resize(it->second.count);
    if (!out.empty()) std::memcpy(out.data(), it->second.data, 4 * out.size());
    return true;
  }
  bool reals(const std::string &name, std::vector<double> &out, std::string &err) const {
    auto it = ten.find(name);
    out.clear();
    if (it == ten.end()) { err = "model blob: missing tensor " + name; return false; }
    if (it->second.dtype != 0) { err = "model blob: tensor " + name + " is not float64"; return false; }
    out.resize(it->second.count);
    if (!out.empty()) std::memcpy(out.data(), it->second.data, 8 * out.size());
    return true;
  }
};

template <class T>
struct Packed {
  Tables<T> tab;  // pointers = byte offsets into `arena` until rebase()
  std::vector<unsigned char> arena;
  std::vector<int> ep_steps;

  template <class U>
  const U *put(const std::vector<U> &v) {
    size_t off = (arena.size() + 15) & ~size_t(15);
    if (off == 0) off = 16;  // offset 0 would read as a NULL pointer
    arena.resize(off + v.size() * sizeof(U) + 16);
    if (!v.empty()) std::memcpy(arena.data() + off, v.data(), v.size() * sizeof(U));
    return reinterpret_cast<const U *>(off);
  }
  template <class U>
  const U *put_as(const double *src, size_t n) {
    std::vector<U> v(n);
    for (size_t i = 0; i < n; i++) v[i] = (U)src[i];
    return put(v);
  }
  // `base`: where arena[0] lives for whoever dereferences the view
  Tables<T> rebase(const void *base) const {
    Tables<T> r = tab;
    const uintptr_t b = reinterpret_cast<uintptr_t>(base);
    r.each_ptr([b](auto &p) { p = reinterpret_cast<std::remove_reference_t<decltype(p)>>(b + reinterpret_cast<uintptr_t>(p)); });
    return r;
  }

  // false + text on every refusal
  bool build(const void *blob, size_t blob_size, const ffe_walk_task *task, std::string &err) {
    const std::string who = "ffe_walktask_create: ";
    auto fail = [&](const std::string &s) { err = who + s; return false; };
    if (!blob || !task) return fail("a null required pointer (blob, task)");
    BlobView bv;
    std::string e;
    if (!bv.parse(blob, blob_size, e)) return fail(e);
    std::vector<int> parent, jntadr, jntnum, jtype, jbody, jqadr, jdadr, sbody, app, obsj, dyn, touch, force;
    std::vector<double> bpos, bquat, jpos, jaxis, qpos0, spos;
    if (!bv.ints("body_parentid", parent, e) || !bv.ints("body_jntadr", jntadr, e) || !bv.ints("body_jntnum", jntnum, e) ||
        !bv.ints("jnt_type", jtype, e) || !bv.ints("jnt_bodyid", jbody, e) || !bv.ints("jnt_qposadr", jqadr, e) ||
        !bv.ints("jnt_dofadr", jdadr, e) || !bv.ints("sites_bodyid", sbody, e) || !bv.ints("appendage_site", app, e) ||
        !bv.ints("obs_jnt", obsj, e) || !bv.ints("act_dyntype", dyn, e) || !bv.ints("touch_site", touch, e) ||
        !bv.ints("force_site", force, e) || !bv.reals("body_pos", bpos, e) || !bv.reals("body_quat", bquat, e) ||
        !bv.reals("jnt_pos", jpos, e) || !bv.reals("jnt_axis", jaxis, e) || !bv.reals("qpos0", qpos0, e) || !bv.reals("sites_pos", spos, e))
      return fail(e);
    std::vector<int> dofj;
    if (!bv.ints("dof_jntid", dofj, e)) return fail(e);
    const int NB = (int)parent.size(), NJ = (int)jtype.size(), NS = (int)sbody.size(), nq = (int)qpos0.size(), nv = (int)dofj.size();
    if (NB < 2 || NJ < 1 || jtype[0] != kJntFree || jbody[0] != 1 || jntnum[1] != 1 || parent[1] != 0)
      return fail("the model's body 1 must carry the free joint (joint 0)");
    std::vector<int> depth(NB, 0);
    int maxdepth = 1;
    for (int b = 1; b < NB; b++) {
      if (parent[b] < 0 || parent[b] >= b) return fail("model blob: bodies are not ordered parent first");
      if (b >= 2 && parent[b] < 1) return fail("body " + std::to_string(b) + " does not hang off the root body: the task layer works in the root frame");
      depth[b] = depth[parent[b]] + 1;
      if (depth[b] > maxdepth) maxdepth = depth[b];
      for (int j = jntadr[b]; b >= 2 && j < jntadr[b] + jntnum[b]; j++)
        if (j < 0 || j >= NJ || jtype[j] != kJntHinge) return fail("body " + std::to_string(b) + " carries a joint that is not a hinge");
    }
    if (task->n_joints < 0 || task->n_sites < 0 || (task->n_joints > 0 && !task->joints) || (task->n_sites > 0 && !task->sites))
      return fail("a null required pointer (joints, sites) or a negative count");
    const int J = task->n_joints, S = task->n_sites;
    std::vector<int> tj(J), tq(J), td(J), ts(S);
    for (int i = 0; i < J; i++) {
      const int j = task->joints[i];
      if (j < 0 || j >= NJ) return fail("tracked joint index " + std::to_string(j) + " is out of range [0, " + std::to_string(NJ) + ")");
      if (jtype[j] != kJntHinge) return fail("tracked joint " + std::to_string(j) + " is not a hinge");
      tj[i] = j; tq[i] = jqadr[j]; td[i] = jdadr[j];
    }
    for (int i = 0; i < S; i++) {
      const int s = task->sites[i];
      if (s < 0 || s >= NS) return fail("tracked site index " + std::to_string(s) + " is out of range [0, " + std::to_string(NS) + ")");
      if (sbody[s] < 1) return fail("tracked site " + std::to_string(s) + " sits on the world body");
      ts[i] = s;
    }
    for (size_t i = 0; i < app.size(); i++)
      if (app[i] < 0 || app[i] >= NS || sbody[app[i]] < 1) return fail("model blob: bad appendage site");
    const int F = task->future_steps;
    if (F < 0) return fail("future_steps " + std::to_string(F) + " is negative");
    if (!(task->control_timestep > 0)) return fail("control_timestep must be positive");
    for (int k = 0; k < 4; k++)
      if (!(task->std[k] > 0)) return fail("std[" + std::to_string(k) + "] must be positive");
    if (task->n_overrides < 0 || (task->n_overrides > 0 && (!task->override_qadr || !task->override_val)))
      return fail("a null required pointer (override_qadr, override_val) or a negative count");
    for (int i = 0; i < task->n_overrides; i++)
      if (task->override_qadr[i] >= 0 && task->override_qadr[i] < 7) return fail("override address " + std::to_string(task->override_qadr[i]) + " lies inside the root pose qpos[0:7]");
    for (int i = 0; i < task->n_overrides; i++)
      if (task->override_qadr[i] < 0 || task->override_qadr[i] >= nq)
        return fail("override address " + std::to_string(task->override_qadr[i]) + " is out of range [0, " + std::to_string(nq) + ")");
    const int ntraj = task->ntraj;
    if (ntraj < 0) return fail("ntraj is negative");
    size_t rows = 0;
    std::vector<int> off(1, 0);
    ep_steps.clear();
    if (ntraj > 0) {
      if (!task->traj_off || !task->ref_qpos || !task->ref_qvel || (S > 0 && !task->ref_root2site) || (J > 0 && !task->ref_joint_quat))
        return fail("a null required pointer (traj_off, ref_qpos, ref_qvel, ref_root2site, ref_joint_quat)");
      if (task->traj_off[0] != 0) return fail("traj_off[0] must be 0");
      const long long max_steps = llround(task->time_limit / task->control_timestep) + 1;
      for (int c = 0; c < ntraj; c++) {
        const long long len = (long long)task->traj_off[c + 1] - task->traj_off[c];
        if (len < F + 2)
          return fail("clip " + std::to_string(c) + " has " + std::to_string(len) + " rows, fewer than future_steps + 2 = " + std::to_string(F + 2));
        const long long snippet_steps = len - F - 1;  // walk_imitation.py:99-100
        ep_steps.push_back((int)(snippet_steps < max_steps ? snippet_steps : max_steps));
        off.push_back(task->traj_off[c + 1]);
      }
      rows = (size_t)task->traj_off[ntraj];
    }
    // observation layout (the oracle's walk_observe): accelerometer 3 | actuator_activation na | appendages_pos | force | gyro 3 |
    // joints_pos | joints_vel | ref_displacement 3 (F+1) | ref_root_quat 4 (F+1) | touch | velocimeter 3 | world_zaxis 3
    int na = 0;
    for (int v : dyn) na += v != 0;
    Tables<T> &t = tab;
    std::memset(&t, 0, sizeof(t));
    t.nbody = NB; t.njnt = NJ; t.nq = nq; t.nv = nv; t.nsite = NS; t.maxdepth = maxdepth;
    t.J = J; t.S = S; t.nappend = (int)app.size(); t.nobsj = (int)obsj.size();
    t.ntraj = ntraj; t.future = F; t.inference = task->inference_mode != 0;
    t.term_dist = task->terminal_com_dist;
    for (int k = 0; k < 4; k++) { t.coef[k] = (T)(-0.5 / (task->std[k] * task->std[k])); t.weight[k] = (T)task->weights[k]; }
    t.off_app = 3 + na;
    t.off_jpos = t.off_app + 3 * t.nappend + 3 * (int)force.size() + 3;
    t.off_jvel = t.off_jpos + t.nobsj;
    t.off_disp = t.off_jvel + t.nobsj;
    t.off_rquat = t.off_disp + 3 * (F + 1);
    t.off_zaxis = t.off_rquat + 4 * (F + 1) + (int)touch.size() + 3;
    t.obs_dim = t.off_zaxis + 3;
    arena.clear();
    auto field_major = [](const std::vector<double> &src, int n, int w) {  // [n][w] -> [w][n]
      std::vector<double> r((size_t)n * w);
      for (int i = 0; i < n; i++)
        for (int c = 0; c < w; c++) r[(size_t)c * n + i] = src[(size_t)i * w + c];
      return r;
    };
    t.b_parent = put(parent); t.b_depth = put(depth); t.b_jntadr = put(jntadr); t.b_jntnum = put(jntnum);
    { auto v = field_major(bpos, NB, 3); t.b_pos = put_as<T>(v.data(), v.size()); }
    { auto v = field_major(bquat, NB, 4); t.b_quat = put_as<T>(v.data(), v.size()); }
    t.j_qadr = put(jqadr);
    { std::vector<double> v(NJ); for (int j = 0; j < NJ; j++) v[j] = qpos0[jqadr[j]]; t.j_q0 = put(v); }
    { auto v = field_major(jpos, NJ, 3); t.j_pos = put_as<T>(v.data(), v.size()); }
    { auto v = field_major(jaxis, NJ, 3); t.j_axis = put_as<T>(v.data(), v.size()); }
    t.s_body = put(sbody);
    { auto v = field_major(spos, NS, 3); t.s_pos = put_as<T>(v.data(), v.size()); }
    t.t_jnt = put(tj); t.t_qadr = put(tq); t.t_dadr = put(td); t.t_site = put(ts);
    t.app_site = put(app);
    { std::vector<int> a(obsj.size()), d(obsj.size());
      for (size_t i = 0; i < obsj.size(); i++) { a[i] = jqadr[obsj[i]]; d[i] = jdadr[obsj[i]]; }
      t.obs_qadr = put(a); t.obs_dadr = put(d); }
    t.traj_off = put(off); t.ep_steps = put(ep_steps);
    { // reference tables: a compact root7 (the 65-row preview otherwise strides over whole qpos rows), the joint angles apart
      const int W = 7 + J;
      std::vector<double> r7(rows * 7), ja(rows * (size_t)J);
      for (size_t r = 0; r < rows; r++) {
        for (int c = 0; c < 7; c++) r7[r * 7 + c] = task->ref_qpos[r * W + c];
        for (int c = 0; c < J; c++) ja[r * J + c] = task->ref_qpos[r * W + 7 + c];
      }
      t.r_root7 = put(r7); t.r_jang = put(ja);
      t.r_qvel = put_as<T>(task->ref_qvel, rows * (size_t)(6 + J));
      t.r_r2s = put_as<T>(task->ref_root2site, rows * (size_t)(3 * S));
      t.r_jq = put_as<T>(task->ref_joint_quat, rows * (size_t)(4 * J));
    }
    { // reference_pose as one source per qpos address: qpos0 < row < overrides, in the order walk_reset writes them
      std::vector<int> src(nq, -1);
      std::vector<double> cst(qpos0);
      for (int c = 0; c < 7 && c < nq; c++) src[c] = c;
      for (int i = 0; i < J; i++) src[tq[i]] = 7 + i;
      for (int i = 0; i < task->n_overrides; i++) { src[task->override_qadr[i]] = -1; cst[task->override_qadr[i]] = task->override_val[i]; }
      t.pose_src = put(src); t.pose_const = put(cst);
    }
    return true;
  }
};

}  // namespace wt
