// walk_floor.hpp - the floor plane against the walking fly's sphere / capsule geoms, in the root body frame (walk_imitation, DESIGN.md
// section 12 step 3b): the formulas of the collision pass and of the contact rows that the floor kernel of walk_env.hip evaluates.
//
// Everything is expressed in the frame of the free root (the thorax) about the root origin, where the leg code keeps its link poses and
// motion axes.  With R the root's rotation, p_w its position (float64 on the device) and the plane through x_0 with the unit normal n_w:
//   normal        n = R' n_w;  tangents R' t1_w, R' t2_w with (n_w, t1_w, t2_w) = mju_makeFrame(n_w), made once on the host: the frame the
//                 oracle gives a plane contact (the plane does not turn, so its frame in the world is a constant of the model)
//   distance      of a sphere centre / capsule end c (root frame) with radius r:  n_w . (p_w - x_0) + n . c - r, the first term in float64
//   position      c - n (r + dist / 2)                                            mjc_PlaneSphere, twice per capsule (mjc_PlaneCapsule)
//   rows          a row along e (normal or tangent) at the point p: J_r = (p x e, e) on the root coordinates (w_b, v_b = R' v_w) and
//                 J_f = e . (lin(cdof_f) + ang(cdof_f) x p) on a hinge f of the geom's chain (cdof about the root origin)
//   y0            the root's share of J qacc_smooth in MuJoCo's coordinates, qacc = (R (vdot_b + w_b x v_b) + g, wdot_b):
//                 e . (vdot_b + w_b x v_b + R' g) + (p x e) . wdot_b
//   G             J M^-1 J' = J_j M_jj^-1 J_j' + w S_m^-1 w',  w = J_r - J_j Y_m,  Y_m = M_jj^-1 M_jr,  S_m = M_rr - M_rj Y_m = L L':
//                 the rank-6 term is u_i . u_k with u = L^-1 w
// Templated on the scalar type so that the host can compile it (tests/walk_floor_host.cpp compares both instantiations with the float64
// oracle); the kernel calls the float32 one.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define WF_FN __host__ __device__ __forceinline__
#else
#define WF_FN inline
#endif

namespace wf {

template <class T>
WF_FN T dot3(const T *a, const T *b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
template <class T>
WF_FN void cross3(T *r, const T *a, const T *b) {
  const T x = a[1] * b[2] - a[2] * b[1], y = a[2] * b[0] - a[0] * b[2], z = a[0] * b[1] - a[1] * b[0];
  r[0] = x; r[1] = y; r[2] = z;
}
template <class T>
WF_FN T sqrt_(T x);
template <>
WF_FN float sqrt_<float>(float x) { return __builtin_sqrtf(x); }
template <>
WF_FN double sqrt_<double>(double x) { return __builtin_sqrt(x); }

// mj: mju_makeFrame - completes a right-handed frame (rows of `frame`) from its first row
template <class T>
WF_FN void make_frame(T *frame) {
  T n = sqrt_<T>(dot3(frame, frame));
  for (int k = 0; k < 3; k++) frame[k] /= n;
  frame[3] = frame[4] = frame[5] = 0;
  if (frame[1] < T(0.5) && frame[1] > T(-0.5)) frame[4] = 1; else frame[5] = 1;
  const T t = dot3(frame, frame + 3);
  for (int k = 0; k < 3; k++) frame[3 + k] -= t * frame[k];
  n = sqrt_<T>(dot3(frame + 3, frame + 3));
  for (int k = 0; k < 3; k++) frame[3 + k] /= n;
  cross3(frame + 6, frame, frame + 3);
}

// the plane's frame (rows: normal, two tangents) carried from the world into the root frame: row_b = R' row_w (R row-major)
template <class T>
WF_FN void frame_in_root(const T *R, const T *frame_w, T *frame_b) {
  for (int r = 0; r < 3; r++) {
    const T *v = frame_w + 3 * r;
    frame_b[3 * r] = R[0] * v[0] + R[3] * v[1] + R[6] * v[2];
    frame_b[3 * r + 1] = R[1] * v[0] + R[4] * v[1] + R[7] * v[2];
    frame_b[3 * r + 2] = R[2] * v[0] + R[5] * v[1] + R[8] * v[2];
  }
}

// distance of the sphere of radius r about c (root frame) from the plane; `height` = n_w . (p_w - x_0) of the root origin, in float64
template <class T>
WF_FN T plane_distance(double height, const T *n, const T *c, T r) { return (T)(height + (double)dot3(n, c) - (double)r); }

// mjc_PlaneSphere: the contact sits half way between the sphere's lowest point and the plane
template <class T>
WF_FN void contact_position(const T *c, const T *n, T r, T dist, T *pos) {
  const T s = r + T(0.5) * dist;
  for (int k = 0; k < 3; k++) pos[k] = c[k] - n[k] * s;
}

// velocity of the point p of a body moving with the spatial velocity (ang, lin about the root origin) `sv`; with sv = cdof_f it is the
// point's velocity per unit rate of hinge f
template <class T>
WF_FN void point_velocity(const T *sv, const T *p, T *v) {
  T w[3];
  cross3(w, sv, p);
  for (int k = 0; k < 3; k++) v[k] = sv[3 + k] + w[k];
}
// J_f of the row along e at p
template <class T>
WF_FN T row_hinge(const T *cdof, const T *p, const T *e) {
  T v[3];
  point_velocity(cdof, p, v);
  return dot3(e, v);
}
// J_r = (p x e, e)
template <class T>
WF_FN void row_root(const T *p, const T *e, T *Jr) {
  cross3(Jr, p, e);
  Jr[3] = e[0]; Jr[4] = e[1]; Jr[5] = e[2];
}
// the root's share of J qacc_smooth: xr = (wdot_b, vdot_b) of the arrowhead solve (no gravity, no w x v), wb / vb = the root's
// velocities in its own frame, gb = R' g (zero with gravity off)
template <class T>
WF_FN T root_y0(const T *Jr, const T *xr, const T *wb, const T *vb, const T *gb) {
  T wv[3];
  cross3(wv, wb, vb);
  T s = 0;
  for (int k = 0; k < 3; k++) s += Jr[k] * xr[k] + Jr[3 + k] * (xr[3 + k] + wv[k] + gb[k]);
  return s;
}

// S = L L' in place (6 x 6, lower triangle), id = 1 / diag(L); returns false when S is not positive definite
template <class T>
WF_FN bool chol6(T (*S)[6], T *id) {
  for (int j = 0; j < 6; j++) {
    T d = S[j][j];
    for (int k = 0; k < j; k++) d -= S[j][k] * S[j][k];
    if (!(d > 0)) return false;
    id[j] = 1 / sqrt_<T>(d);
    S[j][j] = d * id[j];
    for (int i = j + 1; i < 6; i++) {
      T e = S[i][j];
      for (int k = 0; k < j; k++) e -= S[i][k] * S[j][k];
      S[i][j] = e * id[j];
    }
  }
  return true;
}
// u = L^-1 (J_r - J_j Y_m): a row's factor of the rank-6 term of G
template <class T>
WF_FN void rank6_factor(const T (*L)[6], const T *id, const T *Jr, const T *JjY, T *u) {
  for (int i = 0; i < 6; i++) {
    T w = Jr[i] - JjY[i];
    for (int k = 0; k < i; k++) w -= L[i][k] * u[k];
    u[i] = w * id[i];
  }
}

}  // namespace wf
