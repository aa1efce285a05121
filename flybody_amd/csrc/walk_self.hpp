// walk_self.hpp - the walking fly's own contacts in the root body frame (walk_imitation): the formulas of the
// fly-fly contact rows that the sixth free-root kernel (walk_self_env.hip `floor_self_step`) evaluates.
//
// A fly-fly contact is condim 1: one frictionless row along the normal n from geom1 to geom2 at the point p, J = n . (jacp2 - jacp1).
// In the root frame about the root origin both bodies ride the root, so the row has no entry on the root coordinates (w_b, v_b): it is
// built like a joint-limit row that spans the hinges of two chains.  With `pos` the link of geom2 (entries +n . u_f) and `neg` the link of
// geom1 (entries -n . u_f; a hinge on both chains gets both and they cancel), u_f = lin(cdof_f) + ang(cdof_f) x p:
//   row      J_f = (f on pos's chain ? 1 : 0) - (f on neg's chain ? 1 : 0)) n . u_f
//   velocity J qvel = n . (v_pos(p) - v_neg(p)) from the links' spatial velocities (the root's share cancels; a geom of the thorax moves
//            with the root's own spatial velocity)
//   y0       J qacc_smooth - aref = J_j (z_m - Y_m x_r) - aref: no w_b x v_b, no gravity (both are the root's, and J_r = 0)
//   G        J_j M_jj^-1 J_j' + w S_m^-1 w' with w = -J_j Y_m: u = L^-1 w for the rank-6 term (wf::rank6_factor with J_r = 0)
//   force    J_j' f on the hinges, nothing on the root's right-hand side: the thorax recoils through Y alone
// Templated on the scalar type so that the host can compile it (tests/walk_self_host.cpp compares both instantiations with the float64
// oracle); the kernel calls the float32 one.
#pragma once

#include "walk_floor.hpp"

namespace wsf {

// J_f of the pair row on hinge f: `on_pos` / `on_neg` = the hinge lies on the chain of geom2's / geom1's link
template <class T>
WF_FN T row_hinge(const T *cdof, const T *p, const T *n, bool on_pos, bool on_neg) {
  const T s = (on_pos ? T(1) : T(0)) - (on_neg ? T(1) : T(0));
  return s == T(0) ? T(0) : s * wf::row_hinge<T>(cdof, p, n);
}
// J qvel: sv_pos / sv_neg = spatial velocities (ang, lin about the root origin) of the two links (of the root itself for a thorax geom)
template <class T>
WF_FN T row_velocity(const T *sv_pos, const T *sv_neg, const T *p, const T *n) {
  T a[3], b[3];
  wf::point_velocity<T>(sv_pos, p, a);
  wf::point_velocity<T>(sv_neg, p, b);
  return n[0] * (a[0] - b[0]) + n[1] * (a[1] - b[1]) + n[2] * (a[2] - b[2]);
}
// mj: mj_makeImpedance for one row: D = 1 / R, R = (1 - imp) diagApprox / imp with diagApprox = the two bodies' invweight0
template <class T>
WF_FN T row_D(T imp, T invw) {
  const T R = (T(1) - imp) * invw / imp;
  return T(1) / (R > T(1e-15) ? R : T(1e-15));
}
// -aref of the row (mj_referenceConstraint): B vel + K imp (dist - includemargin)
template <class T>
WF_FN T row_neg_aref(T K, T B, T imp, T dist, T incl, T vel) { return B * vel + K * imp * (dist - incl); }
// y0 = J qacc_smooth - aref: jz = J_j z_m, jy = J_j Y_m, xr = the root rows of the arrowhead solve
template <class T>
WF_FN T row_y0(T jz, const T *jy, const T *xr, T neg_aref) {
  T y = jz + neg_aref;
  for (int k = 0; k < 6; k++) y -= jy[k] * xr[k];
  return y;
}
// u = L^-1 (0 - J_j Y_m): the row's factor of the rank-6 term of G
template <class T>
WF_FN void rank6_factor(const T (*L)[6], const T *id, const T *jy, T *u) {
  const T zero[6] = {0, 0, 0, 0, 0, 0};
  wf::rank6_factor<T>(L, id, zero, jy, u);
}

}  // namespace wsf
