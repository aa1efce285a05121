// walk_sense.hpp - the force and touch sensors of the walking fly on a free root (walk_imitation with the floor, DESIGN.md section 12
// step 4c): mj_rnePostConstraint + mj_sensorAcc restated in the frame of the root (the thorax) about the root origin, where the leg code
// keeps its link poses, spatial velocities and motion axes.
//
// A force sensor reads the interaction force between a link's subtree and its parent, in the frame of the sensor's site.  Only the linear
// part of the spatial force is read, and that part is the sum over the subtree of  m (acceleration of the link's centre of mass) - f_ext:
//   cacc     spatial acceleration of the link (angular, linear at the root origin) = root + sum over the path of cdof qacc + cdof_dot qvel.
//            The root's is (wdot_b, vdot_b) of the arrowhead solve as it leaves the solve, without gravity added: with
//            qacc_lin = R (vdot_b + w_b x v_b) + g the spatial acceleration of the root in its own axes is R' (qacc_lin - g) - w_b x v_b
//            once the fictitious -R' g of mj_rnePostConstraint is folded in, and that is vdot_b.
//   f_int    m (a_lin + alpha x r + w x (v_lin + w x r)) - f_ext,  r = centre of mass - root origin, (w, v_lin) the link's spatial velocity.
//            It splits into a part known after the velocity stage (`velocity_term`: cdof_dot qvel and the centripetal term) and a part
//            that needs this substep's qacc (`accel_term`).
//   subtree  Summed over the subtree of the sensor's link t, the second part needs no per-link value.  With A_t = root + the path sum
//            down to t (t's own hinges included), a link l below t has A_l = A_t + sum of cdof_d qacc_d over the hinges d between them, so
//              sum_l m_l (lin A_l + ang A_l x r_l) = m_sub lin A_t + ang A_t x (sum_l m_l r_l)                       (`accel_term` on the sums)
//                                                  + sum over the hinges d strictly below t of lin(crb_d cdof_d) qacc_d,
//            crb_d the composite inertia of d's own subtree: lin(crb_d cdof_d) is the linear half of the hinge's column of M_rj, which
//            the leg code already keeps.  A kernel therefore carries seven floats per sensor (the subtree's sum of velocity terms, its
//            mass, its sum of m r) from the velocity stage to the sensor pass, not twelve per link.
//   f_ext    the floor's force on the link: sum over the link's contacts that have rows of frame' f (frame rows: normal, two tangents, in
//            the root frame; the fly's geom is geom2 of the pair, so the force on it is +frame' f).  A contact inside the gap has no row.
//   touch    the sum of the positive normal forces of the contacts on the sensor's link (the contact points of the claw's sphere lie
//            inside its larger touch site: tests/test_walk_floor_env_cpu.py checks that against the oracle's ray test).
// Templated on the scalar type so that the host can compile it (tests/walk_sense_host.cpp compares both instantiations with the float64
// oracle); the kernel calls the float32 one.
#pragma once

#include "walk_floor.hpp"

namespace ws {

// m (lin(caccb) + ang(caccb) x r + w x (v_lin + w x r)): what the link's velocity contributes (caccb = sum over the path of cdof_dot qvel)
template <class T>
WF_FN void velocity_term(T m, const T *caccb, const T *cvel, const T *r, T *out) {
  T ar[3], wr[3], ww[3];
  wf::cross3(ar, caccb, r);
  wf::cross3(wr, cvel, r);
  for (int k = 0; k < 3; k++) wr[k] += cvel[3 + k];
  wf::cross3(ww, cvel, wr);
  for (int k = 0; k < 3; k++) out[k] = m * (caccb[3 + k] + ar[k] + ww[k]);
}
// m lin(A) + ang(A) x (m r): what the spatial acceleration A contributes to a link (m, m r its own) or to a whole subtree moving with A
// (m, m r summed over it); with A = cdof_d it is the linear half of crb_d cdof_d
template <class T>
WF_FN void accel_term(T m, const T *mr, const T *A, T *out) {
  T ar[3];
  wf::cross3(ar, A, mr);
  for (int k = 0; k < 3; k++) out[k] = m * A[3 + k] + ar[k];
}
// acc += frame' f: a contact's force on the fly's link, in the root frame
template <class T>
WF_FN void add_contact_force(const T *frame, const T *f, T *acc) {
  for (int k = 0; k < 3; k++) acc[k] += frame[k] * f[0] + frame[3 + k] * f[1] + frame[6 + k] * f[2];
}
// a contact's share of the touch sensor of its link
template <class T>
WF_FN T touch_share(T normal_force) { return normal_force > T(0) ? normal_force : T(0); }
// R(q)' v: a vector of the root frame in the frame of a site with the orientation q (unit quaternion, in the root frame)
template <class T>
WF_FN void to_site(const T *q, const T *v, T *out) {
  const T w = q[0], x = q[1], y = q[2], z = q[3];
  const T m[9] = {w * w + x * x - y * y - z * z, 2 * (x * y - w * z), 2 * (x * z + w * y), 2 * (x * y + w * z), w * w - x * x + y * y - z * z,
                  2 * (y * z - w * x),           2 * (x * z - w * y), 2 * (y * z + w * x), w * w - x * x - y * y + z * z};
  for (int k = 0; k < 3; k++) out[k] = m[k] * v[0] + m[3 + k] * v[1] + m[6 + k] * v[2];
}

}  // namespace ws
