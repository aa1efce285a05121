// walk_floor_convex.hpp - the floor plane against the walking fly's ellipsoid and cylinder geoms (walk_imitation, DESIGN.md section 12
// step 3d): the narrow phase of the second floor pass of walk_full_env.hip `floor_full_step`.
//
// Restated from MuJoCo's published mjc_PlaneConvex (for an ellipsoid: the support point against the plane's normal, one contact) and
// mjc_PlaneCylinder (up to four contacts on the rim of the lower disk and at the far end of the lowest generator).  Everything is in one
// frame - the root frame on the device, any frame on the host - with n the plane's unit normal, c and R (row-major) the geom's centre and
// rotation.  Both functions return SURFACE points; the caller forms a point's distance from the plane (the cylinder returns its own,
// from `dist0` = the centre's distance, whose first term the device takes in float64) and the contact position
// "surface point - n dist / 2", which is wf::contact_position with radius 0.
// Templated on the scalar type so that the host can compile it (tests/walk_floor_convex_host.cpp compares both instantiations with a
// float64 numpy restatement); the kernel calls the float32 one.
#pragma once

#include "walk_floor.hpp"

namespace wfc {

// below this length a vector is not normalised (mjMINVAL in float64).  In float32 a cylinder axis "parallel" to the normal leaves
// |a pa - n| at the rounding of the rotation matrix, about 1e-7, which is no direction: the float32 threshold sits above that.
template <class T>
WF_FN T tiny();
template <>
WF_FN float tiny<float>() { return 1e-6f; }
template <>
WF_FN double tiny<double>() { return 1e-15; }

// mjc_PlaneConvex for an ellipsoid with the semi-axes s: the point of the surface that lies deepest along -n.
//   d = -R' n,  w = s o s o d,  p = c + R w / sqrt(d . w)
template <class T>
WF_FN void ellipsoid_support(const T *n, const T *c, const T *R, const T *s, T *p) {
  T d[3], w[3];
  for (int k = 0; k < 3; k++) d[k] = -(R[k] * n[0] + R[3 + k] * n[1] + R[6 + k] * n[2]);
  for (int k = 0; k < 3; k++) w[k] = s[k] * s[k] * d[k];
  const T inv = T(1) / wf::sqrt_<T>(wf::dot3(d, w));
  for (int k = 0; k < 3; k++) p[k] = c[k] + (R[3 * k] * w[0] + R[3 * k + 1] * w[1] + R[3 * k + 2] * w[2]) * inv;
}

// mjc_PlaneCylinder: radius r, half height h, axis = R's third column; `dist0` = n . (c - x0).  Up to four surface points and their
// distances, each in a slot of its own (no slot index depends on the data): 0 the lowest rim point, 1 the rim point above it on the
// other disk, 2 and 3 the two points at +-120 degrees from the lowest on the lower rim.  Returns the mask of the slots that hold a
// contact (bits 2 and 3 come together, nothing without bit 0); MuJoCo lists them in slot order.
template <class T>
WF_FN int plane_cylinder(const T *n, const T *c, const T *R, const T r, const T h, const T dist0, const T margin, T (*sp)[3], T *dist) {
  T a[3] = {R[2], R[5], R[8]};
  T pa = wf::dot3(n, a);
  if (pa > 0) { a[0] = -a[0]; a[1] = -a[1]; a[2] = -a[2]; pa = -pa; }
  T vec[3] = {a[0] * pa - n[0], a[1] * pa - n[1], a[2] * pa - n[2]};
  const T len = wf::sqrt_<T>(wf::dot3(vec, vec));
  if (len < tiny<T>()) { vec[0] = r * R[0]; vec[1] = r * R[3]; vec[2] = r * R[6]; }  // the disk is parallel to the plane
  else { const T sc = r / len; vec[0] *= sc; vec[1] *= sc; vec[2] *= sc; }
  const T pv = wf::dot3(n, vec);
  const T ax[3] = {h * a[0], h * a[1], h * a[2]};
  pa *= h;
  const T d1 = dist0 + pa + pv, d2 = dist0 - pa + pv, d3 = dist0 + pa - pv * T(0.5);
  T v1[3];
  wf::cross3(v1, vec, ax);
  const T sc = r * T(0.86602540378443864676) / wf::sqrt_<T>(wf::dot3(v1, v1));
  for (int k = 0; k < 3; k++) {
    v1[k] *= sc;
    sp[0][k] = c[k] + vec[k] + ax[k];
    sp[1][k] = c[k] + vec[k] - ax[k];
    sp[2][k] = c[k] + v1[k] + ax[k] - vec[k] * T(0.5);
    sp[3][k] = c[k] - v1[k] + ax[k] - vec[k] * T(0.5);
  }
  dist[0] = d1; dist[1] = d2; dist[2] = dist[3] = d3;
  if (d1 > margin) return 0;
  return 1 | (d2 <= margin ? 2 : 0) | (d3 <= margin ? 12 : 0);
}

}  // namespace wfc
