// Host build of the flight broad phase's uniform support function (flybody_amd/csrc/convex.hpp compiled with -DCVX_HOST: GeomU,
// hsupport_u, overlap_u, separation_bound_u) beside the per-type originals, for tests/test_broadphase_uniform_cpu.py: test
// infrastructure only, never linked into the product library.
#define CVX_HOST 1
#include "../flybody_amd/csrc/convex.hpp"

using namespace cvx;

// geom = centre[3], quat[4], size[3], type (as tests/cvx_host.cpp)
static Geom mk(const float *p) { return Geom{{p[0], p[1], p[2]}, {p[3], p[4], p[5], p[6]}, p[7], p[8], p[9], (int)p[10]}; }
static GeomU mku(const float *p) { return make_u(V3{p[0], p[1], p[2]}, Q4{p[3], p[4], p[5], p[6]}, ushape((int)p[10], p[7], p[8], p[9])); }

extern "C" {
void cvxu_ushape(int type, float s0, float s1, float s2, float *out) {
  const UShape u = ushape(type, s0, s1, s2);
  const float v[8] = {u.ex, u.ey, u.ez, u.h, u.kx, u.ky, u.kz, u.kh};
  for (int k = 0; k < 8; k++) out[k] = v[k];
}
void cvxu_support_ref(const float *g, const float *n, float *out) {
  const V3 s = support(mk(g), V3{n[0], n[1], n[2]});
  out[0] = s.x; out[1] = s.y; out[2] = s.z;
}
float cvxu_hsupport(const float *g, const float *n) { return hsupport_u(mku(g), V3{n[0], n[1], n[2]}); }
void cvxu_core(const float *g, float *out) {  // world axis, half-length: uniform form then core_segment
  const GeomU u = mku(g);
  V3 a; float h;
  core_segment(mk(g), a, h);
  out[0] = u.ka.x; out[1] = u.ka.y; out[2] = u.ka.z; out[3] = u.kh; out[4] = a.x; out[5] = a.y; out[6] = a.z; out[7] = h;
}
float cvxu_overlap(const float *g1, const float *g2, const float *u) { return overlap_u(mku(g1), mku(g2), V3{u[0], u[1], u[2]}); }
float cvxu_overlap_ref(const float *g1, const float *g2, const float *u) { return overlap(mk(g1), mk(g2), V3{u[0], u[1], u[2]}); }
float cvxu_separation_bound(const float *g1, const float *g2) { return separation_bound_u(mku(g1), mku(g2)); }
float cvxu_separation_bound_ref(const float *g1, const float *g2) { return separation_bound(mk(g1), mk(g2)); }
}
