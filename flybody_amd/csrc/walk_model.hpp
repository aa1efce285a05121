// walk_model.hpp - host-side construction of the device tables of the free-root walking fly (fly_walk.ffmb).
//
// The walking fly is the tethered fly of ball_model.hpp with the thorax on a free joint: the link, dof, block, factor-schedule,
// solve-schedule and actuator tables are the ball builder's own (`detail::build_fly_model(b, true)`: same 64 links + 2 halteres, same
// hinge order, every frame relative to the thorax frame), and the root comes on top of them:
//   the thorax' own mass, inertia (about the root origin, root axes) and inertia-box drag coefficients - the root link is uniform
//            across the wave;
//   the two halteres as ordinary single-hinge links of the root (on the moving thorax their closed form of ball_model.hpp no longer
//            holds: they feel the root's motion and react on it);
//   the free joint's and the floor's bookkeeping, to refuse what this build does not support.
#pragma once

#include "ball_model.hpp"

namespace ffb {

struct WalkExtra {
  // root link, in its own frame about its own origin: spatial inertia (mju_inertCom layout), inertial frame, drag coefficients
  float r_cin[10], r_ipos[3], r_iquat[4], r_fl[8], r_mass;
  // halteres (x_on lanes, slot 2): frame in the root, hinge axis in the haltere frame, inertial frame, inertia, drag
  float hx_pos[3][NL], hx_quat[4][NL], hx_axis[3][NL], hx_ipos[3][NL], hx_iquat[4][NL], hx_inertia[3][NL], hx_mass[NL], hx_fl[8][NL];
  float qpos0[7];  // free joint reference: position, quaternion
  // what step 3 of DESIGN.md section 12 will need; here it only decides what is refused
  int floor_geom, n_limited;
};

struct WalkModel {
  BallModel b;  // first member: the leg code reads it as a BallModel
  WalkExtra x;
};

struct WalkHost {
  WalkModel m;
  std::vector<float> action_min, action_max;
  double root_mass = 0, total_mass = 0;
  int nq = 109, nv = 108;
};

inline WalkHost build_walk_model(const Blob &b) {
  using namespace detail;
  if (b.get("dof_parentid").count != (size_t)ND + 6) throw std::runtime_error("walk model: expected 108 dofs (is this the walk_imitation blob?)");
  WalkHost W;
  {
    BallHost H = build_fly_model(b, true);
    W.m.b = H.m;
    W.action_min = H.action_min; W.action_max = H.action_max;
  }
  BallModel &M = W.m.b;
  WalkExtra &X = W.m.x;
  std::memset(&X, 0, sizeof(X));
  const Tensor &opt = b.get("opt");
  const double rho = opt.f(1), beta = opt.f(2);
  if (opt.f(3) != 0 || opt.f(4) != 0) throw std::runtime_error("walk model: gravity is expected along z");
  const Tensor &bpar = b.get("body_parentid"), &bpos = b.get("body_pos"), &bquat = b.get("body_quat"), &bmass = b.get("body_mass"),
               &bipos = b.get("body_ipos"), &biquat = b.get("body_iquat"), &binert = b.get("body_inertia"), &bbox = b.get("body_box"),
               &bjadr = b.get("body_jntadr");
  const Tensor &jaxis = b.get("jnt_axis"), &jlim = b.get("jnt_limited"), &jtype = b.get("jnt_type");
  const Tensor &ddamp = b.get("dof_damping"), &darm = b.get("dof_armature"), &qpos0 = b.get("qpos0");
  const int root = 1, nb = (int)bpar.count;
  for (int k = 0; k < 6; k++)
    if (ddamp.f(k) != 0 || darm.f(k) != 0) throw std::runtime_error("walk model: damping / armature on the free joint is not supported");
  if (b.get("jnt_stiffness").f(0) != 0) throw std::runtime_error("walk model: a spring on the free joint is not supported");
  for (int k = 0; k < 7; k++) X.qpos0[k] = (float)qpos0.f(k);
  for (int k = 0; k < 3; k++) if (bpos.f(3 * root + k) != qpos0.f(k)) throw std::runtime_error("walk model: qpos0 of the free joint differs from the thorax pose");
  for (int k = 0; k < 4; k++) if (bquat.f(4 * root + k) != qpos0.f(3 + k)) throw std::runtime_error("walk model: qpos0 of the free joint differs from the thorax pose");
  // ---- root link
  {
    const double mass = bmass.f(root), d[3] = {bipos.f(3 * root), bipos.f(3 * root + 1), bipos.f(3 * root + 2)};
    const double iq[4] = {biquat.f(4 * root), biquat.f(4 * root + 1), biquat.f(4 * root + 2), biquat.f(4 * root + 3)};
    const double in[3] = {binert.f(3 * root), binert.f(3 * root + 1), binert.f(3 * root + 2)};
    double R[9], I[9];
    q2m(iq, R);
    for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) {
      I[3 * r + c] = 0;
      for (int k = 0; k < 3; k++) I[3 * r + c] += R[3 * r + k] * in[k] * R[3 * c + k];
    }
    // mj: mju_inertCom
    const double cin[10] = {I[0] + mass * (d[1] * d[1] + d[2] * d[2]), I[4] + mass * (d[0] * d[0] + d[2] * d[2]), I[8] + mass * (d[0] * d[0] + d[1] * d[1]),
                            I[1] - mass * d[0] * d[1], I[2] - mass * d[0] * d[2], I[5] - mass * d[1] * d[2], mass * d[0], mass * d[1], mass * d[2], mass};
    for (int k = 0; k < 10; k++) X.r_cin[k] = (float)cin[k];
    for (int k = 0; k < 3; k++) X.r_ipos[k] = (float)d[k];
    for (int k = 0; k < 4; k++) X.r_iquat[k] = (float)iq[k];
    X.r_mass = (float)mass;
    double box[3] = {bbox.f(3 * root), bbox.f(3 * root + 1), bbox.f(3 * root + 2)};
    ffe::BoxCoef c = ffe::box_coefs(box, rho, beta);
    if (mass < 1e-15) std::memset(&c, 0, sizeof(c));
    for (int k = 0; k < 8; k++) X.r_fl[k] = c.c[k];
    W.root_mass = mass;
    for (int i = 1; i < nb; i++) W.total_mass += bmass.f(i);
  }
  // ---- halteres: the two bodies the link table leaves out, in the lanes the ball builder parked their dof in
  {
    std::vector<char> is_link((size_t)nb, 0);
    for (int l = 0; l < NL; l++) is_link[(size_t)M.l_body[l]] = 1;
    std::vector<int> halt;
    for (int i = 2; i < nb; i++) if (!is_link[(size_t)i]) halt.push_back(i);
    std::vector<int> lanes;
    for (int l = 0; l < NL; l++) if (M.x_on[l]) lanes.push_back(l);
    if (halt.size() != 2 || lanes.size() != 2) throw std::runtime_error("walk model: expected two halteres");
    for (int xx = 0; xx < 2; xx++) {
      const int i = halt[(size_t)xx], l = lanes[(size_t)xx], j = bjadr.i(i);
      if (bpar.i(i) != root || jtype.i(j) != 3) throw std::runtime_error("walk model: a haltere is expected to be a single hinge on the thorax");
      if (M.s_dof[2][l] != b.get("jnt_dofadr").i(j) - 6) throw std::runtime_error("walk model: haltere tables out of step");
      for (int k = 0; k < 3; k++) {
        X.hx_pos[k][l] = (float)bpos.f(3 * i + k); X.hx_axis[k][l] = (float)jaxis.f(3 * j + k); X.hx_ipos[k][l] = (float)bipos.f(3 * i + k);
        X.hx_inertia[k][l] = (float)binert.f(3 * i + k);
      }
      for (int k = 0; k < 4; k++) { X.hx_quat[k][l] = (float)bquat.f(4 * i + k); X.hx_iquat[k][l] = (float)biquat.f(4 * i + k); }
      X.hx_mass[l] = (float)bmass.f(i);
      double box[3] = {bbox.f(3 * i), bbox.f(3 * i + 1), bbox.f(3 * i + 2)};
      ffe::BoxCoef c = ffe::box_coefs(box, rho, beta);
      if (bmass.f(i) < 1e-15) std::memset(&c, 0, sizeof(c));
      for (int k = 0; k < 8; k++) X.hx_fl[k][l] = c.c[k];
    }
  }
  // ---- floor and limits: counted, not modelled
  {
    const Tensor &gbody = b.get("geom_bodyid"), &gtype = b.get("geom_type");
    X.floor_geom = -1;
    for (int g = 0; g < (int)gbody.count; g++) if (gbody.i(g) == 0 && gtype.i(g) == 0) X.floor_geom = g;
    if (X.floor_geom < 0) throw std::runtime_error("walk model: floor plane missing");
    for (int j = 1; j < (int)jlim.count; j++) X.n_limited += jlim.i(j) ? 1 : 0;
  }
  return W;
}

}  // namespace ffb
