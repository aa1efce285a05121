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
#include "walk_floor.hpp"

namespace ffb {

struct WalkExtra {
  // root link, in its own frame about its own origin: spatial inertia (mju_inertCom layout), inertial frame, drag coefficients
  float r_cin[10], r_ipos[3], r_iquat[4], r_fl[8], r_mass;
  // halteres (x_on lanes, slot 2): frame in the root, hinge axis in the haltere frame, inertial frame, inertia, drag
  float hx_pos[3][NL], hx_quat[4][NL], hx_axis[3][NL], hx_ipos[3][NL], hx_iquat[4][NL], hx_inertia[3][NL], hx_mass[NL], hx_fl[8][NL];
  float qpos0[7];  // free joint reference: position, quaternion
  // what step 3 of DESIGN.md section 12 will need; here it only decides what is refused
  int floor_geom, n_limited;
  // ---- the floor plane against the fly's sphere / capsule geoms (FFE_WALK_FLOOR; lane = geom in the collision pass): the geoms that
  //      pass mj_collision's filters against the floor geom, in model order, with the contact parameters of the pair (mj_contactParam:
  //      friction, margin and gap the larger value, solref / solimp weighted by solmix, condim 3)
  int f_n, f_ok;                     // geoms listed; 0 if some pair is not condim 3 or the solimp is not uniform (the bit is then refused)
  float f_frame[9], f_off;           // mju_makeFrame of the plane's normal, in the world; normal . plane position
  int f_geom[NL];                    // the geom's index in the model
  int f_link[NL], f_adh[NL], f_blk[NL], f_amask[NL];  // link of the geom, its adhesion actuator (-1: none), block and dof mask of its chain
  float f_pos[3][NL], f_axis[3][NL], f_rad[NL], f_half[NL], f_fric[NL], f_K[NL], f_B[NL], f_margin[NL], f_gap[NL], f_invw[NL];
  float f_solimp[5];
  // No geom of the table can touch the floor while the root origin is higher than this over the plane, whatever the joint angles:
  // the largest margin + over the geoms (the lengths of the link offsets down its chain + |local centre| + half length + radius),
  // rounded up.  Above it a substep of the floor kernel is the limits kernel's substep.
  float f_reach;
};

struct WalkModel {
  BallModel b;  // first member: the leg code reads it as a BallModel
  WalkExtra x;
};

// ---- the floor plane against the fly's ellipsoid / cylinder geoms (FFE_WALK_FLOOR_CONVEX; lane = row in
//      the second floor pass): the geoms of these two types that pass mj_collision's filters against the floor geom, in model order, with
//      the pair's parameters by `floor_geom_params`.  A table of its own: WalkExtra keeps its bytes and the 48 rows of f_* their order
//      (`build_walk_self` checks both), and 48 + 22 rows would not fit NL lanes.  A contact names its geom in the tile's c_geom as
//      NPG + row: 0 .. NPG - 1 are the rows of WalkExtra::f_*.
constexpr int NFC = 24;  // rows (22 on the shipped model), padded
struct WalkFloorConvex {
  int n, ok;                         // rows; 0 if some pair is not condim 3 or does not share WalkExtra::f_solimp (the bit is then refused)
  int geom[NFC], type[NFC];          // the geom's index in the model; 4 ellipsoid, 5 cylinder
  int link[NFC], adh[NFC], blk[NFC], amask[NFC];  // link of the geom (-1: a geom of the root body, which has no chain: blk 255, amask 0),
                                                  // its body's adhesion actuator (-1: none), block and dof mask of its chain
  float pos[3][NFC], quat[4][NFC], size[3][NFC];  // frame in its link (in the root for a root geom), sizes
  float fric[NFC], K[NFC], B[NFC], margin[NFC], gap[NFC], invw[NFC];
};
// The model of a handle with that bit: the table lies directly behind the WalkModel every walk kernel reads, so that the one kernel that
// knows of it finds it from the WalkExtra pointer it already carries.
struct WalkModelFull {
  WalkModel m;
  WalkFloorConvex xc;
};

struct WalkHost {
  WalkModel m;
  std::vector<float> action_min, action_max;
  double root_mass = 0, total_mass = 0;
  int nq = 109, nv = 108;
  WalkFloorConvex xc{};  // filled by build_walk_floor_convex (walk_self_model.hpp) for a handle with FFE_WALK_FLOOR_CONVEX alone
};

// One floor candidate in float64: the geom in its link's frame and the contact parameters of the pair (floor geom `fg`, geom `g`) by
// mj_contactParam (geom1 = the floor): friction, margin and gap the larger value, solref / solimp weighted by solmix.  The device table
// holds these rounded to float32; tests/walk_floor_host.cpp reads them unrounded.
struct FloorGeom {
  double pos[3], axis[3], rad, half, fric, K, B, margin, gap, invw, solimp[5];
  int condim;
};
inline FloorGeom floor_geom_params(const Blob &b, int fg, int g) {
  using namespace detail;
  const Tensor &gbody = b.get("geom_bodyid"), &gtype = b.get("geom_type"), &gsize = b.get("geom_size"), &gpos = b.get("geom_pos"),
               &gquat = b.get("geom_quat"), &gfric = b.get("geom_friction"), &gmargin = b.get("geom_margin"), &ggap = b.get("geom_gap"),
               &gsolref = b.get("geom_solref"), &gsolimp = b.get("geom_solimp"), &gsolmix = b.get("geom_solmix"), &gcondim = b.get("geom_condim"),
               &binvw = b.get("body_invweight0");
  FloorGeom o;
  double q[4] = {gquat.f(4 * g), gquat.f(4 * g + 1), gquat.f(4 * g + 2), gquat.f(4 * g + 3)}, mm[9];
  q2m(q, mm);
  for (int k = 0; k < 3; k++) { o.pos[k] = gpos.f(3 * g + k); o.axis[k] = mm[3 * k + 2]; }
  o.rad = gsize.f(3 * g); o.half = gtype.i(g) == 3 ? gsize.f(3 * g + 1) : 0.0;
  o.margin = std::max(gmargin.f(g), gmargin.f(fg)); o.gap = std::max(ggap.f(g), ggap.f(fg));
  o.fric = std::max(gfric.f(3 * g), gfric.f(3 * fg));
  o.condim = std::max(gcondim.i(g), gcondim.i(fg));
  const double s1 = gsolmix.f(fg), s2 = gsolmix.f(g);
  const double mix = (s1 >= 1e-15 && s2 >= 1e-15) ? s1 / (s1 + s2) : ((s1 < 1e-15 && s2 < 1e-15) ? 0.5 : (s1 < 1e-15 ? 0.0 : 1.0));
  double sr[2];
  for (int k = 0; k < 2; k++)
    sr[k] = (gsolref.f(2 * fg) > 0 && gsolref.f(2 * g) > 0) ? mix * gsolref.f(2 * fg + k) + (1 - mix) * gsolref.f(2 * g + k)
                                                             : std::min(gsolref.f(2 * fg + k), gsolref.f(2 * g + k));
  for (int k = 0; k < 5; k++) o.solimp[k] = mix * gsolimp.f(5 * fg + k) + (1 - mix) * gsolimp.f(5 * g + k);
  kb(sr[0], sr[1], o.solimp[1], b.get("opt").f(0), &o.K, &o.B);
  o.invw = binvw.f(2 * gbody.i(fg)) + binvw.f(2 * gbody.i(g));
  return o;
}

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
  // ---- floor contacts: one table row per primitive geom that can touch the floor
  {
    const Tensor &gbody = b.get("geom_bodyid"), &gtype = b.get("geom_type"), &gsize = b.get("geom_size"), &gpos = b.get("geom_pos"),
                 &gquat = b.get("geom_quat"), &gct = b.get("geom_contype"), &gca = b.get("geom_conaffinity"), &excl = b.get("exclude_pairs");
    (void)gsize;
    const int fg = X.floor_geom, nex = (int)excl.count / 2;
    {
      double q[4] = {gquat.f(4 * fg), gquat.f(4 * fg + 1), gquat.f(4 * fg + 2), gquat.f(4 * fg + 3)}, mm[9], wq[4], wp[3], fr[9];
      // (the floor hangs on the world body: its frame in the world is its frame in that body)
      const double bq[4] = {bquat.f(0), bquat.f(1), bquat.f(2), bquat.f(3)}, gp[3] = {gpos.f(3 * fg), gpos.f(3 * fg + 1), gpos.f(3 * fg + 2)};
      qmul(bq, q, wq);
      q2m(wq, mm);
      rot(bq, gp, wp);
      for (int k = 0; k < 3; k++) { fr[k] = mm[3 * k + 2]; wp[k] += bpos.f(k); }
      wf::make_frame(fr);
      for (int k = 0; k < 9; k++) X.f_frame[k] = (float)fr[k];
      X.f_off = (float)(fr[0] * wp[0] + fr[1] * wp[1] + fr[2] * wp[2]);
    }
    std::vector<int> lane_of((size_t)nb, -1);
    for (int l = 0; l < NL; l++) lane_of[(size_t)M.l_body[l]] = l;
    X.f_ok = 1;
    for (int l = 0; l < NL; l++) { X.f_link[l] = -1; X.f_adh[l] = -1; }
    for (int g = 0; g < (int)gbody.count; g++) {
      const int body = gbody.i(g), l = lane_of[(size_t)body], ty = gtype.i(g);
      if (l < 0 || (ty != 2 && ty != 3)) continue;  // (a plane against an ellipsoid or a cylinder: WalkFloorConvex, a table of its own)
      if (!((gct.i(fg) & gca.i(g)) || (gct.i(g) & gca.i(fg)))) continue;
      bool skip = false;
      for (int e = 0; e < nex; e++) skip |= (excl.i(2 * e) == 0 && excl.i(2 * e + 1) == body) || (excl.i(2 * e) == body && excl.i(2 * e + 1) == 0);
      if (skip) continue;
      if (X.f_n >= NL) throw std::runtime_error("walk model: more floor candidates than lanes");
      const int s = X.f_n++;
      const FloorGeom fp = floor_geom_params(b, fg, g);
      X.f_geom[s] = g; X.f_link[s] = l; X.f_adh[s] = M.l_adh[l];
      const int last = M.s_dof[M.l_ndof[l] - 1][l];
      X.f_blk[s] = M.d_blk[last]; X.f_amask[s] = M.d_amask[last];
      for (int k = 0; k < 3; k++) { X.f_pos[k][s] = (float)fp.pos[k]; X.f_axis[k][s] = (float)fp.axis[k]; }
      X.f_rad[s] = (float)fp.rad; X.f_half[s] = (float)fp.half; X.f_margin[s] = (float)fp.margin; X.f_gap[s] = (float)fp.gap;
      X.f_fric[s] = (float)fp.fric; X.f_K[s] = (float)fp.K; X.f_B[s] = (float)fp.B; X.f_invw[s] = (float)fp.invw;
      {
        double reach = std::sqrt(fp.pos[0] * fp.pos[0] + fp.pos[1] * fp.pos[1] + fp.pos[2] * fp.pos[2]) + fp.half + fp.rad + fp.margin;
        for (int a = l; a >= 0; a = M.l_parent[a])
          reach += std::sqrt((double)M.l_pos[0][a] * M.l_pos[0][a] + (double)M.l_pos[1][a] * M.l_pos[1][a] + (double)M.l_pos[2][a] * M.l_pos[2][a]);
        X.f_reach = std::max(X.f_reach, (float)(1.001 * reach + 1e-6));
      }
      if (fp.condim != 3) X.f_ok = 0;
      for (int k = 0; k < 5; k++) {
        if (s == 0) X.f_solimp[k] = (float)fp.solimp[k];
        else if (X.f_solimp[k] != (float)fp.solimp[k]) X.f_ok = 0;
      }
    }
  }
  return W;
}

}  // namespace ffb
