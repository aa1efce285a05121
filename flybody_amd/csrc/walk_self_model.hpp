// walk_self_model.hpp - host-side construction of the collision tables of the walking fly's own contacts (FFE_WALK_SELF; DESIGN.md
// section 12 step 3c).
//
// `detail::build_fly_model(b, true)` leaves the fly-fly collision tables of BallModel empty (the tethered build alone fills them, and its
// code is not touched).  `build_walk_self` fills the same fields of the walk model's BallModel from fly_walk.ffmb, the way the tethered
// build fills them from fly_ball.ffmb, with what differs on the free root:
//   the 48 sphere / capsule slots are the 48 rows of the floor table (WalkExtra::f_*: the same geoms in the same model order, checked), so
//            a slot's geom frame in its link is read from there and `pgs_link[s] == f_link[s]`;
//   a geom of the thorax has no link (`cg_link` -1) and its frame in the root is its frame in the thorax body: the root frame IS the
//            thorax frame;
//   the blob's candidate list (`cand_g1` / `cand_g2`, flybody_amd/model/reach.py) also holds the 70 pairs with the floor plane: the 48
//            (plane, sphere / capsule) ones are the floor pass's, the 22 (plane, ellipsoid / cylinder) ones the second floor pass's
//            (`build_walk_floor_convex` below; the oracle does not restate them); neither kind is a fly-fly pair and both are skipped here.
// No kernel but `floor_self_step` reads these fields, and `walk_create` calls this only for a handle with the bit.
#pragma once

#include "walk_model.hpp"

namespace ffb {

inline void build_walk_self(const Blob &b, WalkHost &W) {
  using namespace detail;
  BallModel &M = W.m.b;
  const WalkExtra &X = W.m.x;
  const Tensor &gbody = b.get("geom_bodyid"), &gtype = b.get("geom_type"), &gsize = b.get("geom_size"), &gpos = b.get("geom_pos"),
               &gquat = b.get("geom_quat"), &gmargin = b.get("geom_margin"), &ggap = b.get("geom_gap"), &gsolref = b.get("geom_solref"),
               &gsolimp = b.get("geom_solimp"), &gcondim = b.get("geom_condim"), &gct = b.get("geom_contype"), &gca = b.get("geom_conaffinity"),
               &excl = b.get("exclude_pairs"), &weld = b.get("body_weldid"), &bpar = b.get("body_parentid"), &binvw = b.get("body_invweight0");
  const double h = b.get("opt").f(0);
  const int nb = (int)bpar.count, ng = (int)gbody.count, thorax = 1, floor = X.floor_geom;
  std::vector<int> lane_of((size_t)nb, -1);
  for (int l = 0; l < NL; l++) lane_of[(size_t)M.l_body[l]] = l;
  // ---- the 48 primitive slots
  std::vector<int> slot_of((size_t)ng, -1);
  int npg = 0;
  double sref[2] = {0, 0}, simp[5] = {0, 0, 0, 0, 0};
  M.sc_margin = M.sc_gap = 0.f; M.sp_claw = 0ull; M.sp_sphere = -1; M.nsp = 0;
  for (int l = 0; l < NL; l++) M.sp_mask[l] = 0ull;
  for (int g = 0; g < ng; g++) {
    const int l = lane_of[(size_t)gbody.i(g)], ty = gtype.i(g);
    if (l < 0 || (ty != 2 && ty != 3)) continue;
    if (npg >= NPG) throw std::runtime_error("walk model: more primitive geoms than slots");
    if (npg >= X.f_n || X.f_geom[npg] != g || X.f_link[npg] != l)
      throw std::runtime_error("walk model: FFE_WALK_SELF expects the floor table to list the fly's sphere / capsule geoms in slot order");
    slot_of[(size_t)g] = npg; M.pgs_link[npg] = l;
    M.pgs_invw[npg] = (float)binvw.f(2 * gbody.i(g));
    if (gcondim.i(g) != 1) throw std::runtime_error("walk model: fly geoms are expected to be condim 1");
    if (npg == 0) { for (int k = 0; k < 2; k++) sref[k] = gsolref.f(2 * g + k); for (int k = 0; k < 5; k++) simp[k] = gsolimp.f(5 * g + k); }
    for (int k = 0; k < 2; k++) if (gsolref.f(2 * g + k) != sref[k]) throw std::runtime_error("walk model: fly geom solref is expected to be uniform");
    for (int k = 0; k < 5; k++) if (gsolimp.f(5 * g + k) != simp[k]) throw std::runtime_error("walk model: fly geom solimp is expected to be uniform");
    if (gmargin.f(g) != 0) {
      if (M.sc_margin != 0 && (M.sc_margin != (float)gmargin.f(g) || M.sc_gap != (float)ggap.f(g))) throw std::runtime_error("walk model: one margin class expected");
      M.sc_margin = (float)gmargin.f(g); M.sc_gap = (float)ggap.f(g);
      M.sp_claw |= 1ull << npg;
    }
    if (ty == 2) { if (M.sp_sphere >= 0) throw std::runtime_error("walk model: one sphere expected among the fly geoms"); M.sp_sphere = npg; }
    npg++;
  }
  if (npg != NPG || X.f_n != NPG) throw std::runtime_error("walk model: the pair enumeration expects exactly NPG primitive geoms, all of them floor candidates");
  M.npg = npg;
  {
    double K, B;
    kb(sref[0], sref[1], simp[1], h, &K, &B);  // mj_contactParam: equal solmix weights of equal parameters
    M.sc_K = (float)K; M.sc_B = (float)B;
    for (int k = 0; k < 5; k++) M.sc_solimp[k] = (float)simp[k];
  }
  // ---- the pair filter of mj_collision (weld, parent-child, <exclude>, contype / conaffinity), body-pair major as the oracle walks it
  const int nex = (int)excl.count / 2;
  for (int b1 = 0; b1 < nb; b1++) for (int b2 = b1 + 1; b2 < nb; b2++) {
    const int w1 = weld.i(b1), w2 = weld.i(b2);
    if (w1 == w2) continue;
    const int wp1 = weld.i(bpar.i(w1)), wp2 = weld.i(bpar.i(w2));
    if (w1 != 0 && w2 != 0 && (w1 == wp2 || w2 == wp1)) continue;
    bool skip = false;
    for (int e = 0; e < nex; e++) skip |= (excl.i(2 * e) == b1 && excl.i(2 * e + 1) == b2) || (excl.i(2 * e) == b2 && excl.i(2 * e + 1) == b1);
    if (skip) continue;
    for (int ga = 0; ga < ng; ga++) {
      if (gbody.i(ga) != b1 || slot_of[(size_t)ga] < 0) continue;
      for (int gb = 0; gb < ng; gb++) {
        if (gbody.i(gb) != b2 || slot_of[(size_t)gb] < 0) continue;
        if (!((gct.i(ga) & gca.i(gb)) || (gct.i(gb) & gca.i(ga)))) continue;
        int g1 = ga, g2 = gb;
        if (gtype.i(g1) > gtype.i(g2)) std::swap(g1, g2);  // mj: lower type code first
        const int s1 = slot_of[(size_t)g1], s2 = slot_of[(size_t)g2];
        // the kernel derives the order instead of storing it
        const int e1 = (s1 == M.sp_sphere || s2 == M.sp_sphere) ? M.sp_sphere : std::min(s1, s2);
        if (e1 != s1) throw std::runtime_error("walk model: unexpected geom order of a fly-fly pair");
        M.sp_mask[s1] |= 1ull << s2; M.sp_mask[s2] |= 1ull << s1;
        M.nsp++;
      }
    }
  }
  // ---- convex pairs: all fly geoms in model order (the floor plane left out), the static candidate list
  if (ng - 1 > NG) throw std::runtime_error("walk model: more collision geoms than the geom table holds");
  std::vector<int> fg((size_t)ng, -1);  // model geom -> fly geom index
  int n = 0;
  M.cg_mmask[0] = M.cg_mmask[1] = 0ull;
  for (int g = 0; g < ng; g++) {
    if (g == floor) continue;
    const int body = gbody.i(g), l = lane_of[(size_t)body], ty = gtype.i(g);
    if (l < 0 && body != thorax) throw std::runtime_error("walk model: collision geom on an unexpected body");
    if (ty < 2 || ty > 5) throw std::runtime_error("walk model: unexpected geom type");
    fg[(size_t)g] = n;
    M.cg_link[n] = l; M.cg_type[n] = ty;  // (l < 0: the thorax, whose frame is the root frame)
    for (int k = 0; k < 3; k++) { M.cg_pos[k][n] = (float)gpos.f(3 * g + k); M.cg_size[k][n] = (float)gsize.f(3 * g + k); }
    for (int k = 0; k < 4; k++) M.cg_quat[k][n] = (float)gquat.f(4 * g + k);
    const double s0 = gsize.f(3 * g), s1 = gsize.f(3 * g + 1), s2 = gsize.f(3 * g + 2);
    M.cg_brad[n] = (float)(ty == 2 ? s0 : ty == 3 ? s0 + s1 : ty == 5 ? std::sqrt(s0 * s0 + s1 * s1) : std::max(s0, std::max(s1, s2)));
    M.cg_invw[n] = (float)binvw.f(2 * body);
    if (gmargin.f(g) != 0) {
      if ((float)gmargin.f(g) != M.sc_margin || (float)ggap.f(g) != M.sc_gap) throw std::runtime_error("walk model: one margin class expected");
      M.cg_mmask[n >> 6] |= 1ull << (n & 63);
    }
    if (gcondim.i(g) != 1) throw std::runtime_error("walk model: fly geoms are expected to be condim 1");
    {
      double K, B;
      kb(gsolref.f(2 * g), gsolref.f(2 * g + 1), gsolimp.f(5 * g + 1), h, &K, &B);
      if ((float)K != M.sc_K || (float)B != M.sc_B) throw std::runtime_error("walk model: fly geom solref is expected to be uniform");
      for (int q = 0; q < 5; q++) if ((float)gsolimp.f(5 * g + q) != M.sc_solimp[q]) throw std::runtime_error("walk model: fly geom solimp is expected to be uniform");
    }
    n++;
  }
  M.ncg = n;
  M.ncp = 0;
  for (int k = 0; k < NCP; k++) M.cp_pair[k] = 0xffffu;
  const Tensor &cg1 = b.get("cand_g1"), &cg2 = b.get("cand_g2");
  for (size_t k = 0; k < cg1.count; k++) {
    int g1 = cg1.i(k), g2 = cg2.i(k);
    if (gtype.i(g1) > gtype.i(g2)) std::swap(g1, g2);
    if (gtype.i(g1) == 0) continue;                      // a pair with the floor plane: one of the two floor passes'
    if (gtype.i(g1) < 4 && gtype.i(g2) < 4) continue;    // a sphere / capsule pair: sp_mask has it
    if (fg[(size_t)g1] < 0 || fg[(size_t)g2] < 0) throw std::runtime_error("walk model: a candidate pair names an unknown geom");
    if (M.ncp >= NCP) throw std::runtime_error("walk model: more convex candidate pairs than the list holds");
    M.cp_pair[M.ncp++] = (unsigned short)(fg[(size_t)g1] | (fg[(size_t)g2] << 8));
  }
}

// The second floor table (FFE_WALK_FLOOR_CONVEX): the (plane, ellipsoid / cylinder) pairs the two tables
// above leave out, filtered as `build_walk_model` filters the 48 primitive ones.  A geom of the thorax has no link: the thorax is the root.
inline void build_walk_floor_convex(const Blob &b, WalkHost &W) {
  using namespace detail;
  const BallModel &M = W.m.b;
  const WalkExtra &X = W.m.x;
  WalkFloorConvex &F = W.xc;
  std::memset(&F, 0, sizeof(F));
  const Tensor &gbody = b.get("geom_bodyid"), &gtype = b.get("geom_type"), &gsize = b.get("geom_size"), &gpos = b.get("geom_pos"),
               &gquat = b.get("geom_quat"), &gct = b.get("geom_contype"), &gca = b.get("geom_conaffinity"), &excl = b.get("exclude_pairs"),
               &bpar = b.get("body_parentid");
  const int nb = (int)bpar.count, fg = X.floor_geom, nex = (int)excl.count / 2, thorax = 1;
  std::vector<int> lane_of((size_t)nb, -1);
  for (int l = 0; l < NL; l++) lane_of[(size_t)M.l_body[l]] = l;
  F.ok = 1;
  for (int g = 0; g < (int)gbody.count; g++) {
    const int body = gbody.i(g), l = lane_of[(size_t)body], ty = gtype.i(g);
    if (g == fg || (ty != 4 && ty != 5)) continue;
    if (!((gct.i(fg) & gca.i(g)) || (gct.i(g) & gca.i(fg)))) continue;
    bool skip = false;
    for (int e = 0; e < nex; e++) skip |= (excl.i(2 * e) == 0 && excl.i(2 * e + 1) == body) || (excl.i(2 * e) == body && excl.i(2 * e + 1) == 0);
    if (skip) continue;
    if (l < 0 && body != thorax) throw std::runtime_error("walk model: a floor candidate on an unexpected body");
    if (F.n >= NFC) throw std::runtime_error("walk model: more ellipsoid / cylinder floor candidates than the table holds");
    const int s = F.n++;
    const FloorGeom fp = floor_geom_params(b, fg, g);
    F.geom[s] = g; F.type[s] = ty; F.link[s] = l;
    if (l >= 0) {
      const int last = M.s_dof[M.l_ndof[l] - 1][l];
      F.adh[s] = M.l_adh[l]; F.blk[s] = M.d_blk[last]; F.amask[s] = M.d_amask[last];
    } else { F.adh[s] = -1; F.blk[s] = 255; F.amask[s] = 0; }
    for (int k = 0; k < 3; k++) { F.pos[k][s] = (float)gpos.f(3 * g + k); F.size[k][s] = (float)gsize.f(3 * g + k); }
    for (int k = 0; k < 4; k++) F.quat[k][s] = (float)gquat.f(4 * g + k);
    F.fric[s] = (float)fp.fric; F.K[s] = (float)fp.K; F.B[s] = (float)fp.B; F.margin[s] = (float)fp.margin; F.gap[s] = (float)fp.gap;
    F.invw[s] = (float)fp.invw;
    if (fp.condim != 3) F.ok = 0;
    for (int k = 0; k < 5; k++) if (X.f_solimp[k] != (float)fp.solimp[k]) F.ok = 0;  // the same rule as f_ok
  }
}

}  // namespace ffb
