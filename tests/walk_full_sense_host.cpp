// Stand-alone host program for tests/test_walk_full_env_cpu.py (built with -fsanitize=address,undefined, never loaded into Python):
//   walk_full_sense_host <fly_walk_round.ffmb> <states.bin>
// tests/walk_self_sense_host.cpp with the contacts of the second floor pass among the floor's: the force
// and touch sensors of the walking fly on a free root (csrc/walk_sense.hpp, csrc/walk_self_sense.hpp) when the contact slots also hold
// plane-ellipsoid contacts, in float64 and in float32, against the float64 oracle's sens_force / sens_touch.  The blob is the round
// device blob of tests/walk_full_env_samples.py (every ellipsoid round), the states come from the oracle on the round oracle blob (the
// same geoms as spheres), so the oracle's plane-sphere contacts are the contacts of the device's ellipsoid path.
// The contacts are put into slots the way the kernel's tile holds them - c_link a byte that is 255 for a geom of the thorax, c_geom a byte
// that is NPG + row for a row of WalkFloorConvex - and the sensor pass reads them the way `contact_sense` does: a slot belongs to link l
// when c_link == l, and nothing is indexed with c_link or c_geom.  Every per-link array here has NL entries and every per-geom table its
// own length, so an index of 255 or of 48 + row into one of them would be a sanitizer report.
// states.bin: as tests/walk_self_sense_host.cpp.
// Prints that program's `key value` lines and: `convex` floor slots with c_geom >= NPG, `convex_root` those with c_link == 255,
// `convex_sensed` those whose link lies under a force sensor, `convex_touch` those on a claw's link.
#define CVX_HOST 1  // convex.hpp (pulled in by dev_model.hpp) without the HIP runtime
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <string>
#include <type_traits>
#include <vector>

struct float4 { float x, y, z, w; };  // the one HIP vector type dev_model.hpp names (flight tables, unused here)

#include "../flybody_amd/csrc/walk_model.hpp"
#include "../flybody_amd/csrc/walk_sense.hpp"
#include "../flybody_amd/csrc/walk_self_sense.hpp"
#include "../flybody_amd/csrc/walk_self_model.hpp"

using namespace ffb;

static std::vector<char> slurp(const char *path) {
  std::ifstream f(path, std::ios::binary);
  if (!f) throw std::runtime_error(std::string("cannot open ") + path);
  return std::vector<char>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

struct Reader {
  const std::vector<char> &b;
  size_t at = 0;
  double next() {
    if (at + sizeof(double) > b.size()) throw std::runtime_error("states file: truncated");
    double v;
    std::memcpy(&v, b.data() + at, sizeof(double));
    at += sizeof(double);
    return v;
  }
};

struct Err {
  double err = 0, scale = 0;
  void add(double x, double ref) { err = std::fmax(err, std::fabs(x - ref)); scale = std::fmax(scale, std::fabs(ref)); }
  double rel() const { return err / std::fmax(1.0, scale); }
};

template <class T>
static void quat2mat(const T *q, T *m) {
  const T w = q[0], x = q[1], y = q[2], z = q[3];
  m[0] = w * w + x * x - y * y - z * z; m[1] = 2 * (x * y - w * z); m[2] = 2 * (x * z + w * y);
  m[3] = 2 * (x * y + w * z); m[4] = w * w - x * x + y * y - z * z; m[5] = 2 * (y * z - w * x);
  m[6] = 2 * (x * z - w * y); m[7] = 2 * (y * z + w * x); m[8] = w * w - x * x - y * y + z * z;
}
template <class T>
static void quatmul(const T *a, const T *b, T *r) {
  const T o[4] = {a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3], a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
                  a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1], a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0]};
  for (int k = 0; k < 4; k++) r[k] = o[k];
}
template <class T>
static void matvec(const T *m, const T *v, T *r) {
  const T o[3] = {m[0] * v[0] + m[1] * v[1] + m[2] * v[2], m[3] * v[0] + m[4] * v[1] + m[5] * v[2], m[6] * v[0] + m[7] * v[1] + m[8] * v[2]};
  for (int k = 0; k < 3; k++) r[k] = o[k];
}
// mj: mju_crossMotion
template <class T>
static void cross_motion(const T *vel, const T *v, T *r) {
  T a[3], b[3], c[3];
  wf::cross3(a, vel, v);
  wf::cross3(b, vel, v + 3);
  wf::cross3(c, vel + 3, v);
  for (int k = 0; k < 3; k++) { r[k] = a[k]; r[3 + k] = b[k] + c[k]; }
}

template <class T>
static void run(const WalkHost &W, const Blob &blob, const std::vector<char> &sb, const char *tag) {
  const BallModel &M = W.m.b;
  const WalkExtra &X = W.m.x;
  constexpr bool F64 = std::is_same<T, double>::value;
  const int nbody = (int)blob.get("body_parentid").count;
  const Tensor &bmass = blob.get("body_mass"), &bipos = blob.get("body_ipos"), &squat = blob.get("sites_quat"), &fsite = blob.get("force_site");
  const Tensor &jaxis = blob.get("jnt_axis"), &bjadr = blob.get("body_jntadr");
  const double gz = blob.get("opt").f(5);
  if (std::fabs(gz - (double)M.gz) > 1e-4 * std::fabs(gz)) throw std::runtime_error("gravity of the blob and of the device tables differ");
  Reader in{sb};
  const int nstates = (int)in.next();
  Err Ef, Et;
  int convex = 0, convex_root = 0, convex_sensed = 0, convex_touch = 0;
  int contacts = 0, rows = 0, most = 0, unmatched = 0, touching = 0, flyfly = 0, ff_rows = 0, ff_pos = 0, ff_neg = 0, ff_thorax = 0, ff_thorax_sensed = 0, ff_touch = 0;
  // links under a force sensor (its own link included): where a fly-fly force shows in a reading
  std::vector<char> sensed((size_t)NL, 0);
  for (int l = 0; l < NL; l++) sensed[(size_t)l] = M.l_force[l] >= 0 || (M.l_parent[l] >= 0 && sensed[(size_t)M.l_parent[l]]);
  auto link_of_body = [&](int body) { for (int l = 0; l < NL; l++) if (M.l_body[l] == body) return l; return -1; };
  double free_force = 0;  // the largest |force| on a state's sensors whose subtrees carry no contact: the inertial term alone
  for (int st = 0; st < nstates; st++) {
    std::vector<double> qpos(109), qvel(108), qacc(108);
    for (double &x : qpos) x = in.next();
    for (double &x : qvel) x = in.next();
    for (double &x : qacc) x = in.next();
    std::vector<double> xpos((size_t)nbody * 3), xquat((size_t)nbody * 4);
    for (double &x : xpos) x = in.next();
    for (double &x : xquat) x = in.next();
    const int ncon = (int)in.next();
    // link: of geom2 (a floor contact's fly geom; `pos` of a fly-fly contact); link1: of geom1 of a fly-fly contact (-1: the thorax)
    // link8 / geom8: the bytes the tile keeps for a floor slot (255: no link; NPG + row: a row of WalkFloorConvex)
    struct OC { int adr, link, link1; bool self; double n[3], f[3]; unsigned char link8, geom8; };
    std::vector<OC> oc((size_t)ncon);
    for (OC &c : oc) {
      c.adr = (int)in.next();
      const int g1 = (int)in.next(), g2 = (int)in.next(), b1 = (int)in.next(), b2 = (int)in.next();
      for (double &x : c.n) x = in.next();
      for (double &x : c.f) x = in.next();
      c.self = g1 != 0;
      c.link = c.link1 = -1;
      if (!c.self) {
        bool found = false;
        c.link8 = 255; c.geom8 = 255;
        for (int g = 0; g < X.f_n; g++) if (X.f_geom[g] == g2) { c.link = X.f_link[g]; c.link8 = (unsigned char)c.link; c.geom8 = (unsigned char)g; found = true; }
        for (int r = 0; r < W.xc.n && !found; r++) {
          if (W.xc.geom[r] != g2) continue;
          found = true;
          c.link = W.xc.link[r];  // (-1: a geom of the thorax)
          c.link8 = (unsigned char)(c.link >= 0 ? c.link : 255); c.geom8 = (unsigned char)(NPG + r);
          convex++;
          if (c.link < 0) convex_root++;
          else {
            if (sensed[(size_t)c.link]) convex_sensed++;
            if (M.l_touch[c.link] >= 0) convex_touch++;
          }
        }
        if (!found) unmatched++;
        if (c.adr >= 0) rows += 3;
      } else {
        c.link = link_of_body(b2); c.link1 = link_of_body(b1);
        if (c.link < 0 && c.link1 < 0) unmatched++;  // (both on the thorax: no such pair)
        flyfly++;
        if (c.adr >= 0) {
          rows += 1; ff_rows++;
          if (c.link >= 0 && sensed[(size_t)c.link]) ff_pos++;
          if (c.link1 >= 0 && sensed[(size_t)c.link1]) ff_neg++;
          if (c.link < 0 || c.link1 < 0) {  // one geom on the thorax: that side has no link and adds to no sensor
            ff_thorax++;
            if (sensed[(size_t)(c.link < 0 ? c.link1 : c.link)]) ff_thorax_sensed++;
          }
        }
      }
    }
    contacts += ncon;
    most = std::max(most, ncon);
    double ref_force[18], ref_touch[6];
    for (double &x : ref_force) x = in.next();
    for (double &x : ref_touch) x = in.next();
    // ---- kinematics of the links in the root frame about the root origin (leg_stage1.inc restated), motion axes of the hinges
    T lp[NL][3], lq[NL][4], cdof[ND][6];
    for (int f = 0; f < ND; f++) for (int k = 0; k < 6; k++) cdof[f][k] = 0;
    for (int l = 0; l < NL; l++) {
      const int par = M.l_parent[l];
      if (par >= l) throw std::runtime_error("links are expected parent first");
      T pp[3] = {0, 0, 0}, pq[4] = {1, 0, 0, 0}, pm[9];
      if (par >= 0) { for (int k = 0; k < 3; k++) pp[k] = lp[par][k]; for (int k = 0; k < 4; k++) pq[k] = lq[par][k]; }
      quat2mat(pq, pm);
      const T pos[3] = {(T)M.l_pos[0][l], (T)M.l_pos[1][l], (T)M.l_pos[2][l]};
      T off[3];
      matvec(pm, pos, off);
      for (int k = 0; k < 3; k++) lp[l][k] = pp[k] + off[k];
      T qrel[4] = {(T)M.l_quat[0][l], (T)M.l_quat[1][l], (T)M.l_quat[2][l], (T)M.l_quat[3][l]};
      for (int s = 0; s < M.l_ndof[l]; s++) {
        const int f = M.s_dof[s][l];
        const T ax[3] = {(T)M.s_axis[0][s][l], (T)M.s_axis[1][s][l], (T)M.s_axis[2][s][l]};
        T rm[9], axp[3], axw[3], neg[3] = {-lp[l][0], -lp[l][1], -lp[l][2]}, lin[3];
        quat2mat(qrel, rm);
        matvec(rm, ax, axp);
        matvec(pm, axp, axw);
        wf::cross3(lin, axw, neg);
        for (int k = 0; k < 3; k++) { cdof[f][k] = axw[k]; cdof[f][3 + k] = lin[k]; }
        const T half = (T)0.5 * (T)qpos[(size_t)(7 + f)], sn = std::sin(half), cs = std::cos(half);
        const T dq[4] = {cs, ax[0] * sn, ax[1] * sn, ax[2] * sn};
        quatmul(qrel, dq, qrel);
      }
      quatmul(pq, qrel, lq[l]);
      T n = 0;
      for (int k = 0; k < 4; k++) n += lq[l][k] * lq[l][k];
      n = 1 / std::sqrt(n);
      for (int k = 0; k < 4; k++) lq[l][k] *= n;
    }
    if (F64) {
      // the same from the oracle's body poses: p = R' (xpos - p_root), q = conj(q_root) xquat; the axis of hinge s of a body is fixed in
      // the frame the body has before that hinge turns: xquat (rot_s ... rot_last)^-1
      const double rqd[4] = {qpos[3], qpos[4], qpos[5], qpos[6]}, rc[4] = {rqd[0], -rqd[1], -rqd[2], -rqd[3]};
      double Rd[9];
      quat2mat(rqd, Rd);
      for (int l = 0; l < NL; l++) {
        const int body = M.l_body[l];
        double dp[3], pl[3], ql[4];
        for (int k = 0; k < 3; k++) dp[k] = xpos[(size_t)(3 * body + k)] - qpos[(size_t)k];
        for (int k = 0; k < 3; k++) pl[k] = Rd[k] * dp[0] + Rd[3 + k] * dp[1] + Rd[6 + k] * dp[2];
        quatmul(rc, &xquat[(size_t)(4 * body)], ql);
        for (int k = 0; k < 3; k++) lp[l][k] = (T)pl[k];
        for (int k = 0; k < 4; k++) lq[l][k] = (T)ql[k];
        double qb[4] = {ql[0], ql[1], ql[2], ql[3]};
        for (int s2 = M.l_ndof[l] - 1; s2 >= 0; s2--) {
          const int f = M.s_dof[s2][l], j = bjadr.i(body) + s2;
          const double ax[3] = {jaxis.f(3 * j), jaxis.f(3 * j + 1), jaxis.f(3 * j + 2)}, half = 0.5 * qpos[(size_t)(7 + f)];
          const double inv[4] = {std::cos(half), -ax[0] * std::sin(half), -ax[1] * std::sin(half), -ax[2] * std::sin(half)};
          quatmul(qb, inv, qb);
          double rm[9], aw[3], neg[3] = {-pl[0], -pl[1], -pl[2]}, li[3];
          quat2mat(qb, rm);
          matvec(rm, ax, aw);
          wf::cross3(li, aw, neg);
          for (int k = 0; k < 3; k++) { cdof[f][k] = (T)aw[k]; cdof[f][3 + k] = (T)li[k]; }
        }
      }
    }
    // ---- root: V0 = (w_b, R' v_w); the root rows of qacc as the arrowhead solve leaves them: wdot_b, R' (a_w - g) - w_b x v_b
    const T rq[4] = {(T)qpos[3], (T)qpos[4], (T)qpos[5], (T)qpos[6]};
    T Rr[9], fw[9], fr[9];
    quat2mat(rq, Rr);
    for (int k = 0; k < 9; k++) fw[k] = (T)X.f_frame[k];
    wf::frame_in_root<T>(Rr, fw, fr);
    const T vw[3] = {(T)qvel[0], (T)qvel[1], (T)qvel[2]};
    T V0[6], xr[6];
    for (int k = 0; k < 3; k++) { V0[k] = (T)qvel[(size_t)(3 + k)]; V0[3 + k] = Rr[k] * vw[0] + Rr[3 + k] * vw[1] + Rr[6 + k] * vw[2]; }
    {
      const T aw[3] = {(T)qacc[0], (T)qacc[1], (T)qacc[2] - (F64 ? (T)gz : (T)M.gz)};
      T wv[3];
      wf::cross3(wv, V0, V0 + 3);
      for (int k = 0; k < 3; k++) { xr[k] = (T)qacc[(size_t)(3 + k)]; xr[3 + k] = Rr[k] * aw[0] + Rr[3 + k] * aw[1] + Rr[6 + k] * aw[2] - wv[k]; }
    }
    // ---- velocities, bias accelerations and the path sums of cdof qacc, parent first; per link the velocity term, m, m r and the
    //      floor's force on it
    T cvel[NL][6], caccb[NL][6], dacc[NL][6], fv[NL][3], ms[NL], mr[NL][3], fext[NL][3];
    std::vector<char> loaded((size_t)NL, 0);
    for (int l = 0; l < NL; l++) {
      const int par = M.l_parent[l];
      T pv[6], da[6], dq[6];
      for (int k = 0; k < 6; k++) { pv[k] = par >= 0 ? cvel[par][k] : V0[k]; da[k] = par >= 0 ? caccb[par][k] : (T)0; dq[k] = par >= 0 ? dacc[par][k] : (T)0; }
      for (int s = 0; s < M.l_ndof[l]; s++) {
        const int f = M.s_dof[s][l];
        const T v = (T)qvel[(size_t)(6 + f)], a = (T)qacc[(size_t)(6 + f)];
        T cdd[6];
        cross_motion(pv, cdof[f], cdd);
        for (int k = 0; k < 6; k++) { pv[k] += v * cdof[f][k]; da[k] += v * cdd[k]; dq[k] += a * cdof[f][k]; }
      }
      for (int k = 0; k < 6; k++) { cvel[l][k] = pv[k]; caccb[l][k] = da[k]; dacc[l][k] = dq[k]; }
      const int body = M.l_body[l];
      const T mass = F64 ? (T)bmass.f(body) : (T)M.l_mass[l];
      T ip[3], lm[9], r[3];
      for (int k = 0; k < 3; k++) ip[k] = F64 ? (T)bipos.f(3 * body + k) : (T)M.l_ipos[k][l];
      quat2mat(lq[l], lm);
      matvec(lm, ip, r);
      for (int k = 0; k < 3; k++) r[k] += lp[l][k] - (T)M.thorax_pos[k];
      ws::velocity_term<T>(mass, da, pv, r, fv[l]);
      ms[l] = mass;
      for (int k = 0; k < 3; k++) { mr[l][k] = mass * r[k]; fext[l][k] = 0; }
      for (const OC &c : oc) {
        if (c.adr < 0) continue;
        if (!c.self) {
          if ((int)c.link8 != l) continue;  // (as `contact_sense`: 255 is no link)
          const T f[3] = {(T)c.f[0], (T)c.f[1], (T)c.f[2]};
          ws::add_contact_force<T>(fr, f, fext[l]);
          loaded[(size_t)l] = 1;
        } else if (c.link == l || c.link1 == l) {
          // the normal in the root frame: R' n
          const T nw[3] = {(T)c.n[0], (T)c.n[1], (T)c.n[2]};
          T n[3];
          for (int k = 0; k < 3; k++) n[k] = Rr[k] * nw[0] + Rr[3 + k] * nw[1] + Rr[6 + k] * nw[2];
          wss::add_pair_force<T>(n, (T)c.f[0], c.link == l, c.link1 == l, fext[l]);
          loaded[(size_t)l] = 1;
        }
      }
    }
    // ---- subtree sums, leaves first (the kernel sums each sensor's depth-first lane range): velocity terms, mass, m r, the floor's force;
    //      g = sum over the hinges d strictly below the link of lin(crb_d cdof_d) qacc_d, crb_d from the sums of d's own link
    T gsum[NL][3];
    for (int l = 0; l < NL; l++) for (int k = 0; k < 3; k++) gsum[l][k] = 0;
    for (int l = NL - 1; l >= 0; l--) {
      const int par = M.l_parent[l];
      if (par < 0) continue;
      if (par >= l) throw std::runtime_error("links are expected parent first");
      for (int s = 0; s < M.l_ndof[l]; s++) {  // (every child of l has been folded into l by now: ms / mr are its subtree's)
        const int f = M.s_dof[s][l];
        T col[3];
        ws::accel_term<T>(ms[l], mr[l], cdof[f], col);
        for (int k = 0; k < 3; k++) gsum[par][k] += col[k] * (T)qacc[(size_t)(6 + f)];
      }
      for (int k = 0; k < 3; k++) { fv[par][k] += fv[l][k]; mr[par][k] += mr[l][k]; fext[par][k] += fext[l][k]; gsum[par][k] += gsum[l][k]; }
      ms[par] += ms[l];
      loaded[(size_t)par] |= loaded[(size_t)l];
    }
    T fint[NL][3];
    for (int l = 0; l < NL; l++) {
      T A[6];
      for (int k = 0; k < 6; k++) A[k] = xr[k] + dacc[l][k];
      ws::accel_term<T>(ms[l], mr[l], A, fint[l]);
      for (int k = 0; k < 3; k++) fint[l][k] += gsum[l][k] + fv[l][k] - fext[l][k];
    }
    for (int l = 0; l < NL; l++) {
      const int fi = M.l_force[l], ti = M.l_touch[l];
      if (fi >= 0) {
        T sq[4], q[4], o[3];
        for (int k = 0; k < 4; k++) sq[k] = F64 ? (T)squat.f(4 * fsite.i(fi) + k) : (T)M.l_fsite[k][l];
        quatmul(lq[l], sq, q);
        ws::to_site<T>(q, fint[l], o);
        for (int k = 0; k < 3; k++) {
          Ef.add((double)o[k], ref_force[3 * fi + k]);
          if (!loaded[(size_t)l]) free_force = std::fmax(free_force, std::fabs(ref_force[3 * fi + k]));
        }
      }
      if (ti >= 0) {
        T touch = 0;
        for (const OC &c : oc) {
          if (c.adr < 0) continue;
          if (!c.self) { if ((int)c.link8 == l) touch += ws::touch_share<T>((T)c.f[0]); }
          else {
            const T share = wss::pair_touch_share<T>((T)c.f[0], c.link == l, c.link1 == l);
            touch += share;
            if (share > 0) ff_touch++;
          }
        }
        Et.add((double)touch, ref_touch[ti]);
        if (ref_touch[ti] > 0) touching++;
      }
    }
  }
  std::printf("%s_states %d\n%s_contacts %d\n%s_rows %d\n%s_most_contacts %d\n%s_unmatched %d\n%s_touching %d\n", tag, nstates, tag, contacts, tag, rows, tag,
              most, tag, unmatched, tag, touching);
  std::printf("%s_force %.3e\n%s_touch %.3e\n%s_force_scale %.6f\n%s_touch_scale %.6f\n%s_free_force %.6f\n", tag, Ef.rel(), tag, Et.rel(), tag, Ef.scale, tag,
              Et.scale, tag, free_force);
  std::printf("%s_flyfly %d\n%s_flyfly_rows %d\n%s_flyfly_pos %d\n%s_flyfly_neg %d\n%s_flyfly_thorax %d\n%s_flyfly_thorax_sensed %d\n%s_flyfly_touch %d\n", tag,
              flyfly, tag, ff_rows, tag, ff_pos, tag, ff_neg, tag, ff_thorax, tag, ff_thorax_sensed, tag, ff_touch);
  std::printf("%s_convex %d\n%s_convex_root %d\n%s_convex_sensed %d\n%s_convex_touch %d\n", tag, convex, tag, convex_root, tag, convex_sensed, tag, convex_touch);
}

int main(int argc, char **argv) {
  if (argc != 3) { std::fprintf(stderr, "usage: %s fly_walk_round.ffmb states.bin\n", argv[0]); return 2; }
  try {
    const std::vector<char> wb = slurp(argv[1]), sb = slurp(argv[2]);
    const Blob blob(wb.data(), wb.size());
    WalkHost W = build_walk_model(blob);
    build_walk_self(blob, W);
    build_walk_floor_convex(blob, W);
    if (!W.xc.ok || W.xc.n > NFC || NPG + W.xc.n > 255) throw std::runtime_error("the second floor table is not what the kernel expects");
    run<double>(W, blob, sb, "f64");
    run<float>(W, blob, sb, "f32");
  } catch (const std::exception &e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
  return 0;
}
