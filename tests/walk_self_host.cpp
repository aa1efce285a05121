// Stand-alone host program for tests/test_walk_self_cpu.py (built with -fsanitize=address,undefined, never loaded into Python):
//   walk_self_host <fly_walk.ffmb> <states.bin> <pairs.txt>
// The collision tables of build_walk_self (written to pairs.txt as model geom ids: `sp g1 g2` for every sphere / capsule candidate
// pair, `cp g1 g2` for every convex candidate pair) and the formulas of csrc/walk_self.hpp (the two-chain row, its velocity, D, aref, y0,
// its share of G and the force's way back to hinges and root), in float64 and in float32, against the float64 oracle's fly-fly
// contacts and constraint rows on the states of states.bin.  The contact points and normals are the oracle's (carried into the root
// frame): the narrow phase is convex.hpp's, float32 only, and has its own host test (tests/cvx_host.cpp).  The link poses and motion
// axes come from a restatement of the leg code's kinematics in the root frame, as in tests/walk_floor_host.cpp.
// states.bin (float64, written by the test from the oracle): nstates; per state: qpos[109], qvel[108], M[108][108], qacc_smooth[108],
// xpos[nbody][3], xquat[nbody][4], n fly-fly contacts, per contact: body1, body2, efc_adr, dist, pos[3], normal[3], includemargin; then
// per contact with a row: J[108], aref, D, force; then G_ref[R][R] = J M^-1 J' over those rows in that order, then dq_ref[108] = M^-1 J' f.
// Prints `key value` lines: worst errors per quantity, each relative to the largest |reference| of that quantity.
#define CVX_HOST 1  // convex.hpp (pulled in by dev_model.hpp) without the HIP runtime
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <map>
#include <string>
#include <type_traits>
#include <vector>

struct float4 { float x, y, z, w; };  // the one HIP vector type dev_model.hpp names (flight tables, unused here)

#include "../flybody_amd/csrc/walk_self_model.hpp"
#include "../flybody_amd/csrc/walk_self.hpp"

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
  double rel() const { return scale > 0 ? err / scale : err; }
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
// mj: getimpedance, in the scalar type
template <class T>
static T impedance(const double *si, T x) {
  const T d0 = std::fmin(std::fmax((T)si[0], (T)1e-4), (T)0.9999), d1 = std::fmin(std::fmax((T)si[1], (T)1e-4), (T)0.9999);
  const T width = std::fmax((T)0, (T)si[2]), mid = std::fmin(std::fmax((T)si[3], (T)1e-4), (T)0.9999), power = std::fmax((T)1, (T)si[4]);
  if (d0 == d1 || width <= (T)1e-15) return (T)0.5 * (d0 + d1);
  x = x / width;
  if (x >= 1) return d1;
  if (x <= 0) return d0;
  T y;
  if (power == 1) y = x;
  else if (x <= mid) y = std::pow(x, power) / std::pow(mid, power - 1);
  else y = 1 - std::pow(1 - x, power) / std::pow(1 - mid, power - 1);
  return d0 + y * (d1 - d0);
}

template <class T>
static void run(const WalkHost &W, const Blob &blob, const std::vector<char> &sb, const char *tag) {
  const BallModel &M = W.m.b;
  constexpr bool F64 = std::is_same<T, double>::value;
  const int nbody = (int)blob.get("body_parentid").count;
  std::vector<int> lane_of((size_t)nbody, -1);
  for (int l = 0; l < NL; l++) lane_of[(size_t)M.l_body[l]] = l;
  const Tensor &binvw = blob.get("body_invweight0"), &gsolref = blob.get("geom_solref"), &gsolimp = blob.get("geom_solimp");
  // contact parameters of a fly-fly pair: uniform over the fly's geoms (checked by build_walk_self); unrounded in the float64 run
  double Kd, Bd, simp[5];
  for (int k = 0; k < 5; k++) simp[k] = F64 ? gsolimp.f(5 * 1 + k) : (double)M.sc_solimp[k];
  if (F64) detail::kb(gsolref.f(2), gsolref.f(3), gsolimp.f(5 + 1), blob.get("opt").f(0), &Kd, &Bd);
  else { Kd = M.sc_K; Bd = M.sc_B; }
  Reader in{sb};
  const int nstates = (int)in.next();
  std::map<std::string, Err> E;
  int contacts = 0, rows = 0, two_block = 0, thorax_rows = 0, most = 0;
  for (int st = 0; st < nstates; st++) {
    std::vector<double> qpos(109), qvel(108), Md(108 * 108), qas(108);
    for (double &x : qpos) x = in.next();
    for (double &x : qvel) x = in.next();
    for (double &x : Md) x = in.next();
    for (double &x : qas) x = in.next();
    std::vector<double> xpos((size_t)nbody * 3), xquat((size_t)nbody * 4);
    for (double &x : xpos) x = in.next();
    for (double &x : xquat) x = in.next();
    const int ncon = (int)in.next();
    struct OC { int b1, b2, adr; double dist, pos[3], nrm[3], incl; };
    std::vector<OC> oc((size_t)ncon);
    int R = 0;
    for (OC &c : oc) {
      c.b1 = (int)in.next(); c.b2 = (int)in.next(); c.adr = (int)in.next(); c.dist = in.next();
      for (double &x : c.pos) x = in.next();
      for (double &x : c.nrm) x = in.next();
      c.incl = in.next();
      if (c.adr >= 0) R++;
    }
    std::vector<double> Jo((size_t)R * 108), arefo((size_t)R), Do((size_t)R), fo((size_t)R), Gref((size_t)R * (size_t)R), dqref(108);
    for (int r = 0; r < R; r++) { for (int k = 0; k < 108; k++) Jo[(size_t)r * 108 + k] = in.next(); arefo[(size_t)r] = in.next(); Do[(size_t)r] = in.next(); fo[(size_t)r] = in.next(); }
    for (double &x : Gref) x = in.next();
    for (double &x : dqref) x = in.next();
    contacts += ncon;
    most = std::max(most, ncon);
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
      // the same from the oracle's body poses (tests/walk_floor_host.cpp)
      const double rqd[4] = {qpos[3], qpos[4], qpos[5], qpos[6]}, rc[4] = {rqd[0], -rqd[1], -rqd[2], -rqd[3]};
      double Rd[9];
      quat2mat(rqd, Rd);
      const Tensor &jaxis = blob.get("jnt_axis"), &bjadr = blob.get("body_jntadr");
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
    // ---- root: rotation, velocities in its own frame, the root rows of qacc_smooth as the arrowhead solve gives them
    const T rq[4] = {(T)qpos[3], (T)qpos[4], (T)qpos[5], (T)qpos[6]};
    T Rr[9];
    quat2mat(rq, Rr);
    const T vw[3] = {(T)qvel[0], (T)qvel[1], (T)qvel[2]}, wb[3] = {(T)qvel[3], (T)qvel[4], (T)qvel[5]};
    const T vb[3] = {Rr[0] * vw[0] + Rr[3] * vw[1] + Rr[6] * vw[2], Rr[1] * vw[0] + Rr[4] * vw[1] + Rr[7] * vw[2], Rr[2] * vw[0] + Rr[5] * vw[1] + Rr[8] * vw[2]};
    const T gz = (T)M.gz;
    T xr[6];
    {
      const T aw[3] = {(T)qas[0], (T)qas[1], (T)qas[2] - gz};
      T wv[3];
      wf::cross3(wv, wb, vb);
      for (int k = 0; k < 3; k++) { xr[k] = (T)qas[(size_t)(3 + k)]; xr[3 + k] = Rr[k] * aw[0] + Rr[3 + k] * aw[1] + Rr[6 + k] * aw[2] - wv[k]; }
    }
    // spatial velocity of every link (ang, lin about the root origin): the root's plus its chain's hinges
    T sv0[6] = {wb[0], wb[1], wb[2], vb[0], vb[1], vb[2]}, sv[NL][6];
    for (int l = 0; l < NL; l++) {
      for (int k = 0; k < 6; k++) sv[l][k] = sv0[k];
      for (int p = 0; p < M.l_nchain[l]; p++) { const int f = M.l_chain[p][l]; for (int k = 0; k < 6; k++) sv[l][k] += cdof[f][k] * (T)qvel[(size_t)(6 + f)]; }
    }
    auto on_chain = [&](int l, int f) { if (l < 0) return false; for (int p = 0; p < M.l_nchain[l]; p++) if (M.l_chain[p][l] == f) return true; return false; };
    // ---- M in the kernel's root coordinates, its factor, Y_m and S_m (tests/walk_floor_host.cpp)
    auto Mk = [&](int i, int j) -> double {
      auto col = [&](int a, int k) -> double {
        if (a >= 6 || k >= 6) return a == k ? 1.0 : 0.0;
        if (a < 3) return k >= 3 ? (double)Rr[3 * a + (k - 3)] : 0.0;
        return k == a - 3 ? 1.0 : 0.0;
      };
      double s = 0;
      const int alo = i < 6 ? 0 : i, ahi = i < 6 ? 6 : i + 1, blo = j < 6 ? 0 : j, bhi = j < 6 ? 6 : j + 1;
      for (int a = alo; a < ahi; a++) for (int b = blo; b < bhi; b++) s += col(a, i) * Md[(size_t)a * 108 + (size_t)b] * col(b, j);
      return s;
    };
    std::vector<T> Lj((size_t)ND * ND);
    for (int i = 0; i < ND; i++) for (int j = 0; j < ND; j++) Lj[(size_t)i * ND + j] = (T)Md[(size_t)(6 + i) * 108 + 6 + j];
    for (int j = 0; j < ND; j++) {
      T d = Lj[(size_t)j * ND + j];
      for (int k = 0; k < j; k++) d -= Lj[(size_t)j * ND + k] * Lj[(size_t)j * ND + k];
      if (!(d > 0)) throw std::runtime_error("M_jj is not positive definite");
      const T ir = 1 / std::sqrt(d);
      Lj[(size_t)j * ND + j] = d * ir;
      for (int i = j + 1; i < ND; i++) {
        T e = Lj[(size_t)i * ND + j];
        for (int k = 0; k < j; k++) e -= Lj[(size_t)i * ND + k] * Lj[(size_t)j * ND + k];
        Lj[(size_t)i * ND + j] = e * ir;
      }
    }
    auto solve = [&](std::vector<T> &x) {
      for (int i = 0; i < ND; i++) { T w = x[(size_t)i]; for (int k = 0; k < i; k++) w -= Lj[(size_t)i * ND + k] * x[(size_t)k]; x[(size_t)i] = w / Lj[(size_t)i * ND + i]; }
      for (int i = ND - 1; i >= 0; i--) { T w = x[(size_t)i]; for (int k = i + 1; k < ND; k++) w -= Lj[(size_t)k * ND + i] * x[(size_t)k]; x[(size_t)i] = w / Lj[(size_t)i * ND + i]; }
    };
    std::vector<std::vector<T>> Y(6, std::vector<T>(ND));
    for (int a = 0; a < 6; a++) { for (int f = 0; f < ND; f++) Y[(size_t)a][(size_t)f] = (T)Mk(6 + f, a); solve(Y[(size_t)a]); }
    T S[6][6], id[6];
    for (int a = 0; a < 6; a++) for (int b = 0; b < 6; b++) {
      T p = 0;
      for (int f = 0; f < ND; f++) p += (T)Mk(a, 6 + f) * Y[(size_t)b][(size_t)f];
      S[a][b] = (T)Mk(a, b) - p;
    }
    if (!wf::chol6<T>(S, id)) throw std::runtime_error("S_m is not positive definite");
    // z_m = M_jj^-1 f_j of the smooth force: recovered from the oracle's qacc_smooth, a_s = z_m - Y_m x_r on the hinges
    std::vector<T> zm(ND);
    for (int f = 0; f < ND; f++) { T z = (T)qas[(size_t)(6 + f)]; for (int a = 0; a < 6; a++) z += Y[(size_t)a][(size_t)f] * xr[a]; zm[(size_t)f] = z; }
    // ---- each fly-fly contact of the oracle: the two-chain row from the formulas
    std::vector<std::vector<T>> Jrow;
    int ro = 0;
    for (const OC &c : oc) {
      int l1 = lane_of[(size_t)c.b1], l2 = lane_of[(size_t)c.b2];
      if ((l1 < 0 && c.b1 != 1) || (l2 < 0 && c.b2 != 1)) throw std::runtime_error("a fly-fly contact on an unknown body");
      // point and normal in the root frame
      double dp[3] = {c.pos[0] - qpos[0], c.pos[1] - qpos[1], c.pos[2] - qpos[2]};
      T p[3], n[3];
      for (int k = 0; k < 3; k++) {
        p[k] = (T)((double)Rr[k] * dp[0] + (double)Rr[3 + k] * dp[1] + (double)Rr[6 + k] * dp[2]);
        n[k] = (T)((double)Rr[k] * c.nrm[0] + (double)Rr[3 + k] * c.nrm[1] + (double)Rr[6 + k] * c.nrm[2]);
      }
      int lpos = l2, lneg = l1;  // as the kernel stores it (self_put): a thorax geom2 turns the pair round
      if (lpos < 0) { lpos = l1; lneg = -1; for (int k = 0; k < 3; k++) n[k] = -n[k]; }
      if (c.adr < 0) continue;
      if (lneg < 0) thorax_rows++;
      else if (M.d_blk[M.l_chain[0][lpos]] != M.d_blk[M.l_chain[0][lneg]]) two_block++;
      std::vector<T> J(108, (T)0);
      for (int f = 0; f < ND; f++) J[(size_t)(6 + f)] = wsf::row_hinge<T>(cdof[f], p, n, on_chain(lpos, f), on_chain(lneg, f));
      const T vel = wsf::row_velocity<T>(sv[lpos], lneg >= 0 ? sv[lneg] : sv0, p, n);
      const double invw = binvw.f(2 * c.b1) + binvw.f(2 * c.b2);
      const T incl = (T)c.incl, dist = (T)c.dist;
      const T imp = impedance<T>(simp, std::fabs(dist - incl));
      const T D = wsf::row_D<T>(imp, F64 ? (T)invw : (T)((float)binvw.f(2 * c.b1) + (float)binvw.f(2 * c.b2)));
      const T naref = wsf::row_neg_aref<T>((T)Kd, (T)Bd, imp, dist, incl, vel);
      T jz = 0, jy[6] = {0, 0, 0, 0, 0, 0};
      for (int f = 0; f < ND; f++) { jz += J[(size_t)(6 + f)] * zm[(size_t)f]; for (int a = 0; a < 6; a++) jy[a] += J[(size_t)(6 + f)] * Y[(size_t)a][(size_t)f]; }
      const T y0 = wsf::row_y0<T>(jz, jy, xr, naref);
      const double *jo = &Jo[(size_t)ro * 108];
      double y0ref = -arefo[(size_t)ro];
      for (int k = 0; k < 108; k++) y0ref += jo[k] * qas[(size_t)k];
      for (int k = 0; k < 108; k++) E["J"].add((double)J[(size_t)k], jo[k]);  // (the oracle's row is zero on the root too)
      E["aref"].add(-(double)naref, arefo[(size_t)ro]);
      E["D"].add((double)D, Do[(size_t)ro]);
      E["y0"].add((double)y0, y0ref);
      Jrow.push_back(J);
      ro++;
    }
    if (ro != R) throw std::runtime_error("row count out of step");
    rows += R;
    // ---- G through the arrowhead, and the force's way back: dq = M^-1 J' f with nothing on the root's right-hand side
    std::vector<std::vector<T>> col((size_t)R, std::vector<T>(ND)), u((size_t)R, std::vector<T>(6));
    for (int r = 0; r < R; r++) {
      T jy[6];
      for (int a = 0; a < 6; a++) { jy[a] = 0; for (int f = 0; f < ND; f++) jy[a] += Jrow[(size_t)r][(size_t)(6 + f)] * Y[(size_t)a][(size_t)f]; }
      wsf::rank6_factor<T>(S, id, jy, u[(size_t)r].data());
      for (int f = 0; f < ND; f++) col[(size_t)r][(size_t)f] = Jrow[(size_t)r][(size_t)(6 + f)];
      solve(col[(size_t)r]);
    }
    for (int i = 0; i < R; i++) for (int k = 0; k < R; k++) {
      T g = 0;
      for (int f = 0; f < ND; f++) g += Jrow[(size_t)i][(size_t)(6 + f)] * col[(size_t)k][(size_t)f];
      for (int a = 0; a < 6; a++) g += u[(size_t)i][(size_t)a] * u[(size_t)k][(size_t)a];
      E["G"].add((double)g, Gref[(size_t)i * (size_t)R + (size_t)k]);
    }
    if (R > 0) {
      std::vector<T> qf(ND, (T)0);  // J_j' f
      for (int r = 0; r < R; r++) for (int f = 0; f < ND; f++) qf[(size_t)f] += Jrow[(size_t)r][(size_t)(6 + f)] * (T)fo[(size_t)r];
      std::vector<T> z = qf;
      solve(z);
      T br[6], x6[6];
      for (int a = 0; a < 6; a++) { br[a] = 0; for (int f = 0; f < ND; f++) br[a] -= (T)Mk(a, 6 + f) * z[(size_t)f]; }  // 0 - M_rj z
      for (int i = 0; i < 6; i++) { T w = br[i]; for (int k = 0; k < i; k++) w -= S[i][k] * x6[k]; x6[i] = w * id[i]; }
      for (int i = 5; i >= 0; i--) { T w = x6[i]; for (int k = i + 1; k < 6; k++) w -= S[k][i] * x6[k]; x6[i] = w * id[i]; }
      for (int k = 0; k < 3; k++) {
        E["qacc"].add((double)(Rr[3 * k] * x6[3] + Rr[3 * k + 1] * x6[4] + Rr[3 * k + 2] * x6[5]), dqref[(size_t)k]);
        E["qacc"].add((double)x6[k], dqref[(size_t)(3 + k)]);
      }
      for (int f = 0; f < ND; f++) {
        T a = z[(size_t)f];
        for (int k = 0; k < 6; k++) a -= Y[(size_t)k][(size_t)f] * x6[k];
        E["qacc"].add((double)a, dqref[(size_t)(6 + f)]);
      }
    }
  }
  std::printf("%s_states %d\n%s_contacts %d\n%s_rows %d\n%s_most_contacts %d\n%s_two_block_rows %d\n%s_thorax_rows %d\n", tag, nstates, tag, contacts, tag, rows, tag,
              most, tag, two_block, tag, thorax_rows);
  for (const auto &kv : E) std::printf("%s_%s %.3e\n", tag, kv.first.c_str(), kv.second.rel());
}

int main(int argc, char **argv) {
  if (argc != 4) { std::fprintf(stderr, "usage: %s fly_walk.ffmb states.bin pairs.txt\n", argv[0]); return 2; }
  try {
    const std::vector<char> wb = slurp(argv[1]), sb = slurp(argv[2]);
    const Blob blob(wb.data(), wb.size());
    WalkHost W = build_walk_model(blob);
    const WalkHost plain = W;
    build_walk_self(blob, W);
    const BallModel &M = W.m.b;
    // the tables FFE_WALK_SELF adds leave everything the other kernels read as it was
    std::printf("extra_untouched %d\n", std::memcmp(&plain.m.x, &W.m.x, sizeof(WalkExtra)) == 0 ? 1 : 0);
    std::printf("slots %d\nsp_pairs %d\ncp_pairs %d\ngeoms %d\nsphere_slot %d\n", M.npg, M.nsp, M.ncp, M.ncg, M.sp_sphere);
    {
      const int floor = W.m.x.floor_geom;
      std::vector<int> geom_of;  // fly geom index -> model geom
      for (int g = 0; g < (int)blob.get("geom_bodyid").count; g++) if (g != floor) geom_of.push_back(g);
      std::ofstream out(argv[3]);
      for (int s1 = 0; s1 < NPG; s1++) for (int s2 = s1 + 1; s2 < NPG; s2++)
        if ((M.sp_mask[s1] >> s2) & 1ull) {
          if (!((M.sp_mask[s2] >> s1) & 1ull)) throw std::runtime_error("sp_mask is not symmetric");
          out << "sp " << W.m.x.f_geom[s1] << " " << W.m.x.f_geom[s2] << "\n";
        }
      for (int k = 0; k < M.ncp; k++) out << "cp " << geom_of[(size_t)(M.cp_pair[k] & 255)] << " " << geom_of[(size_t)(M.cp_pair[k] >> 8)] << "\n";
    }
    run<double>(W, blob, sb, "f64");
    run<float>(W, blob, sb, "f32");
  } catch (const std::exception &e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
  return 0;
}
