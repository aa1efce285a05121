// Stand-alone host program for tests/test_walk_floor_cpu.py (built with -fsanitize=address,undefined, never loaded into Python):
//   walk_floor_host <floor-only fly_walk.ffmb> <states.bin>
// The floor tables of build_walk_model and the formulas of csrc/walk_floor.hpp (plane distance, contact position, frame, J_r, J_f, y0 and
// the rank-6 term of G), in float64 and in float32, against the float64 oracle's contacts and constraint rows on the states of
// states.bin.  The link poses and motion axes come from a restatement of the leg code's kinematics in the root frame (leg_stage1.inc) in
// the same scalar type.
// In the float64 run nothing is rounded to float32 on the way: the geoms and their contact parameters come from the blob through
// floor_geom_params, the link poses from the oracle's xpos / xquat and the hinge axes from the blob's jnt_axis; the float32 run reads
// the device tables as the kernel does.
// states.bin (float64, written by the test from the oracle): nstates; per state: qpos[109], qvel[108], M[108][108], qacc_smooth[108],
// xpos[nbody][3], xquat[nbody][4], ncon, per contact: efc_adr, dist, pos[3], normal[3], includemargin, mu, then per contact with rows: 3 x (J[108], aref, D), then
// G_ref[3 nrc][3 nrc] = J M^-1 J' over those rows in that order.
// Prints `key value` lines: worst errors per quantity, each relative to the largest |reference| of that quantity.
#define CVX_HOST 1  // convex.hpp (pulled in by dev_model.hpp) without the HIP runtime
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <map>
#include <type_traits>
#include <string>
#include <vector>

struct float4 { float x, y, z, w; };  // the one HIP vector type dev_model.hpp names (flight tables, unused here)

#include "../flybody_amd/csrc/walk_model.hpp"

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
  const WalkExtra &X = W.m.x;
  constexpr bool F64 = std::is_same<T, double>::value;
  const int nbody = (int)blob.get("body_parentid").count;
  std::vector<FloorGeom> FG((size_t)X.f_n);
  for (int g = 0; g < X.f_n; g++) {
    FloorGeom &o = FG[(size_t)g];
    if (F64) { o = floor_geom_params(blob, X.floor_geom, X.f_geom[g]); continue; }
    for (int k = 0; k < 3; k++) { o.pos[k] = X.f_pos[k][g]; o.axis[k] = X.f_axis[k][g]; }
    o.rad = X.f_rad[g]; o.half = X.f_half[g]; o.fric = X.f_fric[g]; o.K = X.f_K[g]; o.B = X.f_B[g]; o.margin = X.f_margin[g]; o.gap = X.f_gap[g];
    o.invw = X.f_invw[g]; o.condim = 3;
    for (int k = 0; k < 5; k++) o.solimp[k] = X.f_solimp[k];
  }
  Reader in{sb};
  const int nstates = (int)in.next();
  std::map<std::string, Err> E;
  int contacts = 0, rows = 0, count_match = 1, unmatched = 0, most = 0;
  double far = 0;  // the farthest a geom's surface + margin got from the root origin on these states
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
    struct OC { int adr; double dist, pos[3], nrm[3], incl, mu; };
    std::vector<OC> oc((size_t)ncon);
    int nrc = 0;
    for (OC &c : oc) {
      c.adr = (int)in.next(); c.dist = in.next();
      for (double &x : c.pos) x = in.next();
      for (double &x : c.nrm) x = in.next();
      c.incl = in.next(); c.mu = in.next();
      if (c.adr >= 0) nrc++;
    }
    const int R = 3 * nrc;
    std::vector<double> Jo((size_t)R * 108), arefo((size_t)R), Do((size_t)R), Gref((size_t)R * (size_t)R);
    for (int r = 0; r < R; r++) { for (int k = 0; k < 108; k++) Jo[(size_t)r * 108 + k] = in.next(); arefo[(size_t)r] = in.next(); Do[(size_t)r] = in.next(); }
    for (double &x : Gref) x = in.next();
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
    // ---- root
    const T rq[4] = {(T)qpos[3], (T)qpos[4], (T)qpos[5], (T)qpos[6]};
    T Rr[9], fw[9], fr[9];
    quat2mat(rq, Rr);
    for (int k = 0; k < 9; k++) fw[k] = (T)X.f_frame[k];
    wf::frame_in_root<T>(Rr, fw, fr);
    const double height = (double)X.f_frame[0] * qpos[0] + (double)X.f_frame[1] * qpos[1] + (double)X.f_frame[2] * qpos[2] - (double)X.f_off;
    const T vw[3] = {(T)qvel[0], (T)qvel[1], (T)qvel[2]}, wb[3] = {(T)qvel[3], (T)qvel[4], (T)qvel[5]};
    T vb[3] = {Rr[0] * vw[0] + Rr[3] * vw[1] + Rr[6] * vw[2], Rr[1] * vw[0] + Rr[4] * vw[1] + Rr[7] * vw[2], Rr[2] * vw[0] + Rr[5] * vw[1] + Rr[8] * vw[2]};
    const T gz = (T)M.gz;
    const T gb[3] = {Rr[6] * gz, Rr[7] * gz, Rr[8] * gz};  // R' (0, 0, gz)
    // the root rows of qacc_smooth as the arrowhead solve gives them: wdot_b, vdot_b = R' (a_w - g) - w_b x v_b
    T xr[6];
    {
      const T aw[3] = {(T)qas[0], (T)qas[1], (T)qas[2] - gz};
      T wv[3];
      wf::cross3(wv, wb, vb);
      for (int k = 0; k < 3; k++) { xr[k] = (T)qas[(size_t)(3 + k)]; xr[3 + k] = Rr[k] * aw[0] + Rr[3 + k] * aw[1] + Rr[6 + k] * aw[2] - wv[k]; }
    }
    // ---- collision: every geom of the floor table, both ends of a capsule
    struct PC { int g; T dist, p[3], incl; };
    std::vector<PC> pc;
    for (int g = 0; g < X.f_n; g++) {
      const int l = X.f_link[g];
      T lm[9], c[3], a[3];
      quat2mat(lq[l], lm);
      const FloorGeom &fgm = FG[(size_t)g];
      const T gp[3] = {(T)fgm.pos[0], (T)fgm.pos[1], (T)fgm.pos[2]}, ga[3] = {(T)fgm.axis[0], (T)fgm.axis[1], (T)fgm.axis[2]};
      matvec(lm, gp, c);
      matvec(lm, ga, a);
      for (int k = 0; k < 3; k++) c[k] += lp[l][k];
      const T half = (T)fgm.half, rad = (T)fgm.rad, margin = (T)fgm.margin;
      for (int e = 0; e < (half > 0 ? 2 : 1); e++) {
        const T sgn = e == 0 ? (T)1 : (T)-1, end[3] = {c[0] + sgn * half * a[0], c[1] + sgn * half * a[1], c[2] + sgn * half * a[2]};
        far = std::fmax(far, std::sqrt((double)(end[0] * end[0] + end[1] * end[1] + end[2] * end[2])) + (double)rad + (double)margin);
        const T dist = wf::plane_distance<T>(height, fr, end, rad);
        if (!(dist <= margin)) continue;
        PC o;
        o.g = g; o.dist = dist; o.incl = margin - (T)fgm.gap;
        wf::contact_position<T>(end, fr, rad, dist, o.p);
        pc.push_back(o);
      }
    }
    if ((int)pc.size() != ncon) count_match = 0;
    contacts += ncon;
    most = std::max(most, ncon);
    // ---- each contact of the oracle against the program's contact at the same place
    std::vector<std::vector<T>> Jrow;   // rows in the oracle's order: root (w_b, v_b) 6 | hinges 102
    std::vector<int> rowg;
    for (const OC &c : oc) {
      int best = -1;
      double bd = 1e30;
      for (size_t k = 0; k < pc.size(); k++) {
        T pw[3];
        matvec(Rr, pc[k].p, pw);
        double d2 = 0;
        for (int a = 0; a < 3; a++) { const double d = (double)pw[a] + qpos[(size_t)a] - c.pos[a]; d2 += d * d; }
        if (d2 < bd) { bd = d2; best = (int)k; }
      }
      if (best < 0 || bd > 1e-8) { unmatched++; continue; }
      const PC &p = pc[(size_t)best];
      const int g = p.g, l = X.f_link[g];
      T pw[3], nw[3];
      matvec(Rr, p.p, pw);
      matvec(Rr, fr, nw);
      E["dist"].add((double)p.dist, c.dist);
      for (int a = 0; a < 3; a++) { E["pos"].add((double)pw[a] + qpos[(size_t)a], c.pos[a]); E["normal"].add((double)nw[a], c.nrm[a]); }
      E["includemargin"].add((double)p.incl, c.incl);
      const FloorGeom &fgm = FG[(size_t)g];
      E["friction"].add((double)(T)fgm.fric, c.mu);
      if (((double)p.dist >= (double)p.incl) != (c.adr < 0)) { unmatched++; continue; }
      if (c.adr < 0) continue;
      const T imp = impedance<T>(fgm.solimp, std::fabs(p.dist - p.incl));
      const T D = 1 / std::fmax((T)1e-15, (1 - imp) * (T)fgm.invw / imp);
      // velocity of the contact point in the root frame: root + hinges of the chain
      for (int r = 0; r < 3; r++) {
        const T *e = &fr[3 * r];
        std::vector<T> J(108, (T)0);
        T jr[6];
        wf::row_root<T>(p.p, e, jr);
        for (int k = 0; k < 6; k++) J[(size_t)k] = jr[k];
        for (int q = 0; q < M.l_nchain[l]; q++) { const int f = M.l_chain[q][l]; J[(size_t)(6 + f)] = wf::row_hinge<T>(cdof[f], p.p, e); }
        T vel = 0;
        for (int k = 0; k < 3; k++) vel += jr[k] * wb[k] + jr[3 + k] * vb[k];
        for (int f = 0; f < ND; f++) vel += J[(size_t)(6 + f)] * (T)qvel[(size_t)(6 + f)];
        const T aref = -(T)fgm.B * vel - (r == 0 ? (T)fgm.K * imp * (p.dist - p.incl) : (T)0);
        T y0 = wf::root_y0<T>(jr, xr, wb, vb, gb) - aref;
        for (int f = 0; f < ND; f++) y0 += J[(size_t)(6 + f)] * (T)qas[(size_t)(6 + f)];
        // against the oracle's row: J in MuJoCo's coordinates is (R e, p x e, hinges)
        const size_t ro = (size_t)rowg.size();
        const double *jo = &Jo[ro * 108];
        T ew[3];
        matvec(Rr, e, ew);
        double y0ref = -arefo[ro];
        for (int k = 0; k < 108; k++) y0ref += jo[k] * qas[(size_t)k];
        for (int k = 0; k < 3; k++) { E["J"].add((double)ew[k], jo[k]); E["J"].add((double)jr[k], jo[3 + k]); }
        for (int f = 0; f < ND; f++) E["J"].add((double)J[(size_t)(6 + f)], jo[6 + f]);
        E["aref"].add((double)aref, arefo[ro]);
        E["y0"].add((double)y0, y0ref);
        if (r == 0) E["D"].add((double)D, Do[ro]);
        Jrow.push_back(J);
        rowg.push_back(g);
      }
    }
    if ((int)rowg.size() != R) { unmatched++; continue; }
    rows += R;
    // ---- G through the arrowhead: M in the kernel's root coordinates (w_b, v_b): qvel_mj = (R v_b, w_b, hinges)
    {
      auto Mk = [&](int i, int j) -> double {  // (T' M T)_ij
        auto col = [&](int a, int k) -> double {  // T[a][k]: row a of MuJoCo's qvel, column k of the kernel's
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
      std::vector<std::vector<T>> col((size_t)R, std::vector<T>(ND)), u((size_t)R, std::vector<T>(6));
      for (int r = 0; r < R; r++) {
        T jy[6];
        for (int a = 0; a < 6; a++) { jy[a] = 0; for (int f = 0; f < ND; f++) jy[a] += Jrow[(size_t)r][(size_t)(6 + f)] * Y[(size_t)a][(size_t)f]; }
        wf::rank6_factor<T>(S, id, Jrow[(size_t)r].data(), jy, u[(size_t)r].data());
        for (int f = 0; f < ND; f++) col[(size_t)r][(size_t)f] = Jrow[(size_t)r][(size_t)(6 + f)];
        solve(col[(size_t)r]);
      }
      for (int i = 0; i < R; i++) for (int k = 0; k < R; k++) {
        T g = 0;
        for (int f = 0; f < ND; f++) g += Jrow[(size_t)i][(size_t)(6 + f)] * col[(size_t)k][(size_t)f];
        for (int a = 0; a < 6; a++) g += u[(size_t)i][(size_t)a] * u[(size_t)k][(size_t)a];
        E["G"].add((double)g, Gref[(size_t)i * (size_t)R + (size_t)k]);
      }
    }
  }
  std::printf("%s_states %d\n%s_contacts %d\n%s_rows %d\n%s_most_contacts %d\n%s_count_match %d\n%s_unmatched %d\n", tag, nstates, tag, contacts, tag, rows, tag,
              most, tag, count_match, tag, unmatched);
  std::printf("%s_farthest %.6f\n", tag, far);
  for (const auto &kv : E) std::printf("%s_%s %.3e\n", tag, kv.first.c_str(), kv.second.rel());
}

int main(int argc, char **argv) {
  if (argc != 3) { std::fprintf(stderr, "usage: %s fly_walk_flooronly.ffmb states.bin\n", argv[0]); return 2; }
  try {
    const std::vector<char> wb = slurp(argv[1]), sb = slurp(argv[2]);
    const Blob blob(wb.data(), wb.size());
    const WalkHost W = build_walk_model(blob);
    std::printf("floor_geoms %d\nfloor_tables_ok %d\nfloor_reach %.6f\n", W.m.x.f_n, W.m.x.f_ok, (double)W.m.x.f_reach);
    run<double>(W, blob, sb, "f64");
    run<float>(W, blob, sb, "f32");
  } catch (const std::exception &e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
  return 0;
}
