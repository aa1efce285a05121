// Stand-alone host program for tests/test_walk_limits_cpu.py (built with -fsanitize=address,undefined, never loaded into Python):
//   walk_limits_host <fly_walk.ffmb> <states.bin>
// 1. The limit tables of build_fly_model(walk = true) - s_limited / s_lo / s_hi / s_invw / s_K / s_B / j_solimp, the tables the limits
//    kernel of csrc/walk_env.hip instantiates its rows from - equal the walk blob's own jnt_limited, jnt_range, dof_invweight0,
//    jnt_solref (through mj's K / B formula) and jnt_solimp, joint by joint.
// 2. On the states of states.bin (float64, written by the test from the oracle): the rows instantiated from those tables in float32
//    are the oracle's rows (same hinges, same signs), their D equals the oracle's efc_D, and the arrowhead form of G the kernel uses,
//       G_ik = s_i s_k [(M_jj^-1)_{f_i f_k} + (L^-1 Y_m[f_i]) . (L^-1 Y_m[f_k])],  Y_m = M_jj^-1 M_jr,  S_m = M_rr - M_rj Y_m = L L',
//    evaluated in float32 from the oracle's dense M, equals the float64 J M^-1 J' the test computed from the oracle's efc rows.
// states.bin: nstates; per state: nrows, q[102] (hinge angles), M[108][108], then nrows x (dof, sign, D), then G[nrows][nrows].
// Prints `key value` lines.
#define CVX_HOST 1  // convex.hpp (pulled in by dev_model.hpp) without the HIP runtime
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
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

// mj: getimpedance with margin 0, in float32 as the kernels evaluate it
static float impedance(const float *si, float x) {
  const float d0 = std::fmin(std::fmax(si[0], 1e-4f), 0.9999f), d1 = std::fmin(std::fmax(si[1], 1e-4f), 0.9999f);
  const float width = std::fmax(0.f, si[2]), mid = std::fmin(std::fmax(si[3], 1e-4f), 0.9999f), power = std::fmax(1.f, si[4]);
  if (d0 == d1 || width <= 1e-15f) return 0.5f * (d0 + d1);
  x = x / width;
  if (x >= 1.f) return d1;
  if (x <= 0.f) return d0;
  float y;
  if (power == 1.f) y = x;
  else if (power == 2.f) y = x <= mid ? x * x / mid : 1.f - (1.f - x) * (1.f - x) / (1.f - mid);
  else if (x <= mid) y = std::pow(x, power) / std::pow(mid, power - 1.f);
  else y = 1.f - std::pow(1.f - x, power) / std::pow(1.f - mid, power - 1.f);
  return d0 + y * (d1 - d0);
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

int main(int argc, char **argv) {
  if (argc != 3) { std::fprintf(stderr, "usage: %s fly_walk.ffmb states.bin\n", argv[0]); return 2; }
  try {
    const std::vector<char> wb = slurp(argv[1]), sb = slurp(argv[2]);
    const Blob blob(wb.data(), wb.size());
    const WalkHost W = build_walk_model(blob);
    const BallModel &M = W.m.b;
    // ---- 1. the limit tables against the blob's own tensors, joint by joint
    std::vector<int> lane_of(ND, -1), slot_of(ND, -1);
    for (int l = 0; l < NL; l++) for (int s = 0; s < 4; s++) if (M.s_dof[s][l] >= 0) { lane_of[(size_t)M.s_dof[s][l]] = l; slot_of[(size_t)M.s_dof[s][l]] = s; }
    const Tensor &jtype = blob.get("jnt_type"), &jlim = blob.get("jnt_limited"), &jrange = blob.get("jnt_range"), &jsolref = blob.get("jnt_solref"),
                 &jsolimp = blob.get("jnt_solimp"), &jdadr = blob.get("jnt_dofadr"), &dinvw = blob.get("dof_invweight0"), &opt = blob.get("opt");
    const double h = opt.f(0);
    int checked = 0, limited = 0, bad = 0;
    for (int j = 0; j < (int)jtype.count; j++) {
      if (jtype.i(j) != 3) continue;
      const int od = jdadr.i(j), f = od - 6;
      if (f < 0 || f >= ND || lane_of[(size_t)f] < 0) { bad++; continue; }
      const int l = lane_of[(size_t)f], s = slot_of[(size_t)f];
      double K, B;
      detail::kb(jsolref.f(2 * j), jsolref.f(2 * j + 1), jsolimp.f(5 * j + 1), h, &K, &B);
      bool ok = M.s_limited[s][l] == jlim.i(j) && M.s_lo[s][l] == (float)jrange.f(2 * j) && M.s_hi[s][l] == (float)jrange.f(2 * j + 1) &&
                M.s_invw[s][l] == (float)dinvw.f(od) && M.s_K[s][l] == (float)K && M.s_B[s][l] == (float)B;
      for (int k = 0; k < 5; k++) ok = ok && M.j_solimp[k] == (float)jsolimp.f(5 * j + k) && M.s_solimp[k][s][l] == (float)jsolimp.f(5 * j + k);
      ok = ok && dinvw.f(od) > 0;
      bad += ok ? 0 : 1;
      checked++;
      limited += jlim.i(j) ? 1 : 0;
    }
    std::printf("hinges_checked %d\nlimited %d\nlimit_tables_ok %d\n", checked, limited, bad == 0 ? 1 : 0);
    // ---- 2. rows, D and G on the oracle's states
    Reader in{sb};
    const int nstates = (int)in.next();
    double g_err = 0, d_err = 0;
    int rows_total = 0, rows_match = 1, most = 0;
    for (int st = 0; st < nstates; st++) {
      const int n = (int)in.next();
      std::vector<double> q(ND), Md(108 * 108);
      for (double &x : q) x = in.next();
      for (double &x : Md) x = in.next();
      std::vector<int> odof((size_t)n);
      std::vector<double> osgn((size_t)n), oD((size_t)n), Gref((size_t)n * (size_t)n);
      for (int r = 0; r < n; r++) { odof[(size_t)r] = (int)in.next(); osgn[(size_t)r] = in.next(); oD[(size_t)r] = in.next(); }
      for (double &x : Gref) x = in.next();
      // rows from the tables, in float32, in hinge order (the oracle's order: mj_instantiateLimit walks the joints)
      std::vector<int> rf;
      std::vector<float> rs, rD;
      for (int f = 0; f < ND; f++) {
        const int l = lane_of[(size_t)f], s = slot_of[(size_t)f];
        if (!M.s_limited[s][l]) continue;
        const float qf = (float)q[(size_t)f], dlo = qf - M.s_lo[s][l], dhi = M.s_hi[s][l] - qf;
        float sg = 0.f, dist = 0.f;
        if (dlo < 0.f) { sg = 1.f; dist = dlo; } else if (dhi < 0.f) { sg = -1.f; dist = dhi; }
        if (sg == 0.f) continue;
        const float imp = impedance(M.j_solimp, std::fabs(dist));
        rf.push_back(f); rs.push_back(sg); rD.push_back(1.f / std::fmax(1e-15f, (1.f - imp) * M.s_invw[s][l] / imp));
      }
      if ((int)rf.size() != n) { rows_match = 0; continue; }
      for (int r = 0; r < n; r++) {
        if (rf[(size_t)r] != odof[(size_t)r] - 6 || (double)rs[(size_t)r] != osgn[(size_t)r]) rows_match = 0;
        d_err = std::fmax(d_err, std::fabs((double)rD[(size_t)r] - oD[(size_t)r]) / oD[(size_t)r]);
      }
      rows_total += n;
      most = std::max(most, n);
      // float32 arrowhead: Cholesky of M_jj, Y_m = M_jj^-1 M_jr and the rows' columns of M_jj^-1, S_m = M_rr - M_rj Y_m = L L'
      std::vector<float> Lj((size_t)ND * ND);
      for (int i = 0; i < ND; i++) for (int j = 0; j < ND; j++) Lj[(size_t)i * ND + j] = (float)Md[(size_t)(6 + i) * 108 + 6 + j];
      for (int j = 0; j < ND; j++) {
        float d = Lj[(size_t)j * ND + j];
        for (int k = 0; k < j; k++) d -= Lj[(size_t)j * ND + k] * Lj[(size_t)j * ND + k];
        if (!(d > 0.f)) throw std::runtime_error("M_jj is not positive definite in float32");
        const float ir = 1.f / std::sqrt(d);
        Lj[(size_t)j * ND + j] = d * ir;
        for (int i = j + 1; i < ND; i++) {
          float e = Lj[(size_t)i * ND + j];
          for (int k = 0; k < j; k++) e -= Lj[(size_t)i * ND + k] * Lj[(size_t)j * ND + k];
          Lj[(size_t)i * ND + j] = e * ir;
        }
      }
      auto solve = [&](std::vector<float> &x) {  // x <- M_jj^-1 x
        for (int i = 0; i < ND; i++) { float w = x[(size_t)i]; for (int k = 0; k < i; k++) w -= Lj[(size_t)i * ND + k] * x[(size_t)k]; x[(size_t)i] = w / Lj[(size_t)i * ND + i]; }
        for (int i = ND - 1; i >= 0; i--) { float w = x[(size_t)i]; for (int k = i + 1; k < ND; k++) w -= Lj[(size_t)k * ND + i] * x[(size_t)k]; x[(size_t)i] = w / Lj[(size_t)i * ND + i]; }
      };
      std::vector<std::vector<float>> Y(6, std::vector<float>(ND));
      for (int a = 0; a < 6; a++) { for (int f = 0; f < ND; f++) Y[(size_t)a][(size_t)f] = (float)Md[(size_t)(6 + f) * 108 + a]; solve(Y[(size_t)a]); }
      // the kernel's root order is (angular, linear); the order does not matter for G as long as it is one order throughout
      float S[6][6], id[6];
      for (int a = 0; a < 6; a++) for (int b = 0; b <= a; b++) {
        float p = 0.f;
        for (int f = 0; f < ND; f++) p += (float)Md[(size_t)a * 108 + 6 + f] * Y[(size_t)b][(size_t)f];
        S[a][b] = (float)Md[(size_t)a * 108 + b] - p;
      }
      for (int j = 0; j < 6; j++) {
        float d = S[j][j];
        for (int k = 0; k < j; k++) d -= S[j][k] * S[j][k];
        if (!(d > 0.f)) throw std::runtime_error("S_m is not positive definite in float32");
        id[j] = 1.f / std::sqrt(d);
        S[j][j] = d * id[j];
        for (int i = j + 1; i < 6; i++) { float e = S[i][j]; for (int k = 0; k < j; k++) e -= S[i][k] * S[j][k]; S[i][j] = e * id[j]; }
      }
      std::vector<std::vector<float>> col((size_t)n, std::vector<float>(ND, 0.f));
      std::vector<float> u((size_t)n * 6);
      for (int r = 0; r < n; r++) {
        col[(size_t)r][(size_t)rf[(size_t)r]] = 1.f;
        solve(col[(size_t)r]);
        for (int i = 0; i < 6; i++) {  // u = s L^-1 Y_m[f]
          float w = rs[(size_t)r] * Y[(size_t)i][(size_t)rf[(size_t)r]];
          for (int k = 0; k < i; k++) w -= S[i][k] * u[(size_t)r * 6 + (size_t)k];
          u[(size_t)r * 6 + (size_t)i] = w * id[i];
        }
      }
      double gmax = 0, emax = 0;
      for (int i = 0; i < n; i++) for (int k = 0; k < n; k++) {
        float g = rs[(size_t)i] * rs[(size_t)k] * col[(size_t)k][(size_t)rf[(size_t)i]];
        for (int a = 0; a < 6; a++) g += u[(size_t)i * 6 + (size_t)a] * u[(size_t)k * 6 + (size_t)a];
        gmax = std::fmax(gmax, std::fabs(Gref[(size_t)i * (size_t)n + (size_t)k]));
        emax = std::fmax(emax, std::fabs((double)g - Gref[(size_t)i * (size_t)n + (size_t)k]));
      }
      if (n) g_err = std::fmax(g_err, emax / gmax);
    }
    std::printf("states %d\nrows %d\nmost_rows %d\nrows_match %d\nd_rel_err %.3e\ng_rel_err %.3e\n", nstates, rows_total, most, rows_match, d_err, g_err);
  } catch (const std::exception &e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
  return 0;
}
