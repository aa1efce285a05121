// row_newton.hpp - the constraint solve both fly step kernels run: the dual Newton in the space of the constraint rows (mj:
// mj_fwdConstraint restated), lane = row, with what only the solver uses (the elliptic-cone force law, the noslip QCQP, the solver
// constants).  Written once, instantiated per translation unit with the caller's tile type and one of the two policies below:
//   ball_env.hip  ConeRows:   3-row elliptic-cone contact blocks on lanes < nrc, scalar limit rows after them, warm start from
//                             T.r_lam, noslip sweeps on the same G (walk_on_ball);
//   walk_env.hip  ScalarRows: scalar limit rows only, from lambda = 0 (walk_imitation's joint limits).
// A policy is compile time only: what the scalar solve does not need (the wave shifts inside a contact block, the block factor of
// W, the cone tables of the tile, the noslip sweep, r_lam) is discarded, not branched around, so a tile without those members
// compiles.  The tile provides G, r_y0, r_D, r_f and S, the floats the factor is transposed through (they may be G's own: kSyncAfterLoad).
// The ConeRows instantiations must compile to the instructions the tethered kernel had when the solver lived in ball_env.hip (DESIGN.md
// section 12 has the comparison): statements that look interchangeable are not - declaring the shifted factor entries of the S build
// as variables assigned under `if constexpr`, instead of the constant ternaries below, reordered the line search's phi nodes and with
// them 540 lines of the disassembly.
#pragma once
#include <hip/hip_runtime.h>

#include "ball_model.hpp"
#include "dev_math.hpp"

namespace ffb {
using namespace dm;

constexpr float kNewtonTol2 = 1e-8f;  // stop when |grad| <= 1e-4 |force scale| (M^-1 metric; 1e-7 costs 4x in parity for 1% speed)
constexpr int kLsIter = 10;
constexpr float kLsTol = 1e-2f;  // |phi'(alpha)| <= tol |phi'(0)|: an inexact line search, the Newton loop converges the rest

struct ConeRows {
  static constexpr bool kCones = true;          // contact blocks (cone force law, block factor of W) and the noslip sweep
  static constexpr bool kWarmStart = true;      // lambda from / to T.r_lam; the first iteration is only tested when `have_ws`
  static constexpr bool kSyncAfterLoad = false;
  static constexpr int kMaxNewton = 12;
  static constexpr bool kRevertByResidual = false;  // the noslip sweep's revert test: see ConeRowsResidual
};
// ConeRows with the noslip sweep's revert test scaled by what its rounding error scales with.  mj's costChange reverts an update whose
// cost change is positive (a failed QCQP).  The change is d . res + d' A d / 2 with d the difference of two forces of size |f|, known
// to ~1e-7 |f| in float32, so its error is ~1e-7 |res| |f| whatever the size of the change itself.  ConeRows' threshold, 1e-4 of
// (|d . res| + |d' A d / 2|), is below that error once a sweep's genuine gain is small: on a sliding contact of the free-root fly the
// third sweep then reverts or not by rounding (walk_self_env.hip, R10 state 8: 3e-4 ... 8e-4 rad/s of root angular velocity).  Here the
// threshold is 1e-5 (|res_1| + |res_2|) (|new| + |old|): a hundred times the error, and four orders below the change of a QCQP
// that fails and returns zero.  A policy of its own so that the instantiations of ConeRows compile to the instructions they had.
struct ConeRowsResidual : ConeRows {
  static constexpr bool kRevertByResidual = true;
};
struct ScalarRows {
  static constexpr bool kCones = false;
  static constexpr bool kWarmStart = false;     // a limit row comes and goes with its hinge: from lambda = 0, every iteration tested
  static constexpr bool kSyncAfterLoad = true;  // the scratch is G's own floats: they carry the factor's transpose once G sits in registers
  static constexpr int kMaxNewton = 20;
};

// mj: PrimalUpdateConstraint for one elliptic condim-3 contact.  With U = mu (jar_n, jar_t1, jar_t2), N = U0, T = |U_t|:
// zero force in the top zone N >= mu T, fully quadratic in the bottom zone mu N + T <= 0, and the cone-surface cost
// Dm/2 (N - mu T)^2, Dm = D / (mu^2 (1 + mu^2)), in between.  Hc (optional) is the 3x3 Hessian of that cost in jar.
__device__ __forceinline__ void cone_force(float D, float mu, float j0, float j1, float j2, float &f0, float &f1, float &f2, float *Hc) {
  const float N = j0 * mu, U1 = j1 * mu, U2 = j2 * mu, Tn = fsqrt(U1 * U1 + U2 * U2);
  if (Hc) for (int k = 0; k < 9; k++) Hc[k] = 0.f;
  if (N >= mu * Tn || (Tn <= 0.f && N >= 0.f)) { f0 = f1 = f2 = 0.f; return; }
  if (mu * N + Tn <= 0.f || (Tn <= 0.f && N < 0.f)) {
    f0 = -D * j0; f1 = -D * j1; f2 = -D * j2;
    if (Hc) { Hc[0] = D; Hc[4] = D; Hc[8] = D; }
    return;
  }
  const float Dm = D * frcp(fmaxf(1e-15f, mu * mu * (1.f + mu * mu))), NT = N - mu * Tn, iT = frcp(Tn);
  f0 = -Dm * NT * mu;
  f1 = -f0 * iT * U1 * mu;
  f2 = -f0 * iT * U2 * mu;
  if (Hc) {
    const float a = mu * N * iT * iT * iT, bd = mu * mu - mu * N * iT, s2 = Dm * mu * mu;
    Hc[0] = s2;
    Hc[1] = Hc[3] = s2 * (-mu * U1 * iT);
    Hc[2] = Hc[6] = s2 * (-mu * U2 * iT);
    Hc[4] = s2 * (a * U1 * U1 + bd);
    Hc[8] = s2 * (a * U2 * U2 + bd);
    Hc[5] = Hc[7] = s2 * (a * U1 * U2);
  }
}

// mj: mju_QCQP2 with equal friction coefficients d: min 1/2 x'Ax + x'b, |x| <= d r (root finding differs, see below)
__device__ __forceinline__ bool qcqp2(float &x0, float &x1, float A00, float A01, float A11, float b0, float b1, float d, float r) {
  const float B0 = b0 * d, B1 = b1 * d, P00 = A00 * d * d, P01 = A01 * d * d, P11 = A11 * d * d, r2 = r * r;
  float la = 0.f, v0 = 0.f, v1 = 0.f;
  bool active = false;
  for (int it = 0; it < 20; it++) {
    const float det = (P00 + la) * (P11 + la) - P01 * P01;
    if (det < 1e-10f) { x0 = x1 = 0.f; return false; }
    const float idet = frcp(det), i00 = (P11 + la) * idet, i11 = (P00 + la) * idet, i01 = -P01 * idet;
    v0 = -i00 * B0 - i01 * B1; v1 = -i01 * B0 - i11 * B1;
    const float q = v0 * v0 + v1 * v1, val = q - r2;
    if (val < 1e-10f) break;
    const float deriv = -2.f * (i00 * v0 * v0 + i11 * v1 * v1 + 2.f * i01 * v0 * v1);
    // Newton on 1/r - 1/|v(la)| (nearly linear in la) instead of mju_QCQP2's Newton on |v|^2 - r^2: same root, same stopping
    // tests, monotone from the left as well, 3.4 instead of 5.5 iterations on the sliding contacts of this task
    const float delta = -2.f * q * (fsqrt(q) - r) * frcp(r * deriv);
    if (delta < 1e-10f) break;
    la += delta;
    active = true;
  }
  x0 = v0 * d; x1 = v1 * d;
  return active;
}

// Dense Newton of the constraint solve on R <= RB rows (RB picked per substep by the caller): lane = row, everything in
// registers - the lane's row of G and of S = I + L' G L, other lanes' scalars by v_readlane (uniform index), neighbours'
// by wave shifts.  Loops are fully unrolled over RB so that the register arrays keep static indices.
// With y = y0 + G lambda and the force law f(y) (cone_force on a contact's three rows, -D min(0, y) on a scalar row) the Newton step
// is d = -(I + W G)^-1 (lambda - f), W = df/dy = L L' (block lower triangular; diagonal on scalar rows), solved as d = -e + L u,
// (I + L' G L) u = L' G e, followed by an exact line search on the convex piecewise-quadratic cost.
// Reads T.G, T.r_y0, T.r_D (ConeRows: T.r_lam, T.c_excl / c_D / c_mu of the nrc / 3 contacts, Mp->meaninertia for the `nslip` noslip
// sweeps); leaves the forces in T.r_f (ConeRows: lambda in T.r_lam).  ScalarRows ignores Mp, nrc, nslip and have_ws.  Returns the
// iterations taken.
// A real call (not inlined) and a leaf: the iteration loop then has the whole register file to itself - inlined, the allocator
// kept the caller's ~90 live values resident and spilled 120-200 of the loop's own values per iteration instead.
template <int RB, class P, class Tile>
__device__ __noinline__ int row_newton(Tile *Tp, const BallModel FFE_GLOBAL *Mp, const int lane, const int R, const int nrc, const float scale2,
                                       const int nslip, const int have_ws) {
  Tile &T = *Tp;
  int iters = 0;
  // The row arrays are kept as float pairs so that the broadcast-multiply-accumulate loops (products with G, the Cholesky
  // updates) issue as v_pk_fma_f32 with the two v_readlane results as an SGPR pair: 3 instructions per 2 columns, not 4.
  f2 Gp[RB / 2], Sp[RB / 2];
  auto G_ = [&](int j) -> float { return (j & 1) ? Gp[j >> 1].y : Gp[j >> 1].x; };
  auto S_ = [&](int j) -> float { return (j & 1) ? Sp[j >> 1].y : Sp[j >> 1].x; };
  auto setS = [&](int j, float v) { if (j & 1) Sp[j >> 1].y = v; else Sp[j >> 1].x = v; };
  auto gload = [&](int j) -> float { return (lane < R && j < R) ? T.G[j <= lane ? lane * (lane + 1) / 2 + j : j * (j + 1) / 2 + lane] : 0.f; };
#pragma unroll
  for (int m = 0; m < RB / 2; m++) Gp[m] = f2{gload(2 * m), gload(2 * m + 1)};
  float lam = 0.f;
  if constexpr (P::kWarmStart) lam = lane < R ? T.r_lam[lane] : 0.f;
  const float y0v = lane < R ? T.r_y0[lane] : 0.f;
  float D = 0.f;  // scalar rows alone keep their D in a register (a contact block reads its tables where it evaluates)
  if constexpr (!P::kCones) D = lane < R ? T.r_D[lane] : 0.f;
  if constexpr (P::kSyncAfterLoad) DM_SYNC();
  const bool crow = P::kCones && lane < nrc;  // contact row (else limit row or idle lane)
  const int sub = crow ? lane % 3 : 0;        // position inside the contact's 3-row block
  auto gdot = [&](float vreg) {               // (G v)[lane], v given as one value per lane
    f2 acc = f2{0.f, 0.f};
#pragma unroll
    for (int m = 0; m < RB / 2; m++) acc = __builtin_elementwise_fma(Gp[m], f2{rl_f(vreg, 2 * m), rl_f(vreg, 2 * m + 1)}, acc);  // G = 0 beyond the R live rows
    return acc.x + acc.y;
  };
  float fv = 0.f, yv = 0.f;
  float L0 = 0.f, L1 = 0.f, L2 = 0.f;  // this row of the block-lower Cholesky factor of W: L[row][first .. first+2]
  auto eval = [&](float y, bool want_L) {
    if constexpr (!P::kCones) {
      if (want_L) L0 = (y < 0.f && D > 0.f) ? fsqrt(D) : 0.f;
      return y < 0.f ? -D * y : 0.f;
    } else {
      // a contact's three rows are evaluated on all three lanes (the residuals come by shifts inside the block)
      // (by DPP wave shifts: no LDS round trip in the line search's inner evaluation)
      const float u1 = wshl1(y), u2 = wshl1(u1), d1 = wshr1(y), d2 = wshr1(d1);
      const float ya = sub == 0 ? y : (sub == 1 ? d1 : d2), yb = sub == 0 ? u1 : (sub == 1 ? y : d1), yc = sub == 0 ? u2 : (sub == 1 ? u1 : y);
      float f = 0.f;
      if (want_L) L0 = L1 = L2 = 0.f;
      if (crow) {
        const int k = lane / 3;
        float f0 = 0.f, f1 = 0.f, f2 = 0.f, Hc[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (!T.c_excl[k]) cone_force(T.c_D[k], T.c_mu[k], ya, yb, yc, f0, f1, f2, want_L ? Hc : nullptr);
        f = sub == 0 ? f0 : (sub == 1 ? f1 : f2);
        if (want_L) {  // Hc = L L' (positive semi-definite: a vanishing pivot zeroes its column)
          const float l00 = Hc[0] > 1e-30f ? fsqrt(Hc[0]) : 0.f, i00 = l00 > 0.f ? frcp(l00) : 0.f;
          const float l10 = Hc[3] * i00, l20 = Hc[6] * i00;
          const float d1 = Hc[4] - l10 * l10, l11 = d1 > 1e-7f * Hc[4] ? fsqrt(d1) : 0.f, i11 = l11 > 0.f ? frcp(l11) : 0.f;
          const float l21 = (Hc[7] - l20 * l10) * i11;
          const float d2 = Hc[8] - l20 * l20 - l21 * l21, l22 = d2 > 1e-7f * Hc[8] ? fsqrt(d2) : 0.f;
          if (sub == 0) { L0 = l00; } else if (sub == 1) { L0 = l10; L1 = l11; } else { L0 = l20; L1 = l21; L2 = l22; }
        }
      } else if (lane < R) {
        const float D = T.r_D[lane];
        f = y < 0.f ? -D * y : 0.f;
        if (want_L) L0 = y < 0.f ? fsqrt(D) : 0.f;
      }
      return f;
    }
  };
  bool fresh = false;  // yv, fv belong to the current lam
  yv = y0v;
  if constexpr (P::kWarmStart) yv = y0v + gdot(lam);
#pragma unroll 1
  for (int it = 0; it < P::kMaxNewton; it++) {
    fresh = true;
    fv = eval(yv, true);
    const float ev = lam - fv;
    const float pv = gdot(ev);
    const float gn2 = wave_sum(lane < R ? pv * ev : 0.f);
    if ((!P::kWarmStart || it > 0 || have_ws) && gn2 <= kNewtonTol2 * scale2 + 1e-30f) break;
    iters++;
    // S = I + L' G L.  Column j: t_j = (G L)[lane][j] from this lane's G row and L's column j (read from the owning lanes),
    // then S[i][j] = delta_ij + sum over the rows a >= i of i's block of L[a][i] t_j(a) (neighbour lanes, shifted in).
    // wshl1(x): lane i takes lane i + 1's x (DPP wave shift: no LDS round trip, unlike a bpermute)
    // Scalar rows: L is diagonal, S = I + L G L.
    const bool has1 = crow && sub < 2, has2 = crow && sub == 0;
    // (shifts are whole-wave operations: taken unconditionally, selected afterwards)
    const float Ls1 = P::kCones ? wshl1(sub == 1 ? L0 : (sub == 2 ? L1 : 0.f)) : 0.f, Ls2 = P::kCones ? wshl1(wshl1(L0)) : 0.f;
    const float La1 = has1 ? Ls1 : 0.f;  // L[lane+1][lane] (the source lane picks its entry one column left of its diagonal)
    const float La2 = has2 ? Ls2 : 0.f;  // L[lane+2][lane] (only for sub == 0)
    const float Ld = sub == 0 ? L0 : (sub == 1 ? L1 : L2);                         // L[lane][lane]
#pragma unroll
    for (int j = 0; j < RB; j++) {
      if (j < R) {
        if constexpr (P::kCones) {
          float tj;
          if (j < nrc) {
            const int fj = j - j % 3, sj = j % 3;
            // L[fj + b][j] for b = sj .. 2: lane fj+b holds it at position sj
            tj = G_(j) * rl_f(sj == 0 ? L0 : (sj == 1 ? L1 : L2), j);
            if (sj < 2) tj += G_(fj + sj + 1 < RB ? fj + sj + 1 : 0) * rl_f(sj == 0 ? L0 : L1, fj + sj + 1 < RB ? fj + sj + 1 : 0);
            if (sj < 1) tj += G_(fj + 2 < RB ? fj + 2 : 0) * rl_f(L0, fj + 2 < RB ? fj + 2 : 0);
          } else tj = G_(j) * rl_f(L0, j);
          const float t1 = wshl1(tj), t2 = wshl1(t1);
          setS(j, (j == lane ? 1.f : 0.f) + Ld * tj + La1 * t1 + La2 * t2);
        } else setS(j, (j == lane ? 1.f : 0.f) + Ld * G_(j) * rl_f(Ld, j));
      } else setS(j, j == lane ? 1.f : 0.f);
    }
    // rhs = L' p
    float w;
    if constexpr (P::kCones) {
      const float p1 = wshl1(pv), p2 = wshl1(p1);
      w = Ld * pv + La1 * p1 + La2 * p2;
    } else w = Ld * pv;
    // Cholesky of S (row per lane) as S = Lt D Lt', Lt unit lower triangular: S_(k) ends as Lt[lane][k] below the diagonal and 0
    // on and above it, so that the substitutions are one unconditional FMA per step; ipp = 1 / D[lane]
    float ipp = 1.f;
#pragma unroll
    for (int k = 0; k < RB; k++) {
      if (k < R) {
        const float ip = __builtin_amdgcn_rsqf(rl_f(S_(k), k));
        const float lik = S_(k) * ip;
        if ((k & 1) == 0) Sp[k >> 1].y -= lik * rl_f(lik, k + 1);  // the pair partner of an even pivot column
        const f2 nl = f2{-lik, -lik};
#pragma unroll
        for (int m = (k >> 1) + 1; m < RB / 2; m++)  // rows / columns beyond R are identity: no-ops
          Sp[m] = __builtin_elementwise_fma(nl, f2{rl_f(lik, 2 * m), rl_f(lik, 2 * m + 1)}, Sp[m]);
        setS(k, lane > k ? lik * ip : 0.f);
        ipp = lane == k ? ip * ip : ipp;
      }
    }
    // forward substitution Lt z = w
#pragma unroll
    for (int k = 0; k < RB; k++)
      if (k < R) w -= S_(k) * rl_f(w, k);
    w *= ipp;
    // transpose through LDS (this lane's column of Lt), then backward substitution Lt' u = D^-1 z
    // (only the strict lower triangle is non-zero: packed by rows, row i at i (i - 1) / 2)
    if (lane < R) {
      const int tri = lane * (lane - 1) / 2;
#pragma unroll
      for (int j = 0; j < RB; j++) if (j < lane) T.S[tri + j] = S_(j);
    }
    DM_SYNC();
#pragma unroll
    for (int m = 0; m < RB / 2; m++) Sp[m] = f2{0.f, 0.f};
    if (lane < R) {
#pragma unroll
      for (int k = 0; k < RB; k++) if (k < R && k > lane) setS(k, T.S[k * (k - 1) / 2 + lane]);
    }
    DM_SYNC();
#pragma unroll
    for (int k = RB - 1; k >= 0; k--)
      if (k < R) w -= S_(k) * rl_f(w, k);
    // d = -e + L u, jd = G d
    float dl;
    if constexpr (P::kCones) {
      const float u1 = wshr1(w), u2 = wshr1(u1);
      dl = -ev + Ld * w + (crow && sub >= 1 ? (sub == 1 ? L0 : L1) : 0.f) * u1 + (crow && sub == 2 ? L0 : 0.f) * u2;
      if (lane >= R) dl = 0.f;
    } else dl = lane < R ? -ev + Ld * w : 0.f;
    const float jdv = gdot(dl);
    const float c1s = wave_sum(lane < R ? dl * jdv : 0.f);
    const float d0 = wave_sum(lane < R ? ev * jdv : 0.f);  // phi'(0) = (lambda - f(y)) . G d: the forces at y are already known
    // exact line search on the convex phi(alpha): root of phi'(alpha) = phi'(0) + alpha c1 - sum_rows (f(y + alpha jd) - f(y)) jd
    auto dphi = [&](float al) {
      const float fa = eval(yv + al * jdv, false);
      float acc = lane < R ? (fv - fa) * jdv : 0.f;
      return d0 + al * c1s + wave_sum(acc);
    };
    float alpha = 0.f;
    {
      if (!(d0 < 0.f)) break;  // not a descent direction any more: converged to rounding
      float lo = 0.f, hi = 1.f, dlo = d0, dhi = dphi(1.f);
      int guard = 0;
      while (dhi < 0.f && fabsf(dhi) > kLsTol * fabsf(d0) && guard++ < 8) { lo = hi; dlo = dhi; hi *= 2.f; dhi = dphi(hi); }
      if (dhi < 0.f || fabsf(dhi) <= kLsTol * fabsf(d0)) alpha = hi;  // full (or doubled) Newton step: |phi'| already small
      else {
#pragma unroll 1
        for (int ls = 0; ls < kLsIter; ls++) {
          float mid = lo - dlo * (hi - lo) / (dhi - dlo);
          if (!(mid > lo + 0.05f * (hi - lo)) || !(mid < hi - 0.05f * (hi - lo))) mid = 0.5f * (lo + hi);
          const float dm_ = dphi(mid);
          if (dm_ < 0.f) { lo = mid; dlo = dm_; } else { hi = mid; dhi = dm_; }
          if (fabsf(dm_) <= kLsTol * fabsf(d0) || hi - lo <= 1e-6f * hi) break;
        }
        alpha = (dhi - dlo) != 0.f ? lo - dlo * (hi - lo) / (dhi - dlo) : hi;
        if (!(alpha >= lo) || !(alpha <= hi)) alpha = 0.5f * (lo + hi);
      }
    }
    lam += alpha * dl;
    yv += alpha * jdv;  // y = y0 + G lambda stays current without another product
    fresh = false;
  }
  // forces at the solution
  if (!fresh) fv = eval(yv, false);
  // ---- mj: mj_solNoSlip (ref: fruitfly.xml:4 noslip_iterations="3"): Gauss-Seidel on the tangential rows with the
  //      unregularised A = J M^-1 J' - which is G - normal and limit forces held fixed; res = G f + (J a_s - aref).
  //      G is symmetric, so row r of G against f is a wave sum over the lanes' column-r entries.
  if constexpr (P::kCones) {
    if (nslip > 0) {
      const BallModel FFE_GLOBAL &M = *Mp;
      const float scale = 1.f / (M.meaninertia * 105.f);
      const int nc = nrc / 3;
      float res = y0v + gdot(fv);  // residual row per lane, kept current as the tangential forces move (G is symmetric)
      for (int iter = 0; iter < nslip; iter++) {
        float improvement = 0.f;
#pragma unroll
        for (int k = 0; k < NC; k++) {
          if (3 * k + 2 < RB && k < nc && !T.c_excl[k]) {
            const int r0 = 3 * k + 1, r1 = 3 * k + 2;
            const float res0 = rl_f(res, r0), res1 = rl_f(res, r1);
            const float o0 = rl_f(fv, r0), o1 = rl_f(fv, r1), fn = rl_f(fv, 3 * k);
            const float A00 = rl_f(G_(r0), r0), A01 = rl_f(G_(r1), r0), A11 = rl_f(G_(r1), r1);
            float v0 = 0.f, v1 = 0.f;
            if (fn >= 1e-15f) {
              const float b0 = res0 - A00 * o0 - A01 * o1, b1 = res1 - A01 * o0 - A11 * o1, mu = T.c_mu[k];
              const bool active = qcqp2(v0, v1, A00, A01, A11, b0, b1, mu, fn);
              if (active) {
                const float ssum = (v0 * v0 + v1 * v1) * frcp(mu * mu);
                const float sc2 = fn * __builtin_amdgcn_rsqf(fmaxf(1e-15f, ssum));
                v0 *= sc2; v1 *= sc2;
              }
            }
            float d0 = v0 - o0, d1 = v1 - o1;
            // mj: costChange reverts an update whose cost change is > 1e-10 (a failed QCQP).  In float32 the two terms below
            // cancel to ~1e-7 of their size, so the threshold is taken relative to them; a genuine failure is far above it.
            const float lin_ = d0 * res0 + d1 * res1, quad_ = 0.5f * (d0 * (A00 * d0 + A01 * d1) + d1 * (A01 * d0 + A11 * d1));
            float change = lin_ + quad_;
            if (change > 1e-10f + (P::kRevertByResidual ? 1e-5f * (fabsf(res0) + fabsf(res1)) * (fabsf(v0) + fabsf(v1) + fabsf(o0) + fabsf(o1))
                                                        : 1e-4f * (fabsf(lin_) + fabsf(quad_)))) { v0 = o0; v1 = o1; d0 = d1 = 0.f; change = 0.f; }
            improvement -= fminf(change, 0.f);
            fv = lane == r0 ? v0 : (lane == r1 ? v1 : fv);
            res += G_(r0) * d0 + G_(r1) * d1;
          }
        }
        if (improvement * scale < 1e-6f) break;
      }
    }
  }
  if (lane < R) {
    if constexpr (P::kWarmStart) T.r_lam[lane] = lam;
    T.r_f[lane] = fv;
  }
  DM_SYNC();
  return iters;
}

}  // namespace ffb
