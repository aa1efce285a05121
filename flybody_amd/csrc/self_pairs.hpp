// self_pairs.hpp - the fly's own collision passes, once for the tethered fly on the ball (ball_env.hip) and the free-root walker
// (walk_substeps.hpp; DESIGN.md section 11 "One pair of collision passes").  `prim_pairs` is mj_collision over the sphere / capsule pairs,
// `convex_pairs` over the pairs with an ellipsoid or a cylinder on one side.  Each instantiation is a `__noinline__` leaf function with no
// call inside, which its kernel calls as it is (a `__forceinline__` body inside a per-kernel wrapper is simplified on its own before it is
// inlined and compiled to other code than the functions these replace; hooks inlined into the leaf are not).  A kernel's tile and its
// differences come in through a policy P, statics but for `fill_slots`:
//   p.fill_slots(T, lane) what only this kernel does before prim_pairs: the walker makes the slots from its link poses and synchronises
//   fill_centres(T, M, lane)
//                         likewise before convex_pairs: the walker makes the geom centres
//   slots(T)              the primitive geom slots, float4[NPG] (centre | bounding radius) then float4[NPG] (axis | half length)
//   radii(T)              float[NPG], the slots' radii
//   centres(T)            float4[NG], (centre | bounding radius) of every fly geom
//   quat(T, M, g)         orientation of fly geom g
//   cl1(T), cl2(T)        the pair lists of the convex pass, unsigned short[CL1] / [CL2]
//   put(T, M, at, l1, l2, pid, n, p, dist, margin, invw)
//                         stores contact slot `at`: geom1 on link l1, geom2 on link l2 (-1: the thorax, convex pass only), pair id, normal
//                         from geom1 to geom2, position, distance, margin, the two bodies' inverse weights
//   kSyncAtEnd            prim_pairs ends on a DM_SYNC()
//   kHistory              convex_pairs remembers each pair's separating direction from substep to substep in T.sd_* (through T.tc_* and
//                         T.cl2n), tests it before the narrow phase and starts the narrow phase from it; without, every substep starts cold
//   kFullBit              bit of convex_pairs' return word that reports a full pair list: 8 (with the contact overflow) or 9 (apart)
#pragma once
#include <hip/hip_runtime.h>

#include "ball_model.hpp"
#include "convex.hpp"
#include "dev_math.hpp"
#include "leg_dyn.hpp"

namespace ffb {
using namespace dm;

// mj: mj_collision over the fly's own sphere / capsule pairs (mjc_CapsuleCapsule), condim 1.  Broad phase = MuJoCo's bounding-sphere test: lane s owns slot s
// and meets slots s + 1 .. s + NPG / 2 (mod NPG), every unordered pair once.  A detected contact (dist <= margin) takes the next free
// slot after the `nprev` contacts stored so far; beyond NC the env is flagged and the deepest fly-fly contacts are kept.  Returns contacts
// stored | overflow << 8 | detected contacts without a slot << 16.
template <class P, class Tile>
__device__ __noinline__ int prim_pairs(Tile *Tp, ModelPtr Mp, const P p, const int lane, const int nprev) {
  Tile &T = *Tp;
  const BallModel FFE_GLOBAL &M = *Mp;
  const float4 *pgc = P::slots(T), *pga = pgc + NPG;
  const float *pgr = P::radii(T);
  const bool own = lane < NPG;
  p.fill_slots(T, lane);
  const float mclaw = M.sc_margin;
  const unsigned long long claws = M.sp_claw;
  const int sphere = M.sp_sphere;
  const unsigned long long partners = own ? M.sp_mask[lane] : 0ull;
  const float4 o0 = own ? pgc[lane] : make_float4(0.f, 0.f, 0.f, 0.f);
  const float oreach = o0.w + (((claws >> lane) & 1ull) ? mclaw : 0.f);
  unsigned near = 0u;  // bit t - 1: the pair (lane, lane + t) passed the bounding-sphere test
#pragma unroll 4
  for (int t = 1; t <= NPG / 2; t++) {
    int j = lane + t;
    j = j >= NPG ? j - NPG : j;
    if (own && ((partners >> j) & 1ull) && (t < NPG / 2 || lane < NPG / 2)) {
      const float4 p0 = pgc[j];
      const float dx = p0.x - o0.x, dy = p0.y - o0.y, dz = p0.z - o0.z;
      const float reach = oreach + p0.w + mclaw;  // (the claw margin on both sides: a bound is all that is needed here)
      if (dx * dx + dy * dy + dz * dz <= reach * reach) near |= 1u << (t - 1);
    }
  }
  int nsc = 0, ovf = 0, ndrop = 0;
#pragma unroll 1
  while (__ballot(near != 0u) != 0ull) {
    bool hit = false;
    float dist = 0.f, margin = 0.f;
    V3 nrm = {1.f, 0.f, 0.f}, cpos = {0.f, 0.f, 0.f};
    int s1 = 0, s2 = 0;
    if (near) {
      const int t = __ffs(near);
      near &= near - 1u;
      int j = lane + t;
      j = j >= NPG ? j - NPG : j;
      // mj: geom1 is the one with the lower type code (the sphere), else the one that comes first in the model
      const bool swap = j == sphere || (lane != sphere && j < lane);
      s1 = swap ? j : lane; s2 = swap ? lane : j;
      const float4 ca = pgc[s1], aa = pga[s1], cb_ = pgc[s2], ab = pga[s2];
      const V3 p1 = {ca.x, ca.y, ca.z}, a1 = {aa.x, aa.y, aa.z}, p2 = {cb_.x, cb_.y, cb_.z}, a2 = {ab.x, ab.y, ab.z};
      const float l1 = aa.w, r1 = pgr[s1], l2 = ab.w, r2 = pgr[s2];
      margin = (((claws >> s1) | (claws >> s2)) & 1ull) ? mclaw : 0.f;
      // mj: mjc_CapsuleCapsule, closest points of the two segments (centre p, unit axis a, half length l, radius r), one contact; a sphere
      // is a capsule of zero length, for which the same formulas reduce to mjc_SphereCapsule / mjraw_SphereSphere
      const V3 dif = p1 - p2;
      const float mb = -dot(a1, a2), u = -dot(a1, dif), v = dot(a2, dif), det = 1.f - mb * mb;
      float x1, x2;
      if (fabsf(det) >= 1e-6f) {
        const float idet = 1.f / det;
        x1 = (u - mb * v) * idet; x2 = (v - mb * u) * idet;
        if (x1 > l1) { x1 = l1; x2 = v - mb * l1; } else if (x1 < -l1) { x1 = -l1; x2 = v + mb * l1; }
        if (x2 > l2) { x2 = l2; x1 = fminf(fmaxf(u - mb * l2, -l1), l1); }
        else if (x2 < -l2) { x2 = -l2; x1 = fminf(fmaxf(u + mb * l2, -l1), l1); }
      } else {  // parallel axes: centre of the overlapping stretch
        const float c2 = u, lo = fmaxf(-l1, c2 - l2), hi = fminf(l1, c2 + l2);
        x1 = lo <= hi ? 0.5f * (lo + hi) : (c2 > 0.f ? l1 : -l1);
        x2 = fminf(fmaxf((x1 - c2) * (mb < 0.f ? 1.f : -1.f), -l2), l2);
      }
      const V3 q1 = p1 + x1 * a1, q2 = p2 + x2 * a2, d12 = q2 - q1;
      const float cd = fsqrt(dot(d12, d12));
      hit = cd <= margin + r1 + r2;
      if (cd >= 1e-15f) nrm = frcp(cd) * d12;
      dist = cd - r1 - r2;
      cpos = q1 + (r1 + 0.5f * dist) * nrm;
    }
    // A contact inside its margin but outside margin - gap exerts no force; it only matters as one of the contacts an adhesion
    // actuator spreads its pull over (mjTRN_BODY).  Without such an actuator on either link it gets no slot (and no solver row);
    // it is still counted (ndrop) so that the number of detected contacts stays MuJoCo's.
    const bool dropped = hit && dist >= margin - (margin != 0.f ? M.sc_gap : 0.f) && M.l_adh[M.pgs_link[s1]] < 0 && M.l_adh[M.pgs_link[s2]] < 0;
    hit = hit && !dropped;
    ndrop += __popcll(__ballot(dropped));
    const unsigned long long bal = __ballot(hit);
    if (bal) {
      const int idx = nprev + nsc + __popcll(bal & ((1ull << lane) - 1ull));
      auto store = [&](int at) {
        P::put(T, M, at, M.pgs_link[s1], M.pgs_link[s2], 0x8000 | s1 | (s2 << 6), nrm, cpos, dist, margin, M.pgs_invw[s1] + M.pgs_invw[s2]);
      };
      if (hit && idx < NC) store(idx);
      const int n = __popcll(bal);
      const bool over = nprev + nsc + n > NC;
      nsc = min(nsc + n, NC - nprev);
      if (over && nprev < NC) {
        // More contacts than the tile holds: the env is flagged, and a hit without a slot takes the place of the shallowest fly-fly
        // contact held so far if it is deeper (as for the ball contacts and the convex pairs: a deep contact is never the one dropped).
        ovf = 1;
        DM_SYNC();
        for (unsigned long long left = __ballot(hit && idx >= NC); left; left &= left - 1) {
          const int j = __ffsll((long long)left) - 1;
          float shallow = -1e30f;
          int at = -1;
          for (int k = nprev; k < NC; k++) { const float dk = T.c_dist[k]; if (dk > shallow) { shallow = dk; at = k; } }
          if (__shfl(dist, j) < shallow) { if (lane == j) store(at); DM_SYNC(); }
        }
      } else if (over) ovf = 1;
    }
  }
  if constexpr (P::kSyncAtEnd) DM_SYNC();
  return nsc | (ovf << 8) | (ndrop << 16);
}

// fly geom g in the frame the tile's poses are in
template <class P, class Tile>
__device__ __forceinline__ cvx::Geom load_geom(const Tile &T, const BallModel FFE_GLOBAL &M, const int g) {
  const float4 cc = P::centres(T)[g];
  return cvx::Geom{V3{cc.x, cc.y, cc.z}, P::quat(T, M, g), M.cg_size[0][g], M.cg_size[1][g], M.cg_size[2][g], M.cg_type[g]};
}

// The fly's own convex pairs (mj: mjc_Convex, restated in convex.hpp).  Broad phase: MuJoCo's bounding-sphere test over the static
// candidate list (flybody_amd/model/reach.py), then - on the survivors - a rigorous lower bound of the distance from one separating
// direction (cvx::separation_bound); a pair whose bound exceeds its margin cannot touch.  Narrow phase: one lane per remaining pair
// (cvx::collide).  A contact (dist <= margin) takes the next free slot after the `nprev` contacts already stored; beyond NC the env is
// flagged and the deepest are kept.  Returns contacts stored | overflow << 8 | (a pair list was full: candidates were left out) <<
// P::kFullBit | detected contacts without a slot << 16.
template <class P, class Tile>
__device__ __noinline__ int convex_pairs(Tile *Tp, ModelPtr Mp, const int lane, const int nprev) {
  Tile &T = *Tp;
  const BallModel FFE_GLOBAL &M = *Mp;
  const float4 *gc = P::centres(T);
  unsigned short *cl1 = P::cl1(T), *cl2 = P::cl2(T);
  P::fill_centres(T, M, lane);
  const unsigned long long mm0 = M.cg_mmask[0], mm1 = M.cg_mmask[1];
  const float mclaw = M.sc_margin;
  auto pair_margin = [&](int a, int b) {
    const bool ma = a < 64 ? ((mm0 >> a) & 1ull) : ((mm1 >> (a - 64)) & 1ull), mb = b < 64 ? ((mm0 >> b) & 1ull) : ((mm1 >> (b - 64)) & 1ull);
    return (ma || mb) ? mclaw : 0.f;
  };
  auto no_adhesion = [&](int a, int b) {
    const int la_ = M.cg_link[a], lb_ = M.cg_link[b];
    return (la_ < 0 || M.l_adh[la_] < 0) && (lb_ < 0 || M.l_adh[lb_] < 0);
  };
  int n1 = 0, full = 0;
  const int ncp = M.ncp;
#pragma unroll 1
  for (int base = 0; base < ncp; base += 64) {
    const unsigned w = M.cp_pair[base + lane];
    bool pass = false;
    if (w != 0xffffu) {
      const int a = w & 255, b = w >> 8;
      const float4 ca = gc[a], cb = gc[b];
      const float dx = cb.x - ca.x, dy = cb.y - ca.y, dz = cb.z - ca.z, reach = ca.w + cb.w + pair_margin(a, b);
      pass = dx * dx + dy * dy + dz * dz <= reach * reach;
    }
    const unsigned long long bal = __ballot(pass);
    const int idx = n1 + __popcll(bal & ((1ull << lane) - 1ull));
    if (pass && idx < CL1) cl1[idx] = (unsigned short)w;
    n1 += __popcll(bal);
  }
  if (n1 > CL1) { n1 = CL1; full = 1; }
  DM_SYNC();
  // Second test: a separating direction proves the pair apart.  With kHistory, besides the two directions of cvx::separation_bound, the
  // one the narrow phase found for this pair on the last substep it ran (`sd_*`): pairs that stay near each other without touching (a hind
  // coxa beside the abdomen, stacked abdomen discs) then cost two support evaluations per substep instead of a narrow phase.
  int n2 = 0, nk = 0, ncache = 0;
  if constexpr (P::kHistory) ncache = T.sd_cnt;
#pragma unroll 1
  for (int base = 0; base < n1; base += 64) {
    bool pass = false, keep = false, have_kn = false;
    unsigned w = 0u;
    V3 kn = {0.f, 0.f, 0.f};
    float kt = 0.f;
    if (base + lane < n1) {
      w = cl1[base + lane];
      const int a = w & 255, b = w >> 8;
      // the distance that matters: the margin where an adhesion actuator shares its pull over every detected contact of its body,
      // margin - gap (a contact beyond it exerts no force and gets no slot) otherwise
      float thr = pair_margin(a, b);
      if (thr != 0.f && no_adhesion(a, b)) thr -= M.sc_gap;
      const cvx::Geom ga = load_geom<P>(T, M, a), gb = load_geom<P>(T, M, b);
      pass = cvx::separation_bound(ga, gb) <= thr;
      if constexpr (P::kHistory) {
        if (pass) {
          for (int k = 0; k < ncache; k++) {
            if (T.sd_pid[k] == w) {
              kn = V3{T.sd_n[k][0], T.sd_n[k][1], T.sd_n[k][2]};
              kt = T.sd_n[k][3];
              keep = -cvx::overlap(ga, gb, kn) > thr;
              have_kn = true;
            }
          }
          pass = !keep;
        }
      }
    }
    const unsigned long long bal = __ballot(pass);
    const int idx = n2 + __popcll(bal & ((1ull << lane) - 1ull));
    if (pass && idx < CL2) cl2[idx] = (unsigned short)w;
    n2 += __popcll(bal);
    if constexpr (P::kHistory) {
      const unsigned long long balk = __ballot(keep);
      const int idk = nk + __popcll(balk & ((1ull << lane) - 1ull));
      if (pass && idx < CL2) { float *o = T.cl2n[idx]; o[0] = kn.x; o[1] = kn.y; o[2] = kn.z; o[3] = have_kn ? 1.f : 0.f; o[4] = kt; }
      if (keep && idk < NSD) { T.tc_pid[idk] = (unsigned short)w; T.tc_n[idk][0] = kn.x; T.tc_n[idk][1] = kn.y; T.tc_n[idk][2] = kn.z; T.tc_n[idk][3] = kt; }
      nk = min(nk + __popcll(balk), NSD);
    }
  }
  if (n2 > CL2) { n2 = CL2; full = 1; }
  DM_SYNC();
  bool hit = false, dropped = false;
  float dist = 0.f, margin = 0.f;
  V3 nrm = {1.f, 0.f, 0.f}, cpos = {0.f, 0.f, 0.f};
  int a = 0, b = 0;
  if (lane < n2) {
    const unsigned w = cl2[lane];
    a = w & 255; b = w >> 8;
    margin = pair_margin(a, b);
    V3 n0 = {0.f, 0.f, 0.f};  // where the narrow phase starts: cold, or with kHistory from the pair's remembered direction
    bool have_n = false;
    float t0 = 0.f;
    if constexpr (P::kHistory) { const float *kn = T.cl2n[lane]; n0 = V3{kn[0], kn[1], kn[2]}; have_n = kn[3] != 0.f; t0 = kn[4]; }
    const cvx::Contact ct = cvx::collide(load_geom<P>(T, M, a), load_geom<P>(T, M, b), n0, have_n, t0);
    dist = ct.dist; nrm = ct.n; cpos = ct.pos;
    hit = dist <= margin;
    if (hit && dist >= margin - (margin != 0.f ? M.sc_gap : 0.f)) {  // (inactive and no adhesion actuator takes part: no slot, see prim_pairs)
      dropped = no_adhesion(a, b);
      hit = !dropped;
    }
    if constexpr (P::kHistory) {
      if (nk + lane < NSD) {  // its direction, for the next substep's second test
        T.tc_pid[nk + lane] = (unsigned short)w; T.tc_n[nk + lane][0] = nrm.x; T.tc_n[nk + lane][1] = nrm.y; T.tc_n[nk + lane][2] = nrm.z; T.tc_n[nk + lane][3] = ct.t;
      }
    }
  }
  if constexpr (P::kHistory) {
    nk = min(nk + n2, NSD);
    DM_SYNC();
    if (lane < nk) { T.sd_pid[lane] = T.tc_pid[lane]; T.sd_n[lane][0] = T.tc_n[lane][0]; T.sd_n[lane][1] = T.tc_n[lane][1]; T.sd_n[lane][2] = T.tc_n[lane][2]; T.sd_n[lane][3] = T.tc_n[lane][3]; }
    if (lane == 0) T.sd_cnt = nk;
  }
  unsigned long long bal = __ballot(hit);
  int ovf = 0;
  if (nprev + __popcll(bal) > NC) {  // more than the free slots: the env is flagged and the deepest are kept (as for the ball contacts)
    ovf = 1;
    int rank = 0;
    for (unsigned long long m = bal; m; m &= m - 1) {
      const int j = __ffsll((long long)m) - 1;
      const float dj = __shfl(dist, j);
      if (dj < dist || (dj == dist && j < lane)) rank++;
    }
    hit = hit && rank < NC - nprev;
    bal = __ballot(hit);
  }
  const int n = __popcll(bal), idx = nprev + __popcll(bal & ((1ull << lane) - 1ull));
  if (hit && idx < NC) P::put(T, M, idx, M.cg_link[a], M.cg_link[b], a | (b << 8), nrm, cpos, dist, margin, M.cg_invw[a] + M.cg_invw[b]);
  DM_SYNC();
  return n | (ovf << 8) | (full << P::kFullBit) | (__popcll(__ballot(dropped)) << 16);
}

}  // namespace ffb
