// leg_stage1.inc - the dynamics half of stage 1 of the fly step kernels, as a text fragment: it is included INSIDE the body of
// `template <class C> stage1(C &c)` of ball_env.hip (FREE_ROOT = false) and of walk_env.hip (FREE_ROOT = true), after
//   constexpr bool FREE_ROOT = ...;  auto &T = *c.T;  const BallModel FFE_GLOBAL &M = model(c);
// and leaves lane, parent, ndof, xmat, ximat ... in scope for what the kernel adds (the tethered kernel: collision).  A fragment and
// not a function on purpose: cut out as a function, the tethered kernel's locals end their lives at the cut, and the compiler then
// allocates the benchmarked kernel's registers differently (same instructions, other names); included as text, its device code is
// the one it had before the free-root kernel existed, byte for byte.  What FREE_ROOT adds is described in leg_dyn.hpp.
  const int lane = c.lane, parent = l_parent(c), ndof = l_ndof(c);
  const V3 c0 = {M.thorax_pos[0], M.thorax_pos[1], M.thorax_pos[2]};
  const V3 pos = {M.l_pos[0][lane], M.l_pos[1][lane], M.l_pos[2][lane]};
  const Q4 quat = {M.l_quat[0][lane], M.l_quat[1][lane], M.l_quat[2][lane], M.l_quat[3][lane]};
  V3 axis[3];
#pragma unroll
  for (int s = 0; s < 3; s++) axis[s] = {M.s_axis[0][s][lane], M.s_axis[1][s][lane], M.s_axis[2][s][lane]};
  // Every joint of this model sits at its body's origin (checked on the host), so a link's origin does not depend on
  // its own joint angles and everything that does not involve the parent is done once, before the tree pass:
  // the link's orientation relative to its parent after 0, 1, 2, 3 of its joints and the joint axes in the parent frame.
  Q4 qrel = quat;
  V3 axp[3];
#pragma unroll
  for (int s = 0; s < 3; s++) {
    axp[s] = qrot(qrel, axis[s]);
    if (s < ndof) {
      float sn, cs;
      fsincos(0.5f * c.q[s], &sn, &cs);
      qrel = qmul(qrel, Q4{cs, axis[s].x * sn, axis[s].y * sn, axis[s].z * sn});
    }
  }
  // ---- mj: mj_kinematics by pointer jumping instead of one sweep per tree level: after round r the pose (xp, xq) is
  //      relative to the frame above the link's 2^(r+1)-th ancestor; three rounds cover the deepest chain (8 links) with every
  //      lane at work in every round (a level sweep runs its body once per level with one level's lanes active).
  const unsigned tree = M.l_tree[lane];
  const int sub = (int)(tree & 0xffu), anc2 = (int)((tree >> 8) & 0xffu) - 1, anc4 = (int)((tree >> 16) & 0xffu) - 1;
  V3 axw[3], anc[3];
  {
    V3 xp = pos;
    Q4 xq = qrel;
#pragma unroll
    for (int r = 0; r < 3; r++) {
      const int a = r == 0 ? parent : (r == 1 ? anc2 : anc4);
      float *o = T.lk[lane];
      o[0] = xp.x; o[1] = xp.y; o[2] = xp.z; o[3] = xq.w; o[4] = xq.x; o[5] = xq.y; o[6] = xq.z;
      DM_SYNC();
      if (a >= 0) {
        const float *p = T.lk[a];
        const V3 pp = {p[0], p[1], p[2]};
        const Q4 pq = {p[3], p[4], p[5], p[6]};
        xp = pp + mv(q2m(pq), xp);
        xq = qmul(pq, xq);
      }
      DM_SYNC();
    }
    xq = qnormalize(xq);
    c.xp = xp; c.xq = xq;
    float *o = T.lk[lane];
    o[3] = xq.w; o[4] = xq.x; o[5] = xq.y; o[6] = xq.z;
    DM_SYNC();
    Q4 pq = {1.f, 0.f, 0.f, 0.f};
    if (parent >= 0) { const float *p = T.lk[parent]; pq = {p[3], p[4], p[5], p[6]}; }
    const M3 Rp = q2m(pq);
#pragma unroll
    for (int s = 0; s < 3; s++) { axw[s] = mv(Rp, axp[s]); anc[s] = xp; }
    DM_SYNC();
  }
  BSTAMP(0);  // kinematics
  const M3 xmat = q2m(c.xq);
  c.xip = c.xp + mv(xmat, V3{M.l_ipos[0][lane], M.l_ipos[1][lane], M.l_ipos[2][lane]});
  const M3 ximat = q2m(qmul(c.xq, Q4{M.l_iquat[0][lane], M.l_iquat[1][lane], M.l_iquat[2][lane], M.l_iquat[3][lane]}));
  c.mass = M.l_mass[lane];
  // ---- mj: mj_comPos with the fixed thorax origin as the reference point
  const I10 cinert = inert_com(V3{M.l_inertia[0][lane], M.l_inertia[1][lane], M.l_inertia[2][lane]}, ximat, c.xip - c0, c.mass);
  S6 cdof[3];
#pragma unroll
  for (int s = 0; s < 3; s++) cdof[s] = s < ndof ? mk6(axw[s], cross(axw[s], c0 - anc[s])) : zero6();
  // ---- mj: mj_comVel + the acceleration half of mj_rne.  All motion vectors refer to the fixed thorax origin, so a link's
  //      velocity is the plain sum of v * cdof over its ancestor path: path sums by pointer jumping (published inclusive,
  //      the exclusive one - the parent's velocity - kept privately), the velocity products locally, then the same path
  //      sum for the bias accelerations.
  {
    S6 dv = zero6();
#pragma unroll
    for (int s = 0; s < 3; s++) if (s < ndof) dv = dv + c.v[s] * cdof[s];
    S6 sv = dv, pv = zero6();
#pragma unroll
    for (int r = 0; r < 3; r++) {
      const int a = r == 0 ? parent : (r == 1 ? anc2 : anc4);
      st6(T.lk[lane], sv);
      DM_SYNC();
      if (a >= 0) { const S6 t = ld6(T.lk[a]); sv = sv + t; pv = pv + t; }
      DM_SYNC();
    }
    if constexpr (FREE_ROOT) pv = pv + c.V0;  // every path starts at the moving root
    S6 da = zero6();
#pragma unroll
    for (int s = 0; s < 3; s++) {
      if (s < ndof) {
        const S6 cdd = cross_motion(pv, cdof[s]);
        pv = pv + c.v[s] * cdof[s];
        da = da + c.v[s] * cdd;
      }
    }
    c.cvel = pv;
#pragma unroll
    for (int r = 0; r < 3; r++) {
      const int a = r == 0 ? parent : (r == 1 ? anc2 : anc4);
      st6(T.lk[lane], da);
      DM_SYNC();
      if (a >= 0) da = da + ld6(T.lk[a]);
      DM_SYNC();
    }
    // (free root: gravity is a uniform acceleration of the whole tree and is added to the root's acceleration after the solve)
    if constexpr (!FREE_ROOT) da.l2 += (c.flags & BF_NO_GRAVITY) ? 0.f : -M.gz;
    c.caccb = da;
  }
  BSTAMP(1);  // velocities + bias accelerations
  // ---- body forces: rigid-body bias (mj_rne) minus inertia-box drag (mj_inertiaBoxFluidModel), about c0
  S6 ftot;
  {
    const S6 t1 = mul_inert(cinert, c.caccb), t2 = mul_inert(cinert, c.cvel);
    ftot = t1 + cross_force(c.cvel, t2);
    if (!(c.flags & BF_NO_FLUID)) {
      float fl[8];
#pragma unroll
      for (int k = 0; k < 8; k++) fl[k] = M.l_fl[k][lane];
      const V3 r = c.xip - c0;
      const V3 wl = mtv(ximat, ang(c.cvel)), vl = mtv(ximat, lin(c.cvel) + cross(ang(c.cvel), r));
      const V3 Tl = {-fl[0] * wl.x - fl[5] * fabsf(wl.x) * wl.x, -fl[0] * wl.y - fl[6] * fabsf(wl.y) * wl.y, -fl[0] * wl.z - fl[7] * fabsf(wl.z) * wl.z};
      const V3 Fl = {-fl[1] * vl.x - fl[2] * fabsf(vl.x) * vl.x, -fl[1] * vl.y - fl[3] * fabsf(vl.y) * vl.y, -fl[1] * vl.z - fl[4] * fabsf(vl.z) * vl.z};
      const V3 Tw = mv(ximat, Tl), Fw = mv(ximat, Fl);
      ftot = ftot - mk6(Tw + cross(r, Fw), Fw);
    }
  }
  // ---- subtree sums (mj_crb's composite inertia, then mj_rne's backward pass), leaves first
  //      Links are numbered depth first, so the subtree of link l is lanes l .. l + sub - 1: every lane gathers its own
  //      range from one publication of the per-link values (no level order, no barrier inside the loop).
  I10 crb = cinert;
  const int maxsub = M.maxsub;
  st10(T.lk[lane], cinert);
  DM_SYNC();
#pragma unroll 1
  for (int t = 1; t < maxsub; t++) if (t < sub) crb = add10(crb, ld10(T.lk[lane + t]));
  DM_SYNC();
  st6(T.lk[lane], ftot);
  DM_SYNC();
#pragma unroll 1
  for (int t = 1; t < maxsub; t++) if (t < sub) ftot = ftot + ld6(T.lk[lane + t]);
  DM_SYNC();
  BSTAMP(2);  // body forces + subtree sums
  float hfnb = 0.f;
  if constexpr (FREE_ROOT) {
    // halteres as links of the root; then the whole tree's inertia and bias force: the links hanging on the root hold their subtrees'
    I10 ti = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    S6 tf = zero6();
    if (parent < 0) { ti = crb; tf = ftot; }
    if (c.xh) {
      I10 hi;
      S6 hf;
      hfnb = haltere_link(c, hi, hf);
      ti = add10(ti, hi); tf = tf + hf;
    }
    c.Itree = I10{wave_sum(ti.i0), wave_sum(ti.i1), wave_sum(ti.i2), wave_sum(ti.i3), wave_sum(ti.i4), wave_sum(ti.i5), wave_sum(ti.i6), wave_sum(ti.i7),
                  wave_sum(ti.i8), wave_sum(ti.i9)};
    c.Ftot = S6{wave_sum(tf.a0), wave_sum(tf.a1), wave_sum(tf.a2), wave_sum(tf.l0), wave_sum(tf.l1), wave_sum(tf.l2)};
  }
  // ---- smooth joint forces without actuation: springs, dampers, -(bias - drag)
#pragma unroll
  for (int s = 0; s < 3; s++) {
    float f = 0.f;
    if (s < ndof) {
      if (!(c.flags & BF_NO_SPRING)) f -= M.s_stiff[s][lane] * (c.q[s] - M.s_sref[s][lane]);
      if (!(c.flags & BF_NO_DAMPER)) f -= M.s_damp[s][lane] * c.v[s];
      f -= dot6(cdof[s], ftot);
    }
    c.fnb[s] = f;
  }
  if constexpr (FREE_ROOT) { if (c.xh) c.fnb[2] = hfnb; }
  else if (c.xh) {  // halteres: closed form (see ball_model.hpp)
    float sn, cs;
    fsincos(c.q[2], &sn, &cs);
    float f = 0.f;
    if (!(c.flags & BF_NO_SPRING)) f -= M.s_stiff[2][lane] * (c.q[2] - M.s_sref[2][lane]);
    if (!(c.flags & BF_NO_DAMPER)) f -= M.s_damp[2][lane] * c.v[2];
    if (!(c.flags & BF_NO_GRAVITY)) f += M.x_Gc[lane] * cs + M.x_Gs[lane] * sn;
    if (!(c.flags & BF_NO_FLUID)) f -= M.x_cv[lane] * c.v[2] + M.x_cq[lane] * fabsf(c.v[2]) * c.v[2];
    c.fnb[2] = f;
  }
  // ball: isotropic sphere about its centre, only the box drag acts (mj_inertiaBoxFluidModel in the inertial frame)
  if constexpr (!FREE_ROOT) {
    V3 tau = {0.f, 0.f, 0.f};
    if (!(c.flags & BF_NO_FLUID)) {
      const M3 Ri = q2m(Q4{M.b_iquat[0], M.b_iquat[1], M.b_iquat[2], M.b_iquat[3]});
      const V3 wl = mtv(Ri, c.bw);
      const V3 Tl = {-M.b_fl[0] * wl.x - M.b_fl[5] * fabsf(wl.x) * wl.x, -M.b_fl[0] * wl.y - M.b_fl[6] * fabsf(wl.y) * wl.y, -M.b_fl[0] * wl.z - M.b_fl[7] * fabsf(wl.z) * wl.z};
      tau = mv(Ri, Tl);
    }
    c.btau = tau;
  }
  // ---- mj: mj_crb joint-space inertia, one entry per (lane, slot t)
#pragma unroll
  for (int s = 0; s < 3; s++) {
    if (s < ndof) { st6(T.F[opq(c.sdof[s])], mul_inert(crb, cdof[s])); st6(T.C[opq(c.sdof[s])], cdof[s]); }
  }
  if constexpr (!FREE_ROOT) {  // (free root: haltere_link has stored both)
  if (c.xh) { st6(T.F[c.sdof[2]], S6{M.x_M[lane], 0.f, 0.f, 0.f, 0.f, 0.f}); st6(T.C[c.sdof[2]], S6{1.f, 0.f, 0.f, 0.f, 0.f, 0.f}); }
  }
#pragma unroll
  for (int s = 0; s < 3; s++) if (slot_on(c, s)) T.dadd[opq(c.sdof[s])] = (c.flags & BF_NO_DAMPER) ? 0.f : M.h * M.s_damp[s][lane];
  DM_SYNC();
#pragma unroll
  for (int t = 0; t < ECAP; t++) {
    const unsigned ea = M.ent_a[t][lane];
    if (ea >> 31) {
      const unsigned i = ea & 0xffu, j = (ea >> 8) & 0xffu;
      float mij = dot6(ld6(T.C[j]), ld6(T.F[i]));
      if (i == j) mij += M.d_arm[i];
      T.Mq[(ea >> 16) & 0x3ffu] = mij;
    }
  }
  DM_SYNC();
  BSTAMP(3);  // joint forces + inertia assembly
  factor2(c);
  BSTAMP(4);  // factor M and M + h B
