// walk_substeps.hpp - the device code of the free-root substep that more than one translation unit compiles: the state record, the LDS
// tiles, the wave's context, stage 1 / stage 2 with the limit block and the one contact block (`contact_forces`: the floor's rows and, on
// a self tile, the fly's own) and sensor pass (`contact_sense`), the substep loop and the state export.
// walk_env.hip (the four kernels of bare physics and of the floor-off environment), walk_floor_env.hip (the environment on the floor),
// walk_self_env.hip (bare physics with the fly's own contacts), walk_imit_self_env.hip (the environment on the floor with the fly's
// own contacts), walk_full_env.hip and walk_imit_full_env.hip (the same two with the plane against ellipsoids and cylinders) include it; what the code does is described at the head of walk_env.hip and where each part starts.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>
#include <type_traits>

#include "walk_env.hpp"
#include "walk_model.hpp"
#include "leg_dyn.hpp"
#include "row_newton.hpp"
#include "walk_imu.hpp"
#include "walk_floor.hpp"
#include "walk_floor_convex.hpp"
#include "walk_sense.hpp"
#include "walk_self_sense.hpp"
#include "walk_self.hpp"
#include "self_pairs.hpp"

namespace ffw {
using namespace dm;
using namespace ffb;

// State record of the free-root handle (the tethered handle's BState is untouched).  MuJoCo's free-joint conventions: position and
// linear velocity in the world frame, angular velocity in the body frame.
struct alignas(16) WState {
  double pos[3];
  float quat[4];
  float vlin[3], wb[3];
  float q[NDP], v[NDP], act[64];
  // limits handle only (zero otherwise): limit rows and solver iterations of the last substep, overflow bits of the last launch
  // (2: some substep instantiated more limits than RMAX rows; the rows beyond were dropped for that substep)
  int nlim, iters, step_bits, pad;
};
static_assert(sizeof(WState) == 1168, "the four ints fill what used to be padding");

constexpr int BF_WALK_JOINT_LIMITS = 512;  // FFE_WALK_JOINT_LIMITS: host side only, the kernels do not read it
constexpr int BF_WALK_EPISODES = 1024;     // FFE_WALK_EPISODES: host side only
constexpr int BF_WALK_FLOOR = 2048;        // FFE_WALK_FLOOR: host side only (it selects the floor kernel)
constexpr int BF_WALK_SELF = 4096;         // FFE_WALK_SELF: host side only (it selects the kernel with the fly's own contacts)
constexpr int BF_WALK_SELF_EPISODES = 8192;  // FFE_WALK_SELF_EPISODES: host side only (FFE_WALK_SELF under the environment is asked for by it)
constexpr int BF_WALK_FLOOR_CONVEX = 32768;  // FFE_WALK_FLOOR_CONVEX: host side only (it selects the kernel with the second floor pass)
constexpr int LCOL = 16;                  // solve columns per block of M: a block has at most NSTEP = 14 hinges, each with one limit row
static_assert(NSTEP <= LCOL, "a block's limit rows must fit its columns");

// What a tile adds to the smooth substep: a tile that derives from another sets its own switches to true, and the shared code reads
// `Tile::kFloor` ... under `if constexpr`.
struct TileKind {
  static constexpr bool kFloor = false;         // the floor's contact tables: the collision pass and the contact block
  static constexpr bool kSense = false;         // the sensor sums of the environment on the floor
  static constexpr bool kSelf = false;          // the second chain of a fly-fly contact
  static constexpr bool kPackedNormal = false;  // a fly-fly slot keeps its normal in floats it leaves unused (WTileSX)
  static constexpr bool kConvexFloor = false;   // the second floor pass: the plane against ellipsoids and cylinders (WTileXC)
};

struct alignas(16) WTile : TileKind {
  union {
    struct { float Q[NDP], V[NDP]; };  // joint state staged for the actuators (start of stage 2)
    float4 X4[NDP];                     // right-hand sides / solutions of the block solves
  };
  float dadd[NDP];                      // h * damping: only read by the stage-1 factorisation
  float Mq[NMMAX];                      // joint-space inertia of the hinges: only read by the stage-1 factorisation
  union {
    float F[NDP][6];                    // crb * cdof = the hinge's column of M_rj: written by the assembly, read by stage 2
    float lk[NL][12];                   // link exchange of the tree passes (dead once the assembly starts)
  };
  float Lm[NMMAX], Lh[NMMAX];           // factors of M_jj and of M_jj + h B
  float dinv_m[NDP], dinv_h[NDP];
  float C[NDP][6];
  float frc[64];
  float Y[NDP][6];                      // (M_jj + h B)^-1 M_jr
};
static_assert(sizeof(WTile) <= 20480, "the tile must leave room for 8 waves per CU");

// Tile of the limits kernel: WTile without Y (a row lane reads its hinge's Y_m straight from the solve), with the packed G over the
// two arrays that are dead once stage 1 has factorised (G dies with the substep), and the row tables.
struct alignas(16) WTileL : TileKind {
  union {
    struct { float Q[NDP], V[NDP]; };
    float4 X4[NDP];
  };
  union {
    struct { float dadd[NDP]; float Mq[NMMAX]; };
    float G[RMAX * (RMAX + 1) / 2];     // G = J M^-1 J' over the limit rows, lower triangle packed by rows (lane r owns row r)
    float S[RMAX * (RMAX + 1) / 2];     // the Newton transposes its factor through the same floats once G sits in registers
  };
  union {
    float F[NDP][6];
    float lk[NL][12];
  };
  float Lm[NMMAX], Lh[NMMAX];
  float dinv_m[NDP], dinv_h[NDP];
  float C[NDP][6];
  float frc[64];
  float r_y0[RMAX], r_D[RMAX], r_f[RMAX], r_sgn[RMAX];
  unsigned char r_dof[RMAX], r_blk[RMAX], r_col[RMAX], rowof[NBLK][LCOL];
};
static_assert(sizeof(WTileL) <= 20480, "the tile must leave room for 8 waves per CU");

// Tile of the floor kernel (FFE_WALK_FLOOR): the limits kernel's with the tethered kernel's capacities (NC
// contacts, KCOL columns per block), the contact tables, and the link poses of the collision pass over the floats of G, which are dead
// between the factorisation of stage 1 and the G build of stage 2.  What a contact row needs of its geom is read from the model tables
// through c_geom; the rows' Jacobian entries are evaluated where they are used, as in the tethered kernel.
struct alignas(16) WTileF : TileKind {
  static constexpr bool kFloor = true;
  union {
    struct { float Q[NDP], V[NDP]; };
    float4 X4[NDP];
  };
  union {
    struct { float dadd[NDP]; float Mq[NMMAX]; };
    float G[RMAX * (RMAX + 1) / 2];
    float S[RMAX * (RMAX + 1) / 2];
    float lp[NL][14];                   // collision pass: link position 3, quaternion 4, spatial velocity 6
  };
  union {
    float F[NDP][6];
    float lk[NL][12];
  };
  float Lm[NMMAX], Lh[NMMAX];
  float dinv_m[NDP], dinv_h[NDP];
  float C[NDP][6];
  float frc[64];
  float r_y0[RMAX], r_D[RMAX], r_f[RMAX], r_sgn[RMAX], r_lam[RMAX];
  unsigned char r_dof[RMAX], r_blk[RMAX], r_col[RMAX], rowof[NBLK][KCOL];
  float c_pos[NC][3], c_vel[NC][3], c_dist[NC], c_D[NC], c_mu[NC], c_w[NC];  // point, its velocity (root frame), distance; cone tables; adhesion pull
  unsigned short c_amask[NC];
  unsigned char c_geom[NC], c_excl[NC], c_link[NC], c_blk[NC];
  // adhesion pull + constraint force on the root coordinates (w_b, v_b): joins the Euler solve's root right-hand side; [6] = the sum of
  // the contacts' normal forces.  In the tile, not in registers: uniform values that live from the row build to the end of the substep
  float rootf[8];
  int step_bits;  // overflow bits of the launch so far (beyond the far substep's tile: both kinds of substep leave it alone)
};
static_assert(offsetof(WTileF, step_bits) >= sizeof(WTileL), "the far substep must not reach the launch's overflow bits");
static_assert(sizeof(WTileF) <= 20480, "the tile must leave room for 8 waves per CU");
static_assert(sizeof(float[NL][14]) <= sizeof(float[RMAX * (RMAX + 1) / 2]), "the link poses must fit over G");
// The limits kernel's tile under a name of the floor kernel's own: a floor substep with no floor in reach runs the limits kernel's code
// as an instantiation apart (sharing the limits kernel's own instantiation changed that kernel's register allocation).
struct alignas(16) WTileFar : WTileL {};
static_assert(sizeof(WTileFar) <= sizeof(WTileF), "the far substep runs inside the floor tile");
// what a floor wave carries from stage to stage and reports (per env, in a buffer of the handle)
struct FloorCtx {
  int nc;          // contacts kept in this substep
  float mind;      // smallest distance
};
// (nself: the fly-fly contacts among ncon, 0 without FFE_WALK_SELF; with FFE_WALK_FLOOR_CONVEX bits 8 .. 15 count the plane-ellipsoid /
//  plane-cylinder contacts among ncon: both are at most NC = 16, and every other kernel leaves those bits zero)
struct FloorRec { int ncon; float fsum, mind; int nself; };

// Tile of the episode kernel: the limits kernel's, plus the sensor sums of a control step (accelerometer 3, gyro 3, velocimeter 3,
// force 18, touch 6: the order of the oracle's buffer)
struct alignas(16) WTileE : WTileL {
  float sens[36];
  float qsave[3][64];  // the hinges' right-hand side, parked while the qacc solve runs (three fewer live registers per lane there)
};
static_assert(sizeof(WTileE) <= 20480, "the tile must leave room for 8 waves per CU");

// Tile of the episode kernel on the floor (walk_floor_env.hip `imitation_floor_step`): the floor kernel's,
// plus the sensor sums and the orientation of the six force sites in the root frame (published by their links after stage 1, read by the
// sensor pass of stage 2).  The hinges' right-hand side is parked during the `qacc` solve too, but over the tail of G: by then the solver
// has returned and G is dead, and the sensor pass that follows exchanges its link values through the head of G (`lp`).
struct alignas(16) WTileS : WTileF {
  static constexpr bool kSense = true;
  float sens[36];
  float fsq[6][4];
  // per force sensor, summed over its link's subtree after stage 1 (walk_sense.hpp): the velocity terms 3, the mass, m r 3.  In the
  // tile, not in registers: seven more live values per lane across the solver's call spilled 47 VGPRs.
  float sp[6][8];
};
constexpr int kSensePark = NL * 14;  // floats into G: behind the link exchange
static_assert(kSensePark + 3 * 64 <= RMAX * (RMAX + 1) / 2, "the parked right-hand side must fit behind the link exchange");
static_assert(sizeof(WTileS) <= 20480, "the tile must leave room for 8 waves per CU");

// Tile of the kernel with the fly's own contacts (walk_self_env.hip `floor_self_step`, FFE_WALK_SELF): the
// floor kernel's, whose contact tables now hold the floor contacts in the first slots and the fly-fly contacts behind them (NC in all).
// A fly-fly slot k keeps the link of geom2 in c_link / c_blk / c_amask (entries +n . u of its row), the link of geom1 in c_link1 /
// c_blk1 / c_amask1 (entries -n . u; 255: a geom of the thorax, which is the root and has no chain), its normal in c_nrm, -aref of its
// row in c_vel[k][0] and its D in c_D; c_col1 is the solve column of geom1's chain when that lies in another block of M.  A floor slot has
// c_link1 = 255.  The scratch of the two collision passes lies over floats that are dead between stage 1 and stage 2:
//   sphere / capsule pairs   centre | bounding radius and axis | half length of the 48 slots over X4, their radii over the tail of G
//                            (behind the link poses `lp`)
//   convex pairs             centre | bounding radius of the 70 geoms, then the two pair lists, over X4 (the orientation of a geom is
//                            composed from its link's pose where it is needed)
// F is read by stage 2 on a walker, so - unlike on the tethered fly - the link exchange `lk` over it is not free here.
struct alignas(16) WTileX : WTileF {
  static constexpr bool kSelf = true;
  float c_nrm[NC][3];
  unsigned short c_amask1[NC];
  unsigned char c_link1[NC], c_blk1[NC], c_col1[NC];
  float sv0[8];  // the root's spatial velocity (w_b, v_b): what a geom of the thorax moves with
};
static_assert(sizeof(WTileX) <= 20480, "the tile must leave room for 8 waves per CU");
static_assert(2 * NPG <= NDP && NL * 14 + NPG <= RMAX * (RMAX + 1) / 2, "the primitive slots must fit over X4 and the tail of G");
static_assert((NG + (CL1 * 2 + 15) / 16 + (CL2 * 2 + 15) / 16) <= NDP, "the geom centres and the pair lists must fit over X4");
struct SelfCtx : FloorCtx {
  int ns;          // fly-fly contacts kept in this substep: slots nc .. nc + ns - 1
};
// Tile of the kernel with the second floor pass (walk_full_env.hip `floor_full_step`, FFE_WALK_FLOOR_CONVEX; DESIGN.md section 12 step
// 3d): the self tile as it is.  A plane-ellipsoid / plane-cylinder contact is a floor slot like any other - it sits behind the primitive
// floor contacts and in front of the fly-fly ones, and `nc` counts both kinds - whose c_geom is NPG + its row of WalkFloorConvex; a slot
// of a root geom has c_link = c_blk = 255 and an empty c_amask (no chain: its rows have the root entries alone).  The pass needs no
// scratch: a lane keeps its row's candidates in registers, and in the overflow case a primitive slot moves through its lane's registers.
struct alignas(16) WTileXC : WTileX {
  static constexpr bool kConvexFloor = true;
};
static_assert(sizeof(WTileXC) == sizeof(WTileX), "the second floor pass adds nothing to the tile");
static_assert(NPG + NFC <= 255 && NFC <= 64 && NC <= 64, "c_geom names both tables' rows in a byte; a lane per row and per slot");
struct FullCtx : SelfCtx {
  int nv;          // plane-ellipsoid / plane-cylinder contacts among the nc floor contacts of this substep
};
// the table of the second floor pass: directly behind the WalkModel whose WalkExtra the wave carries (WalkModelFull)
__device__ __forceinline__ const WalkFloorConvex FFE_GLOBAL *convex_table(const WalkExtra FFE_GLOBAL *X) {
  return (const WalkFloorConvex FFE_GLOBAL *)((const char FFE_GLOBAL *)X - offsetof(WalkModel, x) + offsetof(WalkModelFull, xc));
}
struct NoSelf { constexpr operator int() const { return 0; } };  // the fly-fly count of a tile without them: an argument that takes no register
__device__ __forceinline__ NoSelf self_count(const FloorCtx &) { return {}; }
__device__ __forceinline__ int self_count(const SelfCtx &fl) { return fl.ns; }

// Tile of the episode kernel on the floor with the fly's own contacts (walk_imit_self_env.hip `imitation_self_step`; DESIGN.md section
// 12 step 4d): a sense tile and a self tile at once.  WTileF + the sensor part of WTileS (432 B) + the self part of WTileX (304 B) would
// be 20 608 B, 128 B over what 8 waves per CU leave, so the fly-fly normal has no array of its own here (`kPackedNormal`): a fly-fly slot
// k uses c_vel[k][0] alone of its three c_vel floats (-aref of its one row) and never c_mu[k] (the solver reads c_mu of the floor's cone
// blocks k < nc only), and a floor slot never had a stored normal (its normal is the plane's), so the normal of slot k lies in
// c_vel[k][1], c_vel[k][2], c_mu[k] behind `self_nrm` / `self_put`.  That saves c_nrm's 192 B: 20 416 B.
// Overlays, as in the two parents (asserted below where the tile cannot show it by itself):
//   between stage 1 and stage 2   the link poses `lp` over the head of G; the primitive slots over X4[0 .. 2 NPG) and their radii over
//                                 G[NL 14 .. NL 14 + NPG); the convex pass's geom centres and pair lists over X4.  All of it is dead when
//                                 the collision passes have returned: stage 2 starts by staging Q / V over X4 and builds G afresh.
//   after the solver's return     G is dead.  The hinges' right-hand side is parked at G[kSensePark .. kSensePark + 192) - the floats the
//                                 radii used during the collision - while the qacc solve runs; the hinges' qacc stays in X4[.].x for the
//                                 sensor pass, which exchanges its link values through `lp` (the head of G, below kSensePark).
struct alignas(16) WTileSX : WTileF {
  static constexpr bool kSense = true;
  static constexpr bool kSelf = true;
  static constexpr bool kPackedNormal = true;
  float sens[36];
  float fsq[6][4];
  float sp[6][8];
  unsigned short c_amask1[NC];
  unsigned char c_link1[NC], c_blk1[NC], c_col1[NC];
  float sv0[8];
};
static_assert(sizeof(WTileSX) == sizeof(WTileF) + 432 + 304 - sizeof(float[NC][3]), "the sensor part and the self part without c_nrm");
static_assert(sizeof(WTileSX) <= 20480, "the tile must leave room for 8 waves per CU");
static_assert(NL * 14 <= kSensePark && kSensePark + 3 * 64 <= RMAX * (RMAX + 1) / 2,
              "the parked right-hand side lies behind the sensor pass's link exchange, inside G");
static_assert(NPG <= 3 * 64, "the slot radii of the collision pass and the parked right-hand side share the same floats of G, one after the other");
// Tile of the episode kernel with every contact of the reference's task (walk_imit_full_env.hip `imitation_full_step`; DESIGN.md section
// 12 step 4e): `WTileSX` as it is, with the second floor pass switched on.  `floor_convex_collide` runs between `floor_collide` and the
// fly-fly passes and needs no scratch of its own, so the overlays of step 4d hold with it in between:
//   it reads      the link poses `lp` (head of G) that `floor_collide` published and T.sv0; both stay as they are until `prim_pairs`
//                 fills X4 and the radii behind `lp`, which happens after its closing barrier;
//   it writes     contact slots alone (c_pos .. c_amask of slots < NC), none of which lies in a union;
//   afterwards    a plane-ellipsoid / plane-cylinder slot is a floor slot: `kPackedNormal` never packs a normal into it (slots k < nc keep
//                 c_vel and c_mu for the cone block), and `contact_sense` finds its link by comparing c_link with the lane, so 255 (a
//                 thorax geom) matches no lane and c_geom >= NPG is never used as an index there.
struct alignas(16) WTileSXC : WTileSX {
  static constexpr bool kConvexFloor = true;
};
static_assert(sizeof(WTileSXC) == sizeof(WTileSX), "the second floor pass adds nothing to the tile");
static_assert(sizeof(WTileSXC) <= 20480, "the tile must leave room for 8 waves per CU");
static_assert(WTileSXC::kSense && WTileSXC::kSelf && WTileSXC::kPackedNormal && WTileSXC::kFloor, "a sense tile and a self tile with the packed normal");
static_assert(NL <= 64 && NL < 255, "c_link = 255 names no lane: the sensor pass skips a root geom's contact by comparison alone");
static_assert(NPG + NFC <= 255 && NC <= 64 && NFC <= 64, "as for WTileXC: c_geom names both tables' rows in a byte; a lane per row and per slot");
// the normal (from geom1's link to geom2's) of fly-fly slot k
template <class TileX>
__device__ __forceinline__ void self_nrm(const TileX &T, const int k, float (&n)[3]) {
  if constexpr (TileX::kPackedNormal) { n[0] = T.c_vel[k][1]; n[1] = T.c_vel[k][2]; n[2] = T.c_mu[k]; }
  else { n[0] = T.c_nrm[k][0]; n[1] = T.c_nrm[k][1]; n[2] = T.c_nrm[k][2]; }
}

// What the episode kernel reads besides the model and the state: fixed at create, in device memory, fetched by scalar loads where it
// is used (as kernel arguments its thirty dwords stayed in SGPRs over the whole substep loop and spilled into VGPR lanes).
struct ImitArgs {
  const double *pose;    // [B][109] qpos of ffe_walktask_reference_pose(clip, 0): what a reset row starts from
  const int *flag;       // [B] 0 = step, 1 = reset, 2 = leave the env alone (ffe_reset_envs, mask byte 0)
  double *qpos, *qvel;   // [B][109], [B][108] in the ffe_get_state layout, for the task layer
  float *term;           // [B][4]: |velocimeter|, |gyro| and sum qacc^2 of the last substep (not the means), 0
  int obs_dim, off_act, off_force, off_gyro, off_touch, off_velocimeter;  // (the accelerometer heads the row)
  int canonical, clip, pad_first_obs;
  float site_pos[3], site_quat[4];  // the IMU site in the root frame
  FloorRec *rec;         // [B] on the floor (FFE_WALK_FLOOR): where a wave reports its contacts; null otherwise
};
// ... and what changes from call to call
struct ImitCall {
  const ImitArgs *a;
  const float *action;   // [B][NACT] raw (or canonical) actions; not read by a reset row
  float *obs;            // [B][obs_dim]: the 92 physics columns are written here
};
struct NoEpisode {};  // the bare-physics kernels: no episode code is compiled
struct FloorCall { FloorRec *rec; };  // the floor kernel (bare physics too): where a wave reports its contacts
// where a floor wave reports its contacts: the bare-physics call's buffer or the environment's
__device__ __forceinline__ FloorRec *contact_record(const FloorCall &ep) { return ep.rec; }
__device__ __forceinline__ FloorRec *contact_record(const ImitCall &ep) { return ep.a->rec; }

template <class Tile>
struct CtxT {
  const BallModel *M;
  const WalkExtra FFE_GLOBAL *X;
  Tile *T;
  int lane, flags;
  unsigned lpack;
  int sdof[3];
  float q[3], v[3], fnb[3];
  int xh;
  V3 xp, xip;
  Q4 xq;
  S6 cvel, caccb;
  float mass;
  // root
  Q4 rq;        // orientation
  V3 vw, wb;    // linear velocity in the world frame, angular velocity in the body frame
  double pos[3];
  S6 V0;        // (w_b, R' v_w)
  I10 Itree;    // spatial inertia of the whole tree about the root origin = M_rr
  S6 Ftot;      // bias force of the whole tree without gravity = -(root rows of the smooth force)
  int overflow; // limits kernel: overflow bits of this launch
  std::conditional_t<Tile::kConvexFloor, FullCtx, std::conditional_t<Tile::kSelf, SelfCtx, std::conditional_t<Tile::kFloor, FloorCtx, NoEpisode>>> fl;
};

// ------------------------------------------------------------------------------------------------ stage 1
template <class C>  // (a template so that the fragment's tethered branches are discarded, not compiled)
__device__ __forceinline__ void stage1(C &c) {
  constexpr bool FREE_ROOT = true;
  auto &T = *c.T;
  const BallModel FFE_GLOBAL &M = model(c);
  {
    const M3 R = q2m(c.rq);
    c.V0 = mk6(c.wb, mtv(R, c.vw));
  }
#include "leg_stage1.inc"
  (void)xmat;
  // the root link itself: uniform across the wave
  {
    const WalkExtra FFE_GLOBAL &X = *c.X;
    const I10 I0 = {X.r_cin[0], X.r_cin[1], X.r_cin[2], X.r_cin[3], X.r_cin[4], X.r_cin[5], X.r_cin[6], X.r_cin[7], X.r_cin[8], X.r_cin[9]};
    S6 f0 = cross_force(c.V0, mul_inert(I0, c.V0));
    if (!(c.flags & BF_NO_FLUID)) {
      float fl[8];
#pragma unroll
      for (int k = 0; k < 8; k++) fl[k] = X.r_fl[k];
      f0 = f0 - box_drag(fl, q2m(Q4{X.r_iquat[0], X.r_iquat[1], X.r_iquat[2], X.r_iquat[3]}), V3{X.r_ipos[0], X.r_ipos[1], X.r_ipos[2]}, c.V0);
    }
    c.Itree = add10(c.Itree, I0);
    c.Ftot = c.Ftot + f0;
  }
}

// ------------------------------------------------------------------------------------------------ 6 x 6 root system
__device__ __forceinline__ float comp(const S6 &v, int k) { return k == 0 ? v.a0 : (k == 1 ? v.a1 : (k == 2 ? v.a2 : (k == 3 ? v.l0 : (k == 4 ? v.l1 : v.l2)))); }

// Schur complement S = M_rr - M_rj Y (lower triangle) and right-hand side b_r = f_r - M_rj z: wave sums of the lanes' own hinges
template <class C>
__device__ __forceinline__ void schur(const C &c, const S6 (&mrj)[3], const S6 (&y)[3], const float (&z)[3], float (&Sm)[6][6], float (&br)[6]) {
  // M_rr from the tree's spatial inertia: column k = I e_k
#pragma unroll
  for (int k = 0; k < 6; k++) {
    const S6 e = {k == 0 ? 1.f : 0.f, k == 1 ? 1.f : 0.f, k == 2 ? 1.f : 0.f, k == 3 ? 1.f : 0.f, k == 4 ? 1.f : 0.f, k == 5 ? 1.f : 0.f};
    const S6 col = mul_inert(c.Itree, e);
#pragma unroll
    for (int r = 0; r < 6; r++) Sm[r][k] = comp(col, r);
  }
#pragma unroll
  for (int a = 0; a < 6; a++) {
#pragma unroll
    for (int b = 0; b <= a; b++) {
      float p = 0.f;
#pragma unroll
      for (int s = 0; s < 3; s++) p += comp(mrj[s], a) * comp(y[s], b);
      Sm[a][b] -= wave_sum(p);
    }
    float p = 0.f;
#pragma unroll
    for (int s = 0; s < 3; s++) p += comp(mrj[s], a) * z[s];
    br[a] = -comp(c.Ftot, a) - wave_sum(p);
  }
}

// S = L L' in place (lower triangle, in registers, uniform); id = 1 / diag(L)
__device__ __forceinline__ void chol6(float (&Sm)[6][6], float (&id)[6]) {
#pragma unroll
  for (int j = 0; j < 6; j++) {
    float d = Sm[j][j];
#pragma unroll
    for (int k = 0; k < j; k++) d -= Sm[j][k] * Sm[j][k];
    const float r = __builtin_amdgcn_rsqf(d);
    const float ir = r * (1.5f - 0.5f * d * r * r);  // 1 / sqrt(d), one Newton step
    id[j] = ir;
    Sm[j][j] = d * ir;
#pragma unroll
    for (int i = j + 1; i < 6; i++) {
      float e = Sm[i][j];
#pragma unroll
      for (int k = 0; k < j; k++) e -= Sm[i][k] * Sm[j][k];
      Sm[i][j] = e * ir;
    }
  }
}
__device__ __forceinline__ void chol6_forward(const float (&Sm)[6][6], const float (&id)[6], const float (&b)[6], float (&x)[6]) {  // L x = b
#pragma unroll
  for (int i = 0; i < 6; i++) {
    float w = b[i];
#pragma unroll
    for (int k = 0; k < i; k++) w -= Sm[i][k] * x[k];
    x[i] = w * id[i];
  }
}
__device__ __forceinline__ void chol6_backward(const float (&Sm)[6][6], const float (&id)[6], float (&x)[6]) {  // L' x = w, in place
#pragma unroll
  for (int i = 5; i >= 0; i--) {
    float w = x[i];
#pragma unroll
    for (int k = i + 1; k < 6; k++) w -= Sm[k][i] * x[k];
    x[i] = w * id[i];
  }
}

// z = A^-1 f and Y = A^-1 M_jr through the factor (L, dinv) of A - M_jj (Lm, dinv_m) or M_jj + h B (Lh, dinv_h): seven right-hand sides
// in two four-wide block solves.  `cols`: M_jr's columns of the lane's three slots in registers, or T.F, from which they are read where
// they are used.  `rows(half)` runs after each solve while X4 holds its solution (half 0: z and Y's angular columns, half 1: Y's linear).
struct NoRows { __device__ __forceinline__ void operator()(int) const {} };
__device__ __forceinline__ S6 col6(const S6 (&mrj)[3], int s, int) { return mrj[s]; }
__device__ __forceinline__ S6 col6(const float (&F)[NDP][6], int, int f) { return ld6(F[f]); }
template <class C, class Cols, class Rows = NoRows>
__device__ __forceinline__ void solve_zy(C &c, const float *L, const float *dinv, const float (&f)[3], const Cols &cols, float (&z)[3], S6 (&y)[3],
                                         Rows &&rows = Rows()) {
  auto &T = *c.T;
#pragma unroll
  for (int s = 0; s < 3; s++) {
    if (slot_on(c, s)) { const S6 m = col6(cols, s, opq(c.sdof[s])); T.X4[opq(c.sdof[s])] = make_float4(f[s], m.a0, m.a1, m.a2); }
  }
  DM_SYNC();
  solve4(c, L, dinv);
#pragma unroll
  for (int s = 0; s < 3; s++) {
    const float4 x = slot_on(c, s) ? T.X4[opq(c.sdof[s])] : make_float4(0.f, 0.f, 0.f, 0.f);
    z[s] = x.x; y[s].a0 = x.y; y[s].a1 = x.z; y[s].a2 = x.w;
  }
  rows(0);
  DM_SYNC();
#pragma unroll
  for (int s = 0; s < 3; s++) {
    if (slot_on(c, s)) { const S6 m = col6(cols, s, opq(c.sdof[s])); T.X4[opq(c.sdof[s])] = make_float4(m.l0, m.l1, m.l2, 0.f); }
  }
  DM_SYNC();
  solve4(c, L, dinv);
#pragma unroll
  for (int s = 0; s < 3; s++) {
    const float4 x = slot_on(c, s) ? T.X4[opq(c.sdof[s])] : make_float4(0.f, 0.f, 0.f, 0.f);
    y[s].l0 = x.x; y[s].l1 = x.y; y[s].l2 = x.z;
  }
  rows(1);
  DM_SYNC();
}

// ------------------------------------------------------------------------------------------------ joint-limit rows
// The constraint block of a substep with R > 0 limit rows (rows already in T.r_sgn / r_D / r_dof / r_blk, -aref in T.r_y0): adds the
// hinges' constraint forces to `qs`.  Returns the solver's iterations.
template <class C>
__device__ __forceinline__ int limit_forces(C &c, const int R, const int (&lrow)[3], const float (&lsgn)[3], const S6 (&mrj)[3], float (&qs)[3]) {
  WTileL &T = *c.T;
  const int lane = c.lane;
  const bool row = lane < R;
  // ---- z_m = M_jj^-1 f_j and Y_m = M_jj^-1 M_jr through M's own factor; a row lane keeps its hinge's Y_m
  S6 ym[3], yr = zero6();
  float zm[3];
  int rdof = 0;
  solve_zy(c, T.Lm, T.dinv_m, qs, mrj, zm, ym, [&](int half) {
    if (half == 0) {
      rdof = row ? (int)T.r_dof[lane] : 0;
      if (row) { const float4 x = T.X4[rdof]; yr.a0 = x.y; yr.a1 = x.z; yr.a2 = x.w; }
    } else if (row) { const float4 x = T.X4[rdof]; yr.l0 = x.x; yr.l1 = x.y; yr.l2 = x.z; }
  });
  // ---- S_m = L L', x_r = S_m^-1 (b_r - M_rj z_m), the hinges' smooth acceleration a_s = z_m - Y_m x_r (gravity: zero on the hinges)
  float Sm[6][6], br[6], id[6], xr[6];
  schur(c, mrj, ym, zm, Sm, br);
  chol6(Sm, id);
  chol6_forward(Sm, id, br, xr);
  chol6_backward(Sm, id, xr);
  float sq = 0.f;
#pragma unroll
  for (int s = 0; s < 3; s++) {
    if (slot_on(c, s)) {
      float a = zm[s];
#pragma unroll
      for (int k = 0; k < 6; k++) a -= comp(ym[s], k) * xr[k];
      T.X4[opq(c.sdof[s])].x = a;
      sq += qs[s] * a;
    }
  }
  float scale2 = wave_sum(sq);  // qfrc_smooth . qacc_smooth: the scale of the solver's stopping test
#pragma unroll
  for (int k = 0; k < 6; k++) scale2 += br[k] * xr[k];
  DM_SYNC();
  const float sg = row ? T.r_sgn[lane] : 0.f;
  if (row) T.r_y0[lane] += sg * T.X4[rdof].x;  // y0 = J a_s - aref
  // ---- the rank-6 part of G: u_i = s_i L^-1 Y_m[f_i], G_ik = u_i . u_k
  const int gtri = lane * (lane + 1) / 2;  // G is symmetric: row `lane` keeps its columns r2 <= lane
  {
    float yv[6], u[6];
#pragma unroll
    for (int k = 0; k < 6; k++) yv[k] = sg * comp(yr, k);
    chol6_forward(Sm, id, yv, u);
    for (int r2 = 0; r2 < R; r2++) {
      float gv = 0.f;
#pragma unroll
      for (int k = 0; k < 6; k++) gv += u[k] * rl_f(u[k], r2);
      if (row && r2 <= lane) T.G[gtri + r2] = gv;
    }
  }
  // ---- columns: a row's column is its rank among the rows of its block (M_jj^-1 is block diagonal)
  for (int k = lane; k < NBLK * LCOL; k += 64) (&T.rowof[0][0])[k] = 255;
  const int myb = row ? (int)T.r_blk[lane] : -1;
  int mycol = 0, ncol = 0;
  for (int b = 0; b < NBLK; b++) {
    const unsigned long long mb = __ballot(myb == b);
    if (myb == b) mycol = __popcll(mb & ((1ull << lane) - 1ull));
    ncol = max(ncol, (int)__popcll(mb));
  }
  DM_SYNC();
  if (row) T.rowof[myb][mycol] = (unsigned char)lane;  // (mycol < NSTEP <= LCOL: one row per hinge)
  DM_SYNC();
#pragma unroll 1
  for (int cb = 0; cb < ncol; cb += 4) {
    for (int f = lane; f < ND; f += 64) T.X4[f] = make_float4(0.f, 0.f, 0.f, 0.f);
    DM_SYNC();
    if (row) { const int col = mycol - cb; if (col >= 0 && col < 4) (&T.X4[rdof].x)[col] = sg; }
    DM_SYNC();
    solve4(c, T.Lm, T.dinv_m);
    if (row) {
      const float4 y = T.X4[rdof];
#pragma unroll
      for (int q2 = 0; q2 < 4; q2++) {
        const float av = sg * (q2 == 0 ? y.x : (q2 == 1 ? y.y : (q2 == 2 ? y.z : y.w)));
        const int r2 = cb + q2 < LCOL ? (int)T.rowof[myb][cb + q2] : 255;
        if (r2 <= lane) T.G[gtri + r2] += av;  // (255 = no such row)
      }
    }
    DM_SYNC();
  }
  // ---- solve, then qfrc_constraint = s f on the hinges
  int iters;  // (ScalarRows reads no model table and ignores the contact-row count, the noslip sweeps and the warm-start flag)
  if (R <= 8) iters = row_newton<8, ScalarRows>(c.T, nullptr, lane, R, 0, scale2, 0, 0);
  else if (R <= 16) iters = row_newton<16, ScalarRows>(c.T, nullptr, lane, R, 0, scale2, 0, 0);
  else if (R <= 32) iters = row_newton<32, ScalarRows>(c.T, nullptr, lane, R, 0, scale2, 0, 0);
  else iters = row_newton<RMAX, ScalarRows>(c.T, nullptr, lane, R, 0, scale2, 0, 0);
#pragma unroll
  for (int s = 0; s < 3; s++) if (lrow[s] >= 0) qs[s] += lsgn[s] * T.r_f[lrow[s]];
  DM_SYNC();
  return iters;
}

// ------------------------------------------------------------------------------------------------ floor contacts
// mj: mj_collision for the pairs (floor plane, sphere / capsule of the fly): mjc_PlaneSphere at the sphere centre or at both ends of a
// capsule's segment (mjc_PlaneCapsule), in the root frame (walk_floor.hpp).  Lane g tests geom g of the floor table against the pose
// its link published; a contact inside the margin takes a slot in (geom, end) order.  More than NC: the NC deepest are kept.  `n` is
// the plane's normal in the root frame, `height` the root origin's distance from the plane (float64).  Returns contacts | overflow << 8.
// Out of line and a leaf.
__device__ __noinline__ int floor_collide(WTileF *Tp, const WalkExtra FFE_GLOBAL *Xp, const int lane, const float px, const float py, const float pz,
                                          const float qw, const float qx, const float qy, const float qz, const float w0, const float w1, const float w2,
                                          const float v0, const float v1, const float v2, const float nx, const float ny, const float nz, const double height) {
  WTileF &T = *Tp;
  const WalkExtra FFE_GLOBAL &X = *Xp;
  {
    float *o = T.lp[lane];
    o[0] = px; o[1] = py; o[2] = pz; o[3] = qw; o[4] = qx; o[5] = qy; o[6] = qz;
    o[7] = w0; o[8] = w1; o[9] = w2; o[10] = v0; o[11] = v1; o[12] = v2;
  }
  DM_SYNC();
  const float n[3] = {nx, ny, nz};
  bool h0 = false, h1 = false;
  float d0 = 0.f, d1 = 0.f, rad = 0.f, incl = 0.f, e0[3] = {0.f, 0.f, 0.f}, e1[3] = {0.f, 0.f, 0.f};
  int link = 0;
  if (lane < X.f_n) {
    link = X.f_link[lane];
    const float *lp = T.lp[link];
    const M3 R = q2m(Q4{lp[3], lp[4], lp[5], lp[6]});
    const V3 c = V3{lp[0], lp[1], lp[2]} + mv(R, V3{X.f_pos[0][lane], X.f_pos[1][lane], X.f_pos[2][lane]});
    const V3 a = mv(R, V3{X.f_axis[0][lane], X.f_axis[1][lane], X.f_axis[2][lane]});
    const float half = X.f_half[lane], margin = X.f_margin[lane];
    rad = X.f_rad[lane]; incl = margin - X.f_gap[lane];
    e0[0] = c.x + half * a.x; e0[1] = c.y + half * a.y; e0[2] = c.z + half * a.z;
    e1[0] = c.x - half * a.x; e1[1] = c.y - half * a.y; e1[2] = c.z - half * a.z;
    d0 = wf::plane_distance<float>(height, n, e0, rad);
    h0 = d0 <= margin;
    if (half > 0.f) {  // (a sphere gives one contact)
      d1 = wf::plane_distance<float>(height, n, e1, rad);
      h1 = d1 <= margin;
    }
  }
  unsigned long long b0 = __ballot(h0), b1 = __ballot(h1);
  int over = 0;
  if (__popcll(b0) + __popcll(b1) > NC) {
    // the NC deepest, ties by (lane, end): dropping a deep one lets the leg sink in until a later substep answers with an enormous force
    over = 1;
    int r0 = 0, r1 = 0;
    for (unsigned long long m = b0; m; m &= m - 1) {
      const int j = __ffsll((long long)m) - 1;
      const float dj = __shfl(d0, j);
      if (dj < d0 || (dj == d0 && j < lane)) r0++;
      if (dj < d1 || (dj == d1 && j <= lane)) r1++;
    }
    for (unsigned long long m = b1; m; m &= m - 1) {
      const int j = __ffsll((long long)m) - 1;
      const float dj = __shfl(d1, j);
      if (dj < d0 || (dj == d0 && j < lane)) r0++;
      if (dj < d1 || (dj == d1 && j < lane)) r1++;
    }
    h0 = h0 && r0 < NC; h1 = h1 && r1 < NC;
    b0 = __ballot(h0); b1 = __ballot(h1);
  }
  const unsigned long long lt = (1ull << lane) - 1ull;
  const int i0 = __popcll(b0 & lt) + __popcll(b1 & lt), i1 = i0 + (h0 ? 1 : 0);
#pragma unroll
  for (int e = 0; e < 2; e++) {
    const bool hit = e == 0 ? h0 : h1;
    const int idx = e == 0 ? i0 : i1;
    if (hit && idx < NC) {
      const float dist = e == 0 ? d0 : d1;
      float p[3], v[3];
      wf::contact_position<float>(e == 0 ? e0 : e1, n, rad, dist, p);
      wf::point_velocity<float>(&T.lp[link][7], p, v);
      T.c_pos[idx][0] = p[0]; T.c_pos[idx][1] = p[1]; T.c_pos[idx][2] = p[2];
      T.c_vel[idx][0] = v[0]; T.c_vel[idx][1] = v[1]; T.c_vel[idx][2] = v[2];
      T.c_dist[idx] = dist;
      T.c_excl[idx] = dist >= incl ? 1 : 0;  // inside the margin but not inside margin - gap: kept, exerts nothing
      T.c_geom[idx] = (unsigned char)lane; T.c_link[idx] = (unsigned char)link;
      T.c_blk[idx] = (unsigned char)X.f_blk[lane]; T.c_amask[idx] = (unsigned short)X.f_amask[lane];
    }
  }
  DM_SYNC();
  return min((int)(__popcll(b0) + __popcll(b1)), NC) | (over << 8);
}

// row r (0 normal, 1 / 2 tangents) of contact k on hinge f: e_r . (velocity of the contact point per unit rate of f)
__device__ __forceinline__ float fj_row(const WTileF &T, const float (&e)[3], int k, int f) { return wf::row_hinge<float>(T.C[f], T.c_pos[k], e); }
// sum over the contacts whose chain contains hinge f of sum_r J[k][r][f] w[3 k + r] (w: the rows' forces) or J[k][0][f] w[k] (NORMAL)
template <bool NORMAL>
__device__ __forceinline__ float floor_gather(const WTileF &T, const BallModel FFE_GLOBAL &M, const float (&fr)[9], int nc, int f, const float *w) {
  const int blk = M.d_blk[f], li = M.d_li[f];
  float acc = 0.f;
  for (int k = 0; k < nc; k++) {
    if ((int)T.c_blk[k] == blk && (((unsigned)T.c_amask[k] >> li) & 1u)) {
      float v[3];
      wf::point_velocity<float>(T.C[f], T.c_pos[k], v);
      if constexpr (NORMAL) acc += wf::dot3<float>(&fr[0], v) * w[k];
      else acc += wf::dot3<float>(&fr[0], v) * w[3 * k] + wf::dot3<float>(&fr[3], v) * w[3 * k + 1] + wf::dot3<float>(&fr[6], v) * w[3 * k + 2];
    }
  }
  return acc;
}

// the plane's frame (rows: normal, two tangents) in the root frame: uniform, recomputed where it is used rather than kept in registers
template <class C>
__device__ __forceinline__ void floor_frame(const C &c, float (&fr)[9]) {
  const WalkExtra FFE_GLOBAL &X = *c.X;
  Q4 q = c.rq;
  asm volatile("" : "+v"(q.w));  // (an opaque copy: a second call is a second evaluation, not nine registers kept from the first)
  const M3 Rr = q2m(q);
  const float Rm[9] = {Rr.m0, Rr.m1, Rr.m2, Rr.m3, Rr.m4, Rr.m5, Rr.m6, Rr.m7, Rr.m8};
  float fw[9];
#pragma unroll
  for (int k = 0; k < 9; k++) fw[k] = X.f_frame[k];
  wf::frame_in_root<float>(Rm, fw, fr);
}

// The solver stops at |grad| <= 1e-4 sqrt(scale2) (row_newton.hpp).  The free thorax turns on rotational inertias far smaller than anything
// the tethered fly moves, so the same relative force error shows up larger in the root's angular velocity: the floor solve stops ten
// times closer (with FFE_NO_NOSLIP, where no sweep polishes the tangential forces, the one-substep error of root_ang was 3.6e-4 at 1).
constexpr float kFloorScale = 1e-2f;

// ------------------------------------------------------------------------------------------------ the second floor pass
// (FFE_WALK_FLOOR_CONVEX)  mj: mj_collision for the pairs (floor plane, ellipsoid / cylinder of the fly):
// mjc_PlaneConvex and mjc_PlaneCylinder as walk_floor_convex.hpp restates them, in the root frame.  Lane g tests row g of WalkFloorConvex
// against the pose its link published in T.lp (`floor_collide` has run); a root geom's pose is the identity and it moves with the root's
// own (w_b, v_b) in T.sv0.  A row gives up to four contacts, each in a fixed register slot.  Kept contacts follow the `nprim` primitive
// floor contacts in (row, contact) order.  More than NC in all: the NC deepest floor contacts of both kinds are kept - ties go to the
// earlier slot, a primitive contact before any of this pass - and the primitive slots that remain are moved up, in order, through their
// lanes' registers.  Returns contacts of this pass | overflow << 8 | primitive contacts left << 16.  Out of line and a leaf.
template <class TileX>
__device__ __noinline__ int floor_convex_collide(TileX *Tp, const WalkFloorConvex FFE_GLOBAL *Fp, const int lane, const int nprim, const float nx, const float ny,
                                                 const float nz, const double height) {
  TileX &T = *Tp;
  const WalkFloorConvex FFE_GLOBAL &F = *Fp;
  DM_SYNC();  // (T.sv0 was written just before the call)
  const float n[3] = {nx, ny, nz};
  const float inf = __builtin_inff();
  float sp[4][3], dd[4] = {inf, inf, inf, inf}, incl = 0.f;
  int mask = 0, link = -1;
#pragma unroll
  for (int e = 0; e < 4; e++) sp[e][0] = sp[e][1] = sp[e][2] = 0.f;
  const int nrow = F.n;
  if (lane < nrow) {
    link = F.link[lane];
    Q4 q = {F.quat[0][lane], F.quat[1][lane], F.quat[2][lane], F.quat[3][lane]};
    V3 cv = {F.pos[0][lane], F.pos[1][lane], F.pos[2][lane]};
    if (link >= 0) {
      const float *lp = T.lp[link];
      const Q4 lq = {lp[3], lp[4], lp[5], lp[6]};
      cv = V3{lp[0], lp[1], lp[2]} + qrot(lq, cv);
      q = qnormalize(qmul(lq, q));
    }
    const M3 Rr = q2m(q);
    const float R[9] = {Rr.m0, Rr.m1, Rr.m2, Rr.m3, Rr.m4, Rr.m5, Rr.m6, Rr.m7, Rr.m8}, cc[3] = {cv.x, cv.y, cv.z};
    const float margin = F.margin[lane];
    incl = margin - F.gap[lane];
    if (F.type[lane] == 4) {
      const float s[3] = {F.size[0][lane], F.size[1][lane], F.size[2][lane]};
      wfc::ellipsoid_support<float>(n, cc, R, s, sp[0]);
      dd[0] = wf::plane_distance<float>(height, n, sp[0], 0.f);
      mask = dd[0] <= margin ? 1 : 0;
    } else {
      const float dist0 = wf::plane_distance<float>(height, n, cc, 0.f);
      mask = wfc::plane_cylinder<float>(n, cc, R, F.size[0][lane], F.size[1][lane], dist0, margin, sp, dd);
    }
    // inside the margin but not inside margin - gap: exerts nothing, kept only where an adhesion actuator counts it (as the fly-fly passes)
    const bool counted = F.adh[lane] >= 0;
#pragma unroll
    for (int e = 0; e < 4; e++) {
      if (dd[e] >= incl && !counted) mask &= ~(1 << e);
      if (!((mask >> e) & 1)) dd[e] = inf;
    }
  }
  unsigned long long be[4];
  int total = 0;
#pragma unroll
  for (int e = 0; e < 4; e++) { be[e] = __ballot((mask >> e) & 1); total += (int)__popcll(be[e]); }
  const unsigned long long lt = (1ull << lane) - 1ull;
  int np = nprim, over = 0;
  if (nprim + total > NC) {
    over = 1;
    // ranks over the union: key of primitive slot k = k, of (row g, contact e) = NC + 4 g + e
    const float dp = lane < nprim ? T.c_dist[lane] : inf;
    int rp = 0, r[4] = {0, 0, 0, 0};
    const int nj = max(nprim, nrow);
    for (int j = 0; j < nj; j++) {
      const float djp = __shfl(dp, j);
      if (djp < dp || (djp == dp && j < lane)) rp++;
#pragma unroll
      for (int e = 0; e < 4; e++) if (djp <= dd[e]) r[e]++;
#pragma unroll
      for (int e2 = 0; e2 < 4; e2++) {
        const float dj = __shfl(dd[e2], j);
        if (dj < dp) rp++;
#pragma unroll
        for (int e = 0; e < 4; e++) if (dj < dd[e] || (dj == dd[e] && (j < lane || (j == lane && e2 < e)))) r[e]++;
      }
    }
    // (an absent candidate is +inf: it beats nothing that is there, and its own rank is not read)
    const bool keep = lane < nprim && rp < NC;
#pragma unroll
    for (int e = 0; e < 4; e++) if (r[e] >= NC) mask &= ~(1 << e);
    const unsigned long long bk = __ballot(keep);
    np = (int)__popcll(bk);
    // move the primitive slots that stay: read, barrier, write
    float m_pos[3] = {0.f, 0.f, 0.f}, m_vel[3] = {0.f, 0.f, 0.f}, m_dist = 0.f;
    int m_excl = 0, m_geom = 0, m_link = 0, m_blk = 0, m_amask = 0;
    if (keep) {
#pragma unroll
      for (int k = 0; k < 3; k++) { m_pos[k] = T.c_pos[lane][k]; m_vel[k] = T.c_vel[lane][k]; }
      m_dist = T.c_dist[lane]; m_excl = T.c_excl[lane]; m_geom = T.c_geom[lane]; m_link = T.c_link[lane]; m_blk = T.c_blk[lane]; m_amask = T.c_amask[lane];
    }
    DM_SYNC();
    if (keep) {
      const int at = (int)__popcll(bk & lt);
#pragma unroll
      for (int k = 0; k < 3; k++) { T.c_pos[at][k] = m_pos[k]; T.c_vel[at][k] = m_vel[k]; }
      T.c_dist[at] = m_dist; T.c_excl[at] = (unsigned char)m_excl; T.c_geom[at] = (unsigned char)m_geom; T.c_link[at] = (unsigned char)m_link;
      T.c_blk[at] = (unsigned char)m_blk; T.c_amask[at] = (unsigned short)m_amask;
    }
    total = 0;
#pragma unroll
    for (int e = 0; e < 4; e++) { be[e] = __ballot((mask >> e) & 1); total += (int)__popcll(be[e]); }
  }
  int idx = np;
#pragma unroll
  for (int e = 0; e < 4; e++) idx += (int)__popcll(be[e] & lt);
#pragma unroll
  for (int e = 0; e < 4; e++) {
    if ((mask >> e) & 1) {
      if (idx < NC) {
        const float dist = dd[e];
        float p[3], v[3];
        wf::contact_position<float>(sp[e], n, 0.f, dist, p);
        wf::point_velocity<float>(link >= 0 ? &T.lp[link][7] : T.sv0, p, v);
        T.c_pos[idx][0] = p[0]; T.c_pos[idx][1] = p[1]; T.c_pos[idx][2] = p[2];
        T.c_vel[idx][0] = v[0]; T.c_vel[idx][1] = v[1]; T.c_vel[idx][2] = v[2];
        T.c_dist[idx] = dist;
        T.c_excl[idx] = dist >= incl ? 1 : 0;
        T.c_geom[idx] = (unsigned char)(NPG + lane);
        T.c_link[idx] = (unsigned char)(link >= 0 ? link : 255);
        T.c_blk[idx] = (unsigned char)F.blk[lane]; T.c_amask[idx] = (unsigned short)F.amask[lane];
      }
      idx++;
    }
  }
  DM_SYNC();
  return min(total, NC - np) | (over << 8) | (np << 16);
}

// ------------------------------------------------------------------------------------------------ the fly's own contacts
// (FFE_WALK_SELF)  The two collision passes of self_pairs.hpp on the walker's tile, in the root frame: the
// geoms' frames come from the link poses `floor_collide` has published (T.lp), the narrow phase of the convex pairs is cvx:: of
// convex.hpp as it is.  Both run after `floor_collide`, whose contacts keep the first slots; the fly-fly contacts follow.
// Templates on the tile so that only the kernel that calls them instantiates them.
//
// Stores fly-fly contact `at`: geom1 on link l1, geom2 on link l2 (-1: the thorax), normal n from geom1 to geom2.  A pair whose geom2
// is the thorax's is stored the other way round with the normal turned, so that c_link always names a link with a chain.
template <class TileX>
__device__ __forceinline__ void self_put(TileX &T, const BallModel FFE_GLOBAL &M, const int at, const int l1, const int l2, V3 n, const V3 p, const float dist,
                                         const float margin, const float invw) {
  const float incl = margin - (margin != 0.f ? M.sc_gap : 0.f);
  int lpos = l2, lneg = l1;
  if (lpos < 0) { lpos = l1; lneg = -1; n = V3{-n.x, -n.y, -n.z}; }
  const float pp[3] = {p.x, p.y, p.z}, nn[3] = {n.x, n.y, n.z};
  const float vel = wsf::row_velocity<float>(&T.lp[lpos][7], lneg >= 0 ? &T.lp[lneg][7] : T.sv0, pp, nn);
  float si_[5];
#pragma unroll
  for (int q2 = 0; q2 < 5; q2++) si_[q2] = M.sc_solimp[q2];
  const float imp = impedance(si_, fabsf(dist - incl));
  const bool excl = dist >= incl;  // inside the margin but not inside margin - gap: kept (an adhesion actuator counts it), exerts nothing
  T.c_pos[at][0] = p.x; T.c_pos[at][1] = p.y; T.c_pos[at][2] = p.z;
  if constexpr (!TileX::kPackedNormal) { T.c_nrm[at][0] = n.x; T.c_nrm[at][1] = n.y; T.c_nrm[at][2] = n.z; }
  T.c_dist[at] = dist; T.c_excl[at] = excl ? 1 : 0;
  T.c_D[at] = excl ? 0.f : wsf::row_D<float>(imp, invw);
  T.c_vel[at][0] = wsf::row_neg_aref<float>(M.sc_K, M.sc_B, imp, dist, incl, vel);
  if constexpr (TileX::kPackedNormal) { T.c_vel[at][1] = n.x; T.c_vel[at][2] = n.y; T.c_mu[at] = n.z; }  // (the floats such a slot leaves unused)
  else { T.c_vel[at][1] = 0.f; T.c_vel[at][2] = 0.f; T.c_mu[at] = 0.f; }
  T.c_geom[at] = 0;
  const int fp = M.l_chain[M.l_nchain[lpos] - 1][lpos];
  T.c_link[at] = (unsigned char)lpos; T.c_blk[at] = (unsigned char)M.d_blk[fp]; T.c_amask[at] = (unsigned short)M.d_amask[fp];
  if (lneg >= 0) {
    const int fn = M.l_chain[M.l_nchain[lneg] - 1][lneg];
    T.c_link1[at] = (unsigned char)lneg; T.c_blk1[at] = (unsigned char)M.d_blk[fn]; T.c_amask1[at] = (unsigned short)M.d_amask[fn];
  } else { T.c_link1[at] = 255; T.c_blk1[at] = 255; T.c_amask1[at] = 0; }
}

// self_pairs.hpp on a walker's tile: the primitive geom slots and, after them, the geom centres and the pair lists in T.X4, the slots' radii
// behind the link poses in T.G; a geom's orientation from its link's pose; no separating direction is remembered from substep to
// substep (a launch's result is a function of its state alone, the narrow phase always starts cold); a full pair list has its own bit.
template <class TileX>
struct WalkPairs {
  static constexpr bool kSyncAtEnd = true, kHistory = false;
  static constexpr int kFullBit = 9;
  static __device__ __forceinline__ float4 *slots(TileX &T) { return &T.X4[0]; }
  static __device__ __forceinline__ float *radii(TileX &T) { return &T.G[NL * 14]; }
  static __device__ __forceinline__ float4 *centres(TileX &T) { return &T.X4[0]; }
  static __device__ __forceinline__ const float4 *centres(const TileX &T) { return &T.X4[0]; }
  static __device__ __forceinline__ unsigned short *cl1(TileX &T) { return reinterpret_cast<unsigned short *>(&T.X4[0] + NG); }
  static __device__ __forceinline__ unsigned short *cl2(TileX &T) { return cl1(T) + ((CL1 + 7) / 8) * 8; }
  static __device__ __forceinline__ Q4 quat(const TileX &T, const BallModel FFE_GLOBAL &M, const int g) {
    Q4 q = {M.cg_quat[0][g], M.cg_quat[1][g], M.cg_quat[2][g], M.cg_quat[3][g]};
    const int l = M.cg_link[g];
    if (l >= 0) { const float *lp = T.lp[l]; q = qnormalize(qmul(Q4{lp[3], lp[4], lp[5], lp[6]}, q)); }
    return q;
  }
  static __device__ __forceinline__ void put(TileX &T, const BallModel FFE_GLOBAL &M, int at, int l1, int l2, int, V3 n, V3 p, float dist, float margin, float invw) {
    self_put(T, M, at, l1, l2, n, p, dist, margin, invw);
  }
  const WalkExtra FFE_GLOBAL *Xp;
  // lane s makes slot s from the floor table's geom s (the same 48 geoms)
  __device__ __forceinline__ void fill_slots(TileX &T, const int lane) const {
    const WalkExtra FFE_GLOBAL &X = *Xp;
    if (lane < NPG) {
      const float *lp = T.lp[X.f_link[lane]];
      const M3 R = q2m(Q4{lp[3], lp[4], lp[5], lp[6]});
      const V3 gc = V3{lp[0], lp[1], lp[2]} + mv(R, V3{X.f_pos[0][lane], X.f_pos[1][lane], X.f_pos[2][lane]});
      const V3 ga = mv(R, V3{X.f_axis[0][lane], X.f_axis[1][lane], X.f_axis[2][lane]});
      const float half = X.f_half[lane], rad = X.f_rad[lane];
      slots(T)[lane] = make_float4(gc.x, gc.y, gc.z, half + rad);
      slots(T)[NPG + lane] = make_float4(ga.x, ga.y, ga.z, half);
      radii(T)[lane] = rad;
    }
    DM_SYNC();
  }
  // the geoms' centres in the root frame
  static __device__ __forceinline__ void fill_centres(TileX &T, const BallModel FFE_GLOBAL &M, const int lane) {
    const int ncg = M.ncg;
    for (int g = lane; g < ncg; g += 64) {
      const int l = M.cg_link[g];
      V3 gp = {M.cg_pos[0][g], M.cg_pos[1][g], M.cg_pos[2][g]};
      if (l >= 0) { const float *lp = T.lp[l]; gp = V3{lp[0], lp[1], lp[2]} + qrot(Q4{lp[3], lp[4], lp[5], lp[6]}, gp); }
      centres(T)[g] = make_float4(gp.x, gp.y, gp.z, M.cg_brad[g]);
    }
    DM_SYNC();
  }
};


// sum over the fly-fly contacts whose row touches hinge f of J[k][f] w[k - nc] (w: the rows' forces or the adhesion pulls)
template <class TileX>
__device__ __forceinline__ float self_gather(const TileX &T, const BallModel FFE_GLOBAL &M, const int nc, const int ns, const int f, const float *w) {
  const int blk = M.d_blk[f], li = M.d_li[f];
  float acc = 0.f;
  for (int j = 0; j < ns; j++) {
    const int k = nc + j;
    const bool on_pos = (int)T.c_blk[k] == blk && (((unsigned)T.c_amask[k] >> li) & 1u);
    const bool on_neg = (int)T.c_blk1[k] == blk && (((unsigned)T.c_amask1[k] >> li) & 1u);
    if (on_pos != on_neg) {
      if constexpr (TileX::kPackedNormal) { float n[3]; self_nrm(T, k, n); acc += wsf::row_hinge<float>(T.C[f], T.c_pos[k], n, on_pos, on_neg) * w[j]; }
      else acc += wsf::row_hinge<float>(T.C[f], T.c_pos[k], T.c_nrm[k], on_pos, on_neg) * w[j];
    }
  }
  return acc;
}

// ------------------------------------------------------------------------------------------------ the contact block
// The constraint block of a floor substep with R > 0 rows: 3 per floor contact (rows 0 .. 3 nc - 1: the cone blocks come first), on a
// self tile one normal row per fly-fly contact, then the instantiated joint limits (already in T.r_sgn / r_D / r_dof / r_blk, -aref in
// T.r_y0; the oracle lists limits first and the contacts in pair order: the solution of the convex problem does not depend on the order
// of its rows).  ball_env.hip's stage 2 with the ball's rank-3 term replaced by the root's rank-6 term:
//   G = J_j M_jj^-1 J_j' + w S_m^-1 w',  w = J_r - J_j Y_m  (J_r = (p x e, e) on a floor row, 0 on a fly-fly or a limit row)
// and the three root terms a limit row never needed: the adhesion pull enters the smooth force of hinges and root before y0 is formed;
// y0 carries the root's share of J qacc_smooth with w_b x v_b and gravity added by hand (they are outside the arrowhead solve);
// J_r' f joins the root's right-hand side of the Euler solve (T.rootf) and J_j' f the hinges' (qs).
// Everything a fly-fly row adds sits under SELF.  It is a scalar row of the solver, like a limit row, over the hinges of two chains
// (walk_self.hpp) with no entry on the root: w = -J_j Y_m in the rank-6 term, no w_b x v_b / gravity term in y0, nothing on the root's
// right-hand side.  Its two chains may lie in two blocks of M: it then owns a column in each.  The adhesion pull of a body is the mean
// over all of its contacts, fly-fly ones included (mjTRN_BODY).  Where the two kinds of tile form the same number in two ways (seeding a
// column of G, y0, the hinges' gather), each keeps its own: the ways differ in the sign of a zero, and the floor tiles' single chain loop
// with a single accumulator is what holds the floor kernels' register figures.  Returns the solver's iterations.
template <class C>
__device__ __forceinline__ int contact_forces(C &c, const int R, const int (&lrow)[3], const float (&lsgn)[3], float (&qs)[3]) {
  using Tile = std::remove_pointer_t<decltype(c.T)>;
  constexpr bool SELF = Tile::kSelf;
  std::conditional_t<SELF, Tile, WTileF> &T = *c.T;  // (WTileX, or the environment's WTileSX; the floor tiles through their base)
  const BallModel FFE_GLOBAL &M = model(c);
  const WalkExtra FFE_GLOBAL &X = *c.X;
  const int lane = c.lane, nc = c.fl.nc, nrc = 3 * nc;
  const int ns = self_count(c.fl), nrs = nrc + ns, ncs = nc + ns;
  const bool row = lane < R, crow = lane < nrc, srow = SELF && lane >= nrc && lane < nrs, jrow = SELF ? lane < nrs : crow;
  float er[3] = {0.f, 0.f, 0.f};  // this row's direction: a floor row's normal or tangent, a fly-fly row's normal
  // contacts of link `l`: of a fly-fly contact on either side
  auto contacts_of = [&](int l) {
    int n = 0;
    if constexpr (SELF) { for (int j = 0; j < ncs; j++) n += ((int)T.c_link[j] == l || (int)T.c_link1[j] == l) ? 1 : 0; }
    else { for (int j = 0; j < nc; j++) n += T.c_link[j] == l ? 1 : 0; }
    return n;
  };
  {
  float fr[9];
  floor_frame(c, fr);
  if (crow) { const int r3 = 3 * (lane - 3 * (lane / 3)); er[0] = fr[r3]; er[1] = fr[r3 + 1]; er[2] = fr[r3 + 2]; }
  if constexpr (SELF) { if (srow) self_nrm(T, nc + lane - nrc, er); }
  // ---- per floor contact: impedance, D, friction, -aref on its three rows, and the adhesion pull (mj: mj_transmission mjTRN_BODY: -force
  //      along the normal row, the mean over the body's contacts, the ones inside the gap included)
  if constexpr (Tile::kConvexFloor) {
    // c_geom runs over both floor tables: 0 .. NPG - 1 the rows of X.f_*, NPG + row those of the second pass's table
    if (lane < nc) {
      const WalkFloorConvex FFE_GLOBAL &F = *convex_table(c.X);
      const int g = T.c_geom[lane], gc = g - NPG;
      const bool cv = gc >= 0;
      const float dist = T.c_dist[lane], incl = cv ? F.margin[gc] - F.gap[gc] : X.f_margin[g] - X.f_gap[g];
      float si_[5];
#pragma unroll
      for (int q2 = 0; q2 < 5; q2++) si_[q2] = X.f_solimp[q2];
      const float imp = impedance(si_, fabsf(dist - incl));
      const float R0 = fmaxf(1e-15f, (1.f - imp) * (cv ? F.invw[gc] : X.f_invw[g]) * frcp(imp));
      T.c_D[lane] = T.c_excl[lane] ? 0.f : frcp(R0);
      T.c_mu[lane] = cv ? F.fric[gc] : X.f_fric[g];
      const float B = cv ? F.B[gc] : X.f_B[g], K = cv ? F.K[gc] : X.f_K[g];
      T.r_y0[3 * lane] = B * wf::dot3<float>(&fr[0], T.c_vel[lane]) + K * imp * (dist - incl);
      T.r_y0[3 * lane + 1] = B * wf::dot3<float>(&fr[3], T.c_vel[lane]);
      T.r_y0[3 * lane + 2] = B * wf::dot3<float>(&fr[6], T.c_vel[lane]);
      const int adh = cv ? F.adh[gc] : X.f_adh[g];
      const int cnt = adh >= 0 ? contacts_of(T.c_link[lane]) : 1;  // (a root geom has no link and no actuator)
      T.c_w[lane] = adh >= 0 ? -T.frc[adh] / (float)cnt : 0.f;
    }
  } else if (lane < nc) {
    const int g = T.c_geom[lane];
    const float dist = T.c_dist[lane], incl = X.f_margin[g] - X.f_gap[g];
    float si_[5];
#pragma unroll
    for (int q2 = 0; q2 < 5; q2++) si_[q2] = X.f_solimp[q2];
    const float imp = impedance(si_, fabsf(dist - incl));
    const float R0 = fmaxf(1e-15f, (1.f - imp) * X.f_invw[g] * frcp(imp));
    T.c_D[lane] = T.c_excl[lane] ? 0.f : frcp(R0);
    T.c_mu[lane] = X.f_fric[g];
    const float B = X.f_B[g], K = X.f_K[g];
    T.r_y0[3 * lane] = B * wf::dot3<float>(&fr[0], T.c_vel[lane]) + K * imp * (dist - incl);
    T.r_y0[3 * lane + 1] = B * wf::dot3<float>(&fr[3], T.c_vel[lane]);
    T.r_y0[3 * lane + 2] = B * wf::dot3<float>(&fr[6], T.c_vel[lane]);
    const int adh = X.f_adh[g];
    const int cnt = contacts_of(T.c_link[lane]);
    T.c_w[lane] = adh >= 0 ? -T.frc[adh] / (float)cnt : 0.f;
  }
  if constexpr (SELF) {
    if (lane >= nc && lane < ncs) {  // a fly-fly contact: D and -aref are the collision pass's; the pull of both bodies' adhesion actuators
      const int ri = nrc + lane - nc, lp_ = T.c_link[lane], ln_ = T.c_link1[lane];
      T.r_y0[ri] = T.c_vel[lane][0]; T.r_D[ri] = T.c_D[lane]; T.r_sgn[ri] = 0.f; T.r_dof[ri] = 0;
      float w = 0.f;
      const int ap = M.l_adh[lp_], an = ln_ != 255 ? M.l_adh[ln_] : -1;
      if (ap >= 0) w -= T.frc[ap] / (float)contacts_of(lp_);
      if (an >= 0) w -= T.frc[an] / (float)contacts_of(ln_);
      T.c_w[lane] = w;
    }
  }
  if (lane < RMAX) T.r_lam[lane] = 0.f;  // no warm start: a substep's result depends on its state alone
  if (crow) T.r_blk[lane] = T.c_blk[lane / 3];
  if (srow) T.r_blk[lane] = T.c_blk[nc + lane - nrc];
  for (int k = lane; k < NBLK * KCOL; k += 64) (&T.rowof[0][0])[k] = 255;
  DM_SYNC();
  // ---- adhesion into the smooth forces of the hinges and of the root (a fly-fly row has no entry on the root)
  {
    float fa[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int k = 0; k < nc; k++) {
      float jr[6];
      wf::row_root<float>(T.c_pos[k], &fr[0], jr);
#pragma unroll
      for (int a = 0; a < 6; a++) fa[a] += jr[a] * T.c_w[k];
    }
    if (lane == 0) {
#pragma unroll
      for (int a = 0; a < 6; a++) T.rootf[a] = fa[a];
    }
  }
#pragma unroll
  for (int s = 0; s < 3; s++) {
    if (slot_on(c, s)) {
      if constexpr (SELF) qs[s] += floor_gather<true>(T, M, fr, nc, opq(c.sdof[s]), T.c_w) + self_gather(T, M, nc, ns, opq(c.sdof[s]), &T.c_w[nc]);
      else qs[s] += floor_gather<true>(T, M, fr, nc, opq(c.sdof[s]), T.c_w);
    }
  }
  }
  // ---- columns: a row's column is its rank among the rows of its block; a fly-fly row whose chains sit in two blocks takes a column
  //      in each (ball_env.hip).  More than KCOL rows in a block: flagged, the rows without a column are switched off for this substep
  const int myb = row ? (int)T.r_blk[lane] : -1;
  int myb2 = -1;
  if constexpr (SELF) { if (srow) { const int b1 = T.c_blk1[nc + lane - nrc]; if (b1 != 255 && b1 != myb) myb2 = b1; } }
  int ncol, mycol2 = 0;
  {
    int mycol = 0;
    for (int b = 0; b < NBLK; b++) {
      const unsigned long long mb = __ballot(myb == b || (SELF && myb2 == b));
      if (myb == b) mycol = __popcll(mb & ((1ull << lane) - 1ull));
      if constexpr (SELF) { if (myb2 == b) mycol2 = __popcll(mb & ((1ull << lane) - 1ull)); }
    }
    if (row) {
      T.r_col[lane] = (unsigned char)mycol;
      // (a row of a root geom's contact - block 255 - has no hinge entry: no column, and it asks for no block solve)
      if (mycol < KCOL && (!Tile::kConvexFloor || myb != 255)) T.rowof[myb][mycol] = (unsigned char)lane;
      if constexpr (SELF) {
        if (myb2 >= 0 && mycol2 < KCOL) T.rowof[myb2][mycol2] = (unsigned char)lane;
        if (myb2 < 0) mycol2 = mycol;
        if (srow) T.c_col1[nc + lane - nrc] = (unsigned char)mycol2;
        mycol = max(mycol, mycol2) + 1;
        if constexpr (Tile::kConvexFloor) { if (myb == 255) mycol = 0; }
      } else {
        mycol += 1;
      }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) mycol = max(mycol, __shfl_xor(mycol, off));
    ncol = min(mycol, KCOL);
    if (mycol > KCOL) {
      c.overflow |= 4;
      DM_SYNC();
      if (row && ((int)T.r_col[lane] >= KCOL || (SELF && mycol2 >= KCOL))) { if (crow) T.c_excl[lane / 3] = 1; else T.r_D[lane] = 0.f; }
      DM_SYNC();
      if (lane < nc && T.c_excl[lane]) T.c_D[lane] = 0.f;
    }
  }
  DM_SYNC();
  const int mycol = row ? (int)T.r_col[lane] : 0;
  // this row: its contact, the link whose chain it spans (a fly-fly row: the links of geom2 and geom1), a limit row's hinge
  const int ck = crow ? lane / 3 : (srow ? nc + lane - nrc : 0);
  bool rootrow = false;  // a row of a root geom's contact: no chain, the root entries alone
  if constexpr (Tile::kConvexFloor) rootrow = crow && T.c_link[ck] == 255;
  const int lpos = (jrow && !rootrow) ? (int)T.c_link[ck] : 0, npos = (jrow && !rootrow) ? M.l_nchain[lpos] : 0;
  int lneg = 255, nneg = 0;
  if constexpr (SELF) { lneg = jrow ? (int)T.c_link1[ck] : 255; nneg = lneg != 255 ? M.l_nchain[lneg] : 0; }
  const int rdof = (row && !jrow) ? (int)T.r_dof[lane] : 0;
  const float sg = (row && !jrow) ? T.r_sgn[lane] : 0.f;
  // fn(hinge, J entry, 0 = geom2's chain / 1 = geom1's): a hinge on both chains is visited twice and the entries cancel
  auto each = [&](auto &&fn) {
    for (int p = 0; p < npos; p++) { const int f = M.l_chain[p][lpos]; fn(f, fj_row(T, er, ck, f), 0); }
    if constexpr (SELF) { for (int p = 0; p < nneg; p++) { const int f = M.l_chain[p][lneg]; fn(f, -fj_row(T, er, ck, f), 1); } }
  };
  // ---- z_m = M_jj^-1 f_j and Y_m = M_jj^-1 M_jr through M's own factor; a row lane keeps J_j z_m and J_j Y_m of its row
  S6 ym[3];
  float zm[3], jz = 0.f, jy[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  solve_zy(c, T.Lm, T.dinv_m, qs, T.F, zm, ym, [&](int half) {
    if (half == 0) {
      if (jrow) each([&](int f, float jv, int) { const float4 x = T.X4[f]; jz += jv * x.x; jy[0] += jv * x.y; jy[1] += jv * x.z; jy[2] += jv * x.w; });
      else if (row) { const float4 x = T.X4[rdof]; jz = sg * x.x; jy[0] = sg * x.y; jy[1] = sg * x.z; jy[2] = sg * x.w; }
    } else {
      if (jrow) each([&](int f, float jv, int) { const float4 x = T.X4[f]; jy[3] += jv * x.x; jy[4] += jv * x.y; jy[5] += jv * x.z; });
      else if (row) { const float4 x = T.X4[rdof]; jy[3] = sg * x.x; jy[4] = sg * x.y; jy[5] = sg * x.z; }
    }
  });
  // ---- S_m = L L', x_r = S_m^-1 (b_r + adhesion - M_rj z_m); qfrc_smooth . qacc_smooth for the solver's stopping test
  float Sm[6][6], br[6], id[6], xr[6];
  {
    S6 m6[3];
#pragma unroll
    for (int s = 0; s < 3; s++) m6[s] = slot_on(c, s) ? ld6(T.F[opq(c.sdof[s])]) : zero6();
    schur(c, m6, ym, zm, Sm, br);
  }
#pragma unroll
  for (int k = 0; k < 6; k++) br[k] += T.rootf[k];
  chol6(Sm, id);
  chol6_forward(Sm, id, br, xr);
  chol6_backward(Sm, id, xr);
  float sq = 0.f;
#pragma unroll
  for (int s = 0; s < 3; s++) {
    if (slot_on(c, s)) {
      float a = zm[s];
#pragma unroll
      for (int k = 0; k < 6; k++) a -= comp(ym[s], k) * xr[k];
      sq += qs[s] * a;
    }
  }
  float scale2 = wave_sum(sq);
#pragma unroll
  for (int k = 0; k < 6; k++) scale2 += br[k] * xr[k];
  scale2 *= kFloorScale;
  // ---- y0 = J qacc_smooth - aref: the hinges' share J_j (z_m - Y_m x_r); a floor row adds the root's share with w_b x v_b and gravity by
  //      hand, a fly-fly row has none
  if (row) {
    float y;
    if constexpr (SELF) y = wsf::row_y0<float>(jz, jy, xr, 0.f);
    else {
      y = jz;
#pragma unroll
      for (int k = 0; k < 6; k++) y -= jy[k] * xr[k];
    }
    if (crow) {
      const M3 Rr = q2m(c.rq);
      const V3 g3 = (c.flags & BF_NO_GRAVITY) ? V3{0.f, 0.f, 0.f} : mtv(Rr, V3{0.f, 0.f, M.gz});
      const float wb[3] = {c.V0.a0, c.V0.a1, c.V0.a2}, vb[3] = {c.V0.l0, c.V0.l1, c.V0.l2}, gb[3] = {g3.x, g3.y, g3.z};
      float jr[6];
      wf::row_root<float>(T.c_pos[ck], er, jr);
      y += wf::root_y0<float>(jr, xr, wb, vb, gb);
    }
    T.r_y0[lane] += y;
  }
  // ---- the rank-6 part of G: u = L^-1 (J_r - J_j Y_m), G_ik = u_i . u_k
  const int gtri = lane * (lane + 1) / 2;  // G is symmetric: row `lane` keeps its columns r2 <= lane
  {
    float u[6], jr[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (crow) wf::row_root<float>(T.c_pos[ck], er, jr);
    wf::rank6_factor<float>(Sm, id, jr, jy, u);
    for (int r2 = 0; r2 < R; r2++) {
      float gv = 0.f;
#pragma unroll
      for (int k = 0; k < 6; k++) gv += u[k] * rl_f(u[k], r2);
      if (row && r2 <= lane) T.G[gtri + r2] = gv;
    }
  }
  // ---- the block part J_j M_jj^-1 J_j': four columns per block solve, rows of different blocks sharing a column
  auto g_add = [&](const float4 &acc, const int b, const int cb) {
#pragma unroll
    for (int q2 = 0; q2 < 4; q2++) {
      const float av = q2 == 0 ? acc.x : (q2 == 1 ? acc.y : (q2 == 2 ? acc.z : acc.w));
      const int r2 = cb + q2 < KCOL ? (int)T.rowof[b][cb + q2] : 255;
      if (r2 <= lane) T.G[gtri + r2] += av;  // (255 = no such row)
    }
  };
#pragma unroll 1
  for (int cb = 0; cb < ncol; cb += 4) {
    for (int f = lane; f < ND; f += 64) T.X4[f] = make_float4(0.f, 0.f, 0.f, 0.f);
    DM_SYNC();
    if constexpr (SELF) {  // two chains, two columns and two accumulators: one of each per block the row has entries in
      if (jrow) {
        each([&](int f, float jv, int half) {
          const int col = (half == 0 ? mycol : mycol2) - cb;
          if (col >= 0 && col < 4) (&T.X4[f].x)[col] += jv;  // (its own lane alone writes this column of this block)
        });
      } else if (row) {
        const int col = mycol - cb;
        if (col >= 0 && col < 4) (&T.X4[rdof].x)[col] = sg;
      }
      DM_SYNC();
      solve4(c, T.Lm, T.dinv_m);
      if (jrow) {
        float4 a0 = make_float4(0.f, 0.f, 0.f, 0.f), a1 = make_float4(0.f, 0.f, 0.f, 0.f);
        each([&](int f, float jv, int half) {
          const float4 y = T.X4[f];
          if (half == 0) { a0.x += jv * y.x; a0.y += jv * y.y; a0.z += jv * y.z; a0.w += jv * y.w; }
          else { a1.x += jv * y.x; a1.y += jv * y.y; a1.z += jv * y.z; a1.w += jv * y.w; }
        });
        if (!rootrow) g_add(a0, myb, cb);
        if (nneg) g_add(a1, myb2 >= 0 ? myb2 : myb, cb);
      } else if (row) {
        const float4 y = T.X4[rdof];
        g_add(make_float4(sg * y.x, sg * y.y, sg * y.z, sg * y.w), myb, cb);
      }
    } else {  // one chain: the column is stored, not added, and one accumulator takes it back
      {
        const int col = mycol - cb;
        if (row && col >= 0 && col < 4) {
          if (crow) { for (int p = 0; p < npos; p++) { const int f = M.l_chain[p][lpos]; (&T.X4[f].x)[col] = fj_row(T, er, ck, f); } }
          else (&T.X4[rdof].x)[col] = sg;
        }
      }
      DM_SYNC();
      solve4(c, T.Lm, T.dinv_m);
      if (row) {
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        if (crow) {
          for (int p = 0; p < npos; p++) {
            const int f = M.l_chain[p][lpos];
            const float jv = fj_row(T, er, ck, f);
            const float4 y = T.X4[f];
            acc.x += jv * y.x; acc.y += jv * y.y; acc.z += jv * y.z; acc.w += jv * y.w;
          }
        } else { const float4 y = T.X4[rdof]; acc = make_float4(sg * y.x, sg * y.y, sg * y.z, sg * y.w); }
#pragma unroll
        for (int q2 = 0; q2 < 4; q2++) {
          const float av = q2 == 0 ? acc.x : (q2 == 1 ? acc.y : (q2 == 2 ? acc.z : acc.w));
          const int r2 = cb + q2 < KCOL ? (int)T.rowof[myb][cb + q2] : 255;
          if (r2 <= lane) T.G[gtri + r2] += av;  // (255 = no such row)
        }
      }
    }
    DM_SYNC();
  }
  // ---- solve: floor cone blocks first, the scalar rows (fly-fly, limits) after them, the model's noslip sweeps (with the fly's own
  //      contacts under the revert test of ConeRowsResidual: on them ConeRows' test flipped by rounding, row_newton.hpp)
  using Rows = std::conditional_t<SELF, ConeRowsResidual, ConeRows>;
  int nact = 0;
  for (int k = 0; k < nc; k++) nact += T.c_excl[k] ? 0 : 1;
  const int nslip = (nact > 0 && !(c.flags & BF_NO_NOSLIP)) ? M.noslip_iterations : 0;
  ModelPtr mp_ = (ModelPtr)c.M;
  int iters;
  if (R <= 12) iters = row_newton<12, Rows>(c.T, mp_, lane, R, nrc, scale2, nslip, 0);
  else if (R <= 18) iters = row_newton<18, Rows>(c.T, mp_, lane, R, nrc, scale2, nslip, 0);
  else if (R <= 24) iters = row_newton<24, Rows>(c.T, mp_, lane, R, nrc, scale2, nslip, 0);
  else if (R <= 32) iters = row_newton<32, Rows>(c.T, mp_, lane, R, nrc, scale2, nslip, 0);
  else iters = row_newton<RMAX, Rows>(c.T, mp_, lane, R, nrc, scale2, nslip, 0);
  // ---- qfrc_constraint: J_j' f on the hinges, J_r' f (floor rows alone, and the adhesion pull) on the root
  float fr[9];
  floor_frame(c, fr);
  {
    float fsum = 0.f, fa[6];
#pragma unroll
    for (int a = 0; a < 6; a++) fa[a] = T.rootf[a];
    for (int k = 0; k < nc; k++) {
      fsum += T.r_f[3 * k];
#pragma unroll
      for (int r = 0; r < 3; r++) {
        float j6[6];
        wf::row_root<float>(T.c_pos[k], &fr[3 * r], j6);
        const float f = T.r_f[3 * k + r];
#pragma unroll
        for (int a = 0; a < 6; a++) fa[a] += j6[a] * f;
      }
    }
    DM_SYNC();
    if (lane == 0) {
#pragma unroll
      for (int a = 0; a < 6; a++) T.rootf[a] = fa[a];
      T.rootf[6] = fsum;
    }
  }
#pragma unroll
  for (int s = 0; s < 3; s++) {
    if (slot_on(c, s)) {
      if constexpr (SELF) qs[s] += floor_gather<false>(T, M, fr, nc, opq(c.sdof[s]), T.r_f) + self_gather(T, M, nc, ns, opq(c.sdof[s]), &T.r_f[nrc]);
      else qs[s] += floor_gather<false>(T, M, fr, nc, opq(c.sdof[s]), T.r_f);
    }
    if (lrow[s] >= 0) qs[s] += lsgn[s] * T.r_f[lrow[s]];
  }
  DM_SYNC();
  return iters;
}

// ------------------------------------------------------------------------------------------------ force and touch
// mj: mj_rnePostConstraint + mj_sensorAcc for the force and touch sensors, on the free root (walk_sense.hpp): called from the
// acceleration stage with this substep's qacc (the hinges' in T.X4[.].x; `xr`: the root rows of the arrowhead solve, gravity not yet
// added) and contact forces (T.r_f), the state still the one before the integration.  Adds into T.sens[9 .. 32].  The link values go
// through T.lp, which is dead once the solver has returned.  On a tile that also holds the fly's own contacts (slots nc .. nc + ns - 1,
// their forces in T.r_f[3 nc + j]; `ns` is an int there and takes no register otherwise) a fly-fly contact pushes the link of geom2 along
// its normal and the link of geom1 against it (walk_self_sense.hpp); a slot inside the gap has a row with D = 0 and a zero force.  Out of
// line and a leaf.
template <class Tile>
__device__ __noinline__ void contact_sense(Tile *Tp, const BallModel FFE_GLOBAL *Mp, const WalkExtra FFE_GLOBAL *Xp, const int lane, const int nc,
                                           const std::conditional_t<Tile::kSelf, int, NoSelf> ns, const float xr0, const float xr1, const float xr2,
                                           const float xr3, const float xr4, const float xr5, const float qw, const float qx, const float qy, const float qz) {
  Tile &T = *Tp;
  const BallModel FFE_GLOBAL &M = *Mp;
  const WalkExtra FFE_GLOBAL &X = *Xp;
  const unsigned lpack = M.l_pack[lane], tree = M.l_tree[lane];
  const int parent = (int)(lpack & 0xffu) - 1, ndof = (int)((lpack >> 12) & 0x3u);
  const int sub = (int)(tree & 0xffu), anc2 = (int)((tree >> 8) & 0xffu) - 1, anc4 = (int)((tree >> 16) & 0xffu) - 1;
  float fext[3] = {0.f, 0.f, 0.f}, touch = 0.f;
  if (nc > 0) {
    const M3 Rr = q2m(Q4{qw, qx, qy, qz});
    const float Rm[9] = {Rr.m0, Rr.m1, Rr.m2, Rr.m3, Rr.m4, Rr.m5, Rr.m6, Rr.m7, Rr.m8};
    float fw[9], fr[9];
#pragma unroll
    for (int k = 0; k < 9; k++) fw[k] = X.f_frame[k];
    wf::frame_in_root<float>(Rm, fw, fr);
    for (int k = 0; k < nc; k++) {
      if ((int)T.c_link[k] == lane && !T.c_excl[k]) {  // (a contact inside the gap, or one switched off for want of a column, has no row)
        const float f[3] = {T.r_f[3 * k], T.r_f[3 * k + 1], T.r_f[3 * k + 2]};
        ws::add_contact_force<float>(fr, f, fext);
        touch += ws::touch_share<float>(f[0]);
      }
    }
  }
  if constexpr (Tile::kSelf) {
    for (int j = 0; j < ns; j++) {
      const int k = nc + j;
      const bool on_pos = (int)T.c_link[k] == lane, on_neg = (int)T.c_link1[k] == lane;  // (255, the thorax, is no lane's link)
      if ((on_pos || on_neg) && !T.c_excl[k]) {
        float n[3];
        self_nrm(T, k, n);
        const float f = T.r_f[3 * nc + j];
        wss::add_pair_force<float>(n, f, on_pos, on_neg, fext);
        touch += wss::pair_touch_share<float>(f, on_pos, on_neg);
      }
    }
  }
  // sum over the ancestor path of cdof * qacc by pointer jumping, as stage 1 sums the velocities
  S6 dacc = zero6();
  float g[3] = {0.f, 0.f, 0.f};
#pragma unroll
  for (int s = 0; s < 3; s++) {
    if (s < ndof) {
      const int f = M.s_dof[s][lane];
      const float a = T.X4[f].x;
      dacc = dacc + a * ld6(T.C[f]);
      g[0] += a * T.F[f][3]; g[1] += a * T.F[f][4]; g[2] += a * T.F[f][5];
    }
  }
#pragma unroll
  for (int r = 0; r < 3; r++) {
    const int an = r == 0 ? parent : (r == 1 ? anc2 : anc4);
    st6(T.lp[lane], dacc);
    DM_SYNC();
    if (an >= 0) dacc = dacc + ld6(T.lp[an]);
    DM_SYNC();
  }
  // every link publishes its hinges' lin(crb cdof) qacc and its contacts' force; a sensor's link sums them over its depth-first lane
  // range (its own hinges are inside A: not summed)
  {
    float *o = T.lp[lane];
    o[0] = g[0]; o[1] = g[1]; o[2] = g[2]; o[3] = fext[0]; o[4] = fext[1]; o[5] = fext[2];
  }
  DM_SYNC();
  const int fi = M.l_force[lane], ti = M.l_touch[lane];
  if (fi >= 0) {
    float gs[3] = {0.f, 0.f, 0.f};
#pragma unroll 1
    for (int t = 1; t < sub; t++) {
      const float *p = T.lp[lane + t];
      gs[0] += p[0]; gs[1] += p[1]; gs[2] += p[2]; fext[0] += p[3]; fext[1] += p[4]; fext[2] += p[5];
    }
    const float A[6] = {xr0 + dacc.a0, xr1 + dacc.a1, xr2 + dacc.a2, xr3 + dacc.l0, xr4 + dacc.l1, xr5 + dacc.l2};
    const float *sp = T.sp[fi];
    float fint[3], o[3];
    ws::accel_term<float>(sp[3], sp + 4, A, fint);
    fint[0] += gs[0] + sp[0] - fext[0]; fint[1] += gs[1] + sp[1] - fext[1]; fint[2] += gs[2] + sp[2] - fext[2];
    ws::to_site<float>(T.fsq[fi], fint, o);
    T.sens[9 + 3 * fi] += o[0]; T.sens[9 + 3 * fi + 1] += o[1]; T.sens[9 + 3 * fi + 2] += o[2];
  }
  if (ti >= 0) T.sens[27 + ti] += touch;
  DM_SYNC();
}

// ------------------------------------------------------------------------------------------------ stage 2
// EP (the episode kernel): also mj's qacc = M^-1 (qfrc_smooth + qfrc_constraint) through M's own factor - the Euler solve below is
// implicit in the joint damping, so its solution is not qacc - for the accelerometer of this substep (`acc`, from the state before the
// integration) and for sum qacc^2 (`qn2`); `integrate` false stops there (mj_forward of a reset: nothing is advanced).
template <bool LIMITS, bool EP = false, class C>
__device__ __forceinline__ void stage2(C &c, float act_reg, float ctrl_reg, float &act_out, int &nlim_out, int &iters_out,
                                       const ImitArgs *ep = nullptr, bool integrate = true, float *acc = nullptr, float *qn2 = nullptr) {
  auto &T = *c.T;
  using Tile = std::remove_reference_t<decltype(T)>;
  constexpr bool FLOOR = Tile::kFloor;  // the floor kernel: everything it adds is under this switch
  constexpr bool SENSE = Tile::kSense;  // the episode kernel on the floor: likewise
  constexpr bool SELF = Tile::kSelf;    // the kernel with the fly's own contacts: likewise
  const BallModel FFE_GLOBAL &M = model(c);
  const int lane = c.lane;
  const float h = M.h;
#pragma unroll
  for (int s = 0; s < 3; s++) if (slot_on(c, s)) { T.Q[opq(c.sdof[s])] = c.q[s]; T.V[opq(c.sdof[s])] = c.v[s]; }
  DM_SYNC();
  // ---- mj: mj_fwdActuation: first-order activation filter, affine position servo on the activation (as ball_env.hip; an adhesion
  //      actuator has nothing to pull on without contacts)
  float act_dot = 0.f;
  if (lane < NU) {
    float force = 0.f;
    if (!(c.flags & BF_NO_ACTUATION)) {
      float ctrl = ctrl_reg;
      if (M.a_climited[lane]) ctrl = fminf(fmaxf(ctrl, M.a_clo[lane]), M.a_chi[lane]);
      act_dot = (ctrl - act_reg) * frcp(M.a_tau[lane]);
      float length = 0.f, vel = 0.f;
      const int nw = M.a_nwrap[lane];
      for (int w = 0; w < nw; w++) { const int f = M.a_wdof[w][lane]; const float cf = M.a_wcoef[w][lane]; length += cf * T.Q[f]; vel += cf * T.V[f]; }
      force = M.a_gain[lane] * act_reg + M.a_b0[lane] + M.a_b1[lane] * length + M.a_b2[lane] * vel;
      if (M.a_flimited[lane]) force = fminf(fmaxf(force, M.a_flo[lane]), M.a_fhi[lane]);
      if constexpr (FLOOR) { if (M.a_trn[lane] == 2 && (c.flags & BF_NO_ADHESION)) force = 0.f; }
    }
    T.frc[lane] = force;
  }
  act_out = act_reg + h * act_dot;
  DM_SYNC();
  // ---- smooth forces of the hinges (mj: mj_fwdAcceleration's right-hand side)
  float qs[3];
#pragma unroll
  for (int s = 0; s < 3; s++) {
    qs[s] = 0.f;
    if (slot_on(c, s)) {
      float f = c.fnb[s];
      const int a0 = M.s_act[0][s][lane], a1 = M.s_act[1][s][lane];
      if (a0 >= 0) f += M.s_actcoef[0][s][lane] * T.frc[a0];
      if (a1 >= 0) f += M.s_actcoef[1][s][lane] * T.frc[a1];
      qs[s] = f;
    }
  }
  // ---- z = A^-1 f_j and Y = A^-1 M_jr, A = M_jj + h B: seven right-hand sides through two four-wide block solves.  M_jr's column of
  //      hinge f is T.F[f] (the 6-vector crb * cdof of the assembly: the root's motion axes are the unit vectors of this frame).
  S6 mrj[3], y[3];
  float z[3];
#pragma unroll
  for (int s = 0; s < 3; s++) mrj[s] = slot_on(c, s) ? ld6(T.F[opq(c.sdof[s])]) : zero6();
  DM_SYNC();  // (Q / V have been read: X4 lies over them)
  if constexpr (LIMITS) {
    // ---- joint-limit rows (mj: mj_instantiateLimit, margin 0): sign, D, aref per slot, exactly as ball_env.hip's stage 2; one row
    //      per instantiated limit in (slot, lane) order; beyond RMAX the rows are dropped for this substep and the env is flagged
    float lsgn[3];
    int lrow[3] = {-1, -1, -1};
    int R = 0;
    if constexpr (FLOOR) {  // the contact rows come first: three per contact of the collision pass
      R = 3 * c.fl.nc;
      if (lane < 8) T.rootf[lane] = 0.f;
    }
    if constexpr (SELF) R += c.fl.ns;  // ... then one per fly-fly contact
#pragma unroll
    for (int s = 0; s < 3; s++) {
      float lD = 0.f, laref = 0.f;
      lsgn[s] = 0.f;
      if (slot_on(c, s) && M.s_limited[s][lane]) {
        const float dlo = c.q[s] - M.s_lo[s][lane], dhi = M.s_hi[s][lane] - c.q[s];
        float dist = 0.f;
        if (dlo < 0.f) { lsgn[s] = 1.f; dist = dlo; }
        else if (dhi < 0.f) { lsgn[s] = -1.f; dist = dhi; }
        if (lsgn[s] != 0.f) {
          float si_[5];
#pragma unroll
          for (int q2 = 0; q2 < 5; q2++) si_[q2] = M.j_solimp[q2];
          const float imp = impedance(si_, fabsf(dist));
          lD = frcp(fmaxf(1e-15f, (1.f - imp) * M.s_invw[s][lane] * frcp(imp)));
          laref = -M.s_B[s][lane] * (lsgn[s] * c.v[s]) - M.s_K[s][lane] * imp * dist;
        }
      }
      const bool on = lsgn[s] != 0.f;
      const unsigned long long bal = __ballot(on);
      const int idx = R + __popcll(bal & ((1ull << lane) - 1ull));
      if (on && idx < RMAX) {
        lrow[s] = idx;
        T.r_sgn[idx] = lsgn[s]; T.r_D[idx] = lD; T.r_y0[idx] = -laref;
        T.r_dof[idx] = (unsigned char)c.sdof[s]; T.r_blk[idx] = (unsigned char)M.d_blk[c.sdof[s]];
      }
      R += __popcll(bal);
    }
    if (R > RMAX) { R = RMAX; c.overflow |= 2; }
    nlim_out = R;
    if constexpr (FLOOR) nlim_out = R - 3 * c.fl.nc;
    if constexpr (SELF) nlim_out -= c.fl.ns;
    iters_out = 0;
    if (R > 0) {  // wave-uniform: a substep without a row pays the ballots only
      DM_SYNC();
      if constexpr (FLOOR) iters_out = contact_forces(c, R, lrow, lsgn, qs);  // (limit rows alone too: the cone solver with no cone block)
      else iters_out = limit_forces(c, R, lrow, lsgn, mrj, qs);
      // (read again rather than kept in registers across the solver's call: 18 fewer live values there)
#pragma unroll
      for (int s = 0; s < 3; s++) mrj[s] = slot_on(c, s) ? ld6(T.F[opq(c.sdof[s])]) : zero6();
    }
  }
  if constexpr (EP) {
    S6 ym[3];
    float zm[3];
    if constexpr (SENSE) {
#pragma unroll
      for (int s = 0; s < 3; s++) T.G[kSensePark + 64 * s + lane] = qs[s];
    } else {
#pragma unroll
    for (int s = 0; s < 3; s++) T.qsave[s][lane] = qs[s];
    }
    solve_zy(c, T.Lm, T.dinv_m, qs, mrj, zm, ym);
    float Sm[6][6], br[6], id[6], xr[6];
    schur(c, mrj, ym, zm, Sm, br);
    if constexpr (FLOOR) {  // the contacts' force on the root (and the adhesion pull), as in the Euler solve below
#pragma unroll
      for (int k = 0; k < 6; k++) br[k] += T.rootf[k];
    }
    chol6(Sm, id);
    chol6_forward(Sm, id, br, xr);
    chol6_backward(Sm, id, xr);
    float sq = 0.f;
#pragma unroll
    for (int s = 0; s < 3; s++) {
      if (slot_on(c, s)) {
        float a = zm[s];
#pragma unroll
        for (int k = 0; k < 6; k++) a -= comp(ym[s], k) * xr[k];
        sq += a * a;
        if constexpr (SENSE) T.X4[opq(c.sdof[s])].x = a;  // (its own lane reads it back in contact_sense: three fewer live values)
      }
    }
    const M3 R = q2m(c.rq);
    const bool grav = !(c.flags & BF_NO_GRAVITY);
    V3 aw = mv(R, V3{xr[3], xr[4], xr[5]} + cross(ang(c.V0), lin(c.V0)));
    if (grav) aw.z += M.gz;
    *qn2 = wave_sum(sq) + dot(aw, aw) + xr[0] * xr[0] + xr[1] * xr[1] + xr[2] * xr[2];
    const float qr[4] = {c.rq.w, c.rq.x, c.rq.y, c.rq.z}, wb[3] = {c.wb.x, c.wb.y, c.wb.z}, al[3] = {aw.x, aw.y, aw.z}, wd[3] = {xr[0], xr[1], xr[2]};
    wi::imu_acceleration<float>(qr, wb, al, wd, grav ? M.gz : 0.f, ep->site_pos, ep->site_quat, acc);
    if constexpr (SENSE) {  // (last: only the accelerometer and sum qacc^2 are live across the call)
      contact_sense(c.T, (ModelPtr)c.M, c.X, lane, c.fl.nc, self_count(c.fl), xr[0], xr[1], xr[2], xr[3], xr[4], xr[5], c.rq.w, c.rq.x, c.rq.y, c.rq.z);
    }
    if (!integrate) { act_out = act_reg; return; }
#pragma unroll
    for (int s = 0; s < 3; s++) {
      if constexpr (SENSE) qs[s] = T.G[kSensePark + 64 * s + lane];
      else qs[s] = T.qsave[s][lane];
      mrj[s] = slot_on(c, s) ? ld6(T.F[opq(c.sdof[s])]) : zero6();
    }
  }
  solve_zy(c, T.Lh, T.dinv_h, qs, mrj, z, y);
  if constexpr (!LIMITS) {
#pragma unroll
    for (int s = 0; s < 3; s++) if (slot_on(c, s)) st6(T.Y[opq(c.sdof[s])], y[s]);  // (the limits kernel reads its rows' Y_m from the solve instead)
  }
  // ---- Schur complement S = M_rr - M_rj Y and right-hand side f_r - M_rj z; 6 x 6 Cholesky S = L L', x_r = S^-1 b_r
  float Sm[6][6], br[6], id[6], xr[6];
  schur(c, mrj, y, z, Sm, br);
  if constexpr (FLOOR) {
#pragma unroll
    for (int k = 0; k < 6; k++) br[k] += T.rootf[k];
  }
  chol6(Sm, id);
  chol6_forward(Sm, id, br, xr);
  chol6_backward(Sm, id, xr);
  // ---- back substitution of the hinges, integration (mj: mj_Euler, implicit in the joint damping)
#pragma unroll
  for (int s = 0; s < 3; s++) {
    if (slot_on(c, s)) {
      float a = z[s];
#pragma unroll
      for (int k = 0; k < 6; k++) a -= comp(y[s], k) * xr[k];
      c.v[s] += h * a;
      c.q[s] += h * c.v[s];
    }
  }
  {
    // free joint: qacc = (R (vdot_b + w_b x v_b) + g, wdot_b), gravity added here (see the head of this file); mj_integratePos: position with the new velocity, quaternion by mju_quatIntegrate
    const M3 R = q2m(c.rq);
    const V3 wd = {xr[0], xr[1], xr[2]}, vd = {xr[3], xr[4], xr[5]};
    V3 aw = mv(R, vd + cross(ang(c.V0), lin(c.V0)));
    if (!(c.flags & BF_NO_GRAVITY)) aw.z += M.gz;
    c.vw = c.vw + h * aw;
    c.wb = c.wb + h * wd;
    c.pos[0] += (double)h * (double)c.vw.x; c.pos[1] += (double)h * (double)c.vw.y; c.pos[2] += (double)h * (double)c.vw.z;
    const float wn = fsqrt(dot(c.wb, c.wb));
    Q4 q = qnormalize(c.rq);
    if (wn >= 1e-15f) q = qnormalize(qmul(q, axis_angle(frcp(wn) * c.wb, wn * h)));
    c.rq = q;
  }
}

// ------------------------------------------------------------------------------------------------ kernels
// the state in the ffe_get_state layout, from the registers of the wave that holds it
template <class C>
__device__ __forceinline__ void export_state(const C &c, double *__restrict__ qp, double *__restrict__ qv) {
#pragma unroll
  for (int s = 0; s < 3; s++) if (slot_on(c, s)) { qp[7 + c.sdof[s]] = (double)c.q[s]; qv[6 + c.sdof[s]] = (double)c.v[s]; }
  if (c.lane == 0) {
    qp[0] = c.pos[0]; qp[1] = c.pos[1]; qp[2] = c.pos[2];
    qp[3] = (double)c.rq.w; qp[4] = (double)c.rq.x; qp[5] = (double)c.rq.y; qp[6] = (double)c.rq.z;
    qv[0] = (double)c.vw.x; qv[1] = (double)c.vw.y; qv[2] = (double)c.vw.z;
    qv[3] = (double)c.wb.x; qv[4] = (double)c.wb.y; qv[5] = (double)c.wb.z;
  }
}

// `ep` (the episode kernel alone, `Ep` = ImitCall): one control step of the env, or its reset, in place of `nphys` bare substeps - see
// imitation_step_kernel below.  With `Ep` = NoEpisode none of it is compiled.
template <bool LIMITS, class Tile, class Ep = NoEpisode>
__device__ __forceinline__ void walk_substeps(Tile &T, const WalkModel *__restrict__ Wp, int flags, WState *__restrict__ states,
                                              const float *__restrict__ ctrl, int nphys, const Ep &ep = Ep()) {
  constexpr bool EP = !std::is_same<Ep, NoEpisode>::value && !std::is_same<Ep, FloorCall>::value;
  const int env = blockIdx.x, lane = threadIdx.x;
  const BallModel &M = Wp->b;
  WState &S = states[env];
  CtxT<Tile> c;
  c.M = &Wp->b; c.X = (const WalkExtra FFE_GLOBAL *)&Wp->x; c.T = &T; c.lane = lane; c.flags = flags; c.overflow = 0;
  c.lpack = M.l_pack[lane]; c.xh = M.x_on[lane];
#pragma unroll
  for (int s = 0; s < 3; s++) c.sdof[s] = M.s_dof[s][lane];
#pragma unroll
  for (int s = 0; s < 3; s++) { c.q[s] = slot_on(c, s) ? S.q[c.sdof[s]] : 0.f; c.v[s] = slot_on(c, s) ? S.v[c.sdof[s]] : 0.f; }
  c.rq = {S.quat[0], S.quat[1], S.quat[2], S.quat[3]};
  c.vw = {S.vlin[0], S.vlin[1], S.vlin[2]}; c.wb = {S.wb[0], S.wb[1], S.wb[2]};
  c.pos[0] = S.pos[0]; c.pos[1] = S.pos[1]; c.pos[2] = S.pos[2];
  float act_reg = lane < NU ? S.act[lane] : 0.f;
  float ctrl_reg = 0.f;
  int row = 0;  // episode kernel: 0 step, 1 reset
  if constexpr (EP) {
    row = ep.a->flag[env];
    if (row == 2) {  // not this call's env: the task layer still reads its state
      export_state(c, ep.a->qpos + (size_t)env * 109, ep.a->qvel + (size_t)env * 108);
      return;
    }
    if (row == 1) {
      // mj: walk_imitation.py:112-121 initialize_episode: the pose of row 0 of the clip (qpos0, root, tracked joints, retracted wings),
      // zero velocity, activation and ctrl; rounded to float32 as ffe_set_state rounds it
      const double *qp = ep.a->pose + (size_t)env * 109;
#pragma unroll
      for (int s = 0; s < 3; s++) { c.q[s] = slot_on(c, s) ? (float)qp[7 + c.sdof[s]] : 0.f; c.v[s] = 0.f; }
      c.rq = qnormalize(Q4{(float)qp[3], (float)qp[4], (float)qp[5], (float)qp[6]});
      c.vw = {0.f, 0.f, 0.f}; c.wb = {0.f, 0.f, 0.f};
      c.pos[0] = qp[0]; c.pos[1] = qp[1]; c.pos[2] = qp[2];
      act_reg = 0.f;
      c.flags |= BF_NO_ACTUATION;  // dm_control's after_reset: mj_forward with actuation disabled
    } else if (lane < NU) {
      // ref: fruitfly.py:480-492 apply_action (+ the CanonicalSpecWrapper the reference wraps every env in), as ball_env.hip
      const int ai = M.a_action[lane];
      float av = ai >= 0 ? ep.action[(size_t)env * NACT + ai] : 0.f;
      if (!(av == av)) av = 0.f;
      if (ep.a->canonical && ai >= 0) {
        if (ep.a->clip) av = fminf(fmaxf(av, -1.f), 1.f);
        av = M.act_lo[ai] + 0.5f * (av + 1.f) * (M.act_hi[ai] - M.act_lo[ai]);
      }
      ctrl_reg = av;
    }
    nphys = row == 1 ? 1 : M.nsub;
    if constexpr (Tile::kSense) nphys = __builtin_amdgcn_readfirstlane(nphys);  // (the loop bound in an SGPR: it was this kernel's last spilled VGPR)
    if (lane < 36) T.sens[lane] = 0.f;  // (the sums are cleared at substep 0)
    DM_SYNC();
  } else {
    ctrl_reg = lane < NU ? ctrl[(size_t)env * NU + lane] : 0.f;
  }
  int nlim = 0, iters = 0;
  float qn2 = 0.f;
  constexpr bool FLOOR = Tile::kFloor;
#pragma unroll 1
  for (int s = 0; s < nphys; s++) {
    if constexpr (Tile::kSense) {
      // (opaque per substep: the LDS addresses stage 1 forms from the lane and its parent are then formed again in every substep, a
      //  few VALU operations, and not kept in registers over the loop, where they were the two VGPRs this kernel spilled)
      c.lpack = opq(c.lpack); c.lane = opq(c.lane);
    }
    stage1(c);
    if constexpr (Tile::kSense) {
      // ---- what the sensor pass of stage 2 needs of this link, while stage 1's values are at hand (walk_sense.hpp)
      //      every link publishes its velocity term, its mass and m r through T.lp (free between the factorisation and the collision
      //      pass); a sensor's link sums them over its depth-first lane range
      {
        const V3 r = c.xip - V3{M.thorax_pos[0], M.thorax_pos[1], M.thorax_pos[2]};
        const float cb[6] = {c.caccb.a0, c.caccb.a1, c.caccb.a2, c.caccb.l0, c.caccb.l1, c.caccb.l2};
        const float cv[6] = {c.cvel.a0, c.cvel.a1, c.cvel.a2, c.cvel.l0, c.cvel.l1, c.cvel.l2};
        const float r3[3] = {r.x, r.y, r.z};
        float *o = T.lp[lane];
        ws::velocity_term<float>(c.mass, cb, cv, r3, o);
        o[3] = c.mass; o[4] = c.mass * r.x; o[5] = c.mass * r.y; o[6] = c.mass * r.z;
      }
      DM_SYNC();
      // (the table read goes through an opaque lane index: hoisted out of the substep loop, the index and the addresses formed from it
      //  stayed in registers over the whole loop and spilled)
      const int fi = M.l_force[opq(lane)];
      if (fi >= 0) {
        const int sub = (int)(M.l_tree[opq(lane)] & 0xffu);
        float acc[7];
#pragma unroll
        for (int k = 0; k < 7; k++) acc[k] = T.lp[lane][k];
#pragma unroll 1
        for (int t = 1; t < sub; t++) {
#pragma unroll
          for (int k = 0; k < 7; k++) acc[k] += T.lp[lane + t][k];
        }
#pragma unroll
        for (int k = 0; k < 7; k++) T.sp[fi][k] = acc[k];
        const Q4 sq = qmul(c.xq, Q4{M.l_fsite[0][lane], M.l_fsite[1][lane], M.l_fsite[2][lane], M.l_fsite[3][lane]});
        T.fsq[fi][0] = sq.w; T.fsq[fi][1] = sq.x; T.fsq[fi][2] = sq.y; T.fsq[fi][3] = sq.z;
      }
      DM_SYNC();
    }
    if constexpr (FLOOR) {
      // ---- collision pass: the plane's normal in the root frame, the root origin's height over the plane in float64
      const WalkExtra FFE_GLOBAL &X = *c.X;
      const V3 nw = {X.f_frame[0], X.f_frame[1], X.f_frame[2]}, nb = mtv(q2m(c.rq), nw);
      const double height = (double)nw.x * c.pos[0] + (double)nw.y * c.pos[1] + (double)nw.z * c.pos[2] - (double)X.f_off;
      const int fc = __builtin_amdgcn_readfirstlane(floor_collide(c.T, c.X, lane, c.xp.x, c.xp.y, c.xp.z, c.xq.w, c.xq.x, c.xq.y, c.xq.z, c.cvel.a0, c.cvel.a1,
                                                                  c.cvel.a2, c.cvel.l0, c.cvel.l1, c.cvel.l2, nb.x, nb.y, nb.z, height));
      c.fl.nc = fc & 0xff;
      if (fc >> 8) c.overflow |= 1;
      float md = 0.f;
      for (int k = 0; k < c.fl.nc; k++) md = k == 0 ? T.c_dist[0] : fminf(md, T.c_dist[k]);
      c.fl.mind = md;
      if constexpr (Tile::kConvexFloor) {
        // ---- the second floor pass: ellipsoids and cylinders, behind the primitive floor contacts; `nc` then counts both kinds
        if (lane < 6) T.sv0[lane] = comp(c.V0, lane);  // (the pass starts on a barrier)
        const int vc = __builtin_amdgcn_readfirstlane(floor_convex_collide(c.T, convex_table(c.X), lane, c.fl.nc, nb.x, nb.y, nb.z, height));
        c.fl.nv = vc & 0xff;
        c.fl.nc = ((vc >> 16) & 0xff) + c.fl.nv;
        if ((vc >> 8) & 1) c.overflow |= 1;
        md = 0.f;
        for (int k = 0; k < c.fl.nc; k++) md = k == 0 ? T.c_dist[0] : fminf(md, T.c_dist[k]);
        c.fl.mind = md;
      }
      if constexpr (Tile::kSelf) {
        // ---- the fly's own contacts behind the floor's: sphere / capsule pairs, then the pairs with an ellipsoid or a cylinder.
        //      Every substep runs both passes (the mouth parts touch in every pose: there is no "nothing in reach" shortcut).
        if (lane < 6) T.sv0[lane] = comp(c.V0, lane);  // (visible after the first pass's own barrier, as the three stores below)
        if (lane < c.fl.nc) { T.c_link1[lane] = 255; T.c_blk1[lane] = 255; T.c_amask1[lane] = 0; }  // a floor slot: one chain
        const int sc = __builtin_amdgcn_readfirstlane(prim_pairs(c.T, (ModelPtr)c.M, WalkPairs<Tile>{c.X}, lane, c.fl.nc));
        const int cc = __builtin_amdgcn_readfirstlane(convex_pairs<WalkPairs<Tile>>(c.T, (ModelPtr)c.M, lane, c.fl.nc + (sc & 0xff)));
        c.fl.ns = (sc & 0xff) + (cc & 0xff);
        if (((sc | cc) >> 8) & 1) c.overflow |= 1;
        if ((cc >> 9) & 1) c.overflow |= 8;
        for (int k = c.fl.nc; k < c.fl.nc + c.fl.ns; k++) md = k == 0 ? T.c_dist[0] : fminf(md, T.c_dist[k]);
        c.fl.mind = md;
      }
    }
    float act_new;
    if constexpr (EP) {
      // dm_control runs mj_step2 ; mj_step1 and samples: the accelerometer is the acceleration stage's (the state before the
      // integration, this substep's qacc), gyro and velocimeter belong to the state after it.  Force and touch stay zero: no contacts.
      // (On the floor they are the acceleration stage's too: stage 2 calls contact_sense.)
      float acc[3], gy[3], ve[3];
      stage2<LIMITS, true>(c, act_reg, ctrl_reg, act_new, nlim, iters, ep.a, row == 0, acc, &qn2);
      const float qr[4] = {c.rq.w, c.rq.x, c.rq.y, c.rq.z}, vl[3] = {c.vw.x, c.vw.y, c.vw.z}, wb[3] = {c.wb.x, c.wb.y, c.wb.z};
      wi::imu_velocity<float>(qr, vl, wb, ep.a->site_pos, ep.a->site_quat, gy, ve);
      if (lane < 3) {
        T.sens[lane] += lane == 0 ? acc[0] : (lane == 1 ? acc[1] : acc[2]);
        T.sens[3 + lane] += lane == 0 ? gy[0] : (lane == 1 ? gy[1] : gy[2]);
        T.sens[6 + lane] += lane == 0 ? ve[0] : (lane == 1 ? ve[1] : ve[2]);
      }
    } else {
      stage2<LIMITS>(c, act_reg, ctrl_reg, act_new, nlim, iters);
    }
    act_reg = act_new;
  }
#pragma unroll
  for (int s = 0; s < 3; s++) if (slot_on(c, s)) { S.q[c.sdof[s]] = c.q[s]; S.v[c.sdof[s]] = c.v[s]; }
  if (lane < NU) S.act[lane] = act_reg;
  if (lane == 0) {
    S.quat[0] = c.rq.w; S.quat[1] = c.rq.x; S.quat[2] = c.rq.y; S.quat[3] = c.rq.z;
    S.vlin[0] = c.vw.x; S.vlin[1] = c.vw.y; S.vlin[2] = c.vw.z;
    S.wb[0] = c.wb.x; S.wb[1] = c.wb.y; S.wb[2] = c.wb.z;
    S.pos[0] = c.pos[0]; S.pos[1] = c.pos[1]; S.pos[2] = c.pos[2];
    if constexpr (LIMITS) { S.nlim = nlim; S.iters = iters; S.step_bits = c.overflow; }
    if constexpr (FLOOR) {
      const int ns = self_count(c.fl);
      if constexpr (Tile::kConvexFloor) contact_record(ep)[env] = FloorRec{c.fl.nc + ns, T.rootf[6], c.fl.mind, ns | (c.fl.nv << 8)};
      else contact_record(ep)[env] = FloorRec{c.fl.nc + ns, T.rootf[6], c.fl.mind, ns};
    }
  }
  if constexpr (EP) {
    // ---- the 92 physics columns of the observation row (the task layer writes the kinematic ones), the state for the task layer, and
    //      what check_termination reads of the last substep
    DM_SYNC();
    float *ob = ep.obs + (size_t)env * (size_t)ep.a->obs_dim;
    const float inv = (row == 1 && ep.a->pad_first_obs) ? 1.f : 1.f / (float)M.nsub;
    if (lane < 3) {
      ob[lane] = T.sens[lane] * inv;
      ob[ep.a->off_gyro + lane] = T.sens[3 + lane] * inv;
      ob[ep.a->off_velocimeter + lane] = T.sens[6 + lane] * inv;
    }
    if (lane < NU) ob[ep.a->off_act + lane] = act_reg;
    if (lane < 18) ob[ep.a->off_force + lane] = T.sens[9 + lane] * inv;
    if (lane < 6) ob[ep.a->off_touch + lane] = T.sens[27 + lane] * inv;
    export_state(c, ep.a->qpos + (size_t)env * 109, ep.a->qvel + (size_t)env * 108);
    if (lane == 0) {
      float gy[3], ve[3];
      const float qr[4] = {c.rq.w, c.rq.x, c.rq.y, c.rq.z}, vl[3] = {c.vw.x, c.vw.y, c.vw.z}, wb[3] = {c.wb.x, c.wb.y, c.wb.z};
      wi::imu_velocity<float>(qr, vl, wb, ep.a->site_pos, ep.a->site_quat, gy, ve);
      float *t = ep.a->term + (size_t)env * 4;
      t[0] = fsqrt(ve[0] * ve[0] + ve[1] * ve[1] + ve[2] * ve[2]);
      t[1] = fsqrt(gy[0] * gy[0] + gy[1] * gy[1] + gy[2] * gy[2]);
      t[2] = qn2; t[3] = 0.f;
    }
  }
}

// One control step of walk_imitation on the floor (walk_floor_env.hip): launches `imitation_floor_step` on `stream`; the caller checks
// hipGetLastError.
void launch_imitation_floor_step(const WalkModel *model, int flags, WState *states, const ImitArgs *args, const float *action, float *obs, int batch,
                                 hipStream_t stream);
// One control step of walk_imitation on the floor with the fly's own contacts (walk_imit_self_env.hip): launches `imitation_self_step`
// on `stream`; the caller checks hipGetLastError.
void launch_imitation_self_step(const WalkModel *model, int flags, WState *states, const ImitArgs *args, const float *action, float *obs, int batch,
                                hipStream_t stream);
// `nphys` substeps of bare physics with the floor and the fly's own contacts (walk_self_env.hip): launches `floor_self_step` on `stream`;
// the caller checks hipGetLastError.
void launch_floor_self_step(const WalkModel *model, int flags, WState *states, const float *ctrl, FloorRec *rec, int batch, int nphys, hipStream_t stream);
// ... and with the second floor pass, the plane against ellipsoids and cylinders (walk_full_env.hip): launches `floor_full_step`
void launch_floor_full_step(const WalkModelFull *model, int flags, WState *states, const float *ctrl, FloorRec *rec, int batch, int nphys, hipStream_t stream);
// One control step of walk_imitation with every contact of the reference's task (walk_imit_full_env.hip): launches `imitation_full_step`
// on `stream`.  It takes the model with the second floor table behind it, so a plain WalkModel allocation cannot reach it.
void launch_imitation_full_step(const WalkModelFull *model, int flags, WState *states, const ImitArgs *args, const float *action, float *obs, int batch,
                                hipStream_t stream);

}  // namespace ffw
