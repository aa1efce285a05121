// walk_full_env.hip - MI355X (gfx950): bare physics of the walking fly on the floor with the fly's own contacts and with every fly geom
// against the floor (FFE_NO_CONTACT | FFE_WALK_JOINT_LIMITS | FFE_WALK_FLOOR | FFE_WALK_SELF | FFE_WALK_FLOOR_CONVEX; DESIGN.md section
// 12 step 3d).
//
// The eighth free-root step kernel, in a translation unit of its own so that the seven before it are compiled as they were.  It is
// `floor_self_step` of walk_self_env.hip with one more collision pass between `floor_collide` and the fly-fly passes - the code of
// walk_substeps.hpp on the tile `WTileXC`:
//   collision  `floor_collide` (the plane against the 48 spheres / capsules), then `floor_convex_collide` (the plane against the 16
//              ellipsoids and 6 cylinders of WalkFloorConvex: mjc_PlaneConvex / mjc_PlaneCylinder of walk_floor_convex.hpp), then
//              `prim_pairs` and `convex_pairs`; NC = 16 in all, beyond that the deepest floor contacts of both kinds are kept;
//   rows       `contact_forces` unchanged in kind: a plane-ellipsoid / plane-cylinder contact is a floor cone block whose parameters come
//              from the second table; a contact of a root geom (the thorax ellipsoids) has the root entries J_r = (p x e, e) alone.
// No state besides WState: a launch's result is a function of (state, act, ctrl) alone.
// Parity tests: tests/test_gpu_walk_floor_convex.py.
#include "walk_substeps.hpp"

namespace ffw {
using namespace dm;
using namespace ffb;

// (its name carries none of the substrings by which the older tests count the tile-owning kernels of the other units)
__global__ __launch_bounds__(64, 2) void floor_full_step(const WalkModelFull *__restrict__ Wp, int flags, WState *__restrict__ states,
                                                        const float *__restrict__ ctrl, FloorRec *__restrict__ rec, int batch, int nphys) {
  if ((int)blockIdx.x >= batch) return;
  __shared__ WTileXC T;
  walk_substeps<true>(T, &Wp->m, flags, states, ctrl, nphys, FloorCall{rec});
}

void launch_floor_full_step(const WalkModelFull *model, int flags, WState *states, const float *ctrl, FloorRec *rec, int batch, int nphys, hipStream_t stream) {
  hipLaunchKernelGGL(floor_full_step, dim3(batch), dim3(64), 0, stream, model, flags, states, ctrl, rec, batch, nphys);
}

}  // namespace ffw
