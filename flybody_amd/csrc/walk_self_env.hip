// walk_self_env.hip - MI355X (gfx950): bare physics of the walking fly on the floor with the fly's own contacts (FFE_NO_CONTACT |
// FFE_WALK_JOINT_LIMITS | FFE_WALK_FLOOR | FFE_WALK_SELF).
//
// The sixth free-root step kernel, in a translation unit of its own so that the five of walk_env.hip and walk_floor_env.hip are compiled
// as they were.  It is `floor_step` with two more collision passes and one more kind of constraint row - the code of walk_substeps.hpp
// on the tile `WTileX`:
//   collision  `floor_collide`, then `prim_pairs` (the 48 sphere / capsule geoms against each other) and `convex_pairs`
//              (the pairs with an ellipsoid or a cylinder on one side, cvx:: of convex.hpp): the two passes of self_pairs.hpp, which
//              ball_env.hip runs too, here in the root frame; the floor's contacts keep the first slots, NC = 16 in all, the deepest are kept beyond that;
//   rows       `contact_forces`: floor cone blocks, one normal row per fly-fly contact over the hinges of two chains (no entry on the
//              root: walk_self.hpp), joint limits; from lambda = 0, the model's noslip sweeps, adhesion shared over all contacts of a body.
// There is no "no floor in reach" shortcut (the mouth parts touch in every pose) and no state besides WState: a launch's result is a
// function of (state, act, ctrl) alone; in particular no separating direction is kept from substep to substep.
// Parity tests: tests/test_gpu_walk_self.py.
#include "walk_substeps.hpp"

namespace ffw {
using namespace dm;
using namespace ffb;

// (its name carries neither of the two substrings by which the older tests count the tile-owning kernels of walk_env.hip)
__global__ __launch_bounds__(64, 2) void floor_self_step(const WalkModel *__restrict__ Wp, int flags, WState *__restrict__ states,
                                                        const float *__restrict__ ctrl, FloorRec *__restrict__ rec, int batch, int nphys) {
  if ((int)blockIdx.x >= batch) return;
  __shared__ WTileX T;
  walk_substeps<true>(T, Wp, flags, states, ctrl, nphys, FloorCall{rec});
}

void launch_floor_self_step(const WalkModel *model, int flags, WState *states, const float *ctrl, FloorRec *rec, int batch, int nphys, hipStream_t stream) {
  hipLaunchKernelGGL(floor_self_step, dim3(batch), dim3(64), 0, stream, model, flags, states, ctrl, rec, batch, nphys);
}

}  // namespace ffw
