// walk_imit_full_env.hip - MI355X (gfx950): one control step of the walk_imitation environment on the floor with the fly's own contacts
// and with every fly geom against the floor (FFE_WALK_EPISODES | FFE_WALK_FLOOR | FFE_WALK_SELF | FFE_WALK_SELF_EPISODES |
// FFE_WALK_FLOOR_CONVEX).
//
// The ninth free-root step kernel, in a translation unit of its own so that the eight before it are compiled as they were.  It is
// `imitation_self_step` of walk_imit_self_env.hip whose substep is `floor_full_step`'s - the code of walk_substeps.hpp on the tile
// `WTileSXC`, which is `WTileSX` with the second floor pass switched on:
//   front    the action row or the reset row, as `imitation_self_step`;
//   substep  stage 1, `floor_collide`, `floor_convex_collide` (the plane against the 16 ellipsoids and 6 cylinders of WalkFloorConvex),
//            then `prim_pairs` and `convex_pairs`; stage 2 with `contact_forces`, ten times in registers; a reset row runs stage 1, the
//            four collision passes and the acceleration half with its contact solve once and integrates nothing;
//   qacc     the second arrowhead solve, then the sensor pass `contact_sense`: a plane-ellipsoid / plane-cylinder contact is a floor cone
//            block, which adds its force to the link that owns its geom (none for a thorax geom) and to touch only on a claw's link;
//   tail     `imitation_self_step`'s, the record counting all three kinds of contact, the fly-fly ones in the low byte of `nself` and the
//            plane-ellipsoid / plane-cylinder ones in bits 8 .. 15.
// No separating direction or other history is kept between substeps or launches: a step is a function of (state, act, action) alone.
// Parity tests: tests/test_gpu_walk_full_env.py.
#include "walk_substeps.hpp"

namespace ffw {
using namespace dm;
using namespace ffb;

__global__ __launch_bounds__(64, 2) void imitation_full_step(const WalkModelFull *__restrict__ Wp, int flags, WState *__restrict__ states,
                                                            const ImitArgs *__restrict__ args, const float *__restrict__ action, float *__restrict__ obs,
                                                            int batch) {
  if ((int)blockIdx.x >= batch) return;
  __shared__ WTileSXC T;
  walk_substeps<true>(T, &Wp->m, flags, states, nullptr, 0, ImitCall{args, action, obs});
}

void launch_imitation_full_step(const WalkModelFull *model, int flags, WState *states, const ImitArgs *args, const float *action, float *obs, int batch,
                                hipStream_t stream) {
  hipLaunchKernelGGL(imitation_full_step, dim3(batch), dim3(64), 0, stream, model, flags, states, args, action, obs, batch);
}

}  // namespace ffw
