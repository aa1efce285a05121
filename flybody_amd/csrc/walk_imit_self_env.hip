// walk_imit_self_env.hip - MI355X (gfx950): one control step of the walk_imitation environment on the floor with the fly's own contacts
// (FFE_WALK_EPISODES | FFE_WALK_FLOOR | FFE_WALK_SELF).
//
// The seventh free-root step kernel, in a translation unit of its own so that the six of walk_env.hip, walk_floor_env.hip and
// walk_self_env.hip are compiled as they were.  It is `imitation_floor_step` whose substep is `floor_self_step`'s - the code of
// walk_substeps.hpp on the tile `WTileSX`, which is a sense tile and a self tile at once:
//   front    the action row or the reset row, as `imitation_floor_step`;
//   substep  stage 1, `floor_collide`, then `prim_pairs` and `convex_pairs` (self_pairs.hpp); stage 2 with `contact_forces` (floor cone blocks,
//            one normal row per fly-fly contact, joint limits; ConeRowsResidual, from lambda = 0, the model's noslip sweeps, adhesion shared
//            over all contacts of a body), ten times in registers; a reset row runs stage 1, the three collision passes and the
//            acceleration half with its contact solve once and integrates nothing;
//   qacc     the second arrowhead solve, then the sensor pass `contact_sense`: force and touch with the fly-fly contacts' forces on both
//            of their links (walk_self_sense.hpp);
//   tail     `imitation_floor_step`'s, the record counting both kinds of contact and the fly-fly ones among them.
// No separating direction or other history is kept between substeps or launches: a step is a function of (state, act, action) alone.
// Parity tests: tests/test_gpu_walk_self_env.py.
#include "walk_substeps.hpp"

namespace ffw {
using namespace dm;
using namespace ffb;

// (its name carries neither of the two substrings by which the older tests count the tile-owning kernels of walk_env.hip)
__global__ __launch_bounds__(64, 2) void imitation_self_step(const WalkModel *__restrict__ Wp, int flags, WState *__restrict__ states,
                                                            const ImitArgs *__restrict__ args, const float *__restrict__ action, float *__restrict__ obs,
                                                            int batch) {
  if ((int)blockIdx.x >= batch) return;
  __shared__ WTileSX T;
  walk_substeps<true>(T, Wp, flags, states, nullptr, 0, ImitCall{args, action, obs});
}

void launch_imitation_self_step(const WalkModel *model, int flags, WState *states, const ImitArgs *args, const float *action, float *obs, int batch,
                                hipStream_t stream) {
  hipLaunchKernelGGL(imitation_self_step, dim3(batch), dim3(64), 0, stream, model, flags, states, args, action, obs, batch);
}

}  // namespace ffw
