// walk_floor_env.hip - MI355X (gfx950): one control step of the walk_imitation environment with the floor under the fly (FFE_WALK_EPISODES |
// FFE_WALK_FLOOR).
//
// The fifth free-root step kernel, in a translation unit of its own so that the four of walk_env.hip are compiled as they were.  It is
// `imitation_step_kernel` with the floor kernel's substep in place of the limits kernel's - the code of walk_substeps.hpp on the tile
// `WTileS`:
//   front    the action row (NaN -> 0, act_action, canonical / clipped actions) or the reset row (the reference pose, at rest, actuation
//            disabled);
//   substep  stage 1, the collision pass (`floor_collide`), stage 2 with `contact_forces` (contact rows first, limit rows after, noslip,
//            adhesion, always from lambda = 0), ten times in registers; a reset row runs stage 1, the collision pass and the
//            acceleration half of stage 2 once and integrates nothing (mj_forward with contacts on);
//   qacc     each substep's second arrowhead solve through M's own factor, its root right-hand side carrying the contacts' force on the
//            root as the Euler solve's does; the accelerometer, and force and touch (`contact_sense`, walk_sense.hpp), are sampled there:
//            the state before the integration, this substep's qacc and contact forces;
//   tail     the 92 physics columns, qpos / qvel for the task layer, the three termination reads, and per env the contacts kept, the
//            sum of their normal forces and the smallest distance of the last substep.
// There is no "no floor in reach" shortcut: every substep is the floor's, and without a contact the force columns are the inertial
// interaction force.  Parity tests: tests/test_gpu_walk_floor_env.py.
#include "walk_substeps.hpp"

namespace ffw {
using namespace dm;
using namespace ffb;

// (its name carries neither of the two substrings by which the older tests count the tile-owning kernels of walk_env.hip)
__global__ __launch_bounds__(64, 2) void imitation_floor_step(const WalkModel *__restrict__ Wp, int flags, WState *__restrict__ states,
                                                             const ImitArgs *__restrict__ args, const float *__restrict__ action, float *__restrict__ obs,
                                                             int batch) {
  if ((int)blockIdx.x >= batch) return;
  __shared__ WTileS T;
  walk_substeps<true>(T, Wp, flags, states, nullptr, 0, ImitCall{args, action, obs});
}

void launch_imitation_floor_step(const WalkModel *model, int flags, WState *states, const ImitArgs *args, const float *action, float *obs, int batch,
                                 hipStream_t stream) {
  hipLaunchKernelGGL(imitation_floor_step, dim3(batch), dim3(64), 0, stream, model, flags, states, args, action, obs, batch);
}

}  // namespace ffw
