// walk_env.hpp - internal C++ interface between the C ABI (fly_env.hip) and the free-root walking-fly kernel (walk_env.hip).
#pragma once
#include <cstddef>
#include <cstdint>

namespace ffw {

struct WalkEnv;  // opaque

// All functions throw std::runtime_error on failure; the C ABI wrappers translate that into error codes.
// The caller has made `device` current.  `physics_flags` must contain FFE_NO_CONTACT | FFE_NO_LIMIT in this build.
WalkEnv *walk_create(const void *blob, size_t blob_size, int physics_flags, int batch, int device);
void walk_destroy(WalkEnv *e);
void walk_spec(const WalkEnv *e, int *nq, int *nv, int *nu, int *action_dim, int *obs_dim, int *nsub, double *h, double *ctrl_dt);
void walk_action_bounds(const WalkEnv *e, float *mn, float *mx);
void walk_physics(WalkEnv *e, const float *ctrl, int nphys, void *stream);  // ctrl[B][59]
void walk_get_state(WalkEnv *e, double *qpos, double *qvel, void *stream);  // qpos[B][109], qvel[B][108]: MuJoCo's free-joint layout
void walk_set_state(WalkEnv *e, const double *qpos, const double *qvel, void *stream);
void walk_get_act(WalkEnv *e, double *act, void *stream);
void walk_set_act(WalkEnv *e, const double *act, void *stream);
void walk_get_task_state(WalkEnv *e, int32_t *ints, double *reals, void *stream);  // int32[B][8] and float64[B][8]: zeros but ints[2]
void walk_get_validity(WalkEnv *e, int32_t *info, void *stream);                   // int32[B][4]: zeros

}  // namespace ffw
