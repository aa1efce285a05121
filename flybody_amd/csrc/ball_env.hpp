// ball_env.hpp - the walk_on_ball backend (ball_env.hip) as the C ABI (capi.hip) sees it.
#pragma once
#include <memory>

#include "env_backend.hpp"

namespace ffb {

struct BallTaskHost {
  int time_limit_steps, pad_first_obs, physics_flags, canonical_actions, clip_actions;
  double control_timestep;
};

// Throws on failure (capi.hip turns that into the ABI's codes).  The caller has made `device` current.
std::unique_ptr<ffe::EnvBackend> ball_create(const void *blob, size_t blob_size, const BallTaskHost &task, int batch, int device);

}  // namespace ffb
