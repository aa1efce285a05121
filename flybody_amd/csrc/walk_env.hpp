// walk_env.hpp - the free-root walk physics backend (walk_env.hip) as the C ABI (capi.hip) sees it.
#pragma once
#include <memory>

#include "env_backend.hpp"

namespace ffw {

// Throws on failure (capi.hip turns that into the ABI's codes).  The caller has made `device` current.  `task.physics_flags` must
// contain FFE_NO_CONTACT and exactly one of FFE_NO_LIMIT (smooth dynamics) or FFE_WALK_JOINT_LIMITS (joint limits on) in this build;
// FFE_WALK_FLOOR on top of FFE_NO_CONTACT | FFE_WALK_JOINT_LIMITS adds the floor plane, FFE_WALK_SELF on top of that the fly's own
// contacts (bare physics only: walk_self_env.hip); FFE_WALK_EPISODES on top of either of the first two makes the
// handle the walk_imitation environment (with the floor off, or on it), and only then are the fields of `task` behind `physics_flags`
// read.
std::unique_ptr<ffe::EnvBackend> walk_create(const void *blob, size_t blob_size, const ffe_walk_physics_task &task, int batch, int device);

}  // namespace ffw
