// walk_env.hpp - the free-root walk physics backend (walk_env.hip) as the C ABI (capi.hip) sees it.
#pragma once
#include <memory>

#include "env_backend.hpp"

namespace ffw {

// Throws on failure (capi.hip turns that into the ABI's codes).  The caller has made `device` current.  `task.physics_flags` must
// contain FFE_NO_CONTACT and exactly one of FFE_NO_LIMIT (smooth dynamics) or FFE_WALK_JOINT_LIMITS (joint limits on) in this build;
// FFE_WALK_FLOOR on top of FFE_NO_CONTACT | FFE_WALK_JOINT_LIMITS adds the floor plane, FFE_WALK_SELF on top of that the fly's own
// contacts (walk_self_env.hip); FFE_WALK_EPISODES on top of any of these but FFE_WALK_SELF without the floor (and, next to
// FFE_WALK_SELF, together with FFE_WALK_SELF_EPISODES only) makes the handle the walk_imitation environment (with the floor off, on it, or on it with the fly's own contacts: walk_imit_self_env.hip), and
// only then are the fields of `task` behind `physics_flags` read.
std::unique_ptr<ffe::EnvBackend> walk_create(const void *blob, size_t blob_size, const ffe_walk_physics_task &task, int batch, int device);

}  // namespace ffw
