// walk_env.hpp - the free-root walk physics backend (walk_env.hip) as the C ABI (capi.hip) sees it.
#pragma once
#include <memory>

#include "env_backend.hpp"

namespace ffw {

// Throws on failure (capi.hip turns that into the ABI's codes).  The caller has made `device` current.  `physics_flags` must contain
// FFE_NO_CONTACT and exactly one of FFE_NO_LIMIT (smooth dynamics) or FFE_WALK_JOINT_LIMITS (joint limits on) in this build.
std::unique_ptr<ffe::EnvBackend> walk_create(const void *blob, size_t blob_size, int physics_flags, int batch, int device);

}  // namespace ffw
