// fly_env.hpp - the flight backend (fly_env.hip) as the C ABI (capi.hip) sees it.
#pragma once
#include <memory>

#include "env_backend.hpp"

namespace ffe {

// Throws on failure (capi.hip turns that into the ABI's codes).  The caller has made `device` current.
std::unique_ptr<EnvBackend> flight_create(const void *blob, size_t blob_size, const ffe_flight_task &task, int batch, int device, uint64_t seed,
                                          uint64_t env_id_base);

}  // namespace ffe
