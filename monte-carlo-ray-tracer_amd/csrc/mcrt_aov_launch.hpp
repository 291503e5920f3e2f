// The two launches of the first-hit AOV pass: defined in csrc/mcrt_aov.hip (libmcrt_aov.so, the pass's own code object), called by
// csrc/mcrt_aov_host.hip (libmcrt_hip.so). Both queue one kernel on `stream` (a hipStream_t) and return the launch's hipError_t as an int.
#pragma once

#include "mcrt_aov.hpp"

namespace mcrt {

int launchAovRays(void* stream, const AovChunk& c, double scene_ior, const uint32_t* sobol_tab, const AovRays& rays);
int launchAovResolve(void* stream, const AovChunk& c, const AovScene& scene, const AovRays& rays, const mcrt_aov_buffers& out);

}  // namespace mcrt
