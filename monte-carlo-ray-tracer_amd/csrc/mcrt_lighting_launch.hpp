// The two launches of the lighting passes: defined in csrc/mcrt_lighting.hip (libmcrt_lighting.so, the pass's own code object), called by
// csrc/mcrt_lighting_host.hip (libmcrt_hip.so). Both queue one kernel on `stream` (a hipStream_t) and return the launch's hipError_t as an int.
#pragma once

#include "mcrt_lighting.hpp"

namespace mcrt {

// cam: the chunk's camera rays and their closest hits; lit: start and direction of its 2 * pixels * spp shadow and bounce rays are written.
int launchLightingRays(void* stream, const AovChunk& c, const AovScene& scene, const uint32_t* sobol_tab, const AovRays& cam, const AovRays& lit);
// lit: the shadow and bounce rays with their closest hits.
int launchLightingResolve(void* stream, const AovChunk& c, const AovScene& scene, const uint32_t* sobol_tab, const AovRays& cam, const AovRays& lit,
                          const mcrt_lighting_buffers& out);

}  // namespace mcrt
