// The two launches of the occlusion pass: defined in csrc/mcrt_occlusion.hip (libmcrt_occlusion.so, the pass's own code object), called by
// csrc/mcrt_occlusion_host.hip (libmcrt_hip.so). Both queue one kernel on `stream` (a hipStream_t) and return the launch's hipError_t as an int.
#pragma once

#include "mcrt_occlusion.hpp"

namespace mcrt {

// cam: the chunk's camera rays and their closest hits; occ: start and direction of its pixels * spp * rays occlusion rays are written.
int launchOcclusionRays(void* stream, const AovChunk& c, const AovScene& scene, const OcclusionSettings& o, const uint32_t* sobol_tab, const AovRays& cam,
                        const AovRays& occ);
// occ: the occlusion rays with their closest hits.
int launchOcclusionResolve(void* stream, const AovChunk& c, const OcclusionSettings& o, const AovRays& cam, const AovRays& occ, const mcrt_occlusion_buffers& out);

}  // namespace mcrt
