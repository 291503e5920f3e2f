// The launch of the camera rays under a lens: defined in csrc/mcrt_aov.hip next to launchAovRays (libmcrt_aov.so: the models are
// branches of aovRayKernel, the one kernel that makes the passes' camera rays), called by the camera-ray passes' chunk loop
// (mcrt_camera_pass.hpp LensPixels) and by csrc/mcrt_lens_host.hip (libmcrt_hip.so). It queues one kernel on `stream` (a hipStream_t) and
// returns the launch's hipError_t as an int. lens.model MCRT_LENS_NONE: the camera's own rays, what launchAovRays queues.
// launchSourceRays: the same kernel's two loops for a ray source (mcrt_ray_source.hpp; SourcePixels, csrc/mcrt_lens_host.hip); a chunk
// that does not lie inside the source's arrays is hipErrorInvalidValue and nothing is queued. launchProbeRays: its loop for a probe call's
// rays (mcrt_probes.hpp; ProbePixels), positions [pixels][3] in device memory, refused the same way.
#pragma once

#include "mcrt_lens.hpp"
#include "mcrt_ray_source.hpp"

namespace mcrt {

int launchLensRays(void* stream, const AovChunk& c, const LensSettings& lens, double scene_ior, const uint32_t* sobol_tab, const AovRays& rays);
int launchSourceRays(void* stream, const AovChunk& c, const RaySource& source, double scene_ior, const uint32_t* sobol_tab, const AovRays& rays);
int launchProbeRays(void* stream, const AovChunk& c, const double* positions, uint64_t pixels, double scene_ior, const uint32_t* sobol_tab, const AovRays& rays);

}  // namespace mcrt
