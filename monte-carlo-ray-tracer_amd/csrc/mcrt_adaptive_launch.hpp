// The launches of adaptive sampling: defined in csrc/mcrt_adaptive.hip (libmcrt_adaptive.so, the pass's own code object), called by
// csrc/mcrt_adaptive_host.hip (libmcrt_hip.so). All queue one kernel on `stream` (a hipStream_t) and return the launch's hipError_t as
// an int.
#pragma once

#include "mcrt_adaptive.hpp"

namespace mcrt {

// The rule: flags[q] = pixel q is listed for the next batch, for the `pixels` = rule.width * rule.height pixels of the frame.
int launchAdaptiveFlags(void* stream, const AdaptiveFrame& f, const AdaptiveRule& rule, uint8_t* flags);
// The list, three launches: block_counts[b] = the flags set among pixels [256 b, 256 b + 256); offsets[b] = the flags set before block b
// and *length = all of them (one workgroup); list[0 .. *length) = the flagged pixels, ascending.
int launchAdaptiveCount(void* stream, const uint8_t* flags, uint64_t pixels, uint32_t* block_counts);
int launchAdaptiveScan(void* stream, const uint32_t* block_counts, uint32_t blocks, uint32_t* offsets, uint32_t* length);
int launchAdaptiveScatter(void* stream, const uint8_t* flags, uint64_t pixels, const uint32_t* offsets, uint32_t* list);
// The walk over a chunk of the list: the camera rays of the chunk's samples (the AOV pass's, the pixel taken from the list), then the
// light groups' begin, rays and step with these meanings (mcrt_light_groups_launch.hpp), then the resolve: the batch summary of every
// pixel of the chunk merged into its accumulators.
int launchAdaptiveCameraRays(void* stream, const AdaptiveChunk& c, double scene_ior, const uint32_t* sobol_tab, const AovRays& rays);
int launchAdaptiveBegin(void* stream, const LgState& st, uint64_t n, double scene_ior, const LgParams& par, uint32_t* list, LgCounters* counters);
int launchAdaptiveRays(void* stream, const AdaptiveChunk& c, const AovScene& scene, const uint32_t* sobol_tab, const LgState& st, const uint32_t* list, uint32_t n_live,
                       uint32_t k, const AovRays& lit, LgCounters* counters, uint32_t next);
int launchAdaptiveStep(void* stream, const AdaptiveChunk& c, const AovScene& scene, const uint32_t* sobol_tab, const LgState& st, const LgParams& par, const uint32_t* list,
                       uint32_t n_live, uint32_t k, bool last, const AovRays& lit, uint32_t* next_list, LgCounters* counters, uint32_t next);
int launchAdaptiveResolve(void* stream, const AdaptiveChunk& c, const LgState& st, const AdaptiveFrame& f);
// A rendered full batch (the frames of `batch`, n samples a pixel; its count is not read) merged into the accumulators of every pixel.
int launchAdaptiveMerge(void* stream, const AdaptiveFrame& f, const AdaptiveFrame& batch, uint64_t pixels, uint32_t n);

}  // namespace mcrt
