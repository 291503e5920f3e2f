// Firefly suppression (include/mcrt.h mcrt_render_highlights*, mcrt_robust_resolve*): the two kernels and their launch functions. This
// translation unit is the whole of libmcrt_robust.so, which libmcrt_hip.so (and its tolerance twin: the same exact object) links, the
// way libmcrt_pixel_stats.so is built - the device code of libmcrt_hip.so stays the render path's. The host side is
// csrc/mcrt_robust_host.hip; the launch of a pass sits in the pass loops of csrc/mcrt_hip.hip.
//   robustHighlightsKernel   a lane per pixel of a pass's per-sample store: the K brightest samples and the level of the rest
//   robustResolveKernel      a lane per pixel of the gathered frame: the window's level, the clamp of the pixel's tops
// Text: mcrt_robust.hpp.
#include <hip/hip_runtime.h>

#include "mcrt_robust.hpp"
#include "mcrt_robust_launch.hpp"

using namespace mcrt;

namespace {

__global__ void __launch_bounds__(kHighlightsBlock) robustHighlightsKernel(HighlightsPass hp) {
    highlightsLane(hp, (uint64_t)blockIdx.x * kHighlightsBlock + threadIdx.x);
}

__global__ void __launch_bounds__(kRobustResolveBlock) robustResolveKernel(RobustResolve rr) {
    robustResolveLane(rr, (uint64_t)blockIdx.x * kRobustResolveBlock + threadIdx.x);
}

}  // namespace

namespace mcrt {
int launchHighlights(void* stream, const HighlightsPass& hp) {
    const uint64_t blocks = (hp.pixels + kHighlightsBlock - 1) / kHighlightsBlock;
    if (blocks == 0) return (int)hipSuccess;
    if (blocks > 0x7FFFFFFFull) return (int)hipErrorInvalidConfiguration;
    hipLaunchKernelGGL(robustHighlightsKernel, dim3((uint32_t)blocks), dim3(kHighlightsBlock), 0, (hipStream_t)stream, hp);
    return (int)hipGetLastError();
}
int launchRobustResolve(void* stream, const RobustResolve& rr) {
    const uint64_t blocks = ((uint64_t)rr.width * rr.height + kRobustResolveBlock - 1) / kRobustResolveBlock;
    if (blocks == 0 || blocks > 0x7FFFFFFFull) return (int)hipErrorInvalidConfiguration;
    hipLaunchKernelGGL(robustResolveKernel, dim3((uint32_t)blocks), dim3(kRobustResolveBlock), 0, (hipStream_t)stream, rr);
    return (int)hipGetLastError();
}
}  // namespace mcrt
