// Adaptive sampling (include/mcrt.h mcrt_render_adaptive*): built BESIDE the render path like the light groups - kernels of its own
// around the closest-hit search mcrt_intersect already has and around mcrt_render_pixel_stats_device, none of the render kernels
// touched. This translation unit is the whole of libmcrt_adaptive.so, which libmcrt_hip.so (and its tolerance twin: the same exact
// object) links: the kernels and their launch functions; the host side of the pass is csrc/mcrt_adaptive_host.hip. Per batch:
//   adaptiveFlagKernel        one lane per pixel of the frame: the criterion over the pixel's window on the accumulators (a neighbour is
//                             evaluated again by every lane that has it in its window: at most 81 pixels of 52 B each, from cache)
//   adaptiveCountKernel       one workgroup per 256 pixels: the flags it holds - a ballot and a population count per wave, four words of
//                             LDS across the waves
//   adaptiveScanKernel        ONE workgroup: the exclusive scan of the block counts, and the list's length, which the host reads
//   adaptiveScatterKernel     one workgroup per 256 pixels: its flagged pixels to their places, ascending
//   per chunk of the list:
//   adaptiveCameraRayKernel   one lane per listed pixel: the AOV pass's camera rays of its samples, pixel and seed looked up once
//   adaptiveBeginKernel, adaptiveRayKernel, adaptiveStepKernel
//                             the light groups' walk (mcrt_light_groups.hpp, one plane) as instances of this code object
//   adaptiveResolveKernel     one lane per listed pixel: its samples in ascending order into the batch summary, merged into the pixel's
//                             accumulators - no batch frame is kept
//   adaptiveMergeKernel       a full batch that was rendered: one lane per pixel, the batch frames into the accumulators
// No workgroup waits for another anywhere: the list is three launches, not a look-back.
#include <hip/hip_runtime.h>

#include "mcrt_adaptive.hpp"
#include "mcrt_adaptive_launch.hpp"
#include "mcrt_light_groups_device.hpp"

using namespace mcrt;

namespace {

static_assert(kAdaptiveBlock == kLgBlock, "the walk's kernels are the light groups' shape");

__global__ void __launch_bounds__(kAdaptiveBlock) adaptiveFlagKernel(AdaptiveFrame f, AdaptiveRule rule, uint8_t* flags) {
    const uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= (uint64_t)rule.width * rule.height) return;
    flags[q] = adaptiveListed(f, rule, q) ? 1 : 0;
}

__global__ void __launch_bounds__(kAdaptiveBlock) adaptiveCountKernel(const uint8_t* flags, uint64_t pixels, uint32_t* block_counts) {
    __shared__ uint32_t wave_sums[kAdaptiveWaves];
    adaptiveCountBlock(flags, pixels, blockIdx.x, threadIdx.x, wave_sums, block_counts);
}

__global__ void __launch_bounds__(kAdaptiveBlock) adaptiveScanKernel(const uint32_t* block_counts, uint32_t blocks, uint32_t* offsets, uint32_t* length) {
    __shared__ uint32_t sums[2 * kAdaptiveBlock];
    adaptiveScanBlocks(block_counts, blocks, threadIdx.x, sums, offsets, length);
}

__global__ void __launch_bounds__(kAdaptiveBlock) adaptiveScatterKernel(const uint8_t* flags, uint64_t pixels, const uint32_t* offsets, uint32_t* list) {
    __shared__ uint32_t wave_sums[kAdaptiveWaves];
    adaptiveScatterBlock(flags, pixels, blockIdx.x, threadIdx.x, wave_sums, offsets, list);
}

__global__ void __launch_bounds__(kAdaptiveBlock) adaptiveCameraRayKernel(AdaptiveChunk c, double scene_ior, const uint32_t* sobol_tab, double* start,
                                                                          double* direction) {  // (of the records only what is written: fewer argument words)
    __shared__ uint32_t ltab[kSobolTableWords];
    for (uint32_t i = threadIdx.x; i < (uint32_t)kSobolTableWords; i += blockDim.x) ltab[i] = sobol_tab[i];
    __syncthreads();
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p < c.pixels) adaptiveCameraRays<false>(c, scene_ior, p, (SobolTab)ltab, start, direction);
}

__global__ void __launch_bounds__(kAdaptiveBlock) adaptiveBeginKernel(LgState st, uint64_t n, double scene_ior, LgParams par, uint32_t* list, LgCounters* counters) {
    for (uint64_t base = (uint64_t)blockIdx.x * blockDim.x; base < n; base += (uint64_t)gridDim.x * blockDim.x) {  // (whole blocks: lgAppendLive)
        const uint64_t s = base + threadIdx.x;
        const bool alive = s < n && lgBegin(st, s, scene_ior, par);
        lgAppendLive(list, &counters->live[0], alive, (uint32_t)s);
    }
}

__global__ void __launch_bounds__(kAdaptiveBlock) adaptiveRayKernel(AdaptiveChunk c, AovScene scene, const uint32_t* sobol_tab, LgState st, const uint32_t* list,
                                                                    uint32_t n_live, uint32_t k, AovRays lit, LgCounters* counters, uint32_t next) {
    __shared__ uint32_t ltab[kSobolTableWords];
    __shared__ double liors[kMaxIors * kLgBlock];
    if (blockIdx.x == 0 && threadIdx.x == 0) counters->live[next] = 0u;  // the list this iteration's step kernel appends to
    lgStageTables(ltab, sobol_tab);
    RefractionHistory rh = lgLaneHistory(liors);
    for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < n_live; j += (uint64_t)gridDim.x * blockDim.x)
        lgRays(c, scene, st, list, n_live, (uint32_t)j, k, lit, rh, (SobolTab)ltab);
}

__global__ void __launch_bounds__(kAdaptiveBlock) adaptiveStepKernel(AdaptiveChunk c, AovScene scene, const uint32_t* sobol_tab, LgState st, LgParams par,
                                                                     const uint32_t* list, uint32_t n_live, uint32_t k, uint32_t last, AovRays lit, uint32_t* next_list,
                                                                     LgCounters* counters, uint32_t next) {
    __shared__ uint32_t ltab[kSobolTableWords];
    __shared__ double liors[kMaxIors * kLgBlock];
    lgStageTables(ltab, sobol_tab);
    RefractionHistory rh = lgLaneHistory(liors);
    // whole blocks go round together, so that every lane of a wave reaches lgAppendLive
    for (uint64_t base = (uint64_t)blockIdx.x * blockDim.x; base < n_live; base += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t j = base + threadIdx.x;
        bool alive = false, too_deep = false;
        uint32_t sample = 0u;
        if (j < n_live) {
            sample = list[j];
            alive = lgStep(c, scene, st, par, list, n_live, (uint32_t)j, k, last != 0u, lit, rh, too_deep, (SobolTab)ltab);
        }
        if (too_deep) counters->too_deep = 1u;
        lgAppendLive(next_list, &counters->live[next], alive, sample);
    }
}

__global__ void __launch_bounds__(kAdaptiveBlock) adaptiveResolveKernel(AdaptiveChunk c, LgState st, AdaptiveFrame f) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= c.pixels) return;
    adaptiveResolvePixel(c, st, p, f);
}

__global__ void __launch_bounds__(kAdaptiveBlock) adaptiveMergeKernel(AdaptiveFrame f, AdaptiveFrame batch, uint64_t pixels, uint32_t n) {
    const uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= pixels) return;
    adaptiveMergeFramePixel(f, batch, q, n);
}

}  // namespace

namespace mcrt {
int launchAdaptiveFlags(void* stream, const AdaptiveFrame& f, const AdaptiveRule& rule, uint8_t* flags) {
    hipLaunchKernelGGL(adaptiveFlagKernel, dim3(adaptiveBlocks((uint64_t)rule.width * rule.height)), dim3(kAdaptiveBlock), 0, (hipStream_t)stream, f, rule, flags);
    return (int)hipGetLastError();
}
int launchAdaptiveCount(void* stream, const uint8_t* flags, uint64_t pixels, uint32_t* block_counts) {
    hipLaunchKernelGGL(adaptiveCountKernel, dim3(adaptiveBlocks(pixels)), dim3(kAdaptiveBlock), 0, (hipStream_t)stream, flags, pixels, block_counts);
    return (int)hipGetLastError();
}
int launchAdaptiveScan(void* stream, const uint32_t* block_counts, uint32_t blocks, uint32_t* offsets, uint32_t* length) {
    hipLaunchKernelGGL(adaptiveScanKernel, dim3(1), dim3(kAdaptiveBlock), 0, (hipStream_t)stream, block_counts, blocks, offsets, length);
    return (int)hipGetLastError();
}
int launchAdaptiveScatter(void* stream, const uint8_t* flags, uint64_t pixels, const uint32_t* offsets, uint32_t* list) {
    hipLaunchKernelGGL(adaptiveScatterKernel, dim3(adaptiveBlocks(pixels)), dim3(kAdaptiveBlock), 0, (hipStream_t)stream, flags, pixels, offsets, list);
    return (int)hipGetLastError();
}
int launchAdaptiveCameraRays(void* stream, const AdaptiveChunk& c, double scene_ior, const uint32_t* sobol_tab, const AovRays& rays) {
    hipLaunchKernelGGL(adaptiveCameraRayKernel, dim3((c.pixels + kAdaptiveBlock - 1) / kAdaptiveBlock), dim3(kAdaptiveBlock), 0, (hipStream_t)stream, c, scene_ior, sobol_tab, rays.start, rays.direction);
    return (int)hipGetLastError();
}
int launchAdaptiveBegin(void* stream, const LgState& st, uint64_t n, double scene_ior, const LgParams& par, uint32_t* list, LgCounters* counters) {
    hipLaunchKernelGGL(adaptiveBeginKernel, dim3(lgGridFor(n)), dim3(kAdaptiveBlock), 0, (hipStream_t)stream, st, n, scene_ior, par, list, counters);
    return (int)hipGetLastError();
}
int launchAdaptiveRays(void* stream, const AdaptiveChunk& c, const AovScene& scene, const uint32_t* sobol_tab, const LgState& st, const uint32_t* list, uint32_t n_live,
                       uint32_t k, const AovRays& lit, LgCounters* counters, uint32_t next) {
    hipLaunchKernelGGL(adaptiveRayKernel, dim3(lgGridFor(n_live)), dim3(kAdaptiveBlock), 0, (hipStream_t)stream, c, scene, sobol_tab, st, list, n_live, k, lit, counters, next);
    return (int)hipGetLastError();
}
int launchAdaptiveStep(void* stream, const AdaptiveChunk& c, const AovScene& scene, const uint32_t* sobol_tab, const LgState& st, const LgParams& par, const uint32_t* list,
                       uint32_t n_live, uint32_t k, bool last, const AovRays& lit, uint32_t* next_list, LgCounters* counters, uint32_t next) {
    hipLaunchKernelGGL(adaptiveStepKernel, dim3(lgGridFor(n_live)), dim3(kAdaptiveBlock), 0, (hipStream_t)stream, c, scene, sobol_tab, st, par, list, n_live, k,
                       last ? 1u : 0u, lit, next_list, counters, next);
    return (int)hipGetLastError();
}
int launchAdaptiveResolve(void* stream, const AdaptiveChunk& c, const LgState& st, const AdaptiveFrame& f) {
    hipLaunchKernelGGL(adaptiveResolveKernel, dim3((c.pixels + kAdaptiveBlock - 1) / kAdaptiveBlock), dim3(kAdaptiveBlock), 0, (hipStream_t)stream, c, st, f);
    return (int)hipGetLastError();
}
int launchAdaptiveMerge(void* stream, const AdaptiveFrame& f, const AdaptiveFrame& batch, uint64_t pixels, uint32_t n) {
    hipLaunchKernelGGL(adaptiveMergeKernel, dim3(adaptiveBlocks(pixels)), dim3(kAdaptiveBlock), 0, (hipStream_t)stream, f, batch, pixels, n);
    return (int)hipGetLastError();
}
}  // namespace mcrt
