// Lighting passes (include/mcrt.h mcrt_render_lighting*): built BESIDE the render path like the occlusion pass - two kernels of their own
// around the closest-hit search mcrt_intersect already has (intersectDeviceArrays, mcrt_hip.hip), none of the render kernels touched. This
// translation unit is the whole of libmcrt_lighting.so, which libmcrt_hip.so (and its tolerance twin: the same exact object) links: the
// kernels and their two launch functions; the host side of the pass is csrc/mcrt_lighting_host.hip.
// Per chunk of whole pixels, after the AOV pass's camera rays and their closest hits:
//   lightingRayKernel       one lane per camera sample: vertex 0 of the path tracer's path rebuilt from the camera record (lightingVertex),
//                           its shadow ray and its bounce ray into ONE array of 2n rays at (2 i) * chunk_pixels + p and
//                           (2 i + 1) * chunk_pixels + p
//   (closest hits)          the same search once more, over both rays of every sample: t and surface per slot
//   lightingResolveKernel   one lane per pixel: vertex 0 rebuilt once more (nothing of it is stored), the two hits turned into the
//                           sample's parts, the samples in ascending order into one FP64 accumulator per word (mcrt_lighting.hpp)
// Both kernels shade, so both stage what the shading code reads from LDS: the Sobol byte tables and the sine / cosine table.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "mcrt_lighting.hpp"
#include "mcrt_lighting_launch.hpp"

using namespace mcrt;

namespace {

constexpr uint32_t kLightingBlock = 256;

__global__ void __launch_bounds__(kLightingBlock) lightingRayKernel(AovChunk c, AovScene scene, const uint32_t* sobol_tab, AovRays cam, AovRays lit) {
    __shared__ uint32_t ltab[kSobolTableWords];
    for (uint32_t i = threadIdx.x; i < (uint32_t)kSobolTableWords; i += blockDim.x) ltab[i] = sobol_tab[i];
    glibc235::stageSinCosTab();
    __syncthreads();
    const uint64_t n = (uint64_t)c.pixels * c.spp;
    for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += (uint64_t)gridDim.x * blockDim.x)
        lightingChunkRays(c, scene, cam, lit, r, (SobolTab)ltab);
}

__global__ void __launch_bounds__(kLightingBlock) lightingResolveKernel(AovChunk c, AovScene scene, const uint32_t* sobol_tab, AovRays cam, AovRays lit,
                                                                        mcrt_lighting_buffers out) {
    __shared__ uint32_t ltab[kSobolTableWords];
    for (uint32_t i = threadIdx.x; i < (uint32_t)kSobolTableWords; i += blockDim.x) ltab[i] = sobol_tab[i];
    glibc235::stageSinCosTab();
    __syncthreads();
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= c.pixels) return;
    LightingAccum acc;
    lightingPixel(acc, c, scene, cam, lit, p, (SobolTab)ltab);
    lightingFinish(acc, c.spp, out, c.first_pixel + p);
}

}  // namespace

namespace mcrt {
int launchLightingRays(void* stream, const AovChunk& c, const AovScene& scene, const uint32_t* sobol_tab, const AovRays& cam, const AovRays& lit) {
    const uint64_t n = (uint64_t)c.pixels * c.spp;
    const uint32_t grid = (uint32_t)std::min<uint64_t>((n + kLightingBlock - 1) / kLightingBlock, 4096);
    hipLaunchKernelGGL(lightingRayKernel, dim3(grid), dim3(kLightingBlock), 0, (hipStream_t)stream, c, scene, sobol_tab, cam, lit);
    return (int)hipGetLastError();
}
int launchLightingResolve(void* stream, const AovChunk& c, const AovScene& scene, const uint32_t* sobol_tab, const AovRays& cam, const AovRays& lit,
                          const mcrt_lighting_buffers& out) {
    hipLaunchKernelGGL(lightingResolveKernel, dim3((c.pixels + kLightingBlock - 1) / kLightingBlock), dim3(kLightingBlock), 0, (hipStream_t)stream, c, scene,
                       sobol_tab, cam, lit, out);
    return (int)hipGetLastError();
}
}  // namespace mcrt
