// First-hit AOV pass (include/mcrt.h mcrt_render_aov*): built BESIDE the render path - two small kernels of its own around the closest-hit
// search mcrt_intersect already has (intersectDeviceArrays, mcrt_hip.hip), none of the render kernels touched. This translation unit is
// the whole of libmcrt_aov.so, which libmcrt_hip.so (and its tolerance twin: the same exact object) links: the kernels and their two
// launch functions; the host side of the pass is csrc/mcrt_aov_host.hip. Per chunk of whole pixels:
//   aovRayKernel      one lane per camera ray: Camera::samplePixel's ray (camera/camera.cpp:73-95) into [n][3] start / direction arrays,
//                     sample-major (r = i * chunk_pixels + p)
//   (closest hits)    the trace kernel for trees in memory, the intersect kernel for staged scenes: t, surface, uv per ray
//   aovResolveKernel  one lane per pixel: its samples in index order - ray, hit, surface and material gathered - summed by one FP64
//                     accumulator per channel word and written to the requested channels (mcrt_aov.hpp)
// The pass is bound by the closest-hit search; the two kernels stream 76 B per ray each way (scratch and chunks: mcrt_aov_host.hip).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "mcrt_aov.hpp"
#include "mcrt_aov_launch.hpp"

using namespace mcrt;

namespace {

constexpr uint32_t kAovBlock = 256;

__global__ void __launch_bounds__(kAovBlock) aovRayKernel(AovChunk c, double scene_ior, const uint32_t* sobol_tab, AovRays rays) {
    __shared__ uint32_t ltab[kSobolTableWords];
    for (uint32_t i = threadIdx.x; i < (uint32_t)kSobolTableWords; i += blockDim.x) ltab[i] = sobol_tab[i];
    __syncthreads();
    const uint64_t n = (uint64_t)c.pixels * c.spp;
    for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += (uint64_t)gridDim.x * blockDim.x) {
        const Ray ray = aovCameraRay<false>(c, scene_ior, (uint32_t)(r % c.pixels), (uint32_t)(r / c.pixels), (SobolTab)ltab);
        aovStore3(rays.start, r, ray.start);
        aovStore3(rays.direction, r, ray.direction);
    }
}

__global__ void __launch_bounds__(kAovBlock) aovResolveKernel(AovChunk c, AovScene scene, AovRays rays, mcrt_aov_buffers out) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= c.pixels) return;
    AovAccum acc;
    aovBegin(acc);
    for (uint32_t i = 0; i < c.spp; i++) {
        const uint64_t r = (uint64_t)i * c.pixels + p;
        aovAddRay(acc, scene, i, rays, r);
    }
    aovFinish(acc, c.spp, out, c.first_pixel + p);
}

}  // namespace

namespace mcrt {
int launchAovRays(void* stream, const AovChunk& c, double scene_ior, const uint32_t* sobol_tab, const AovRays& rays) {
    const uint64_t n = (uint64_t)c.pixels * c.spp;
    const uint32_t grid = (uint32_t)std::min<uint64_t>((n + kAovBlock - 1) / kAovBlock, 4096);
    hipLaunchKernelGGL(aovRayKernel, dim3(grid), dim3(kAovBlock), 0, (hipStream_t)stream, c, scene_ior, sobol_tab, rays);
    return (int)hipGetLastError();
}
int launchAovResolve(void* stream, const AovChunk& c, const AovScene& scene, const AovRays& rays, const mcrt_aov_buffers& out) {
    hipLaunchKernelGGL(aovResolveKernel, dim3((c.pixels + kAovBlock - 1) / kAovBlock), dim3(kAovBlock), 0, (hipStream_t)stream, c, scene, rays, out);
    return (int)hipGetLastError();
}
}  // namespace mcrt
