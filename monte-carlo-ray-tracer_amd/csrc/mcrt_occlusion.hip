// Occlusion pass (include/mcrt.h mcrt_render_occlusion*): built BESIDE the render path like the first-hit AOV pass it continues - two
// small kernels of its own around the closest-hit search mcrt_intersect already has (intersectDeviceArrays, mcrt_hip.hip), none of the
// render kernels touched. This translation unit is the whole of libmcrt_occlusion.so, which libmcrt_hip.so (and its tolerance twin: the
// same exact object) links: the kernels and their two launch functions; the host side of the pass is csrc/mcrt_occlusion_host.hip.
// Per chunk of whole pixels, after the AOV pass's camera rays and their closest hits:
//   occlusionRayKernel      one lane per occlusion ray: the first hit rebuilt (aovSampleOf), the sampler restored at 1 + j shuffles, the
//                           cosine-weighted direction and the lifted start into [n][3] arrays, ordered r = (i * rays + j) * chunk_pixels + p
//   (closest hits)          the same search once more: t and surface per occlusion ray
//   occlusionResolveKernel  one lane per pixel: its occlusion rays in (i, j) order summed by one FP64 accumulator per word and written
//                           to the requested channels (mcrt_occlusion.hpp)
// Both kernels stream: 76 B of camera record in and 48 B of ray out per occlusion ray, then 12 B of hit (and 24 B of direction for an
// open ray) in per occlusion ray and 40 B out per pixel.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "mcrt_occlusion.hpp"
#include "mcrt_occlusion_launch.hpp"

using namespace mcrt;

namespace {

constexpr uint32_t kOcclusionBlock = 256;

__global__ void __launch_bounds__(kOcclusionBlock) occlusionRayKernel(AovChunk c, AovScene scene, OcclusionSettings o, const uint32_t* sobol_tab, AovRays cam, AovRays occ) {
    __shared__ uint32_t ltab[kSobolTableWords];
    for (uint32_t i = threadIdx.x; i < (uint32_t)kSobolTableWords; i += blockDim.x) ltab[i] = sobol_tab[i];
    __syncthreads();
    const uint64_t n = (uint64_t)c.pixels * c.spp * o.rays;
    for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += (uint64_t)gridDim.x * blockDim.x) {
        d3 start, direction;
        occlusionChunkRay<false>(c, scene, o, cam, r, (SobolTab)ltab, start, direction);
        aovStore3(occ.start, r, start);
        aovStore3(occ.direction, r, direction);
    }
}

__global__ void __launch_bounds__(kOcclusionBlock) occlusionResolveKernel(AovChunk c, OcclusionSettings o, AovRays cam, AovRays occ, mcrt_occlusion_buffers out) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= c.pixels) return;
    OcclusionAccum acc;
    occlusionPixel(acc, c, o, cam, occ, p);
    occlusionFinish(acc, o.rays, out, c.first_pixel + p);
}

}  // namespace

namespace mcrt {
int launchOcclusionRays(void* stream, const AovChunk& c, const AovScene& scene, const OcclusionSettings& o, const uint32_t* sobol_tab, const AovRays& cam,
                        const AovRays& occ) {
    const uint64_t n = (uint64_t)c.pixels * c.spp * o.rays;
    const uint32_t grid = (uint32_t)std::min<uint64_t>((n + kOcclusionBlock - 1) / kOcclusionBlock, 4096);
    hipLaunchKernelGGL(occlusionRayKernel, dim3(grid), dim3(kOcclusionBlock), 0, (hipStream_t)stream, c, scene, o, sobol_tab, cam, occ);
    return (int)hipGetLastError();
}
int launchOcclusionResolve(void* stream, const AovChunk& c, const OcclusionSettings& o, const AovRays& cam, const AovRays& occ, const mcrt_occlusion_buffers& out) {
    hipLaunchKernelGGL(occlusionResolveKernel, dim3((c.pixels + kOcclusionBlock - 1) / kOcclusionBlock), dim3(kOcclusionBlock), 0, (hipStream_t)stream, c, o, cam, occ, out);
    return (int)hipGetLastError();
}
}  // namespace mcrt
