// First-hit AOV pass (include/mcrt.h mcrt_render_aov*): built BESIDE the render path - two small kernels of its own around the closest-hit
// search mcrt_intersect already has (intersectDeviceArrays, mcrt_hip.hip), none of the render kernels touched. This translation unit is
// the whole of libmcrt_aov.so, which libmcrt_hip.so (and its tolerance twin: the same exact object) links: the kernels and their two
// launch functions; the host side of the pass is csrc/mcrt_aov_host.hip. Per chunk of whole pixels:
//   aovRayKernel      one lane per camera ray: Camera::samplePixel's ray (camera/camera.cpp:73-95) into [n][3] start / direction arrays,
//                     sample-major (r = i * chunk_pixels + p); under a lens (include/mcrt.h "Camera models", mcrt_lens.hpp) the model's
//                     ray of the same film position instead - the model a kernel argument, the branch on it uniform over the wave
//   (closest hits)    the trace kernel for trees in memory, the intersect kernel for staged scenes: t, surface, uv per ray
//   aovResolveKernel  one lane per pixel: its samples in index order - ray, hit, surface and material gathered - summed by one FP64
//                     accumulator per channel word and written to the requested channels (mcrt_aov.hpp)
// The pass is bound by the closest-hit search; the two kernels stream 76 B per ray each way (scratch and chunks: mcrt_aov_host.hip).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "mcrt_aov.hpp"
#include "mcrt_aov_launch.hpp"
#include "mcrt_lens.hpp"
#include "mcrt_lens_launch.hpp"
#include "mcrt_probes.hpp"
#include "mcrt_ray_source.hpp"

using namespace mcrt;

namespace {

constexpr uint32_t kAovBlock = 256;

template <class T>
__device__ __forceinline__ void toVgpr(T& v) {
    asm volatile("" : "+v"(v));
}

// The grid-stride loop of one lens model. The model is a constant of the loop, so each loop keeps only its own model's camera fields and
// sincos constants in SGPRs.
template <uint32_t kModel>
__device__ __forceinline__ void lensRaysOf(const AovChunk& c, LensSettings lens, double scene_ior, SobolTab tab, const AovRays& rays) {
    lens.model = kModel;
    const uint64_t n = (uint64_t)c.pixels * c.spp;
    for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += (uint64_t)gridDim.x * blockDim.x) {
        const Ray ray = lensRay<true>(c, lens, scene_ior, (uint32_t)(r % c.pixels), (uint32_t)(r / c.pixels), tab);
        aovStore3(rays.start, r, ray.start);
        aovStore3(rays.direction, r, ray.direction);
    }
}

// What the kernel takes of a lens OR a ray source (they exclude each other), in the bytes of LensSettings: the model, in LensSettings'
// padding the stride between two samples of a source's arrays (a shard has fewer than 2^32 pixels; 0: per-pixel arrays), and three
// words - a lens's width_world, fov_x, fov_y or a source's two arrays and its offset. So a source adds no argument to the kernel: the
// loops of calls without one keep their registers (profiles/NOTES_ray_source.md: as arguments of their own the source's words spilled).
struct RayHead {
    uint32_t model, stride;
    union Word {
        double d;
        const double* p;
    } w[3];
};
static_assert(sizeof(RayHead) == sizeof(LensSettings), "RayHead is LensSettings' bytes");

// The grid-stride loop of one kind of ray source (mcrt_ray_source.hpp): RAYS a guarded gather - chunk record i * c.pixels + p reads source
// record i * stride + (c.first_pixel + p), consecutive lanes consecutive 24-byte records -, SURFACE 48 bytes per pixel and the
// cosine-weighted direction about its normal.
template <uint32_t kKind>
__device__ __forceinline__ void sourceRaysOf(const AovChunk& c, const RayHead& h, double scene_ior, SobolTab tab, const AovRays& rays) {
    const RaySource source{kKind, h.stride == 0u ? 1u : 0u, h.stride, 0u, h.w[0].p, h.w[1].p, h.w[2].d};
    const uint64_t n = (uint64_t)c.pixels * c.spp;
    for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += (uint64_t)gridDim.x * blockDim.x) {
        const Ray ray = sourceRay<true>(c, source, scene_ior, (uint32_t)(r % c.pixels), (uint32_t)(r / c.pixels), tab);
        aovStore3(rays.start, r, ray.start);
        aovStore3(rays.direction, r, ray.direction);
    }
}

// The grid-stride loop of a probe call's rays (mcrt_probes.hpp): sourceRaysOf's shape - 24 bytes per pixel, the position, in the head's
// first word, and a direction uniform over the sphere.
__device__ __forceinline__ void probeRaysOf(const AovChunk& c, const RayHead& h, double scene_ior, SobolTab tab, const AovRays& rays) {
    const double* positions = h.w[0].p;
    const uint64_t n = (uint64_t)c.pixels * c.spp;
    for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += (uint64_t)gridDim.x * blockDim.x) {
        const Ray ray = probeRay<true>(c, positions, scene_ior, (uint32_t)(r % c.pixels), (uint32_t)(r / c.pixels), tab);
        aovStore3(rays.start, r, ray.start);
        aovStore3(rays.direction, r, ray.direction);
    }
}

// h.model MCRT_LENS_NONE: the camera's own rays, the loop this kernel has always run (the sine / cosine table read from memory, not
// staged). Any other model: the table staged in LDS as lightingRayKernel does, then that model's loop - the internal models past
// MCRT_LENS_FISHEYE are the ray source's two loops (launchSourceRays) and the probe rays' (launchProbeRays), which read nothing of the
// camera but the pixels' names.
// Four waves a SIMD, what the kernel had before it learned the models (98 VGPRs then): left alone the compiler takes 140 VGPRs, three
// waves; held to 128 it still spills nothing (profiles/NOTES_lens.md).
__global__ void __launch_bounds__(kAovBlock) __attribute__((amdgpu_waves_per_eu(4, 4))) aovRayKernel(AovChunk c, RayHead h, double scene_ior, const uint32_t* sobol_tab, AovRays rays) {
    __shared__ uint32_t ltab[kSobolTableWords];
    for (uint32_t i = threadIdx.x; i < (uint32_t)kSobolTableWords; i += blockDim.x) ltab[i] = sobol_tab[i];
    if (h.model != MCRT_LENS_NONE) glibc235::stageSinCosTab();  // (a kernel argument: every lane of the workgroup takes the same side)
    __syncthreads();
    // The arguments' doubles and pointers into VGPRs before the branch: as SGPRs the union of what the loops read stays live across the
    // staging loops and the branch next to each loop's own FP64 constants (a pair each), and SGPRs spill to lanes. The values are the
    // same bits; there are VGPRs to spare (profiles/NOTES_lens.md). (The head's three words as doubles, whatever they hold.)
#pragma unroll
    for (int k = 0; k < 3; k++) {
        toVgpr(c.cam.eye[k]);
        toVgpr(c.cam.forward[k]);
        toVgpr(c.cam.left[k]);
        toVgpr(c.cam.up[k]);
    }
    toVgpr(c.cam.focal_length);
    toVgpr(c.cam.sensor_width);
    toVgpr(c.cam.aperture_radius);
    toVgpr(c.cam.focus_distance);
    toVgpr(h.w[0].d);
    toVgpr(h.w[1].d);
    toVgpr(h.w[2].d);
    toVgpr(scene_ior);
    toVgpr(rays.start);
    toVgpr(rays.direction);
    toVgpr(c.first_pixel);
    const LensSettings lens{h.model, h.w[0].d, h.w[1].d, h.w[2].d};
    switch (h.model) {
        case MCRT_LENS_NONE: {
            const uint64_t n = (uint64_t)c.pixels * c.spp;
            for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += (uint64_t)gridDim.x * blockDim.x) {
                const Ray ray = aovCameraRay<false>(c, scene_ior, (uint32_t)(r % c.pixels), (uint32_t)(r / c.pixels), (SobolTab)ltab);
                aovStore3(rays.start, r, ray.start);
                aovStore3(rays.direction, r, ray.direction);
            }
            break;
        }
        case MCRT_LENS_PERSPECTIVE: lensRaysOf<MCRT_LENS_PERSPECTIVE>(c, lens, scene_ior, (SobolTab)ltab, rays); break;
        case MCRT_LENS_ORTHOGRAPHIC: lensRaysOf<MCRT_LENS_ORTHOGRAPHIC>(c, lens, scene_ior, (SobolTab)ltab, rays); break;
        case MCRT_LENS_EQUIRECTANGULAR: lensRaysOf<MCRT_LENS_EQUIRECTANGULAR>(c, lens, scene_ior, (SobolTab)ltab, rays); break;
        // (the source's two loops as cases of their own and FISHEYE the default, as it was: with a source's loop as the default the
        // compiler spills three constants of the thin-lens PERSPECTIVE loop, the kernel's register maximum - profiles/NOTES_ray_source.md)
        case kLensModelSourceRays: sourceRaysOf<MCRT_RAY_SOURCE_RAYS>(c, h, scene_ior, (SobolTab)ltab, rays); break;
        case kLensModelSourceSurface: sourceRaysOf<MCRT_RAY_SOURCE_SURFACE>(c, h, scene_ior, (SobolTab)ltab, rays); break;
        case kLensModelProbe: probeRaysOf(c, h, scene_ior, (SobolTab)ltab, rays); break;
        default: lensRaysOf<MCRT_LENS_FISHEYE>(c, lens, scene_ior, (SobolTab)ltab, rays); break;
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

int launchRays(void* stream, const AovChunk& c, const RayHead& h, double scene_ior, const uint32_t* sobol_tab, const AovRays& rays) {
    const uint64_t n = (uint64_t)c.pixels * c.spp;
    const uint32_t grid = (uint32_t)std::min<uint64_t>((n + kAovBlock - 1) / kAovBlock, 4096);
    hipLaunchKernelGGL(aovRayKernel, dim3(grid), dim3(kAovBlock), 0, (hipStream_t)stream, c, h, scene_ior, sobol_tab, rays);
    return (int)hipGetLastError();
}
}  // namespace

namespace mcrt {
int launchLensRays(void* stream, const AovChunk& c, const LensSettings& lens, double scene_ior, const uint32_t* sobol_tab, const AovRays& rays) {
    RayHead h{};
    h.model = lens.model;
    h.w[0].d = lens.width_world;
    h.w[1].d = lens.fov_x;
    h.w[2].d = lens.fov_y;
    return launchRays(stream, c, h, scene_ior, sobol_tab, rays);
}
// The chunk's records must lie inside the source's arrays (first_pixel + pixels <= source.pixels < 2^32, and no more samples than
// per-sample arrays hold): the calls check the camera's shard against the descriptor before any chunk is cut (checkCamera), and the
// launch refuses what would read past them.
int launchSourceRays(void* stream, const AovChunk& c, const RaySource& source, double scene_ior, const uint32_t* sobol_tab, const AovRays& rays) {
    if ((source.kind != MCRT_RAY_SOURCE_RAYS && source.kind != MCRT_RAY_SOURCE_SURFACE) || !source.a || !source.b || source.pixels > 0xFFFFFFFFull ||
        c.first_pixel + c.pixels > source.pixels || (raySourceReadsSpp(source) && c.spp > source.spp))
        return (int)hipErrorInvalidValue;
    RayHead h{};
    h.model = source.kind == MCRT_RAY_SOURCE_RAYS ? kLensModelSourceRays : kLensModelSourceSurface;
    h.stride = source.kind == MCRT_RAY_SOURCE_RAYS && !source.per_pixel ? (uint32_t)source.pixels : 0u;
    h.w[0].p = source.a;
    h.w[1].p = source.b;
    h.w[2].d = source.offset;
    return launchRays(stream, c, h, scene_ior, sobol_tab, rays);
}
// The chunk's pixels must lie inside positions' `pixels` records.
int launchProbeRays(void* stream, const AovChunk& c, const double* positions, uint64_t pixels, double scene_ior, const uint32_t* sobol_tab, const AovRays& rays) {
    if (!positions || pixels > 0xFFFFFFFFull || c.first_pixel + c.pixels > pixels) return (int)hipErrorInvalidValue;
    RayHead h{};
    h.model = kLensModelProbe;
    h.w[0].p = positions;
    return launchRays(stream, c, h, scene_ior, sobol_tab, rays);
}
int launchAovRays(void* stream, const AovChunk& c, double scene_ior, const uint32_t* sobol_tab, const AovRays& rays) {
    return launchLensRays(stream, c, LensSettings{MCRT_LENS_NONE, 0.0, 0.0, 0.0}, scene_ior, sobol_tab, rays);
}
int launchAovResolve(void* stream, const AovChunk& c, const AovScene& scene, const AovRays& rays, const mcrt_aov_buffers& out) {
    hipLaunchKernelGGL(aovResolveKernel, dim3((c.pixels + kAovBlock - 1) / kAovBlock), dim3(kAovBlock), 0, (hipStream_t)stream, c, scene, rays, out);
    return (int)hipGetLastError();
}
}  // namespace mcrt
