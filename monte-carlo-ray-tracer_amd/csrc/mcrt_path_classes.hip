// Path classes (include/mcrt.h mcrt_render_path_classes*): built BESIDE the render path like the light groups, whose walk this is - four
// kernels of their own around the closest-hit search mcrt_intersect already has, none of the render kernels touched. This translation
// unit is the whole of libmcrt_path_classes.so, which libmcrt_hip.so (and its tolerance twin: the same exact object) links: the kernels
// and their launch functions; the host side of the pass is csrc/mcrt_path_classes_host.hip.
//   pathClassesBeginKernel    one lane per sample: pathBegin, the sky of a camera ray that missed into the background's plane, and the
//                             first live list
//   pathClassesRayKernel      one lane per LIVE sample: lgRays, the light groups' shadow and bounce rays of vertex k
//   pathClassesStepKernel     one lane per live sample: pcStep - the terms of vertex k into the planes of the path's class (step 0 finds
//                             the class and stores it), the state of vertex k + 1, the sample appended to the other list
//   pathClassesResolveKernel  one lane per pixel: lgResolvePixel (a call with the FILM flag: the three branches of mcrt_film_gather.hpp)
// Launch shape, the tables and the refraction history in LDS ([entry][lane]) and the wave-aggregated append (one ballot, one atomic per
// wave, mbcnt for the lane's place) are mcrt_light_groups_device.hpp's, as in mcrt_light_groups.hip.
#include <hip/hip_runtime.h>

#include "mcrt_light_groups_device.hpp"
#include "mcrt_path_classes_launch.hpp"

using namespace mcrt;

namespace {

__global__ void __launch_bounds__(kLgBlock) pathClassesBeginKernel(PcState st, uint64_t n, double scene_ior, PcParams par, uint32_t* list, LgCounters* counters) {
    for (uint64_t base = (uint64_t)blockIdx.x * blockDim.x; base < n; base += (uint64_t)gridDim.x * blockDim.x) {  // (whole blocks: lgAppendLive)
        const uint64_t s = base + threadIdx.x;
        const bool alive = s < n && pcBegin(st, s, scene_ior, par);
        lgAppendLive(list, &counters->live[0], alive, (uint32_t)s);
    }
}

__global__ void __launch_bounds__(kLgBlock) pathClassesRayKernel(AovChunk c, AovScene scene, const uint32_t* sobol_tab, LgState st, const uint32_t* list, uint32_t n_live,
                                                                 uint32_t k, AovRays lit, LgCounters* counters, uint32_t next) {
    __shared__ uint32_t ltab[kSobolTableWords];
    __shared__ double liors[kMaxIors * kLgBlock];
    if (blockIdx.x == 0 && threadIdx.x == 0) counters->live[next] = 0u;  // the list this iteration's step kernel appends to
    lgStageTables(ltab, sobol_tab);
    RefractionHistory rh = lgLaneHistory(liors);
    for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < n_live; j += (uint64_t)gridDim.x * blockDim.x)
        lgRays(c, scene, st, list, n_live, (uint32_t)j, k, lit, rh, (SobolTab)ltab);
}

__global__ void __launch_bounds__(kLgBlock) pathClassesStepKernel(AovChunk c, AovScene scene, const uint32_t* sobol_tab, PcState st, PcParams par, const uint32_t* list,
                                                                  uint32_t n_live, uint32_t k, uint32_t last, AovRays lit, uint32_t* next_list, LgCounters* counters,
                                                                  uint32_t next) {
    __shared__ uint32_t ltab[kSobolTableWords];
    __shared__ double liors[kMaxIors * kLgBlock];
    lgStageTables(ltab, sobol_tab);
    RefractionHistory rh = lgLaneHistory(liors);
    // whole blocks go round together, so that every lane of a wave reaches lgAppendLive; j < n_live bounds every access of the lane
    for (uint64_t base = (uint64_t)blockIdx.x * blockDim.x; base < n_live; base += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t j = base + threadIdx.x;
        bool alive = false, too_deep = false;
        uint32_t sample = 0u;
        if (j < n_live) {
            sample = list[j];
            alive = pcStep(c, scene, st, par, list, n_live, (uint32_t)j, k, last != 0u, lit, rh, too_deep, (SobolTab)ltab);
        }
        if (too_deep) counters->too_deep = 1u;
        lgAppendLive(next_list, &counters->live[next], alive, sample);
    }
}

// film.mode != 0: a branch of the filtered planes (mcrt_film_gather.hpp), as in lightGroupsResolveKernel; a kernel argument, uniform
// over the launch.
__global__ void __launch_bounds__(kLgBlock) pathClassesResolveKernel(AovChunk c, LgState st, uint32_t planes, double* out, uint64_t frame_pixels, FilmGather film) {
    if (film.mode != kFilmGatherNone) {
        // (one lane each, no stride: in a loop the compiler keeps the constants of every filter in registers across it)
        const uint64_t x = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
        if (x < filmGatherLanesX(c, film, frame_pixels)) filmGatherDo(c, st, film, blockIdx.y, (uint32_t)x, out, frame_pixels);
        return;
    }
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= c.pixels) return;
    lgResolvePixel(c, st, planes, p, out, frame_pixels);
}

}  // namespace

namespace mcrt {
int launchPathClassesBegin(void* stream, const PcState& st, uint64_t n, double scene_ior, const PcParams& par, uint32_t* list, LgCounters* counters) {
    hipLaunchKernelGGL(pathClassesBeginKernel, dim3(lgGridFor(n)), dim3(kLgBlock), 0, (hipStream_t)stream, st, n, scene_ior, par, list, counters);
    return (int)hipGetLastError();
}
int launchPathClassesRays(void* stream, const AovChunk& c, const AovScene& scene, const uint32_t* sobol_tab, const PcState& st, const uint32_t* list, uint32_t n_live,
                          uint32_t k, const AovRays& lit, LgCounters* counters, uint32_t next) {
    hipLaunchKernelGGL(pathClassesRayKernel, dim3(lgGridFor(n_live)), dim3(kLgBlock), 0, (hipStream_t)stream, c, scene, sobol_tab, st.lg, list, n_live, k, lit, counters, next);
    return (int)hipGetLastError();
}
int launchPathClassesStep(void* stream, const AovChunk& c, const AovScene& scene, const uint32_t* sobol_tab, const PcState& st, const PcParams& par, const uint32_t* list,
                          uint32_t n_live, uint32_t k, bool last, const AovRays& lit, uint32_t* next_list, LgCounters* counters, uint32_t next) {
    hipLaunchKernelGGL(pathClassesStepKernel, dim3(lgGridFor(n_live)), dim3(kLgBlock), 0, (hipStream_t)stream, c, scene, sobol_tab, st, par, list, n_live, k,
                       last ? 1u : 0u, lit, next_list, counters, next);
    return (int)hipGetLastError();
}
int launchPathClassesResolve(void* stream, const AovChunk& c, const PcState& st, uint32_t planes, double* out, uint64_t frame_pixels) {
    hipLaunchKernelGGL(pathClassesResolveKernel, dim3((c.pixels + kLgBlock - 1) / kLgBlock), dim3(kLgBlock), 0, (hipStream_t)stream, c, st.lg, planes, out, frame_pixels,
                       FilmGather{});
    return (int)hipGetLastError();
}
int launchPathClassesFilm(void* stream, const AovChunk& c, const PcState& st, uint32_t planes, const FilmGather& film, double* out, uint64_t frame_pixels) {
    if (!filmGatherLaunchable(c, st.lg, planes, film, out, frame_pixels)) return (int)hipErrorInvalidValue;
    const uint64_t blocks = ((uint64_t)filmGatherLanesX(c, film, frame_pixels) + kLgBlock - 1) / kLgBlock;
    if (blocks == 0) return (int)hipSuccess;
    hipLaunchKernelGGL(pathClassesResolveKernel, dim3((uint32_t)blocks, filmGatherLaneRows(planes, film)), dim3(kLgBlock), 0, (hipStream_t)stream, c, st.lg, planes, out,
                       frame_pixels, film);
    return (int)hipGetLastError();
}
}  // namespace mcrt
