// Light groups (include/mcrt.h mcrt_render_light_groups*): built BESIDE the render path like the lighting passes - four kernels of their
// own around the closest-hit search mcrt_intersect already has (intersectDeviceArrays, mcrt_hip.hip), none of the render kernels touched.
// This translation unit is the whole of libmcrt_light_groups.so, which libmcrt_hip.so (and its tolerance twin: the same exact object)
// links: the kernels and their launch functions; the host side of the pass is csrc/mcrt_light_groups_host.hip.
// Per chunk of whole pixels, after the AOV pass's camera rays and their closest hits (written straight into the samples' state):
//   lightGroupsBeginKernel    one lane per sample: pathBegin (throughput 1, the history's first entry, R_p = 0), the sky of a camera ray
//                             that missed, and the first live list: the samples that hit
//   per iteration k, while a sample is alive:
//   lightGroupsRayKernel      one lane per LIVE sample: vertex k rebuilt from the stored ray and hit (lgVertex), its shadow ray into record
//                             j, its bounce ray into record n_live + j of ONE array
//   (closest hits)            the search once, over both rays of every live sample
//   lightGroupsStepKernel     one lane per live sample: vertex k rebuilt once more (nothing of it is stored), its terms added to their
//                             planes - the sky's too when the bounce ray missed -, otherwise the state of vertex k + 1 stored and the
//                             sample appended to the OTHER list
//   lightGroupsResolveKernel  one lane per pixel: the samples' R_p in ascending order into one FP64 accumulator per word (a probe call:
//                             one lane per output word, R_p times a function of the first ray's direction - mcrt_probes.hpp; a call
//                             with the FILM flag: the three branches of mcrt_film_gather.hpp)
// The live list is what keeps the iterations as wide as the work: paths die at very different depths, and an iteration costs its live
// samples only. A wave appends with ONE atomic: the ballot of its surviving lanes, its population count for the leader's atomicAdd on
// the list's counter, mbcnt for each lane's place behind the leader's base. The order of the list depends on the order in which waves
// reach their atomic; nothing of it reaches the output, because a sample's words are its own (state and R_p are indexed by sample).
// The shading kernels stage what the shading code reads from LDS - the Sobol byte tables and the sine / cosine table - and keep the lane's
// refraction history there ([entry][lane], loaded from the state at entry and written back at exit).
#include <hip/hip_runtime.h>

#include "mcrt_light_groups_device.hpp"
#include "mcrt_light_groups_launch.hpp"

using namespace mcrt;

namespace {

__global__ void __launch_bounds__(kLgBlock) lightGroupsBeginKernel(LgState st, uint64_t n, double scene_ior, LgParams par, uint32_t* list, LgCounters* counters) {
    for (uint64_t base = (uint64_t)blockIdx.x * blockDim.x; base < n; base += (uint64_t)gridDim.x * blockDim.x) {  // (whole blocks: lgAppendLive)
        const uint64_t s = base + threadIdx.x;
        const bool alive = s < n && lgBegin(st, s, scene_ior, par);
        lgAppendLive(list, &counters->live[0], alive, (uint32_t)s);
    }
}

__global__ void __launch_bounds__(kLgBlock) lightGroupsRayKernel(AovChunk c, AovScene scene, const uint32_t* sobol_tab, LgState st, const uint32_t* list, uint32_t n_live,
                                                                 uint32_t k, AovRays lit, LgCounters* counters, uint32_t next) {
    __shared__ uint32_t ltab[kSobolTableWords];
    __shared__ double liors[kMaxIors * kLgBlock];
    if (blockIdx.x == 0 && threadIdx.x == 0) counters->live[next] = 0u;  // the list this iteration's step kernel appends to (one fill launch less per iteration)
    lgStageTables(ltab, sobol_tab);
    RefractionHistory rh = lgLaneHistory(liors);
    for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < n_live; j += (uint64_t)gridDim.x * blockDim.x)
        lgRays(c, scene, st, list, n_live, (uint32_t)j, k, lit, rh, (SobolTab)ltab);
}

__global__ void __launch_bounds__(kLgBlock) lightGroupsStepKernel(AovChunk c, AovScene scene, const uint32_t* sobol_tab, LgState st, LgParams par, const uint32_t* list,
                                                                  uint32_t n_live, uint32_t k, uint32_t last, AovRays lit, uint32_t* next_list, LgCounters* counters,
                                                                  uint32_t next) {
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

// proj.coefficients == 0: the plain mean, one lane per pixel, as ever. Otherwise a probe call's projection (mcrt_probes.hpp), one lane per
// output word - (plane, k, channel) of a pixel -, because such a call has few pixels and many samples: 64 probes of 4096 rays would be
// one wave looping 4096 times per plane as lanes per pixel, and are 64 * planes * K * 3 lanes this way. The branch is a kernel argument,
// uniform over the launch.
// film.mode != 0: a branch of the filtered planes (mcrt_film_gather.hpp) - the samples' film positions, the gather that continues S and
// W, or the division after the last chunk -, lanes striding over that branch's work; like proj a kernel argument, uniform over the launch.
__global__ void __launch_bounds__(kLgBlock) lightGroupsResolveKernel(AovChunk c, LgState st, uint32_t planes, double* out, uint64_t frame_pixels, ProbeProjection proj,
                                                                     FilmGather film) {
    if (film.mode != kFilmGatherNone) {
        // (one lane each, no stride: in a loop the compiler keeps the constants of every filter in registers across it)
        const uint64_t x = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
        if (x < filmGatherLanesX(c, film, frame_pixels)) filmGatherDo(c, st, film, blockIdx.y, (uint32_t)x, out, frame_pixels);
        return;
    }
    if (proj.coefficients == 0u) {
        const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
        if (p >= c.pixels) return;
        lgResolvePixel(c, st, planes, p, out, frame_pixels);
        return;
    }
    const uint64_t lanes = probeLanes(c, planes, proj);
    for (uint64_t lane = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; lane < lanes; lane += (uint64_t)gridDim.x * blockDim.x)
        probeResolveLane(c, st, proj, lane, out, frame_pixels);
}

}  // namespace

namespace mcrt {
int launchLightGroupsBegin(void* stream, const LgState& st, uint64_t n, double scene_ior, const LgParams& par, uint32_t* list, LgCounters* counters) {
    hipLaunchKernelGGL(lightGroupsBeginKernel, dim3(lgGridFor(n)), dim3(kLgBlock), 0, (hipStream_t)stream, st, n, scene_ior, par, list, counters);
    return (int)hipGetLastError();
}
int launchLightGroupsRays(void* stream, const AovChunk& c, const AovScene& scene, const uint32_t* sobol_tab, const LgState& st, const uint32_t* list, uint32_t n_live,
                          uint32_t k, const AovRays& lit, LgCounters* counters, uint32_t next) {
    hipLaunchKernelGGL(lightGroupsRayKernel, dim3(lgGridFor(n_live)), dim3(kLgBlock), 0, (hipStream_t)stream, c, scene, sobol_tab, st, list, n_live, k, lit, counters, next);
    return (int)hipGetLastError();
}
int launchLightGroupsStep(void* stream, const AovChunk& c, const AovScene& scene, const uint32_t* sobol_tab, const LgState& st, const LgParams& par, const uint32_t* list,
                          uint32_t n_live, uint32_t k, bool last, const AovRays& lit, uint32_t* next_list, LgCounters* counters, uint32_t next) {
    hipLaunchKernelGGL(lightGroupsStepKernel, dim3(lgGridFor(n_live)), dim3(kLgBlock), 0, (hipStream_t)stream, c, scene, sobol_tab, st, par, list, n_live, k,
                       last ? 1u : 0u, lit, next_list, counters, next);
    return (int)hipGetLastError();
}
int launchLightGroupsResolve(void* stream, const AovChunk& c, const LgState& st, uint32_t planes, double* out, uint64_t frame_pixels) {
    hipLaunchKernelGGL(lightGroupsResolveKernel, dim3((c.pixels + kLgBlock - 1) / kLgBlock), dim3(kLgBlock), 0, (hipStream_t)stream, c, st, planes, out, frame_pixels,
                       ProbeProjection{}, FilmGather{});
    return (int)hipGetLastError();
}
int launchProbeResolve(void* stream, const AovChunk& c, const LgState& st, uint32_t planes, const ProbeProjection& proj, double* out, uint64_t frame_pixels) {
    if (proj.coefficients == 0u || proj.coefficients > kProbeCoefficientsMax || !proj.direction || planes == 0u || planes > kLgPlanesMax || !out ||
        c.first_pixel + c.pixels > frame_pixels || (uint64_t)c.pixels * c.spp > st.n)
        return (int)hipErrorInvalidValue;
    const uint64_t blocks = (probeLanes(c, planes, proj) + kLgBlock - 1) / kLgBlock;
    if (blocks == 0) return (int)hipSuccess;
    hipLaunchKernelGGL(lightGroupsResolveKernel, dim3((uint32_t)std::min<uint64_t>(blocks, 1u << 20)), dim3(kLgBlock), 0, (hipStream_t)stream, c, st, planes, out, frame_pixels, proj, FilmGather{});
    return (int)hipGetLastError();
}
int launchLightGroupsFilm(void* stream, const AovChunk& c, const LgState& st, uint32_t planes, const FilmGather& film, double* out, uint64_t frame_pixels) {
    if (!filmGatherLaunchable(c, st, planes, film, out, frame_pixels)) return (int)hipErrorInvalidValue;
    const uint64_t blocks = ((uint64_t)filmGatherLanesX(c, film, frame_pixels) + kLgBlock - 1) / kLgBlock;
    if (blocks == 0) return (int)hipSuccess;
    hipLaunchKernelGGL(lightGroupsResolveKernel, dim3((uint32_t)blocks, filmGatherLaneRows(planes, film)), dim3(kLgBlock), 0, (hipStream_t)stream, c, st, planes, out, frame_pixels,
                       ProbeProjection{}, film);
    return (int)hipGetLastError();
}
}  // namespace mcrt
