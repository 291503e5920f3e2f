// Light probes (include/mcrt.h mcrt_render_probes*, mcrt_probe_rays_device, mcrt_probe_coefficients), host side. No kernel here: the probe
// rays are a loop of aovRayKernel (csrc/mcrt_aov.hip, libmcrt_aov.so; launchProbeRays), the projection a branch of
// lightGroupsResolveKernel (csrc/mcrt_light_groups.hip, libmcrt_light_groups.so; launchProbeResolve), and the walk between them is the
// light groups' own: their state and scratch (mcrt_light_groups_host.hpp, kPassLightGroups slots 0 .. 4), their begin / ray / step
// launches through runLivePaths. What this call adds per chunk is one copy, device to device on the stream: the first rays' directions
// (24 B a sample) out of the samples' state after the camera rays' search and before begin - the walk overwrites st.ray.direction with
// every bounce. The family's scratch (kPassProbes): slot 0 those directions, 1 the host-pointer form's frames, 2 and 3 its positions and
// weights.
#include "mcrt_light_groups_host.hpp"

using namespace mcrt;

namespace {

int validate(mcrt_ctx* ctx, const mcrt_camera_desc* cam, const mcrt_probe_params* params, const void* coefficients, LgSettings& r, const char* what) {
    if (!params) return ctxFail(ctx, MCRT_ERR_INVALID, std::string(what) + ": params is NULL");
    if (int rc = cameraPassReady(ctx, what)) return rc;
    if (!coefficients) return ctxFail(ctx, MCRT_ERR_INVALID, std::string(what) + ": coefficients is NULL");
    const char* why = nullptr;
    if (int rc = probeSettings(*params, &why)) return ctxFail(ctx, rc, std::string(what) + ": " + why);
    if (params->positions && ctxLens(ctx))
        return ctxFail(ctx, MCRT_ERR_INVALID, std::string(what) + ": positions with a lens set (mcrt_set_lens) - the probe rays are the call's own; mcrt_set_lens(ctx, NULL) takes it off");
    if (params->positions && ctxRaySource(ctx))
        return ctxFail(ctx, MCRT_ERR_INVALID, std::string(what) + ": positions with a ray source set (mcrt_set_ray_source) - the probe rays are the call's own; "
                                                                 "mcrt_set_ray_source(ctx, NULL) takes it off");
    return lgValidate(ctx, cam, &params->groups, coefficients, r, what);
}

}  // namespace

extern "C" uint32_t mcrt_probe_coefficients(uint32_t order) { return probeCoefficients(order); }

extern "C" int mcrt_render_probes_device(mcrt_ctx* ctx, const mcrt_camera_desc* cam, uint32_t global_seed, const mcrt_probe_params* params, double* d_coefficients,
                                         mcrt_stats* stats) {
    const char* what = "mcrt_render_probes_device";
    if (!ctx) return MCRT_ERR_INVALID;
    LgSettings r;
    if (int rc = validate(ctx, cam, params, d_coefficients, r, what)) return rc;
    PassTimer timer(ctx);
    const CameraPass cp(ctx);
    const hipStream_t stream = cp.stream;
    const AovScene& scene = cp.scene;
    const uint32_t* sobol_tab = cp.sobol_tab;
    LgWalk w;
    if (int rc = lgWalkPrepare(ctx, cam, scene, r, what, w)) return rc;
    const LgParams& par = w.par;
    const LgState& st = w.st;
    const uint64_t total_pixels = w.plan.total_pixels;
    double* first_direction = (double*)ctxPassScratch(ctx, kPassProbes, 0, w.plan.max_rays * 24);
    if (!first_direction)
        return ctxFail(ctx, MCRT_ERR_HIP, std::string(what) + ": " + std::to_string((w.plan.max_rays * 24) >> 20) +
                                              " MiB for the first rays' directions could not be allocated (option MCRT_AOV_CHUNK_RAYS sizes it)");
    const ProbeProjection proj{probeCoefficients(params->order), 0u, first_direction, params->weight};

    const auto begin = [&](const AovChunk&, uint64_t n, uint32_t* list, LgCounters* counters) {
        const hipError_t e = hipMemcpyAsync(first_direction, st.ray.direction, n * 24, hipMemcpyDeviceToDevice, stream);
        return e != hipSuccess ? (int)e : launchLightGroupsBegin(stream, st, n, scene.sh.scene_ior, par, list, counters);
    };
    const auto rays_of = [&](const AovChunk& c, const uint32_t* list, uint32_t live, uint32_t k, const AovRays& lit, LgCounters* counters, uint32_t next) {
        return launchLightGroupsRays(stream, c, scene, sobol_tab, st, list, live, k, lit, counters, next);
    };
    const auto step = [&](const AovChunk& c, const uint32_t* list, uint32_t live, uint32_t k, bool last, const AovRays& lit, uint32_t* next_list, LgCounters* counters,
                          uint32_t next) { return launchLightGroupsStep(stream, c, scene, sobol_tab, st, par, list, live, k, last, lit, next_list, counters, next); };
    const auto resolve = [&](const AovChunk& c) { return launchProbeResolve(stream, c, st, r.planes, proj, d_coefficients, total_pixels); };
    const bool log = ctxOptOn(ctx, "MCRT_LIGHT_GROUPS_LOG");
    if (params->positions)
        return runLivePathsOf(ProbePixels{params->positions, total_pixels}, ctx, what, cp, timer, cam, global_seed, w.plan, st.ray, stats, w.sc, r.max_depth, log,
                              "probes_chunk", begin, rays_of, step, resolve);
    return runLivePaths(ctx, what, cp, timer, cam, global_seed, w.plan, st.ray, stats, w.sc, r.max_depth, log, "probes_chunk", begin, rays_of, step, resolve);
}

extern "C" int mcrt_render_probes(mcrt_ctx* ctx, const mcrt_camera_desc* cam, uint32_t global_seed, const mcrt_probe_params* params, double* coefficients,
                                  mcrt_stats* stats) {
    const char* what = "mcrt_render_probes";
    if (!ctx) return MCRT_ERR_INVALID;
    LgSettings r;
    if (int rc = validate(ctx, cam, params, coefficients, r, what)) return rc;
    const uint64_t pixels = (uint64_t)mcrt_shard_rows(cam, nullptr) * cam->width;
    const uint32_t spp = cam->sqrtspp * cam->sqrtspp, frames = r.planes * probeCoefficients(params->order);
    mcrt_probe_params on_device = *params;
    const auto upload = [&](const double* host, int slot, size_t bytes, const double** dev, const char* noun) {
        if (!host) return (int)MCRT_OK;
        void* d = ctxPassScratch(ctx, kPassProbes, slot, bytes);
        if (!d) return ctxFail(ctx, MCRT_ERR_HIP, std::string(what) + ": the " + noun + " device copy could not be allocated");
        MCRT_HIP_TRY(ctx, hipMemcpy(d, host, bytes, hipMemcpyHostToDevice));
        *dev = (const double*)d;
        return (int)MCRT_OK;
    };
    if (int rc = upload(params->positions, 2, (size_t)pixels * 24, &on_device.positions, "positions'")) return rc;
    if (int rc = upload(params->weight, 3, (size_t)pixels * spp * 8, &on_device.weight, "weights'")) return rc;
    FrameChannel ch[kLgPlanesMax * kProbeCoefficientsMax];  // the coefficients' frames, one behind the other
    const size_t frame = (size_t)cam->width * cam->height * 3;
    for (uint32_t f = 0; f < frames; f++) ch[f] = FrameChannel{nullptr, coefficients + f * frame, 24};
    return hostPointerForm(ctx, what, cam, kPassProbes, 1, ch, (int)frames, "coefficients'", stats,
                           [&](mcrt_stats* st) { return mcrt_render_probes_device(ctx, cam, global_seed, &on_device, (double*)ch[0].dev, st); });
}

extern "C" int mcrt_probe_rays_device(mcrt_ctx* ctx, const mcrt_camera_desc* cam, uint32_t global_seed, const double* d_positions, double* d_start,
                                      double* d_direction, mcrt_stats* stats) {
    const char* what = "mcrt_probe_rays_device";
    if (!ctx) return MCRT_ERR_INVALID;
    if (int rc = cameraPassReady(ctx, what)) return rc;
    if (ctxLens(ctx)) return ctxFail(ctx, MCRT_ERR_INVALID, std::string(what) + ": a lens is set (mcrt_set_lens) - the probe rays are the call's own; mcrt_set_lens(ctx, NULL) takes it off");
    if (ctxRaySource(ctx))
        return ctxFail(ctx, MCRT_ERR_INVALID, std::string(what) + ": a ray source is set (mcrt_set_ray_source) - the probe rays are the call's own; "
                                                                 "mcrt_set_ray_source(ctx, NULL) takes it off");
    if (int rc = checkCamera(ctx, cam, d_positions && d_start && d_direction, what, "cam, positions, start or direction is NULL")) return rc;
    const uint64_t pixels = (uint64_t)mcrt_shard_rows(cam, nullptr) * cam->width;
    const uint32_t spp = cam->sqrtspp * cam->sqrtspp;
    if (pixels * spp > kClosestHitMaxRays)
        return ctxFail(ctx, MCRT_ERR_UNSUPPORTED, std::string(what) + ": more rays than one closest-hit launch takes (" + std::to_string(kClosestHitMaxRays) + ")");
    PassTimer timer(ctx);
    const CameraPass cp(ctx);
    const AovRays rays{d_start, d_direction, nullptr, nullptr, nullptr};
    if (int rc = timer.begin(cp.stream)) return rc;
    if (pixels) {  // one chunk: the shard's packed pixels
        const ProbePixels naming{d_positions, pixels};
        MCRT_HIP_TRY(ctx, (hipError_t)naming.rays(cp.stream, chunkAt(*cam, global_seed, spp, 0, pixels, pixels), cp.scene.sh.scene_ior, cp.sobol_tab, rays));
    }
    if (int rc = timer.end(cp.stream)) return rc;
    if (int rc = timer.finish(stats, pixels ? 1 : 0)) return rc;
    if (stats) stats->paths = stats->rays = pixels * spp;
    return MCRT_OK;
}
