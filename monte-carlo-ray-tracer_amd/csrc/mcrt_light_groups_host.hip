// Light groups (include/mcrt.h mcrt_render_light_groups*), host side: the group map, the samples' state, and behind the camera-ray
// passes' chunk loop (mcrt_camera_pass.hpp), which writes the camera rays and their hits straight into that state, the bounce loop
// (runLivePaths, mcrt_live_paths_host.hpp, which the path classes run too):
// launchLightGroupsBegin starts the paths, then per iteration launchLightGroupsRays -> intersectDeviceArrays over 2 rays per LIVE sample
// -> launchLightGroupsStep, the host reading the next list's count (and the pass's error word) after every step;
// launchLightGroupsResolve when no sample is alive. No kernel here: they are libmcrt_light_groups.so (csrc/mcrt_light_groups.hip;
// DESIGN.md "Image passes" says why). The family's scratch: slot 0 the samples' state, 1 the planes' radiances, 2 the shadow and bounce
// records, 3 the two live lists and the counters, 4 the surfaces' planes, 5 the host-pointer form's frames. Option MCRT_AOV_CHUNK_RAYS
// bounds the shadow and bounce SLOTS of iteration 0: pixels * spp * 2 (its default: lightGroupsDefaultChunkSlots).
// With MCRT_LIGHT_GROUPS_FILM and a film that splats (or option MCRT_FILM_GATHER=force) a chunk's resolve is the filtered planes' three
// launches of the same kernel (FilmPlanes, mcrt_light_groups_host.hpp).
// Option MCRT_LIGHT_GROUPS_LOG (tools/light_groups_probe.py sets it): one JSON line per chunk on stderr - the live samples of every
// iteration and the host-clock milliseconds of the chunk and of its searches, the stream drained before each bounce search so that the
// kernels queued before it are not counted as search (the camera rays' kernel is counted with their search). It changes no result.
#include "mcrt_light_groups_host.hpp"

using namespace mcrt;

extern "C" uint32_t mcrt_light_group_planes(const mcrt_light_group_params* params) {
    LgSettings r;
    return lgSettingsOf(params, r);
}

extern "C" int mcrt_render_light_groups_device(mcrt_ctx* ctx, const mcrt_camera_desc* cam, uint32_t global_seed, const mcrt_light_group_params* params,
                                               double* d_planes, mcrt_stats* stats) {
    const char* what = "mcrt_render_light_groups_device";
    if (!ctx) return MCRT_ERR_INVALID;
    LgSettings r;
    if (int rc = lgValidate(ctx, cam, params, d_planes, r, what)) return rc;
    const uint32_t flags = params ? params->flags : 0u;
    FilmPlanes film;
    if (int rc = filmPlanesValidate(ctx, cam, (flags & MCRT_LIGHT_GROUPS_FILM) != 0u, what, film)) return rc;
    PassTimer timer(ctx);
    const CameraPass cp(ctx);
    const hipStream_t stream = cp.stream;
    const AovScene& scene = cp.scene;
    const uint32_t* sobol_tab = cp.sobol_tab;
    LgWalk w;
    if (int rc = lgWalkPrepare(ctx, cam, scene, r, what, w, filmPlanesFrameBytes(film, cam), filmPlanesSampleBytes(film, cam))) return rc;
    const LgParams& par = w.par;
    const LgState& st = w.st;
    const uint64_t total_pixels = w.plan.total_pixels;
    if (film.on)
        if (int rc = filmPlanesPrepare(ctx, cam, (flags & MCRT_LIGHT_GROUPS_FILM_CLAMP) != 0u, cp, w.extra, w.sc.lit.start, d_planes, r.planes, film)) return rc;
    const int rc = runLivePaths(
        ctx, what, cp, timer, cam, global_seed, w.plan, st.ray, stats, w.sc, r.max_depth, ctxOptOn(ctx, "MCRT_LIGHT_GROUPS_LOG"), "light_groups_chunk",
        [&](const AovChunk&, uint64_t n, uint32_t* list, LgCounters* counters) { return launchLightGroupsBegin(stream, st, n, scene.sh.scene_ior, par, list, counters); },
        [&](const AovChunk& c, const uint32_t* list, uint32_t live, uint32_t k, const AovRays& lit, LgCounters* counters, uint32_t next) {
            return launchLightGroupsRays(stream, c, scene, sobol_tab, st, list, live, k, lit, counters, next);
        },
        [&](const AovChunk& c, const uint32_t* list, uint32_t live, uint32_t k, bool last, const AovRays& lit, uint32_t* next_list, LgCounters* counters, uint32_t next) {
            return launchLightGroupsStep(stream, c, scene, sobol_tab, st, par, list, live, k, last, lit, next_list, counters, next);
        },
        [&](const AovChunk& c) {
            if (!film.on) return launchLightGroupsResolve(stream, c, st, r.planes, d_planes, total_pixels);
            return filmPlanesChunk(film, c, total_pixels, [&](const FilmGather& g) { return launchLightGroupsFilm(stream, c, st, r.planes, g, d_planes, total_pixels); });
        });
    return filmPlanesFinish(film, rc, stats);
}

extern "C" int mcrt_render_light_groups(mcrt_ctx* ctx, const mcrt_camera_desc* cam, uint32_t global_seed, const mcrt_light_group_params* params, double* planes,
                                        mcrt_stats* stats) {
    const char* what = "mcrt_render_light_groups";
    if (!ctx) return MCRT_ERR_INVALID;
    LgSettings r;
    if (int rc = lgValidate(ctx, cam, params, planes, r, what)) return rc;
    FrameChannel ch[kLgPlanesMax];  // the planes, one behind the other
    const size_t frame = (size_t)cam->width * cam->height * 3;
    for (uint32_t p = 0; p < r.planes; p++) ch[p] = FrameChannel{nullptr, planes + p * frame, 24};
    return hostPointerForm(ctx, what, cam, kPassLightGroups, 5, ch, (int)r.planes, "planes'", stats,
                           [&](mcrt_stats* st) { return mcrt_render_light_groups_device(ctx, cam, global_seed, params, (double*)ch[0].dev, st); });
}
